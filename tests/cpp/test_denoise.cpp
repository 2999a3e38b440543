// tests/cpp/test_denoise.cpp -- RayTracer::denoise (an addition to the drop-in class): argv[1] = .scn, argv[2] = width, argv[3] = height,
// argv[4] = feature samples, argv[5] = iterations.  Renders the feature buffers, builds a noisy colour from them with integer-hash noise (so that
// the test can build the same doubles), denoises, and prints the sum of the result with all digits for the test to compare with the Python mirror's.
// argv[6] (optional): a file that gets the raw doubles of albedo, normal, depth, coverage, the colour and the result, in this order.
#include <cstdio>
#include <cstdlib>
#include "../../include/gi/builtin_loaders.h"

int main(int argc, char** argv)
{
    if (argc < 6) return 2;
    Camera camera(gi::dvec3(10, 5, 0), gi::dvec3(0, 0, 0));
    RayTracer raytracer(camera);
    Octree* scene = new Octree();
    loadScene(scene, raytracer, argv[1]);
    raytracer.setScene(scene);
    scene->rebuild();
    RayTracer::Features f;
    if (!raytracer.renderFeatures(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), f)) { printf("failed: %s\n", raytracer.last_error().c_str()); return 1; }
    const size_t npix = (size_t)f.width * f.height;
    std::vector<double> color(npix * 3), out;
    for (size_t i = 0; i < npix * 3; i++) {
        const uint32_t hsh = (uint32_t)i * 2654435761u;
        color[i] = f.albedo[i] * ((double)((hsh >> 8) & 0xffffu) / 65536.0) + 0.0625 * f.coverage[i / 3];
    }
    gi_denoise_params p;
    gi_denoise_default_params(&p);
    p.iterations = atoi(argv[5]);
    if (!raytracer.denoise(color, f, out, &p)) { printf("failed: %s\n", raytracer.last_error().c_str()); return 1; }
    double s = 0, s0 = 0;
    for (double v : out) s += v;
    for (double v : color) s0 += v;
    printf("denoise %dx%d iterations %d size %zu\n", f.width, f.height, p.iterations, out.size());
    printf("sums %.17g %.17g\n", s0, s);
    if (argc > 6) {
        FILE* fp = fopen(argv[6], "wb");
        if (!fp) return 3;
        for (const std::vector<double>* v : {&f.albedo, &f.normal, &f.depth, &f.coverage, &color, &out}) fwrite(v->data(), sizeof(double), v->size(), fp);
        fclose(fp);
    }
    std::vector<double> def, keep(3, 7.0);
    printf("defaults ok %d\n", (int)raytracer.denoise(color, f, def));
    double sd = 0;
    for (double v : def) sd += v;
    printf("default sum %.17g\n", sd);
    p.iterations = 9;
    printf("iterations=9 ok %d kept %d\n", (int)raytracer.denoise(color, f, keep, &p), (int)(keep.size() == 3 && keep[0] == 7.0));
    color.pop_back();
    printf("short colour ok %d\n", (int)raytracer.denoise(color, f, keep));
    return 0;
}
