// tests/cpp/test_features.cpp -- RayTracer::renderFeatures (an addition to the drop-in class) on a loaded scene: argv[1] = .scn, argv[2] = width,
// argv[3] = height, argv[4] = samples.  Prints sums of every buffer with all digits and the number of misses, for the test to compare with the Python mirror's.
#include <cstdio>
#include <cstdlib>
#include "../../include/gi/builtin_loaders.h"

int main(int argc, char** argv)
{
    if (argc < 5) return 2;
    Camera camera(gi::dvec3(10, 5, 0), gi::dvec3(0, 0, 0));
    RayTracer raytracer(camera);
    Octree* scene = new Octree();
    loadScene(scene, raytracer, argv[1]);
    raytracer.setScene(scene);
    scene->rebuild();
    RayTracer::Features f;
    if (!raytracer.renderFeatures(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), f)) { printf("failed: %s\n", raytracer.last_error().c_str()); return 1; }
    double a = 0, n = 0, d = 0, c = 0;
    long long e = 0, m = 0;
    for (double v : f.albedo) a += v;
    for (double v : f.normal) n += v;
    for (double v : f.depth) d += v;
    for (double v : f.coverage) c += v;
    for (int32_t v : f.entity) e += v < 0;     // misses (the entity numbering is the C++ Octree's own: Octree::entities())
    for (int32_t v : f.material) m += v < 0;
    printf("features %dx%d n %d sizes %zu %zu %zu %zu %zu %zu\n", f.width, f.height, f.samples, f.albedo.size(), f.normal.size(), f.depth.size(), f.coverage.size(),
           f.entity.size(), f.material.size());
    printf("sums %.17g %.17g %.17g %.17g %lld %lld\n", a, n, d, c, e, m);
    RayTracer::Features bad;
    printf("n=0 ok %d\n", (int)raytracer.renderFeatures(16, 16, 0, bad));
    return 0;
}
