// tests/cpp/test_upsample.cpp -- RayTracer::upsample (an addition to the drop-in class): argv[1] = width, argv[2] = height, argv[3] = factor,
// argv[4] = a file that gets the raw doubles of the low colour, the low features [hl][wl][8], the full features [h][w][8] and the result, in this
// order.  The buffers are built from an integer hash (two surfaces with orthogonal normals), so the test needs no scene: the upsampler needs none.
#include <cstdio>
#include <cstdlib>
#include "../../include/gi/builtin_loaders.h"

static double hash01(uint32_t i) { return (double)(((i * 2654435761u) >> 8) & 0xffffu) / 65536.0; }

static RayTracer::Features features(int w, int h, uint32_t salt)
{
    RayTracer::Features f;
    f.width = w; f.height = h; f.samples = 1;
    const size_t npix = (size_t)w * h;
    f.albedo.resize(npix * 3); f.normal.assign(npix * 3, 0.0); f.depth.resize(npix); f.coverage.assign(npix, 1.0);
    f.entity.assign(npix, 0); f.material.assign(npix, 0);
    for (size_t i = 0; i < npix; i++) {
        for (int k = 0; k < 3; k++) f.albedo[i * 3 + k] = 0.25 + 0.5 * hash01((uint32_t)(i * 3 + k) + salt);
        f.normal[i * 3 + ((int)(i % w) * 2 < w ? 1 : 0)] = 1.0;
        f.depth[i] = 4.0 + 0.01 * (double)(i / w);
    }
    return f;
}

int main(int argc, char** argv)
{
    if (argc < 5) return 2;
    const int w = atoi(argv[1]), h = atoi(argv[2]), S = atoi(argv[3]);
    const int wl = (w + S - 1) / S, hl = (h + S - 1) / S;
    Camera camera(gi::dvec3(10, 5, 0), gi::dvec3(0, 0, 0));
    RayTracer raytracer(camera);
    const RayTracer::Features low = features(wl, hl, 7u), full = features(w, h, 1u);
    std::vector<double> color((size_t)wl * hl * 3), out, keep(3, 7.0);
    for (size_t i = 0; i < color.size(); i++) color[i] = 2.0 * hash01((uint32_t)i + 99u);
    if (!raytracer.upsample(color, low, full, S, out)) { printf("failed: %s\n", raytracer.last_error().c_str()); return 1; }
    printf("upsample %dx%d from %dx%d size %zu\n", w, h, wl, hl, out.size());
    FILE* fp = fopen(argv[4], "wb");
    if (!fp) return 3;
    std::vector<double> lbuf, fbuf;
    RayTracer::pack_features(low, lbuf); RayTracer::pack_features(full, fbuf);
    lbuf.resize((size_t)wl * hl * 8); fbuf.resize((size_t)w * h * 8);
    for (const std::vector<double>* v : {&color, &lbuf, &fbuf, &out}) fwrite(v->data(), sizeof(double), v->size(), fp);
    fclose(fp);
    gi_upsample_params p;
    gi_upsample_default_params(&p);
    p.sigma_depth = -1.0;
    printf("sigma_depth=-1 ok %d kept %d\n", (int)raytracer.upsample(color, low, full, S, keep, &p), (int)(keep.size() == 3 && keep[0] == 7.0));
    printf("factor+1 ok %d kept %d\n", (int)raytracer.upsample(color, low, full, S + 1, keep), (int)(keep.size() == 3 && keep[0] == 7.0));
    color.pop_back();
    printf("short colour ok %d\n", (int)raytracer.upsample(color, low, full, S, keep));
    return 0;
}
