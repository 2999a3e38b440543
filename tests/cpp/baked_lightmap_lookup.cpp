// tests/cpp/baked_lightmap_lookup.cpp -- the per-lane functions of the baked-light pass's lightmap look-up (gi_baked.h: lm_coord, lm_bilinear,
// lm_nearest) compiled for the host the way tests/cpp/baked_lookup.cpp compiles the grid's, as a program of its own (tests/test_baked_lightmap_cpu.py
// builds and runs it, once plainly and once under the address and undefined-behaviour sanitizers, and compares its output with
// tests/baked_lightmap_expect.py bit for bit).  TEST INFRASTRUCTURE ONLY.
//
//   baked_lightmap_lookup coord IN OUT          IN: records of 18 doubles, p0 e1v e2v P (3 each) and the chart row uv [3][2]; OUT: u v per record
//   baked_lightmap_lookup filter W H ATLAS UV OUT   ATLAS: W * H * 3 doubles, exactly; UV: pairs u v; OUT: per pair bilinear rgb, nearest rgb
// Files are raw little-endian doubles, so every bit passes both ways.  The atlas is held in a vector of exactly its size: an index past it is the
// sanitizer's to find.
#include <cstdio>
#include <cstdlib>
#define GI_HD static inline
#define GI_HDM inline
#include "../../gi_raytracer_amd/csrc/gi_layout.h"

namespace gi {
#include "../../gi_raytracer_amd/csrc/gi_cubemap.h"
#include "../../gi_raytracer_amd/csrc/gi_baked.h"
}

using namespace gi;

static std::vector<double> read_all(const char* path)
{
    std::vector<double> v;
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "baked_lightmap_lookup: cannot read %s\n", path); exit(2); }
    double buf[4096];
    size_t n;
    while ((n = fread(buf, sizeof(double), 4096, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

static int write_all(const char* path, const std::vector<double>& v)
{
    FILE* f = fopen(path, "wb");
    if (!f) return 2;
    const size_t n = fwrite(v.data(), sizeof(double), v.size(), f);
    return fclose(f) == 0 && n == v.size() ? 0 : 2;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string what = argv[1];
    if (what == "coord" && argc == 4) {
        const std::vector<double> in = read_all(argv[2]);
        if (in.size() % 18) return 2;
        std::vector<double> out;
        for (size_t i = 0; i < in.size(); i += 18) {
            TriGeom g{};
            for (int k = 0; k < 3; k++) { g.p0[k] = in[i + k]; g.e1[k] = in[i + 3 + k]; g.e2[k] = in[i + 6 + k]; }
            const LmCoord c = lm_coord(g, ld3(&in[i + 9]), &in[i + 12]);
            out.push_back(c.u); out.push_back(c.v);
        }
        return write_all(argv[3], out);
    }
    if (what == "filter" && argc == 7) {
        const int32_t w = atoi(argv[2]), h = atoi(argv[3]);
        const std::vector<double> atlas = read_all(argv[4]), uv = read_all(argv[5]);
        if (w < 1 || h < 1 || atlas.size() != (size_t)w * (size_t)h * 3 || uv.size() % 2) return 2;
        std::vector<double> out;
        for (size_t i = 0; i < uv.size(); i += 2) {
            LmCoord c;
            c.u = uv[i]; c.v = uv[i + 1];
            const V3 b = lm_bilinear(atlas.data(), w, h, c), n = lm_nearest(atlas.data(), w, h, c);
            for (double x : {b.x, b.y, b.z, n.x, n.y, n.z}) out.push_back(x);
        }
        return write_all(argv[6], out);
    }
    fprintf(stderr, "baked_lightmap_lookup: coord IN OUT | filter W H ATLAS UV OUT\n");
    return 2;
}
