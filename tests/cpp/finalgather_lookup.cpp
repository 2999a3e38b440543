// tests/cpp/finalgather_lookup.cpp -- the walk-free per-lane functions of the final-gather pass (gi_finalgather.h: fg_secondary, fg_add, fg_mean,
// fg_diffuse, fg_id) compiled for the host the way tests/cpp/reflections_lookup.cpp compiles gi_reflections.h, as a program of its own
// (tests/test_finalgather_cpu.py builds and runs it, once plainly and once under the address and undefined-behaviour sanitizers, and compares its
// output with tests/finalgather_expect.py bit for bit).  TEST INFRASTRUCTURE ONLY.
//
//   finalgather_lookup lookup FILE     FILE holds, as whitespace-separated numbers: nx, ny, nz, the grid box (min xyz, max xyz), face, levels (0: no
//                                      chain), n_mat, n; then sh [nz][ny][nx][9][3], the chain [texels][3], level_of_mat [n_mat], then n rows
//                                      Q xyz, Nf xyz, color rgb, emissive rgb, roughness, material, d xyz, i rgb.  Per row: L.  Every table is exactly
//                                      as large as the head says: an index past one is the sanitizer's
//   finalgather_lookup fold FILE       FILE holds n_dirs, color rgb, then n_dirs rows L rgb.  Prints fg_diffuse of the fold in ascending j
//   finalgather_lookup edges           the ids codes, and NaN / infinite / huge Q, normals and directions against a small grid and chain
// Doubles are read with strtod, so hexadecimal floats pass exactly, and printed as hexadecimal floats.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>
#define GI_HD static inline
#define GI_HDM inline
#include "../../gi_raytracer_amd/csrc/gi_layout.h"

namespace gi {
#include "../../gi_raytracer_amd/csrc/gi_cubemap.h"
#include "../../gi_raytracer_amd/csrc/gi_baked.h"
#include "../../gi_raytracer_amd/csrc/gi_finalgather.h"
}

using namespace gi;

static size_t texels_before(int face, int l)
{
    size_t t = 0;
    for (int k = 0; k < l; k++) t += (size_t)6 * (size_t)(face >> k) * (size_t)(face >> k);
    return t;
}

struct Tables {
    int32_t n3[3];
    double gmin[3], gmax[3];
    std::vector<double> sh, chain;
    std::vector<int32_t> level_of_mat;
    std::vector<uint32_t> level_off;
    int face = 0, levels = 0;
    FgLook look() const
    {
        FgLook K;
        K.sh = sh.data(); K.n3 = n3; K.gmin = gmin; K.gmax = gmax;
        K.chain = levels ? chain.data() : nullptr; K.level_of_mat = level_of_mat.data(); K.face = (uint32_t)face; K.level_off = level_off.data();
        return K;
    }
};

static std::vector<double> numbers(const char* path)
{
    std::ifstream f(path);
    std::vector<double> v;
    std::string tok;
    while (f >> tok) v.push_back(strtod(tok.c_str(), nullptr));
    return v;
}

static int lookup(const char* path)
{
    const std::vector<double> v = numbers(path);
    if (v.size() < 13) return 2;
    Tables T;
    for (int k = 0; k < 3; k++) { T.n3[k] = (int32_t)v[k]; T.gmin[k] = v[3 + k]; T.gmax[k] = v[6 + k]; }
    T.face = (int)v[9]; T.levels = (int)v[10];
    const size_t n_mat = (size_t)v[11], n = (size_t)v[12];
    const size_t n_sh = (size_t)T.n3[0] * (size_t)T.n3[1] * (size_t)T.n3[2] * 27, n_chain = texels_before(T.face, T.levels) * 3;
    if (T.n3[0] < 1 || T.n3[1] < 1 || T.n3[2] < 1 || v.size() != 13 + n_sh + n_chain + n_mat + n * 20) return 2;
    const double* q = v.data() + 13;
    T.sh.assign(q, q + n_sh); q += n_sh;                                  // copies of exactly the tables' sizes
    T.chain.assign(q, q + n_chain); q += n_chain;
    for (size_t m = 0; m < n_mat; m++) T.level_of_mat.push_back((int32_t)q[m]);
    q += n_mat;
    for (int l = 0; l < T.levels; l++) T.level_off.push_back((uint32_t)texels_before(T.face, l));
    const FgLook K = T.look();
    for (size_t i = 0; i < n; i++, q += 20) {
        FgHit h;
        h.Q = ld3(q); h.nf = ld3(q + 3); h.color = ld3(q + 6); h.emissive = ld3(q + 9); h.roughness = q[12]; h.mat = (int32_t)q[13];
        if (h.mat < 0 || (size_t)h.mat >= n_mat) return 2;
        const V3 L = fg_secondary(K, h, ld3(q + 14), ld3(q + 17));
        printf("%a %a %a\n", L.x, L.y, L.z);
    }
    return 0;
}

static int fold(const char* path)
{
    const std::vector<double> v = numbers(path);
    if (v.size() < 4) return 2;
    const int32_t n_dirs = (int32_t)v[0];
    if (n_dirs < 1 || n_dirs > GI_FG_MAX_DIRS || v.size() != 4 + (size_t)n_dirs * 3) return 2;
    V3 acc = v3(0, 0, 0);
    for (int32_t j = 0; j < n_dirs; j++) acc = fg_add(acc, ld3(v.data() + 4 + (size_t)j * 3));
    const V3 d = fg_diffuse(ld3(v.data() + 1), acc, n_dirs);
    printf("%a %a %a\n", d.x, d.y, d.z);
    return 0;
}

static int edges()
{
    int bad = 0;
    if (fg_id(false, 7) != -1 || fg_id(true, 7) != 7 || fg_id(true, 0) != 0 || GI_FG_ID_NONE != -2 || GI_FG_ID_MISS != -1) bad++;
    const double nan = NAN, inf = INFINITY;
    const double vals[] = {0.0, -0.0, 1.0, -1.0, 0.25, 1e300, -1e300, 5e-324, inf, -inf, nan};
    for (int levels : {0, 3}) {
        Tables T;
        T.n3[0] = 2; T.n3[1] = 1; T.n3[2] = 3;
        for (int k = 0; k < 3; k++) { T.gmin[k] = -1.0; T.gmax[k] = 1.0; }
        T.sh.assign((size_t)6 * 27, 0.0);
        for (size_t p = 0; p < 6; p++) for (int ch = 0; ch < 3; ch++) T.sh[p * 27 + ch] = 1.0 + (double)p;      // band 0 only: D = 0.282 (1 + probe), whatever the normal
        T.face = 4; T.levels = levels;
        T.chain.assign(texels_before(4, levels) * 3, 2.0);
        T.level_of_mat = {0, 1, 2};
        for (int l = 0; l < levels; l++) T.level_off.push_back((uint32_t)texels_before(4, l));
        const FgLook K = T.look();
        for (double qx : vals)
            for (double qz : vals)
                for (double nx : vals)
                    for (double dx : vals)
                        for (double rough : {1.0, 0.5, 0.0005, nan})
                            for (int mat = 0; mat < 3; mat++) {
                                FgHit h;
                                h.Q = v3(qx, 0.25, qz); h.nf = v3(nx, 0.0, 1.0); h.color = v3(1, 1, 1); h.emissive = v3(0, 0, 0); h.roughness = rough; h.mat = mat;
                                const V3 L = fg_secondary(K, h, v3(dx, -0.5, 0.25 * dx), v3(0, 0, 0));
                                // diffuse (a NaN roughness too): band 0 of a probe between 1 and 6, or NaN from a NaN normal; specular: 2 with a chain, 0 without, or NaN
                                const bool diffuse = !(rough < .9);
                                const double lo = diffuse ? 0.28 * 1.0 : (levels ? 2.0 : 0.0), hi = diffuse ? 0.29 * 6.0 : (levels ? 2.0 : 0.0);
                                if (L.x == L.x && !(L.x >= lo && L.x <= hi)) { printf("levels %d Q %g . %g n %g d %g rough %g mat %d: %a\n", levels, qx, qz, nx, dx, rough, mat, L.x); bad++; }
                            }
    }
    printf("edges: %d bad\n", bad);
    return bad ? 1 : 0;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string what = argv[1];
    if (what == "edges") return edges();
    if (what == "lookup" && argc == 3) return lookup(argv[2]);
    if (what == "fold" && argc == 3) return fold(argv[2]);
    fprintf(stderr, "finalgather_lookup: lookup FILE | fold FILE | edges\n");
    return 2;
}
