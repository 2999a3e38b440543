// tests/cpp/baked_lookup.cpp -- the per-lane functions of the baked-light pass (gi_baked.h: grid_cell, sh9_factor, grid_irradiance, cube_texel, and
// the host's baked_level_of) compiled for the host the way tests/host_emul compiles the device functions, as a program of its own
// (tests/test_baked_cpu.py builds and runs it, once plainly and once under the address and undefined-behaviour sanitizers, and compares its output
// with tests/baked_expect.py bit for bit).  TEST INFRASTRUCTURE ONLY.
//
//   baked_lookup cell GMIN GMAX N P...                   per P: i0 i1 t of one axis
//   baked_lookup factor X Y Z ...                        per normal: the nine factors
//   baked_lookup texel N X Y Z ...                       per direction: its texel of a cube of face N
//   baked_lookup level LEVELS E0 .. E(LEVELS-1) R...     per roughness: the level of the chain it reads
//   baked_lookup grid NX NY NZ BOX6 SEED  X Y Z NX NY NZ ...   per point and normal: D of a grid filled from a small generator (see fill)
//   baked_lookup edges                                   the edge inputs: points on grid_min and grid_max, n = 1 axes, cube edges and corners, zero
//                                                        components; every index is checked against its table here, under the sanitizers
// Doubles are read with strtod, so hexadecimal floats pass exactly, and printed as hexadecimal floats.
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

// sh [nz][ny][nx][9][3], exactly that many values: entry i = ((i * 2654435761 + seed) mod 2^32) / 2^32 * 1.25 - 0.25, every step exact in f64
static std::vector<double> fill(size_t n, uint32_t seed)
{
    std::vector<double> v(n);
    for (size_t i = 0; i < n; i++) v[i] = (double)(uint32_t)((uint32_t)i * 2654435761u + seed) / 4294967296.0 * 1.25 - 0.25;
    return v;
}

static int edges()
{
    int bad = 0;
    // points exactly on grid_min and grid_max, just outside, and n = 1 axes
    for (int32_t n : {1, 2, 3, 7}) {
        for (double p : {-1.0, -1.0000000000000002, 3.0, 3.0000000000000004, 1.0, -1e300, 1e300}) {
            const GridCell c = grid_cell(p, -1.0, 3.0, n);
            if (c.i0 < 0 || c.i0 > n - 1 || c.i1 < c.i0 || c.i1 > n - 1 || !(c.t >= 0.0 && c.t < 1.0)) { printf("cell n %d p %a: %d %d %a\n", n, p, c.i0, c.i1, c.t); bad++; }
            if (n == 1 && (c.i0 != 0 || c.i1 != 0 || c.t != 0.0)) bad++;
        }
        const GridCell lo = grid_cell(-1.0, -1.0, 3.0, n), hi = grid_cell(3.0, -1.0, 3.0, n);
        if (lo.i0 != 0 || lo.t != 0.0 || hi.i0 != n - 1 || hi.i1 != n - 1 || hi.t != 0.0) bad++;
    }
    // a grid of exactly 1 x 2 x 3 probes, read at the corners of its box and beyond: the sanitizer sees any index past the table
    const int32_t n3[3] = {1, 2, 3};
    const double gmin[3] = {0.0, -2.0, 1.0}, gmax[3] = {1.0, 2.0, 4.0};
    const std::vector<double> sh = fill((size_t)n3[0] * n3[1] * n3[2] * 27, 7u);
    for (double x : {0.0, 1.0, -5.0, 5.0})
        for (double y : {-2.0, 2.0, 0.0})
            for (double z : {1.0, 4.0, 9.0}) {
                const V3 d = grid_irradiance(sh.data(), n3, gmin, gmax, v3(x, y, z), v3(0.0, 1.0, 0.0));
                if (!(d.x >= 0.0 && d.y >= 0.0 && d.z >= 0.0)) bad++;
            }
    // directions on cube edges and corners, with zero components, of every sign: the texel must be one of the cube's, and that of the first largest axis
    for (uint32_t n : {1u, 2u, 5u, 8u}) {
        std::vector<int> seen(6u * n * n, 0);      // exactly the cube: an index past it is the sanitizer's to find
        for (double x : {-1.0, 0.0, 1.0, -0.0})
            for (double y : {-1.0, 0.0, 1.0, -0.0})
                for (double z : {-1.0, 0.0, 1.0, -0.0}) {
                    if (x == 0.0 && y == 0.0 && z == 0.0) continue;
                    const uint32_t t = cube_texel(v3(x, y, z), n);
                    seen[t]++;
                    const uint32_t f = t / (n * n);
                    const uint32_t want = x != 0.0 ? (x < 0 ? 1u : 0u) : (y != 0.0 ? (y < 0 ? 3u : 2u) : (z < 0 ? 5u : 4u));
                    if (f != want) { printf("texel n %u of %g %g %g: face %u, not %u\n", n, x, y, z, f, want); bad++; }
                }
        // the centre of every texel falls into that texel
        for (uint32_t t = 0; t < 6u * n * n; t++)
            if (cube_texel(cm_centre_dir(t, n), n) != t) { printf("texel n %u: the centre of %u falls into %u\n", n, t, cube_texel(cm_centre_dir(t, n), n)); bad++; }
    }
    // the level table at its ends: one level, two levels, a mirror, a roughness of 0 and of 1
    const int32_t e[4] = {0, 9, 4, 1};
    if (baked_level_of(0.5, 1, e) != 0 || baked_level_of(0.5, 2, e) != 1 || baked_level_of(0.0005, 4, e) != 0 || baked_level_of(0.0, 4, e) != 0) bad++;
    if (baked_level_of(1.0, 4, e) != 3 || baked_level_of(0.002, 4, e) != 1) bad++;      // log2(2) = 1 -> e = 1; log2(501) = 8.97 -> e = 9
    printf("edges: %d bad\n", bad);
    return bad ? 1 : 0;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string what = argv[1];
    if (what == "edges") return edges();
    if (what == "cell" && argc >= 5) {
        const double gmin = strtod(argv[2], nullptr), gmax = strtod(argv[3], nullptr);
        const int32_t n = atoi(argv[4]);
        for (int i = 5; i < argc; i++) {
            const GridCell c = grid_cell(strtod(argv[i], nullptr), gmin, gmax, n);
            printf("%a %a %a\n", (double)c.i0, (double)c.i1, c.t);
        }
        return 0;
    }
    if (what == "factor" && (argc - 2) % 3 == 0) {
        for (int i = 2; i + 2 < argc; i += 3) {
            double F[9];
            sh9_factor(v3(strtod(argv[i], nullptr), strtod(argv[i + 1], nullptr), strtod(argv[i + 2], nullptr)), F);
            for (int j = 0; j < 9; j++) printf("%a%c", F[j], j == 8 ? '\n' : ' ');
        }
        return 0;
    }
    if (what == "texel" && argc >= 3 && (argc - 3) % 3 == 0) {
        const uint32_t n = (uint32_t)strtoul(argv[2], nullptr, 0);
        for (int i = 3; i + 2 < argc; i += 3)
            printf("%a\n", (double)cube_texel(v3(strtod(argv[i], nullptr), strtod(argv[i + 1], nullptr), strtod(argv[i + 2], nullptr)), n));
        return 0;
    }
    if (what == "level" && argc >= 3) {
        const int32_t levels = atoi(argv[2]);
        if (levels < 1 || levels > GI_CUBEMAP_MAX_LEVELS || argc < 3 + levels) return 2;
        int32_t e[GI_CUBEMAP_MAX_LEVELS] = {0};
        for (int l = 0; l < levels; l++) e[l] = atoi(argv[3 + l]);
        for (int i = 3 + levels; i < argc; i++) printf("%a\n", (double)baked_level_of(strtod(argv[i], nullptr), levels, e));
        return 0;
    }
    if (what == "grid" && argc >= 12 && (argc - 12) % 6 == 0) {
        const int32_t n3[3] = {atoi(argv[2]), atoi(argv[3]), atoi(argv[4])};
        double gmin[3], gmax[3];
        for (int k = 0; k < 3; k++) { gmin[k] = strtod(argv[5 + k], nullptr); gmax[k] = strtod(argv[8 + k], nullptr); }
        const std::vector<double> sh = fill((size_t)n3[0] * n3[1] * n3[2] * 27, (uint32_t)strtoul(argv[11], nullptr, 0));
        for (int i = 12; i + 5 < argc; i += 6) {
            const V3 P = v3(strtod(argv[i], nullptr), strtod(argv[i + 1], nullptr), strtod(argv[i + 2], nullptr));
            const V3 N = v3(strtod(argv[i + 3], nullptr), strtod(argv[i + 4], nullptr), strtod(argv[i + 5], nullptr));
            const V3 d = grid_irradiance(sh.data(), n3, gmin, gmax, P, N);
            printf("%a %a %a\n", d.x, d.y, d.z);
        }
        return 0;
    }
    fprintf(stderr, "baked_lookup: cell | factor | texel | level | grid | edges\n");
    return 2;
}
