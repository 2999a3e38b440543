// tests/cpp/visibility_lookup.cpp -- the per-lane functions of probe visibility (gi_visibility.h: octa_decode, octa_encode, the fold's sums,
// pv_bilinear, pv_irradiance) compiled for the host the way tests/cpp/baked_lookup.cpp compiles gi_baked.h, as a program of its own
// (tests/test_visibility_cpu.py builds and runs it, once plainly and once under the address and undefined-behaviour sanitizers, and compares its
// output with tests/visibility_expect.py bit for bit).  TEST INFRASTRUCTURE ONLY.
//
//   visibility_lookup decode A B ...            per pair: vx vy vz
//   visibility_lookup encode X Y Z ...          per vector: a b
//   visibility_lookup fold N R...               per N distances: m m2
//   visibility_lookup lookup FILE               FILE holds, as whitespace-separated numbers: nx ny nz, box (min xyz, max xyz), M, normal_bias,
//                                               vis_floor, n; then sh [nz][ny][nx][9][3], vis [nz][ny][nx][M][M][2], then n rows P xyz, Nf xyz.
//                                               Per row: D.  Both tables are exactly as large as the grid says: an index past one is the sanitizer's
//   visibility_lookup edges                     the edge inputs: axis directions, zero components of either sign, texel centres and map corners
//                                               there and back, maps of one texel, hits on a probe; every index checked under the sanitizers
// Doubles are read with strtod, so hexadecimal floats pass exactly, and printed as hexadecimal floats.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#define GI_HD static inline
#define GI_HDM inline
#include "../../gi_raytracer_amd/csrc/gi_layout.h"

namespace gi {
#include "../../gi_raytracer_amd/csrc/gi_cubemap.h"
#include "../../gi_raytracer_amd/csrc/gi_baked.h"
#include "../../gi_raytracer_amd/csrc/gi_visibility.h"
}

using namespace gi;

static int edges()
{
    int bad = 0;
    // every direction with components in {-1, -0, 0, 1} but 0 0 0: (a, b) inside the square, and decode(encode(v)) parallel to v
    for (double x : {-1.0, 0.0, 1.0, -0.0})
        for (double y : {-1.0, 0.0, 1.0, -0.0})
            for (double z : {-1.0, 0.0, 1.0, -0.0}) {
                if (x == 0.0 && y == 0.0 && z == 0.0) continue;
                const OctaUV c = octa_encode(v3(x, y, z));
                if (!(c.a >= 0.0 && c.a <= 1.0 && c.b >= 0.0 && c.b <= 1.0)) { printf("encode %g %g %g: %a %a\n", x, y, z, c.a, c.b); bad++; continue; }
                const V3 d = octa_decode(c.a, c.b);
                const double s = (fabs(x) + fabs(y)) + fabs(z);
                if (fabs(d.x * s - x) > 1e-15 || fabs(d.y * s - y) > 1e-15 || fabs(d.z * s - z) > 1e-15) { printf("round trip %g %g %g: %a %a %a\n", x, y, z, d.x, d.y, d.z); bad++; }
            }
    // texel centres and the square's corners and edge middles, there and back: the same point of the square (the corners all mean -z: any of them)
    for (int M : {1, 2, 3, 8, 64})
        for (int y = 0; y < M; y++)
            for (int x = 0; x < M; x++) {
                const double a = ((double)x + 0.5) / (double)M, b = ((double)y + 0.5) / (double)M;
                const OctaUV c = octa_encode(octa_decode(a, b));
                if (fabs(c.a - a) > 1e-15 || fabs(c.b - b) > 1e-15) { printf("centre M %d (%d, %d): %a %a\n", M, x, y, c.a, c.b); bad++; }
            }
    for (double a : {0.0, 0.5, 1.0})
        for (double b : {0.0, 0.5, 1.0}) {
            const V3 d = octa_decode(a, b);
            if ((fabs(d.x) + fabs(d.y)) + fabs(d.z) != 1.0) { printf("decode %g %g: not on the octahedron\n", a, b); bad++; }
        }
    // maps of exactly M x M texels read at the square's border, beyond it and at a NaN: the sanitizer sees any index past the table
    for (int M : {1, 2, 5}) {
        std::vector<double> map((size_t)M * M * 2);
        for (size_t i = 0; i < map.size(); i++) map[i] = 1.0 + (double)i;
        for (double a : {0.0, 1.0, -3.0, 4.0, 0.5, (double)NAN})
            for (double b : {0.0, 1.0, -3.0, 4.0, 0.5, (double)NAN}) {
                OctaUV c; c.a = a; c.b = b;
                const PvMoments q = pv_bilinear(map.data(), M, c);
                if (!(q.m >= 1.0 && q.m <= (double)map.size() && q.m2 >= 2.0 && q.m2 <= (double)map.size())) { printf("bilinear M %d at %g %g: %a %a\n", M, a, b, q.m, q.m2); bad++; }
            }
    }
    // the Chebyshev weight at its ends
    PvMoments q;
    q.m = 2.0; q.m2 = 4.0;
    if (pv_chebyshev(2.0, q, 0.05) != 1.0 || pv_chebyshev(1.0, q, 0.05) != 1.0 || pv_chebyshev(3.0, q, 0.05) != 0.05) bad++;      // r == m, r < m, no variance
    q.m = 0.0; q.m2 = 0.0;
    if (pv_chebyshev(1.0, q, 0.25) != 0.25) bad++;
    q.m = 2.0; q.m2 = 5.0;                                                                                                       // var 1, dd 1: (1 / 2)^3
    if (pv_chebyshev(3.0, q, 0.05) != 0.125 || pv_chebyshev(3.0, q, 1.0) != 1.0) bad++;
    // a hit on a probe: le == 0 and, without a bias, r == 0
    const std::vector<double> one = {1.0, 1.0};
    if (pv_backface(v3(1, 2, 3), v3(0, 1, 0), v3(1, 2, 3)) != 1.2 || pv_visibility(one.data(), 1, v3(1, 2, 3), v3(0, 1, 0), v3(1, 2, 3), 0.0, 0.05) != 1.0) bad++;
    printf("edges: %d bad\n", bad);
    return bad ? 1 : 0;
}

static int lookup(const char* path)
{
    std::ifstream f(path);
    std::vector<double> v;
    std::string tok;
    while (f >> tok) v.push_back(strtod(tok.c_str(), nullptr));
    if (v.size() < 13) return 2;
    const int32_t n3[3] = {(int32_t)v[0], (int32_t)v[1], (int32_t)v[2]};
    const double gmin[3] = {v[3], v[4], v[5]}, gmax[3] = {v[6], v[7], v[8]};
    const int32_t M = (int32_t)v[9];
    const double bias = v[10], floor = v[11];
    const size_t n = (size_t)v[12], n_probe = (size_t)n3[0] * n3[1] * n3[2];
    if (v.size() != 13 + n_probe * 27 + n_probe * (size_t)M * M * 2 + n * 6) return 2;
    const std::vector<double> sh(v.begin() + 13, v.begin() + 13 + n_probe * 27);            // copies of exactly the tables' sizes
    const std::vector<double> vis(v.begin() + 13 + n_probe * 27, v.begin() + 13 + n_probe * 27 + n_probe * (size_t)M * M * 2);
    const double* row = v.data() + 13 + sh.size() + vis.size();
    for (size_t i = 0; i < n; i++, row += 6) {
        const V3 d = pv_irradiance(sh.data(), vis.data(), M, n3, gmin, gmax, v3(row[0], row[1], row[2]), v3(row[3], row[4], row[5]), bias, floor);
        printf("%a %a %a\n", d.x, d.y, d.z);
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string what = argv[1];
    if (what == "edges") return edges();
    if (what == "lookup" && argc == 3) return lookup(argv[2]);
    if (what == "decode" && (argc - 2) % 2 == 0) {
        for (int i = 2; i + 1 < argc; i += 2) {
            const V3 d = octa_decode(strtod(argv[i], nullptr), strtod(argv[i + 1], nullptr));
            printf("%a %a %a\n", d.x, d.y, d.z);
        }
        return 0;
    }
    if (what == "encode" && (argc - 2) % 3 == 0) {
        for (int i = 2; i + 2 < argc; i += 3) {
            const OctaUV c = octa_encode(v3(strtod(argv[i], nullptr), strtod(argv[i + 1], nullptr), strtod(argv[i + 2], nullptr)));
            printf("%a %a\n", c.a, c.b);
        }
        return 0;
    }
    if (what == "fold" && argc >= 4) {
        const int n = atoi(argv[2]);
        if (n < 1 || (argc - 3) % n) return 2;
        for (int i = 3; i < argc; i += n) {
            PvSums s = {0.0, 0.0};
            for (int k = 0; k < n; k++) pv_add(s, strtod(argv[i + k], nullptr));
            const PvMoments q = pv_moments(s, (double)n);
            printf("%a %a\n", q.m, q.m2);
        }
        return 0;
    }
    fprintf(stderr, "visibility_lookup: decode | encode | fold | lookup | edges\n");
    return 2;
}
