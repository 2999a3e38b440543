// tests/cpp/reflections_lookup.cpp -- the per-lane functions of a reflection probe set (gi_reflections.h: rs_contains, rs_edge, rs_weight,
// rs_exit, rs_direction, rs_nearest, rs_specular) compiled for the host the way tests/cpp/visibility_lookup.cpp compiles gi_visibility.h, as a
// program of its own (tests/test_reflections_cpu.py builds and runs it, once plainly and once under the address and undefined-behaviour
// sanitizers, and compares its output with tests/reflections_expect.py bit for bit).  TEST INFRASTRUCTURE ONLY.
//
//   reflections_lookup lookup FILE      FILE holds, as whitespace-separated numbers: K, face, levels, n; then probes [K][10], chains
//                                       [K][texels][3], then n rows P xyz, R xyz, level.  Per row: S.  Both tables are exactly as large as
//                                       K, face and levels say: an index past one is the sanitizer's
//   reflections_lookup edges            P, R and table entries that are NaN, infinite, zero or huge against sets of 1 and 64 probes: every index
//                                       checked under the sanitizers, every S one of the chains' values
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
#include "../../gi_raytracer_amd/csrc/gi_reflections.h"
}

using namespace gi;

static size_t texels_before(int face, int l)
{
    size_t t = 0;
    for (int k = 0; k < l; k++) t += (size_t)6 * (size_t)(face >> k) * (size_t)(face >> k);
    return t;
}

static int edges()
{
    int bad = 0;
    const double nan = NAN, inf = INFINITY;
    const double vals[] = {0.0, -0.0, 1.0, -1.0, 0.25, 1e300, -1e300, 5e-324, inf, -inf, nan};
    const int face = 4, levels = 3;
    const size_t texels = texels_before(face, levels);
    for (int K : {1, GI_REFLECTIONS_MAX_PROBES}) {
        std::vector<double> probes((size_t)K * GI_RS_ROW), chains((size_t)K * texels * 3);
        for (size_t i = 0; i < chains.size(); i++) chains[i] = 1.0 + (double)(i / 3);            // a texel's three channels name the texel
        for (int variant = 0; variant < 4; variant++) {
            for (int k = 0; k < K; k++) {
                double* pr = &probes[(size_t)k * GI_RS_ROW];
                const double c = 0.1 * k;
                pr[0] = c; pr[1] = -c; pr[2] = 0.5 * c;
                pr[3] = -1.0 - c; pr[4] = -1.0; pr[5] = -2.0; pr[6] = 1.0; pr[7] = 1.0 + c; pr[8] = 2.0;
                pr[9] = (k & 1) ? 0.5 : 0.0;
                if (variant == 1 && k == 0) { pr[0] = nan; pr[9] = nan; }                        // a table the device entry would not have looked at
                if (variant == 2) { pr[3] = -inf; pr[6] = inf; pr[1] = inf; }
                if (variant == 3) { pr[4] = nan; pr[8] = 1e308; pr[5] = -1e308; pr[9] = 5e-324; }
            }
            for (double px : vals)
                for (double pz : vals)
                    for (double rx : vals)
                        for (double ry : vals)
                            for (int l = 0; l < levels; l++) {
                                const V3 S = rs_specular(probes.data(), chains.data(), K, texels, (uint32_t)texels_before(face, l), (uint32_t)(face >> l), v3(px, 0.25, pz), v3(rx, ry, -0.5 * rx));
                                // whatever came in, S is a weighted mean of texel values, up to its roundings (or NaN where a weight is): never something read elsewhere
                                const double top = (double)(K * texels);
                                if (S.x == S.x && !(S.x >= 1.0 * (1.0 - 1e-12) && S.x <= top * (1.0 + 1e-12))) { printf("K %d variant %d P %g . %g R %g %g level %d: %a\n", K, variant, px, pz, rx, ry, l, S.x); bad++; }
                            }
        }
    }
    // the pieces at their ends
    const double pr[GI_RS_ROW] = {0.0, 0.0, 0.0, -1.0, -2.0, -3.0, 1.0, 2.0, 3.0, 0.5};
    if (!rs_contains(pr, v3(1.0, -2.0, 3.0)) || rs_contains(pr, v3(1.0000000000000002, 0, 0)) || rs_contains(pr, v3(nan, 0, 0)) || rs_contains(pr, v3(0, 0, -inf))) bad++;
    if (rs_edge(pr, v3(1.0, 0, 0)) != 0.0 || rs_edge(pr, v3(0.5, 0, 0)) != 0.5 || rs_edge(pr, v3(0, 0, 0)) != 1.0 || rs_edge(pr, v3(0, -1.75, 0)) != 0.25) bad++;
    if (rs_weight(0.5, 0.5) != 1.0 || rs_weight(0.25, 0.5) != 0.5 || rs_weight(0.0, 0.5) != 0.0 || rs_weight(0.0, 0.0) != 1.0 || rs_weight(3.0, 0.0) != 1.0 || rs_weight(1.0, nan) != 1.0) bad++;
    if (rs_exit(pr, v3(0, 0, 0), v3(0, 0, 0)) != 0.0 || rs_exit(pr, v3(0, 0, 0), v3(1, 0, 0)) != 1.0 || rs_exit(pr, v3(0, 0, 0), v3(-2, 0, 0)) != 0.5 ||
        rs_exit(pr, v3(0, 0, 0), v3(0, -1, 0)) != 2.0 || rs_exit(pr, v3(0, 0, 0), v3(1, 1, 1)) != 1.0 || rs_exit(pr, v3(0, 0, 0), v3(0, 4, 3)) != 0.5 || rs_exit(pr, v3(1, 0, 0), v3(1, 1, 0)) != 0.0) bad++;
    const V3 d0 = rs_direction(pr, v3(0, 0, 0), v3(0, 0, 0)), d1 = rs_direction(pr, v3(0.5, 0, 0), v3(0, 1, 0)), d2 = rs_direction(pr, v3(0, 0, 0), v3(inf, 1, 0));
    if (d0.x != 0.0 || d0.y != 0.0 || d0.z != 0.0 || d1.x != 0.5 || d1.y != 2.0 || d1.z != 0.0 || d2.x != inf || d2.y != 1.0) bad++;      // P = pos, t = 0: R; projected; not finite: R
    const double two[2 * GI_RS_ROW] = {1.0, 0, 0, 0, 0, 0, 1, 1, 1, 0, -1.0, 0, 0, 0, 0, 0, 1, 1, 1, 0};
    if (rs_nearest(two, 2, v3(0, 5, 0)) != 0 || rs_nearest(two, 2, v3(-0.5, 0, 0)) != 1 || rs_nearest(two, 2, v3(nan, 0, 0)) != 0 || rs_nearest(two, 2, v3(inf, 0, 0)) != 0) bad++;
    printf("edges: %d bad\n", bad);
    return bad ? 1 : 0;
}

static int lookup(const char* path)
{
    std::ifstream f(path);
    std::vector<double> v;
    std::string tok;
    while (f >> tok) v.push_back(strtod(tok.c_str(), nullptr));
    if (v.size() < 4) return 2;
    const int K = (int)v[0], face = (int)v[1], levels = (int)v[2];
    const size_t n = (size_t)v[3], texels = texels_before(face, levels);
    if (K < 1 || K > GI_REFLECTIONS_MAX_PROBES || v.size() != 4 + (size_t)K * GI_RS_ROW + (size_t)K * texels * 3 + n * 7) return 2;
    const std::vector<double> probes(v.begin() + 4, v.begin() + 4 + (size_t)K * GI_RS_ROW);      // copies of exactly the tables' sizes
    const std::vector<double> chains(v.begin() + 4 + probes.size(), v.begin() + 4 + probes.size() + (size_t)K * texels * 3);
    const double* row = v.data() + 4 + probes.size() + chains.size();
    for (size_t i = 0; i < n; i++, row += 7) {
        const int l = (int)row[6];
        if (l < 0 || l >= levels) return 2;
        const V3 S = rs_specular(probes.data(), chains.data(), K, texels, (uint32_t)texels_before(face, l), (uint32_t)(face >> l), v3(row[0], row[1], row[2]), v3(row[3], row[4], row[5]));
        printf("%a %a %a\n", S.x, S.y, S.z);
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string what = argv[1];
    if (what == "edges") return edges();
    if (what == "lookup" && argc == 3) return lookup(argv[2]);
    fprintf(stderr, "reflections_lookup: lookup | edges\n");
    return 2;
}
