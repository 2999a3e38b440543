// tests/cpp/cubemap_kat.cpp -- the per-lane functions of a reflection probe (gi_cubemap.h: cm_coord, cm_face_dir, cm_unit, cm_measure, cm_weight,
// cm_box) compiled for the host the way tests/host_emul compiles the device functions, as a program of its own (tests/test_cubemap_cpu.py builds
// and runs it, once plainly and once under the address and undefined-behaviour sanitizers, and compares its output with tests/cubemap_expect.py
// bit for bit).  TEST INFRASTRUCTURE ONLY.
//
//   cubemap_kat dirs N JU JV        per texel of a cube of face N: the unnormalised direction, the unit direction and the measure at that jitter
//   cubemap_kat weights N_OUT N_SRC E   per output texel centre of face N_OUT and source texel centre of face N_SRC: the lobe weight squared E times
//   cubemap_kat box V...            per four values p00 p01 p10 p11: the box mean
// Doubles are read with strtod, so hexadecimal floats pass exactly, and printed as hexadecimal floats.
#include <cstdio>
#include <cstdlib>
#define GI_HD static inline
#define GI_HDM inline
#include "../../gi_raytracer_amd/csrc/gi_layout.h"

namespace gi {
#include "../../gi_raytracer_amd/csrc/gi_cubemap.h"
}

using namespace gi;

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string what = argv[1];
    if (what == "dirs" && argc == 5) {
        const uint32_t n = (uint32_t)strtoul(argv[2], nullptr, 0);
        const double ju = strtod(argv[3], nullptr), jv = strtod(argv[4], nullptr);
        for (uint32_t t = 0; t < 6u * n * n; t++) {
            const CmTexel q = cm_texel(t, n);
            const double a = cm_coord(q.x, ju, n), b = cm_coord(q.y, jv, n);
            const V3 u = cm_face_dir(q.f, a, b), d = cm_unit(u);
            printf("%a %a %a %a %a %a %a\n", u.x, u.y, u.z, d.x, d.y, d.z, cm_measure(a, b));
        }
        return 0;
    }
    if (what == "weights" && argc == 5) {
        const uint32_t n = (uint32_t)strtoul(argv[2], nullptr, 0), ns = (uint32_t)strtoul(argv[3], nullptr, 0);
        const int e = atoi(argv[4]);
        for (uint32_t o = 0; o < 6u * n * n; o++) {
            const V3 R = cm_centre_dir(o, n);
            for (uint32_t s = 0; s < 6u * ns * ns; s++) {
                const CmTexel q = cm_texel(s, ns);
                const double a = cm_coord(q.x, 0.5, ns), b = cm_coord(q.y, 0.5, ns);
                printf("%a\n", cm_weight(R, cm_unit(cm_face_dir(q.f, a, b)), cm_measure(a, b), e));
            }
        }
        return 0;
    }
    if (what == "box" && argc >= 6 && (argc - 2) % 4 == 0) {
        for (int i = 2; i + 3 < argc; i += 4)
            printf("%a\n", cm_box(strtod(argv[i], nullptr), strtod(argv[i + 1], nullptr), strtod(argv[i + 2], nullptr), strtod(argv[i + 3], nullptr)));
        return 0;
    }
    fprintf(stderr, "cubemap_kat: dirs N JU JV | weights N_OUT N_SRC E | box V...\n");
    return 2;
}
