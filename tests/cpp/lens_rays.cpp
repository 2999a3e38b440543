// tests/cpp/lens_rays.cpp -- primary_ray_at (gi_path.h) under a thin lens, compiled for the host the way tests/host_emul compiles the device
// functions, as a program of its own (tests/test_lens_cpu.py builds and runs it, once plainly and once under the address and undefined-behaviour
// sanitizers, and compares its output with tests/lens_expect.py bit for bit).  TEST INFRASTRUCTURE ONLY.
//
//   lens_rays W H SEED RADIUS ROTATION BLADES  POS3 UP3 FORWARD3 SENSOR_DIAG FOCAL_DIST  IDX...
// Doubles are read with strtod, so hexadecimal floats ("0x1.8p+1") pass exactly; SEED and IDX are unsigned integers.  One line per index:
// the six doubles of the ray (origin, direction) as hexadecimal floats.
#include <cstdio>
#include <cstdlib>
#define GI_HD static inline
#define GI_HDM inline
#include "../../gi_raytracer_amd/csrc/gi_layout.h"

using namespace gi;

int main(int argc, char** argv)
{
    if (argc < 18) { fprintf(stderr, "lens_rays: 17 arguments and the indices expected\n"); return 2; }
    gi_render_params p;
    memset(&p, 0, sizeof p);
    p.width = atoi(argv[1]); p.height = atoi(argv[2]);
    p.seed = strtoull(argv[3], nullptr, 0);
    gi_lens lens;
    lens.radius = strtod(argv[4], nullptr); lens.rotation = strtod(argv[5], nullptr); lens.blades = atoi(argv[6]); lens.reserved = 0;
    for (int k = 0; k < 3; k++) { p.cam_pos[k] = strtod(argv[7 + k], nullptr); p.cam_up[k] = strtod(argv[10 + k], nullptr); p.cam_forward[k] = strtod(argv[13 + k], nullptr); }
    p.sensor_diag = strtod(argv[16], nullptr); p.focal_dist = strtod(argv[17], nullptr);
    p.stripe_h = p.height; p.stripe_rank = 0; p.stripe_world = 1; p.min_samples = p.max_samples = 1;
    Frame F;
    std::string err;
    if (!make_frame(&p, F, err)) { fprintf(stderr, "lens_rays: %s\n", err.c_str()); return 2; }
    if (!lens_valid(&lens)) { fprintf(stderr, "lens_rays: not a lens gi_set_lens accepts\n"); return 2; }
    std::vector<HaltonDim> hdims;
    std::vector<uint16_t> htable;
    build_halton_tables(hdims, htable);
    std::vector<double> verts(2 * ((size_t)lens.blades + 1));      // exactly the table's size: a read past v_B is the sanitizer's to find
    lens_vertices(lens, verts.data());
    Scene S{};
    S.hdims = hdims.data(); S.htable = htable.data();
    if (lens.radius > 0) { S.lens_verts = verts.data(); S.lens_radius = lens.radius; S.lens_blades = lens.blades; }
    printf("tag %u\n", lens_tag(lens));
    for (int i = 18; i < argc; i++) {
        const Ray r = primary_ray_at(S, F, (uint32_t)strtoul(argv[i], nullptr, 0));
        printf("%a %a %a %a %a %a\n", r.o.x, r.o.y, r.o.z, r.d.x, r.d.y, r.d.z);
    }
    return 0;
}
