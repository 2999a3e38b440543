// tests/cpp/test_progressive.cpp -- a progressive render session driven through the C ABI (include/gi_hip.h: gi_progressive_*) by a C++ caller:
// argv[1] = .scn, argv[2] = width, argv[3] = height, argv[4] = samples per pixel, argv[5] = photon indices per light, argv[6] (optional) = a file
// that gets the raw doubles of the session's final frame.  Renders the frame with gi_render_host, then in a session (0, 3 and the remaining samples),
// then from a checkpoint taken after 3 samples and restored; prints what the test reads.  Exit status 0 when every comparison held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../gi_raytracer_amd/csrc/gi_host.h"

static int check(gi_ctx* c, int rc, const char* what)
{
    if (rc < 0) { printf("%s failed (%d): %s\n", what, rc, gi_last_error(c)); exit(1); }
    return rc;
}

int main(int argc, char** argv)
{
    if (argc < 6) return 2;
    const int w = atoi(argv[2]), h = atoi(argv[3]), spp = atoi(argv[4]), photons = atoi(argv[5]);
    gih_scene* hs = gih_scene_create();
    if (gih_load_scn(hs, argv[1]) != 0 || gih_build_octree(hs) != 0) { printf("scene: %s\n", gih_last_error(hs)); return 1; }
    gi_scene_desc sd;
    gih_settings st;
    if (gih_get_scene_desc(hs, &sd) != 0 || gih_get_settings(hs, &st) != 0) return 1;
    gi_ctx* c = nullptr;
    if (gi_create(&c, 0) != 0) { printf("no device\n"); return 1; }
    gi_render_params rp;
    memset(&rp, 0, sizeof rp);
    for (int k = 0; k < 3; k++) { rp.cam_pos[k] = st.cam_pos[k]; rp.cam_up[k] = st.cam_up[k]; rp.cam_forward[k] = st.cam_forward[k]; }
    rp.sensor_diag = st.sensor_diag; rp.focal_dist = st.focal_dist;
    rp.width = w; rp.height = h; rp.stripe_h = h; rp.stripe_rank = 0; rp.stripe_world = 1;
    rp.min_samples = spp; rp.max_samples = spp; rp.noise_thresh = st.noise_thresh;
    rp.seed = 0x9E3779B97F4A7C15ull;
    const size_t npix = (size_t)w * h;
    std::vector<double> out(npix * 3);
    std::vector<int32_t> n(npix);
    printf("begin without scene %d\n", gi_progressive_begin(c, &rp));
    check(c, gi_upload_scene(c, &sd), "upload_scene");
    check(c, gi_clear_photons(c), "clear_photons");
    check(c, gi_trace_photons(c, photons, 5, rp.seed, nullptr, nullptr), "trace_photons");
    printf("step without session %d\n", gi_progressive_step_host(c, 1, out.data(), 1, nullptr, nullptr));
    std::vector<double> ref(npix * 3);
    std::vector<int32_t> ref_n(npix);
    check(c, gi_render_host(c, &rp, ref.data(), 1, ref_n.data(), nullptr), "render_host");

    check(c, gi_progressive_begin(c, &rp), "progressive_begin");
    check(c, gi_progressive_step_host(c, 0, out.data(), 1, n.data(), nullptr), "step 0");
    bool initial = true;
    for (size_t i = 0; i < npix; i++) initial = initial && out[i * 3] == 0.5 && out[i * 3 + 1] == 0.5 && out[i * 3 + 2] == 0.5 && n[i] == 0;
    printf("initial frame ok %d\n", (int)initial);
    printf("negative step %d\n", gi_progressive_step_host(c, -1, out.data(), 1, nullptr, nullptr));
    check(c, gi_progressive_step_host(c, 3, out.data(), 1, n.data(), nullptr), "step 3");
    int64_t bytes = 0;
    check(c, gi_progressive_state_bytes(c, &bytes), "state_bytes");
    std::vector<unsigned char> blob((size_t)bytes);
    check(c, gi_progressive_save(c, blob.data(), bytes), "save");
    check(c, gi_progressive_step_host(c, spp, out.data(), 1, n.data(), nullptr), "last step");      // clamped to the remaining samples
    const bool steps_ok = memcmp(out.data(), ref.data(), npix * 24) == 0 && memcmp(n.data(), ref_n.data(), npix * 4) == 0;
    printf("steps equal one-shot %d\n", (int)steps_ok);
    int32_t end = -1;
    int64_t wanting = -1;
    check(c, gi_progressive_status(c, &end, &wanting), "status");
    printf("status end %d wanting %lld\n", end, (long long)wanting);
    if (argc > 6) {
        FILE* fp = fopen(argv[6], "wb");
        if (!fp) return 3;
        fwrite(out.data(), sizeof(double), out.size(), fp);
        fclose(fp);
    }
    check(c, gi_progressive_end(c), "end");

    check(c, gi_progressive_restore(c, blob.data(), bytes), "restore");
    check(c, gi_progressive_status(c, &end, nullptr), "status");
    std::fill(out.begin(), out.end(), 0.0);
    check(c, gi_progressive_step_host(c, spp - end, out.data(), 1, n.data(), nullptr), "step after restore");
    const bool restored_ok = end == 3 && memcmp(out.data(), ref.data(), npix * 24) == 0 && memcmp(n.data(), ref_n.data(), npix * 4) == 0;
    printf("restored equal one-shot %d\n", (int)restored_ok);
    check(c, gi_progressive_end(c), "end");
    gi_destroy(c);
    gih_scene_destroy(hs);
    return initial && steps_ok && restored_ok ? 0 : 1;
}
