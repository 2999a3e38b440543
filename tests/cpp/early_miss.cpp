// tests/cpp/early_miss.cpp -- CPU build of ray_leaves_scene (gi_walk.h) next to the host emulator's trace, for tests/test_early_miss_cpu.py.
//
// TEST INFRASTRUCTURE ONLY.  The host emulator (tests/host_emul/emul.cpp: scene layout, Emul::bind, emul_create / emul_upload_scene) is taken in
// as it is; this file adds the probe the deferred shade kernel runs on the next ray of a vertex, and the rays to ask it about.
#include "../host_emul/emul.cpp"

extern "C" {

// leaves[i] = ray_leaves_scene(ray i) within max_turns turns, over the records and content boxes of the closest-hit walk -- what k_st_shade stages.
// hit_wide[i] / hit_nodes[i]: what trace() answers for the same ray over the wide records (the streaming kernels' walk) and over the per-node
// links (the reference's order of box tests).  -1: the scene has no wide records.
int em_probe(Emul* e, int n, const double* rays, int max_turns, int32_t* leaves, int32_t* hit_wide, int32_t* hit_nodes)
{
    if (!e->S.wnodes) return -1;
    GlobalWide W;
    W.g = e->S.wnodes; W.cboxes = e->S.tcboxes; W.cuse = e->S.tcuse;
    Scene Sn = e->S;
    Sn.wnodes = nullptr;
    for (int i = 0; i < n; i++) {
        const double* r = rays + (size_t)i * 6;
        const Ray ray = make_ray_exact(v3(r[0], r[1], r[2]), v3(r[3], r[4], r[5]));
        leaves[i] = ray_leaves_scene(e->S, W, ray, max_turns) ? 1 : 0;
        const Rng rng = rng_make(0, (uint32_t)i);
        HitRec h;
        hit_wide[i] = trace(e->S, ray, rng, P_TRACE_ALPHA, h, nullptr) ? 1 : 0;
        hit_nodes[i] = trace(Sn, ray, rng, P_TRACE_ALPHA, h, nullptr) ? 1 : 0;
    }
    return 0;
}

// The rays the shade stage would ask the probe about: every sample of the frame is followed through trace and shade, and the next ray of every
// vertex that continues is written to rays6 (up to cap of them, in path order).  Returns how many.
int em_next_rays(Emul* e, const gi_render_params* p, int cap, double* rays6)
{
    Frame F;
    if (!make_frame(p, F, e->err)) return GI_E_INVALID;
    int n = 0;
    for (int s = 0; s < F.max_samples; s++)
        for (int y = 0; y < F.local_rows; y++)
            for (int x = 0; x < F.w; x++) {
                uint32_t idx;
                const Ray ray = primary_ray(e->S, F, s, x, global_row(F, y), idx);
                PathRec q;
                path_begin(q, ray, idx);
                for (;;) {
                    if (!stage_trace(e->S, q, F.seed, nullptr)) break;
                    const int fl = stage_shade(e->S, q, F.seed, nullptr);
                    if (!(fl & ST_CONTINUE)) break;
                    if (n >= cap) return n;
                    for (int k = 0; k < 3; k++) { rays6[(size_t)n * 6 + k] = q.o[k]; rays6[(size_t)n * 6 + 3 + k] = q.d[k]; }
                    n++;
                }
            }
    return n;
}

}
