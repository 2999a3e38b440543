// gi_visibility.inc -- probe visibility (gi_probe_visibility_*, gi_render_baked_visibility_*; an addition beside the bakes: what keeps a probe
// grid from leaking light through walls).  Included by gi_kernels.hip behind gi_baked.inc, whose lit_check and lit_run the look-up's entries use and
// which includes the per-lane functions (gi_visibility.h) in front of k_lit.  The definition is stated in include/gi_hip.h.  Two halves: the
// capture of the probes' octahedral depth maps, a kernel of its own, and the look-up, the PV instances of k_lit (gi_baked.inc).

// What the capture reads beside the scene
struct PvArgs {
    const double* points;       // [n_points][3]
    uint32_t size, n_samples;   // M; rays per texel
    uint32_t stream_base;
    uint64_t seed;
    double max_dist;
};

// One kernel, k_pv_capture<FEAT, WIDE>, of k_aov's shape with texels for pixels: one lane per texel t = (i M + y) M + x of the whole call, so the
// lanes of a wave are neighbouring texels of one probe (at M = 8 a wave is a map) and their rays leave one point into neighbouring directions.  A
// lane loops over its samples, carries the two f64 sums and stores once: no path pool, no sort, no queue, no atomics and no reduction across lanes,
// so the sums run in ascending k whatever the launch.  The closest hit is the frame's primary ray's (lit_first_hit): trace_nodes with the alpha
// draws keyed by (seed, stream) at depth 0, and on the wide walk the hit point again from the entity's record.  LDS as k_aov's: the records of the
// octree's top with the closest-hit walk's content boxes -- there is no any-hit walk here.  GI_PV_BLOCK: gi_instances.inc.
template <int FEAT, int WIDE>
__global__ __launch_bounds__(GI_PV_BLOCK) void k_pv_capture(Scene S, PvArgs A, unsigned long long n_texels, void* out, int out_f64)
{
    const typename LdsSrc<WIDE>::type N = LdsSrc<WIDE>::stage_for_trace(S);   // ends with a barrier
    const unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_texels) return;
    const uint32_t M = A.size;
    const uint32_t x = (uint32_t)(t % M), y = (uint32_t)((t / M) % M);
    const V3 P = ld3(A.points + (size_t)(t / ((unsigned long long)M * M)) * 3);
    uint32_t stream = A.stream_base + (uint32_t)t * A.n_samples;   // (the entry has checked that the last index fits 32 bits)
    PvSums sums = {0.0, 0.0};
    for (uint32_t k = 0; k < A.n_samples; k++, stream++) {
        const Ray ray = pv_ray(S, P, M, x, y, stream);
        const Rng rng = rng_make(A.seed, stream);   // depth 0
        HitRec h;
        h.tu = 0; h.tv = 0;
        double r = A.max_dist;
        if (trace_nodes<FEAT>(S, N, ray, rng, P_TRACE_ALPHA, h, nullptr)) {
            if constexpr (WIDE != 0) {   // as aov_sample
                const TriGeom& tg = S.tris[h.tri];
                h.mf = ((uint32_t)tg.mat << 3) | tg.flags;
                ent_hit<FEAT>(tg, h.mf, ray, h.u, h.v, h.pos);
            }
            r = pv_hit_distance(h.pos, P);
        }
        pv_add(sums, pv_clamp(r, A.max_dist));
    }
    const PvMoments q = pv_moments(sums, (double)A.n_samples);
    if (out_f64) { double* o = (double*)out + (size_t)t * 2; o[0] = q.m; o[1] = q.m2; }
    else { float* o = (float*)out + (size_t)t * 2; o[0] = (float)q.m; o[1] = (float)q.m2; }
}

// the rays k_pv_capture makes, sample by sample (gi_probe_visibility_rays): ray j = sample j % n_samples of texel j / n_samples
__global__ __launch_bounds__(GI_BLOCK) void k_pv_rays(Scene S, PvArgs A, uint32_t n_rays, double* rays, uint32_t* streams)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_rays) return;
    const uint32_t t = j / A.n_samples, M = A.size;
    const uint32_t stream = A.stream_base + j;
    const Ray r = pv_ray(S, ld3(A.points + (size_t)(t / (M * M)) * 3), M, t % M, (t / M) % M, stream);
    double* o = rays + (size_t)j * 6;
    o[0] = r.o.x; o[1] = r.o.y; o[2] = r.o.z; o[3] = r.d.x; o[4] = r.d.y; o[5] = r.d.z;
    streams[j] = stream;
}

// the capture's sums on caller distances (gi_probe_visibility_fold): one lane per texel, dist [n_texels][n_samples]
__global__ __launch_bounds__(GI_BLOCK) void k_pv_fold(const double* dist, uint32_t n_texels, uint32_t n_samples, double* out2)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_texels) return;
    PvSums sums = {0.0, 0.0};
    for (uint32_t k = 0; k < n_samples; k++) pv_add(sums, dist[(size_t)t * n_samples + k]);
    const PvMoments q = pv_moments(sums, (double)n_samples);
    out2[(size_t)t * 2] = q.m; out2[(size_t)t * 2 + 1] = q.m2;
}

namespace {

// false + message when parameters and point count are not the header's
bool pv_check(const gi_probe_visibility_params* p, int32_t n_points, std::string& err)
{
    if (!p) { err = "probe_visibility: null parameters"; return false; }
    if (p->size < 1 || p->size > GI_PV_MAX_SIZE) { err = "probe_visibility: size must be 1 .. " + std::to_string(GI_PV_MAX_SIZE) + ", got " + std::to_string(p->size); return false; }
    if (p->n_samples < 1) { err = "probe_visibility: n_samples must be at least 1, got " + std::to_string(p->n_samples); return false; }
    if (n_points < 0) { err = "probe_visibility: n_points must not be negative, got " + std::to_string(n_points); return false; }
    if (!std::isfinite(p->max_dist) || !(p->max_dist > 0.0)) { err = "probe_visibility: max_dist must be finite and > 0, got " + std::to_string(p->max_dist); return false; }
    // (texels: at most 2^31 x 2^12; with no more than 2^32 of them, times at most 2^31 samples fits 64 bits)
    const unsigned long long texels = (unsigned long long)n_points * (unsigned long long)(p->size * p->size);
    if (texels > (1ull << 32) || (unsigned long long)p->stream_base + texels * (unsigned long long)p->n_samples > (1ull << 32)) {
        err = "probe_visibility: " + std::to_string(n_points) + " maps of " + std::to_string(p->size) + " x " + std::to_string(p->size) + " texels of " + std::to_string(p->n_samples) +
              " samples from stream_base " + std::to_string(p->stream_base) + " take the stream index beyond 32 bits";
        return false;
    }
    return true;
}
// the host entries look at the points: every position finite
bool pv_points_ok(const double* points, int32_t n_points, std::string& err)
{
    for (size_t i = 0; i < (size_t)n_points * 3; i++)
        if (!std::isfinite(points[i])) { err = "probe_visibility: point " + std::to_string(i / 3) + " has a non-finite position"; return false; }
    return true;
}
PvArgs pv_args(const gi_probe_visibility_params& p, const double* d_points)
{
    PvArgs A;
    A.points = d_points;
    A.size = (uint32_t)p.size; A.n_samples = (uint32_t)p.n_samples;
    A.stream_base = p.stream_base; A.seed = p.seed; A.max_dist = p.max_dist;
    return A;
}

// the capture itself: d_points and d_out on the device, arguments checked, n_points > 0
int pv_run(gi_ctx* c, const double* d_points, int32_t n_points, const gi_probe_visibility_params& p, void* d_out, int out_is_f64)
{
    HIP_TRY(c, hipSetDevice(c->device));
    AuxPass& pass = c->pv;
    if (pass.lds_refused < 0) { pass.lds_refused = 0; ask_for_lds(kPv, pass.lds_refused); }
    if (pass.lds_refused) return fail(c, GI_E_HIP, "probe_visibility: the device refused " + std::to_string(pass.lds_refused) + " bytes of dynamic LDS per workgroup");
    const unsigned long long n_texels = (unsigned long long)n_points * (unsigned long long)(p.size * p.size);
    const PvK k = kPv[first_hit_row(scene_trace_feat(c->S), c->S.wnodes != nullptr)];
    HIP_TRY(c, pass.timer.begin(c->stream));
    hipLaunchKernelGGL(k.fn, dim3((unsigned)((n_texels + GI_PV_BLOCK - 1) / GI_PV_BLOCK)), dim3(GI_PV_BLOCK), k.lds, c->stream, c->S, pv_args(p, d_points), n_texels, d_out, out_is_f64);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, pass.timer.end(c->stream));
    return GI_OK;
}

// ---- gi_render_baked_visibility_*
std::string pv_named(const std::string& err) { return lit_named(err, "render_baked_visibility"); }
// false + message when the look-up's parameters are not the header's
bool lit_pv_check(const gi_baked_visibility_params* vp, std::string& err)
{
    if (!vp) { err = "render_baked_visibility: null visibility parameters"; return false; }
    if (vp->size < 1 || vp->size > GI_PV_MAX_SIZE) { err = "render_baked_visibility: size must be 1 .. " + std::to_string(GI_PV_MAX_SIZE) + ", got " + std::to_string(vp->size); return false; }
    if (!std::isfinite(vp->normal_bias) || !(vp->normal_bias >= 0.0)) { err = "render_baked_visibility: normal_bias must be finite and >= 0, got " + std::to_string(vp->normal_bias); return false; }
    if (!(vp->vis_floor > 0.0) || !(vp->vis_floor <= 1.0)) { err = "render_baked_visibility: vis_floor must be in (0, 1], got " + std::to_string(vp->vis_floor); return false; }
    return true;
}

}  // namespace

extern "C" {

void gi_probe_visibility_default_params(gi_probe_visibility_params* p)
{
    if (!p) return;
    p->size = 8; p->n_samples = 16;
    p->stream_base = 0u;
    p->seed = 0x9E3779B97F4A7C15ull;
    p->max_dist = 1e30;
}

int gi_probe_visibility_device(gi_ctx* c, const double* d_points, int32_t n_points, const gi_probe_visibility_params* p, void* d_out, int out_is_f64)
{
    if (!c) return GI_E_INVALID;
    std::string err;
    if (!pv_check(p, n_points, err)) return fail(c, GI_E_INVALID, err);
    if (n_points && (!d_points || !d_out)) return fail(c, GI_E_INVALID, "probe_visibility: null points or output pointer");
    if (!c->scene.have_scene) return fail(c, GI_E_STATE, "probe_visibility: no scene uploaded");
    c->pv.timer.reset();
    if (n_points == 0) return GI_OK;
    return pv_run(c, d_points, n_points, *p, d_out, out_is_f64);
}

int gi_probe_visibility_host(gi_ctx* c, const double* points, int32_t n_points, const gi_probe_visibility_params* p, void* h_out, int out_is_f64)
{
    if (!c) return GI_E_INVALID;
    std::string err;
    if (!pv_check(p, n_points, err)) return fail(c, GI_E_INVALID, err);
    if (n_points && (!points || !h_out)) return fail(c, GI_E_INVALID, "probe_visibility: null points or output pointer");
    if (!pv_points_ok(points, n_points, err)) return fail(c, GI_E_INVALID, err);
    if (!c->scene.have_scene) return fail(c, GI_E_STATE, "probe_visibility: no scene uploaded");
    c->pv.timer.reset();
    if (n_points == 0) return GI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t N = (size_t)n_points, bytes = N * (size_t)(p->size * p->size) * 2 * (out_is_f64 ? 8 : 4);
    DevBuf<double> d_points;
    DevBuf<unsigned char> d_out;
    HIP_TRY(c, d_points.upload(points, N * 3));
    HIP_TRY(c, d_out.alloc(bytes));
    const int rc = pv_run(c, d_points.p, n_points, *p, d_out.p, out_is_f64);
    return rc != GI_OK ? rc : finish_to_host(c, "probe_visibility_host", {{h_out, d_out.p, bytes}}, &c->pv.timer);
}

int gi_last_probe_visibility_ms(gi_ctx* c, float* ms) { return pass_ms(c, &gi_ctx::pv, ms); }

int gi_probe_visibility_rays(gi_ctx* c, const double* points, int32_t n_points, const gi_probe_visibility_params* p, double* rays6_out, uint32_t* stream_out)
{
    if (!c) return GI_E_INVALID;
    std::string err;
    if (!pv_check(p, n_points, err)) return fail(c, GI_E_INVALID, err);
    if (n_points && (!points || !rays6_out || !stream_out)) return fail(c, GI_E_INVALID, "probe_visibility_rays: null points or output pointer");
    if (!pv_points_ok(points, n_points, err)) return fail(c, GI_E_INVALID, err);
    const size_t n_rays = (size_t)n_points * (size_t)(p->size * p->size) * (size_t)p->n_samples;
    if (n_rays > 0x7fffffffull) return fail(c, GI_E_INVALID, "probe_visibility_rays: more than 2^31 - 1 rays");
    if (n_rays == 0) return GI_OK;
    Entry e(c, "probe_visibility_rays");
    const double* d_p = e.in(points, (size_t)n_points * 3);
    double* d_r = e.out(rays6_out, n_rays * 6);
    uint32_t* d_s = e.out(stream_out, n_rays);
    return e.run([&] { hipLaunchKernelGGL(k_pv_rays, GI_GRID(n_rays), 0, c->stream, c->S, pv_args(*p, d_p), (uint32_t)n_rays, d_r, d_s); });
}

int gi_probe_visibility_fold(gi_ctx* c, int32_t n_texels, int32_t n_samples, const double* dist, double* out2)
{
    if (!c) return GI_E_INVALID;
    if (n_texels < 0 || n_samples < 1) return fail(c, GI_E_INVALID, "probe_visibility_fold: n_texels >= 0, n_samples >= 1");
    if (n_texels && (!dist || !out2)) return fail(c, GI_E_INVALID, "probe_visibility_fold: null pointer");
    if ((unsigned long long)n_texels * (unsigned long long)n_samples > 0x7fffffffull) return fail(c, GI_E_INVALID, "probe_visibility_fold: more than 2^31 - 1 distances");
    if (n_texels == 0) return GI_OK;
    Entry e(c, "probe_visibility_fold");
    const double* d_d = e.in(dist, (size_t)n_texels * (size_t)n_samples);
    double* d_o = e.out(out2, (size_t)n_texels * 2);
    return e.run([&] { hipLaunchKernelGGL(k_pv_fold, GI_GRID(n_texels), 0, c->stream, d_d, (uint32_t)n_texels, (uint32_t)n_samples, d_o); });
}

void gi_baked_visibility_default_params(gi_baked_visibility_params* p)
{
    if (!p) return;
    p->size = 8;
    p->normal_bias = 0.0; p->vis_floor = 0.05;
}

int gi_render_baked_visibility_device(gi_ctx* c, const gi_render_params* p, const gi_baked_params* bp, const gi_baked_visibility_params* vp, const double* d_sh, const double* d_chain,
                                      const double* d_vis, void* d_out, int out_is_f64)
{
    if (!c) return GI_E_INVALID;
    if (!p || !d_out) return fail(c, GI_E_INVALID, "render_baked_visibility: null frame parameters or output pointer");
    std::string err;
    if (!lit_check(bp, d_sh, d_chain, err)) return fail(c, GI_E_INVALID, pv_named(err));
    if (!lit_pv_check(vp, err)) return fail(c, GI_E_INVALID, err);
    Frame F;
    if (const int rc = pixel_pass_frame(c, "render_baked_visibility", p, F)) return rc;
    if (!d_vis || !(bp->terms & GI_BAKED_DIFFUSE))      // no map takes part: the PV = 0 instances, gi_render_baked_*'s bits
        return lit_run(c, "render_baked_visibility", F, bp, bp->terms, d_sh, d_chain, nullptr, d_out, out_is_f64);
    HIP_TRY(c, hipSetDevice(c->device));
    LitPass& lit = c->lit;
    if (lit.lds_refused < 0) { lit.lds_refused = 0; ask_for_lds(kLit, lit.lds_refused); }       // (pixel_pass would take the PV table's answer for this one)
    if (lit.pv_lds_refused < 0) { lit.pv_lds_refused = 0; ask_for_lds(kLitPv, lit.pv_lds_refused); }
    if (lit.pv_lds_refused) return fail(c, GI_E_HIP, "render_baked_visibility: the device refused " + std::to_string(lit.pv_lds_refused) + " bytes of dynamic LDS per workgroup");
    LitArgs pv{};
    pv.vis = d_vis; pv.vis_size = vp->size; pv.normal_bias = vp->normal_bias; pv.vis_floor = vp->vis_floor;
    return lit_run(c, "render_baked_visibility", F, bp, bp->terms, d_sh, d_chain, &pv, d_out, out_is_f64);
}

int gi_render_baked_visibility_host(gi_ctx* c, const gi_render_params* p, const gi_baked_params* bp, const gi_baked_visibility_params* vp, const double* sh, const double* chain,
                                    const void* vis, int vis_is_f64, void* h_out, int out_is_f64)
{
    if (!c) return GI_E_INVALID;
    if (!p || !h_out) return fail(c, GI_E_INVALID, "render_baked_visibility: null frame parameters or output pointer");
    std::string err;
    if (!lit_check(bp, sh, chain, err)) return fail(c, GI_E_INVALID, pv_named(err));
    if (!lit_pv_check(vp, err)) return fail(c, GI_E_INVALID, err);
    if (!c->scene.have_scene) return fail(c, GI_E_STATE, "render_baked_visibility: no scene uploaded");
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf<double> d_sh, d_chain, d_vis;
    const size_t n_probe = (size_t)bp->nx * (size_t)bp->ny * (size_t)bp->nz;
    if (bp->terms & GI_BAKED_DIFFUSE) HIP_TRY(c, d_sh.upload(sh, n_probe * 27));
    if (bp->terms & GI_BAKED_SPECULAR) HIP_TRY(c, d_chain.upload(chain, cm_texels_before(bp->face, bp->levels) * 3));
    if (vis && (bp->terms & GI_BAKED_DIFFUSE)) {
        const size_t n = n_probe * (size_t)(vp->size * vp->size) * 2;
        if (vis_is_f64) HIP_TRY(c, d_vis.upload((const double*)vis, n));
        else {                                                // widened here, exactly: the device reads f64
            std::vector<double> wide(n);
            for (size_t i = 0; i < n; i++) wide[i] = (double)((const float*)vis)[i];
            HIP_TRY(c, d_vis.upload(wide));
        }
    }
    return pixel_pass_to_host(c, c->lit, "render_baked_visibility_host", p, 12, h_out, out_is_f64, nullptr, [&](void* d_out, int32_t*) {
        return gi_render_baked_visibility_device(c, p, bp, vp, d_sh.p, d_chain.p, d_vis.p, d_out, out_is_f64);
    });
}

}  // extern "C"
