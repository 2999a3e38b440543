// gi_features.inc -- the first-hit feature pass (gi_render_features_*; an addition: the reference renders radiance only; the values are those
// RayTracer::radiance holds after trace() of the primary ray, include/raytracer.h:186-210).  Included by gi_kernels.hip behind gi_upsample.inc.
// It also holds what this pass and the occlusion pass (gi_occlusion.inc) share on the host: pixel_pass_frame, pixel_pass and pixel_pass_to_host.
// The per-sample function, aov_sample(), stands first, in namespace gi beside the functions of gi_device.h it calls.

namespace gi {
// ------------------------------------------------------------------------------------------------ first-hit features (an addition: the reference has no such pass)
// What RayTracer::radiance holds right after trace() of the primary ray of the sample with Halton index idx (include/raytracer.h:186-210):
// current->material.diffuse->get(minUV), minNorm as trace returned it (not flipped, not renormalised), glm::length(minHit - ray.origin),
// the entity and its material.  Same ray, same RNG keys (seed, stream idx, depth 0, P_TRACE_ALPHA) as the beauty pass, so the alpha-test
// draws -- and with them the first hit -- are the beauty pass's.  Fog is not looked at: the features are those of the first surface.
struct AovSample { V3 albedo, normal; double depth; int32_t ent, mat; };
template <int FEAT, class Nodes>
GI_HD bool aov_sample(const Scene& S, const Nodes& N, const Frame& F, uint64_t seed, uint32_t idx, AovSample& a)
{
    const Ray ray = primary_ray_at(S, F, idx);
    const Rng rng = rng_make(seed, idx);   // depth 0
    HitRec h;
    h.tu = 0; h.tv = 0;
    if (!trace_nodes<FEAT>(S, N, ray, rng, P_TRACE_ALPHA, h, nullptr)) return false;
    if constexpr (Nodes::kWide) {
        // as the streaming trace kernel does: hit point and barycentrics again from the entity's record, by the same test with the same
        // operands, so that the walk has to carry only WHICH entity it hit
        const TriGeom& tg = S.tris[h.tri];
        h.mf = ((uint32_t)tg.mat << 3) | tg.flags;
        ent_hit<FEAT>(tg, h.mf, ray, h.u, h.v, h.pos);
    }
    const Mat& m = S.mats[h.mf >> 3];
    a.albedo = ld3(m.diffuse);
    if (FEAT & GI_FEAT_TEX) a.albedo = tex_get(S, m.dtex, a.albedo, h.tu, h.tv);
    a.normal = shading_normal(S, h);
    a.depth = length(h.pos - ray.o);
    a.ent = h.tri; a.mat = (int32_t)(h.mf >> 3);
    return true;
}
}  // namespace gi

// One kernel, k_aov<FEAT, WIDE> (aov_sample above): one lane per pixel of this rank's rows in the 8x8-tile order of st_pixel_xy, so a wave
// is a tile and all its lanes are on the same sample index s -- rays as coherent as the new paths of k_st_trace, on the same records in LDS and the
// same wave-uniform leaves.  A lane loops over s (Halton index of sample s = that of sample 0 + s * inc), keeps its eight sums in registers and
// writes once: no queue, no sort, no per-sample buffer, no atomics, and nothing of the path pool.
// out [local_rows][w][8] = albedo rgb, normal xyz, depth, coverage: the f64 sums in ascending s, divided once by n.  ids [local_rows][w][2]
// (optional) = entity and material of sample 0's hit, -1 on a miss.  GI_AOV_BLOCK: gi_instances.inc.
template <int FEAT, int WIDE>
__global__ __launch_bounds__(GI_AOV_BLOCK) void k_aov(Scene S, Frame F, uint32_t n_pix, int32_t n, void* out, int out_f64, int32_t* ids)
{
    const typename LdsSrc<WIDE>::type N = LdsSrc<WIDE>::stage_for_trace(S);   // ends with a barrier
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pix) return;
    int x, ly;
    st_pixel_xy(F, p, x, ly);
    uint32_t idx = halton_index(F.he, 0u, (uint32_t)x, (uint32_t)global_row(F, ly));
    double sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int32_t ent0 = -1, mat0 = -1;
    for (int32_t s = 0; s < n; s++, idx += F.he.inc) {
        AovSample a;
        if (!aov_sample<FEAT>(S, N, F, F.seed, idx, a)) continue;
        sum[0] += a.albedo.x; sum[1] += a.albedo.y; sum[2] += a.albedo.z;
        sum[3] += a.normal.x; sum[4] += a.normal.y; sum[5] += a.normal.z;
        sum[6] += a.depth; sum[7] += 1.0;
        if (s == 0) { ent0 = a.ent; mat0 = a.mat; }
    }
    const size_t o = (size_t)ly * F.w + x;
    const double dn = (double)n;
    if (out_f64) {
        double* q = (double*)out + o * 8;
        for (int k = 0; k < 8; k++) q[k] = sum[k] / dn;
    } else {
        float* q = (float*)out + o * 8;
        for (int k = 0; k < 8; k++) q[k] = (float)(sum[k] / dn);
    }
    if (ids) { ids[o * 2] = ent0; ids[o * 2 + 1] = mat0; }
}

namespace {

// ---- the frame of a per-pixel auxiliary pass `name` ("render_features", "render_occlusion").  An entry checks its own arguments first, in its
// own order; then the scene and the frame (pixel_pass_frame); then, behind what else it has to refuse, the pass itself (pixel_pass).
int pixel_pass_frame(gi_ctx* c, const char* name, const gi_render_params* p, Frame& F)
{
    if (!c->scene.have_scene) return fail(c, GI_E_STATE, std::string(name) + ": no scene uploaded");
    std::string ferr;
    if (!make_frame(p, F, ferr)) return fail(c, GI_E_INVALID, ferr);
    return GI_OK;
}

// the one refusal that needs the frame: Halton index of sample s = (offset of the pixel < inc) + s * inc, in 32 bits as in the beauty pass.
// pixel_pass asks it; an entry that has work to do between the frame and the pass (a table to replace) asks it first, so that a refused call
// has touched nothing
int pixel_pass_cap(gi_ctx* c, const char* name, const Frame& F, int32_t n_samples)
{
    if ((unsigned long long)n_samples * F.he.inc > (1ull << 32))
        return fail(c, GI_E_INVALID, std::string(name) + ": n_samples = " + std::to_string(n_samples) + " takes the Halton index of a " + std::to_string(F.w) + " x " + std::to_string(F.h) +
                                     " frame beyond 32 bits (at most " + std::to_string((1ull << 32) / F.he.inc) + ")");
    return GI_OK;
}

// n_samples of every pixel of F through the instance of `kernels` (a first-hit family, gi_instances.inc) that fits the scene, in workgroups of
// `block` lanes, timed by the pass's timer.  launch(kernel, grid, block, n_pix) makes the one launch.
template <class K, size_t N, class Launch>
int pixel_pass(gi_ctx* c, AuxPass& pass, const char* name, const Frame& F, int32_t n_samples, const K (&kernels)[N], unsigned block, Launch launch)
{
    if (const int rc = pixel_pass_cap(c, name, F, n_samples)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    if (F.local_rows == 0) return GI_OK;
    if (pass.lds_refused < 0) { pass.lds_refused = 0; ask_for_lds(kernels, pass.lds_refused); }
    if (pass.lds_refused) return fail(c, GI_E_HIP, std::string(name) + ": the device refused " + std::to_string(pass.lds_refused) + " bytes of dynamic LDS per workgroup");
    const uint32_t n_pix = (uint32_t)F.w * (uint32_t)F.local_rows;
    const K k = kernels[first_hit_row(scene_trace_feat(c->S), c->S.wnodes != nullptr)];
    HIP_TRY(c, pass.timer.begin(c->stream));
    launch(k, dim3((n_pix + block - 1) / block), dim3(block), n_pix);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, pass.timer.end(c->stream));
    return GI_OK;
}

// The host-pointer form of such a pass, as frame_to_host (gi_api.inc): `render(d_out, d_ids)` leaves `channels` values per pixel, and two ids
// where h_ids asks for them, in scratch of this call; they are copied to the caller's arrays.  p is not null.
template <class Render>
int pixel_pass_to_host(gi_ctx* c, AuxPass& pass, const char* what, const gi_render_params* p, size_t channels, void* h_out, int out_is_f64, int32_t* h_ids, Render render)
{
    const size_t npix = (size_t)gi_local_rows(p) * (size_t)std::max(p->width, 0);
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = npix * channels * (out_is_f64 ? 8 : 4);
    DevBuf<unsigned char> d_out;
    DevBuf<int32_t> d_ids;
    HIP_TRY(c, d_out.alloc(bytes));
    if (h_ids) HIP_TRY(c, d_ids.alloc(npix * 2));
    const int rc = render((void*)d_out.p, d_ids.p);
    return rc != GI_OK ? rc : finish_to_host(c, what, {{h_out, d_out.p, bytes}, to_host(h_ids, d_ids, npix * 2)}, &pass.timer);
}

}  // namespace

extern "C" {

int gi_render_features_device(gi_ctx* c, const gi_render_params* p, int32_t n_samples, void* d_out, int out_is_f64, int32_t* d_ids)
{
    if (!c) return GI_E_INVALID;
    c->feat.timer.reset();
    if (!d_out) return GI_E_INVALID;
    Frame F;
    if (const int rc = pixel_pass_frame(c, "render_features", p, F)) return rc;
    if (n_samples < 1) return fail(c, GI_E_INVALID, "render_features: n_samples must be at least 1");
    return pixel_pass(c, c->feat, "render_features", F, n_samples, kAov, GI_AOV_BLOCK, [&](const AovK& k, dim3 grid, dim3 block, uint32_t n_pix) {
        hipLaunchKernelGGL(k.fn, grid, block, k.lds, c->stream, c->S, F, n_pix, n_samples, d_out, out_is_f64, d_ids);
    });
}

int gi_render_features_host(gi_ctx* c, const gi_render_params* p, int32_t n_samples, void* h_out, int out_is_f64, int32_t* h_ids)
{
    if (!c) return GI_E_INVALID;
    c->feat.timer.reset();
    if (!h_out || !p) return GI_E_INVALID;
    return pixel_pass_to_host(c, c->feat, "render_features_host", p, 8, h_out, out_is_f64, h_ids,
                              [&](void* d_out, int32_t* d_ids) { return gi_render_features_device(c, p, n_samples, d_out, out_is_f64, d_ids); });
}

int gi_last_features_ms(gi_ctx* c, float* ms) { return pass_ms(c, &gi_ctx::feat, ms); }

}  // extern "C"
