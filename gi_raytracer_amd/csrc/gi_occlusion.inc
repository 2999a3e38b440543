// gi_occlusion.inc -- the ambient-occlusion / bent-normal pass (gi_render_occlusion_*; an addition: the reference has none).  Included by
// gi_kernels.hip behind gi_features.inc, whose host frame of a per-pixel pass it shares (pixel_pass_frame, pixel_pass, pixel_pass_to_host).  The definition is stated in include/gi_hip.h; the per-sample functions are ao_first_hit() and ao_segments()
// in gi_device.h.
//
// One kernel, k_ao<FEAT, WIDE>, of k_aov's shape: one lane per pixel of this rank's rows in the 8x8-tile order of st_pixel_xy, a lane loops over its
// samples and, per sample, over the n_dirs segments; it keeps its four f64 sums in registers and stores once.  No queue, no sort, no atomics, nothing
// of the path pool -- and no reduction across lanes, so the bent vector is summed in ascending j and then ascending s whatever the launch shape.
// A sample's first-hit state (ray, hit record, entity record) is dead when its segments start: what lives across the segment loop is O, Nf, the RNG
// key and the sums, so the kernel's register need is the larger of the two walks', not their sum.
//
// LDS as k_aov's (the records of the octree's top, wide: with their content boxes), with one difference: the boxes staged are the whole entities'
// (Scene::cboxes, valid for any walk), because the n_dirs any-hit walks of a sample read them and its one closest-hit walk does not have to: that one
// takes the tables k_aov's takes (Scene::tcboxes, cut to the leaves) through L2 where the two differ.  The segments end anywhere, not at a light, so
// the any-hit walk uses the whole entities' boxes (Scene::leaf_boxes), as gi_visible does, never the ones cut for segments that end at a light.
template <int FEAT, int WIDE>
__global__ __launch_bounds__(GI_AO_BLOCK) void k_ao(Scene S, Frame F, uint32_t n_pix, int32_t n, int32_t n_dirs, double radius, void* out, int out_f64)
{
    const typename LdsSrc<WIDE>::type NV = LdsSrc<WIDE>::stage_with_boxes(S);   // ends with a barrier
    typename LdsSrc<WIDE>::type NT = NV;                                        // the closest-hit walk's view of the same records
    if constexpr (WIDE != 0) {
        if (S.tcboxes != S.cboxes || S.tcuse != S.cuse) { NT.cboxes = S.tcboxes; NT.cuse = S.tcuse; NT.n_lc = 0; }
    }
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pix) return;
    int x, ly;
    st_pixel_xy(F, p, x, ly);
    uint32_t idx = halton_index(F.he, 0u, (uint32_t)x, (uint32_t)global_row(F, ly));
    const double nd = (double)n_dirs;
    double sum[4] = {0, 0, 0, 0};
    for (int32_t s = 0; s < n; s++, idx += F.he.inc) {
        AoHit a;
        Rng rng;
        if (!ao_first_hit<FEAT>(S, NT, F, F.seed, idx, rng, a)) { sum[0] += 1.0; continue; }   // a miss is open, its bent vector 0
        V3 bent;
        const int32_t open = ao_segments<FEAT & ~GI_FEAT_FOG>(S, NV, a, rng, n_dirs, radius, bent);
        sum[0] += (double)open / nd;
        sum[1] += bent.x / nd; sum[2] += bent.y / nd; sum[3] += bent.z / nd;
    }
    const size_t o = ((size_t)ly * F.w + x) * 4;
    const double dn = (double)n;
    if (out_f64) {
        double* q = (double*)out + o;
        for (int k = 0; k < 4; k++) q[k] = sum[k] / dn;
    } else {
        float* q = (float*)out + o;
        for (int k = 0; k < 4; k++) q[k] = (float)(sum[k] / dn);
    }
}

namespace {

// false + message when the parameters are not the header's
bool ao_check(const gi_occlusion_params* p, std::string& err)
{
    if (!p) { err = "render_occlusion: null parameters"; return false; }
    if (p->n_samples < 1) { err = "render_occlusion: n_samples must be at least 1, got " + std::to_string(p->n_samples); return false; }
    if (p->n_dirs < 1 || p->n_dirs > GI_AO_MAX_DIRS) { err = "render_occlusion: n_dirs must be 1 .. " + std::to_string(GI_AO_MAX_DIRS) + ", got " + std::to_string(p->n_dirs); return false; }
    if (!(p->radius >= 0.0) || !(p->radius <= 1.7976931348623157e308)) { err = "render_occlusion: radius must be finite and >= 0 (0: a tenth of the scene box's diagonal), got " + std::to_string(p->radius); return false; }
    return true;
}

}  // namespace

extern "C" {

void gi_occlusion_default_params(gi_occlusion_params* p)
{
    if (!p) return;
    p->n_samples = 16; p->n_dirs = 16;
    p->radius = 0.0;
}

int gi_render_occlusion_device(gi_ctx* c, const gi_render_params* p, const gi_occlusion_params* op, void* d_out, int out_is_f64)
{
    if (!c) return GI_E_INVALID;
    c->ao.timer.reset();
    if (!p || !d_out) return fail(c, GI_E_INVALID, "render_occlusion: null frame parameters or output pointer");
    std::string err;
    if (!ao_check(op, err)) return fail(c, GI_E_INVALID, err);
    Frame F;
    if (const int rc = pixel_pass_frame(c, "render_occlusion", p, F)) return rc;
    double radius = op->radius;
    if (radius == 0.0) {   // a tenth of the diagonal of the scene's root box
        const double dx = c->S.root_bmax[0] - c->S.root_bmin[0], dy = c->S.root_bmax[1] - c->S.root_bmin[1], dz = c->S.root_bmax[2] - c->S.root_bmin[2];
        radius = 0.1 * sqrt((dx * dx + dy * dy) + dz * dz);
    }
    return pixel_pass(c, c->ao, "render_occlusion", F, op->n_samples, kAo, GI_AO_BLOCK, [&](const AoK& k, dim3 grid, dim3 block, uint32_t n_pix) {
        hipLaunchKernelGGL(k.fn, grid, block, k.lds, c->stream, c->S, F, n_pix, op->n_samples, op->n_dirs, radius, d_out, out_is_f64);
    });
}

int gi_render_occlusion_host(gi_ctx* c, const gi_render_params* p, const gi_occlusion_params* op, void* h_out, int out_is_f64)
{
    if (!c) return GI_E_INVALID;
    c->ao.timer.reset();
    if (!p || !h_out) return fail(c, GI_E_INVALID, "render_occlusion: null frame parameters or output pointer");
    std::string err;
    if (!ao_check(op, err)) return fail(c, GI_E_INVALID, err);
    return pixel_pass_to_host(c, c->ao, "render_occlusion_host", p, 4, h_out, out_is_f64, nullptr,
                              [&](void* d_out, int32_t*) { return gi_render_occlusion_device(c, p, op, d_out, out_is_f64); });
}

int gi_last_occlusion_ms(gi_ctx* c, float* ms) { return pass_ms(c, &gi_ctx::ao, ms); }

}  // extern "C"
