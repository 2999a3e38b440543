// gi_occlusion.inc -- the ambient-occlusion / bent-normal pass (gi_render_occlusion_*; an addition: the reference has none).  Included by
// gi_kernels.hip behind gi_features.inc, whose host frame of a per-pixel pass it shares (pixel_pass_frame, pixel_pass, pixel_pass_to_host).  The definition is stated in include/gi_hip.h; the per-sample functions,
// ao_first_hit() and ao_segments(), stand first with their constants, in namespace gi beside the functions of gi_device.h they call.

namespace gi {
// ------------------------------------------------------------------------------------------------ ambient occlusion / bent normals (an addition: the reference has no such pass)
// gi_hip.h: gi_render_occlusion_*.  The first hit of the sample with Halton index idx is aov_sample's (same ray, same RNG keys, same recomputation
// of the hit from the entity's record on the wide walk); from it n_dirs segments of length `radius` go into the cosine hemisphere around the
// normal turned towards the viewer, each asked of the any-hit walk as a shadow segment is -- RayTracer::visible on (O, O + radius d_j) -- with
// alpha keys of its own (light index GI_AO_LIGHT_INDEX + j) and without the medium: fog does not occlude.
enum { P_AO_U = 32, P_AO_V = 33 };      // RNG purposes of a direction's two numbers; `a` = j
#define GI_AO_LIGHT_INDEX 0x10000u      // + j: the `light index` of segment j's alpha draws, beyond every real light's
#define GI_AO_MAX_DIRS 64
struct AoHit { V3 o, nf; };             // O = P + GI_SHADOW_BIAS Nf, and Nf = the unit shading normal on the viewer's side
template <int FEAT, class Nodes>
GI_HD bool ao_first_hit(const Scene& S, const Nodes& N, const Frame& F, uint64_t seed, uint32_t idx, Rng& rng, AoHit& a)
{
    const Ray ray = primary_ray_at(S, F, idx);
    rng = rng_make(seed, idx);   // depth 0
    HitRec h;
    h.tu = 0; h.tv = 0;
    if (!trace_nodes<FEAT>(S, N, ray, rng, P_TRACE_ALPHA, h, nullptr)) return false;
    if constexpr (Nodes::kWide) {   // as aov_sample
        const TriGeom& tg = S.tris[h.tri];
        h.mf = ((uint32_t)tg.mat << 3) | tg.flags;
        ent_hit<FEAT>(tg, h.mf, ray, h.u, h.v, h.pos);
    }
    const V3 nh = normalize(shading_normal(S, h));
    a.nf = dot(nh, ray.d) > 0 ? v3(-nh.x, -nh.y, -nh.z) : nh;
    a.o = h.pos + GI_SHADOW_BIAS * a.nf;
    return true;
}
// the n_dirs segments of one hit: returns the number of open ones, bent = the sum of their directions in ascending j.  VFEAT: the walk's level
// without GI_FEAT_FOG.  mt is formed as k_visible forms it from (O, T_j), so gi_visible on those rows is the statement.
template <int VFEAT, class Nodes>
GI_HD int32_t ao_segments(const Scene& S, const Nodes& N, const AoHit& a, const Rng& rng, int32_t n_dirs, double radius, V3& bent)
{
    static_assert((VFEAT & GI_FEAT_FOG) == 0, "fog does not occlude");
    int32_t open = 0;
    bent = v3(0, 0, 0);
    for (int32_t j = 0; j < n_dirs; j++) {
        const float u = (float)rng_draw(rng, P_AO_U, (uint32_t)j);
        const float v = (float)rng_draw(rng, P_AO_V, (uint32_t)j);
        const V3 d = hemi_cos_n(a.nf, u, v, 1);
        const V3 t = a.o + radius * d;
        const double mt = len2(t - a.o);
        const Ray sr = make_ray(a.o, d);
        if (visible_nodes<VFEAT>(S, N, sr, mt, rng, GI_AO_LIGHT_INDEX + (uint32_t)j, nullptr)) { open++; bent = bent + d; }
    }
    return open;
}
}  // namespace gi

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
