// gi_finalgather.inc -- the final-gather pass (gi_render_final_gather_*; an addition: one bounce from the first hits into the baked light).  Included
// by gi_kernels.hip behind gi_baked.inc, whose first hit (lit_first_hit), light loop (lit_direct), look-ups (gi_baked.h), LitArgs and parameter
// check (lit_check) it calls; the host frame of a per-pixel pass is gi_features.inc's (pixel_pass_frame, pixel_pass, pixel_pass_to_host).  The
// definition is stated in include/gi_hip.h; the per-lane functions that need no walk are gi_finalgather.h, and fg_trace() stands here.

namespace gi {
#include "gi_finalgather.h"

enum { P_FG_U = 36, P_FG_V = 37 };      // RNG purposes of a gather direction's two numbers (stream at depth 0); `a` = j

// The closest hit of the gather ray (O, d), d as hemi_cos_n gave it (gi_trace's ray, not renormalised), with the stream's RNG at depth 1 + j: what
// the light loop needs of it and no more -- Q, the shading normal turned against d (not renormalised, as the shade stage holds it), and the keys
// of the material's values (matflags, the reference's `uv`), which fg_material() reads behind the light loop, where the any-hit walks' registers
// are free again.  The hit is recomputed from the entity's record on the wide walk as lit_first_hit does.
struct FgRay { V3 Q, norm; double tu, tv; uint32_t mf; int32_t ent; };
template <int FEAT, class Nodes>
GI_HD bool fg_trace(const Scene& S, const Nodes& N, V3 o, V3 d, const Rng& rng, FgRay& r)
{
    const Ray ray = make_ray_exact(o, d);
    HitRec h;
    h.tu = 0; h.tv = 0;
    if (!trace_nodes<FEAT>(S, N, ray, rng, P_TRACE_ALPHA, h, nullptr)) return false;
    if constexpr (Nodes::kWide) {   // as aov_sample
        const TriGeom& tg = S.tris[h.tri];
        h.mf = ((uint32_t)tg.mat << 3) | tg.flags;
        ent_hit<FEAT>(tg, h.mf, ray, h.u, h.v, h.pos);
    }
    const V3 n = shading_normal(S, h);
    r.norm = dot(n, d) > 0 ? n * -1.0 : n;
    r.Q = h.pos;
    r.mf = h.mf; r.tu = h.tu; r.tv = h.tv;
    r.ent = h.tri;
    return true;
}
// colour and emission of a material at the hit's `uv`, as lit_first_hit takes them
template <int FEAT>
GI_HD void fg_material(const Scene& S, uint32_t mat, double tu, double tv, V3& color, V3& emissive)
{
    const Mat& m = S.mats[mat];
    color = ld3(m.diffuse); emissive = ld3(m.emissive);
    if (FEAT & GI_FEAT_TEX) {
        color = tex_get(S, m.dtex, color, tu, tv);
        emissive = tex_get(S, m.etex, emissive, tu, tv);
    }
}
}  // namespace gi

// One kernel, k_fg<FEAT, WIDE>, of k_ao's shape: one lane per pixel of this rank's rows in the 8x8-tile order of st_pixel_xy; a lane loops over its
// samples and, per sample with a first hit on the diffuse lobe, over the n_dirs gather rays.  It keeps its twelve f64 sums in registers and stores
// once.  No queue, no sort, no atomics, nothing of the path pool, no reduction across lanes: L_j is summed in ascending j and the samples in
// ascending s whatever the launch shape.
// A gather ray is three phases that follow one another -- the closest-hit walk, the light loop's any-hit walks at Q, the look-ups.  The walk hands
// on Q, the turned normal and the material's keys (FgRay); the hit's colour and emission are read behind the light loop, the first hit's again
// behind the loop over j where the material alone gives them, so neither rides through the any-hit walks.  Across the loop over j live O, Nf, the
// RNG key, the running sum, the first hit's direct term and the pixel's sums.  At the 256 registers of a 512-lane workgroup that spills 96 to
// 224 bytes per lane more than k_lit; GI_FG_BLOCK is 256, where a wave may take the whole register file and nothing spills (gi_instances.inc,
// DESIGN.md).
// LDS as k_lit's: the records of the octree's top with the whole entities' content boxes, which the any-hit walks of lit_direct read (NV); the
// closest-hit walks -- the first hit's and the gather rays' -- take the tables cut to the leaves through L2 where the two differ (NT).
// ids [local_rows][w][n][n_dirs] (optional): fg_id per gather ray, GI_FG_ID_NONE for every ray of a sample without a gather.
template <int FEAT, int WIDE>
__global__ __launch_bounds__(GI_FG_BLOCK) void k_fg(Scene S, Frame F, LitArgs A, uint32_t n_pix, int32_t n, int32_t n_dirs, void* out, int out_f64, int32_t* ids)
{
    const typename LdsSrc<WIDE>::type NV = LdsSrc<WIDE>::stage_with_boxes(S);   // ends with a barrier
    typename LdsSrc<WIDE>::type NT = NV;                                        // the closest-hit walks' view of the same records
    if constexpr (WIDE != 0) {
        if (S.tcboxes != S.cboxes || S.tcuse != S.cuse) { NT.cboxes = S.tcboxes; NT.cuse = S.tcuse; NT.n_lc = 0; }
    }
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pix) return;
    int x, ly;
    st_pixel_xy(F, p, x, ly);
    uint32_t idx = halton_index(F.he, 0u, (uint32_t)x, (uint32_t)global_row(F, ly));
    const size_t pix = (size_t)ly * F.w + x;
    FgLook K;
    K.sh = A.sh; K.n3 = A.n3; K.gmin = A.gmin; K.gmax = A.gmax; K.chain = A.chain; K.level_of_mat = A.level_of_mat; K.face = A.face; K.level_off = A.level_off;
    V3 sum[4] = {v3(0, 0, 0), v3(0, 0, 0), v3(0, 0, 0), v3(0, 0, 0)};   // beauty, direct, diffuse, specular
    for (int32_t s = 0; s < n; s++, idx += F.he.inc) {
        int32_t* const id = ids ? ids + (pix * (size_t)n + (size_t)s) * (size_t)n_dirs : nullptr;
        LitHit a;
        Rng rng;
        const bool hit = lit_first_hit<FEAT>(S, NT, F, F.seed, idx, rng, a);
        const bool gather = hit && !(a.roughness < .9) && (A.terms & GI_BAKED_DIFFUSE);
        if (id && !gather)
            for (int32_t j = 0; j < n_dirs; j++) id[j] = GI_FG_ID_NONE;
        if (!hit) { sum[0] = sum[0] + ld3(S.ambient); continue; }   // a miss: the ambient term, no share of the three
        V3 direct = v3(0, 0, 0), diffuse = v3(0, 0, 0), specular = v3(0, 0, 0);
        if (A.terms & GI_BAKED_DIRECT) direct = a.color * lit_direct<FEAT | GI_FEAT_FOG>(S, NV, a.P, a.norm, a.roughness, rng);
        if (a.roughness < .9) {             // mirror or glossy: k_lit's specular term, no gather
            if (A.terms & GI_BAKED_SPECULAR) {
                const uint32_t l = a.roughness < .001 ? 0u : (uint32_t)A.level_of_mat[a.mat];
                const size_t t = (size_t)A.level_off[l] + cube_texel(reflect(a.d, a.nf), A.face >> l);
                specular = a.color * ld3(A.chain + t * 3);
            }
        } else if (gather) {
            // across the loop live O, Nf, the RNG key, the running sum, the first hit's direct term and the pixel's sums; its colour and emission
            // are read again behind the loop where the material alone gives them (no textures)
            const V3 o = a.P + GI_SHADOW_BIAS * a.nf, nf = a.nf;
            const int32_t mat0 = a.mat;
            V3 acc = v3(0, 0, 0);
            for (int32_t j = 0; j < n_dirs; j++) {
                const float u = (float)rng_draw(rng, P_FG_U, (uint32_t)j);
                const float v = (float)rng_draw(rng, P_FG_V, (uint32_t)j);
                const V3 d = hemi_cos_n(nf, u, v, 2);
                Rng rj = rng;
                rj.depth = 1u + (uint32_t)j;
                FgRay r;
                r.ent = -1;
                const bool qhit = fg_trace<FEAT>(S, NT, o, d, rj, r);
                if (id) id[j] = fg_id(qhit, r.ent);
                if (!qhit) { acc = fg_add(acc, ld3(S.ambient)); continue; }
                FgHit q;
                q.mat = (int32_t)(r.mf >> 3);
                q.roughness = S.mats[q.mat].roughness;
                const V3 i = lit_direct<FEAT | GI_FEAT_FOG>(S, NV, r.Q, r.norm, q.roughness, rj);
                fg_material<FEAT>(S, (uint32_t)q.mat, r.tu, r.tv, q.color, q.emissive);
                q.Q = r.Q; q.nf = normalize(r.norm);
                acc = fg_add(acc, fg_secondary(K, q, d, i));
            }
            if constexpr (!(FEAT & GI_FEAT_TEX)) fg_material<FEAT>(S, (uint32_t)mat0, 0, 0, a.color, a.emissive);
            diffuse = fg_diffuse(a.color, acc, n_dirs);
        }
        const V3 beauty = ((direct + diffuse) + specular) + ((A.terms & GI_BAKED_EMISSIVE) ? a.emissive : v3(0, 0, 0));
        sum[0] = sum[0] + beauty; sum[1] = sum[1] + direct; sum[2] = sum[2] + diffuse; sum[3] = sum[3] + specular;
    }
    const size_t o = pix * 12;
    const double dn = (double)n;
    GI_UNROLL
    for (int k = 0; k < 4; k++) {
        const V3 v = sum[k] / dn;
        if (out_f64) { double* q = (double*)out + o + k * 3; q[0] = v.x; q[1] = v.y; q[2] = v.z; }
        else { float* q = (float*)out + o + k * 3; q[0] = (float)v.x; q[1] = (float)v.y; q[2] = (float)v.z; }
    }
}

namespace {

// false + message when the parameters and pointers are not the header's: lit_check's on the baked block -- with a chain given, its face, levels and
// exponents are checked whether GI_BAKED_SPECULAR is set or not, because secondary hits read it -- then n_dirs and the reserved field
bool fg_check(const gi_final_gather_params* p, const void* sh, const void* chain, std::string& err)
{
    if (!p) { err = "render_final_gather: null parameters"; return false; }
    gi_baked_params bp = p->baked;
    if (chain && bp.terms != 0 && !(bp.terms & ~GI_BAKED_ALL_TERMS)) bp.terms |= GI_BAKED_SPECULAR;
    if (!lit_check(&bp, sh, chain, err)) { err = lit_named(err, "render_final_gather"); return false; }
    if (p->n_dirs < 1 || p->n_dirs > GI_FG_MAX_DIRS) { err = "render_final_gather: n_dirs must be 1 .. " + std::to_string(GI_FG_MAX_DIRS) + ", got " + std::to_string(p->n_dirs); return false; }
    if (p->reserved != 0) { err = "render_final_gather: reserved must be 0, got " + std::to_string(p->reserved); return false; }
    return true;
}

}  // namespace

extern "C" {

void gi_final_gather_default_params(gi_final_gather_params* p)
{
    if (!p) return;
    gi_baked_default_params(&p->baked);
    p->baked.terms = GI_BAKED_DIRECT | GI_BAKED_DIFFUSE | GI_BAKED_EMISSIVE;
    p->n_dirs = 16; p->reserved = 0;
}

int gi_render_final_gather_device(gi_ctx* c, const gi_render_params* p, const gi_final_gather_params* fp, const double* d_sh, const double* d_chain, void* d_out, int out_is_f64, int32_t* d_ids)
{
    if (!c) return GI_E_INVALID;
    if (!p || !d_out) return fail(c, GI_E_INVALID, "render_final_gather: null frame parameters or output pointer");
    std::string err;
    if (!fg_check(fp, d_sh, d_chain, err)) return fail(c, GI_E_INVALID, err);
    Frame F;
    if (const int rc = pixel_pass_frame(c, "render_final_gather", p, F)) return rc;
    const gi_baked_params* bp = &fp->baked;
    if (const int rc = pixel_pass_cap(c, "render_final_gather", F, bp->n_samples)) return rc;      // the last refusal, before the table is touched
    LitArgs A{};
    A.terms = bp->terms;
    A.n3[0] = bp->nx; A.n3[1] = bp->ny; A.n3[2] = bp->nz;
    for (int k = 0; k < 3; k++) { A.gmin[k] = bp->grid_min[k]; A.gmax[k] = bp->grid_max[k]; }
    A.sh = (bp->terms & GI_BAKED_DIFFUSE) ? d_sh : nullptr; A.chain = d_chain;
    if (d_chain)        // the level every material reads: here whenever there is a chain, in a table of the pass's own
        if (const int rc = lit_level_table(c, bp, c->fg.d_levels, A)) return rc;
    return pixel_pass(c, c->fg, "render_final_gather", F, bp->n_samples, kFg, GI_FG_BLOCK, [&](const FgK& k, dim3 grid, dim3 block, uint32_t n_pix) {
        hipLaunchKernelGGL(k.fn, grid, block, k.lds, c->stream, c->S, F, A, n_pix, bp->n_samples, fp->n_dirs, d_out, out_is_f64, d_ids);
    });
}

int gi_render_final_gather_host(gi_ctx* c, const gi_render_params* p, const gi_final_gather_params* fp, const double* sh, const double* chain, void* h_out, int out_is_f64, int32_t* h_ids)
{
    if (!c) return GI_E_INVALID;
    if (!p || !h_out) return fail(c, GI_E_INVALID, "render_final_gather: null frame parameters or output pointer");
    std::string err;
    if (!fg_check(fp, sh, chain, err)) return fail(c, GI_E_INVALID, err);
    Frame F;
    if (const int rc = pixel_pass_frame(c, "render_final_gather", p, F)) return rc;      // the frame is checked before anything is sized by it
    const gi_baked_params* bp = &fp->baked;
    if (const int rc = pixel_pass_cap(c, "render_final_gather", F, bp->n_samples)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf<double> d_sh, d_chain;
    DevBuf<unsigned char> d_out;
    DevBuf<int32_t> d_ids;
    if (bp->terms & GI_BAKED_DIFFUSE) HIP_TRY(c, d_sh.upload(sh, (size_t)bp->nx * (size_t)bp->ny * (size_t)bp->nz * 27));
    if (chain) HIP_TRY(c, d_chain.upload(chain, cm_texels_before(bp->face, bp->levels) * 3));
    const size_t npix = (size_t)F.local_rows * (size_t)F.w;
    const size_t bytes = npix * 12 * (out_is_f64 ? 8 : 4), n_ids = npix * (size_t)bp->n_samples * (size_t)fp->n_dirs;
    HIP_TRY(c, d_out.alloc(bytes));
    if (h_ids && n_ids) HIP_TRY(c, d_ids.alloc(n_ids));
    if (const int rc = gi_render_final_gather_device(c, p, fp, d_sh.p, d_chain.p, (void*)d_out.p, out_is_f64, d_ids.p)) return rc;
    // one end for both results: a copy that fails leaves the time unreported, as in every host-pointer pass
    return finish_to_host(c, "render_final_gather_host", {{h_out, d_out.p, bytes}, to_host(h_ids, d_ids, n_ids)}, &c->fg.timer);
}

int gi_last_final_gather_ms(gi_ctx* c, float* ms) { return pass_ms(c, &gi_ctx::fg, ms); }

}  // extern "C"
