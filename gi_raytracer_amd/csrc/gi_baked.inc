// gi_baked.inc -- the baked-light pass (gi_render_baked_*; an addition: the consumer of the bakes).  Included by gi_kernels.hip behind gi_cubemap.inc,
// whose gi_cubemap.h gives the cube's texel order; the host frame of a per-pixel pass is gi_features.inc's (pixel_pass_frame, pixel_pass,
// pixel_pass_to_host).  The definition is stated in include/gi_hip.h; the per-lane functions are gi_baked.h, and lit_first_hit() stands here with
// what a lane carries from it.

namespace gi {
#include "gi_baked.h"
#include "gi_visibility.h"      // probe visibility: the PV instances' step 4 (pv_irradiance), and what gi_visibility.inc captures the maps with
#include "gi_reflections.h"     // reflection probe sets: the RS instances' step 5 (rs_specular); the entries are gi_reflections.inc's

// ------------------------------------------------------------------------------------------------ baked light at the first hit (an addition: the reference has no such pass)
// The first hit of the sample with Halton index idx: aov_sample's (same ray, same RNG keys, same recomputation of the hit from the entity's record on
// the wide walk), and from it what the three later steps need.  norm is the shade stage's normal (secondary_ray turns it, nothing renormalises it),
// nf ao_first_hit's.
struct LitHit { V3 P, d, norm, nf, color, emissive; double roughness; int32_t mat; };   // mat: under LM, on the diffuse lobe, the ENTITY instead (the lobe needs one of the two)
template <int FEAT, int LM = 0, class Nodes>
GI_HD bool lit_first_hit(const Scene& S, const Nodes& N, const Frame& F, uint64_t seed, uint32_t idx, Rng& rng, LitHit& a)
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
    const Mat& m = S.mats[h.mf >> 3];
    a.color = ld3(m.diffuse); a.emissive = ld3(m.emissive);
    if (FEAT & GI_FEAT_TEX) {
        a.color = tex_get(S, m.dtex, a.color, h.tu, h.tv);
        a.emissive = tex_get(S, m.etex, a.emissive, h.tu, h.tv);
    }
    const V3 n = shading_normal(S, h);
    a.norm = dot(n, ray.d) > 0 ? n * -1.0 : n;
    const V3 nh = normalize(n);
    a.nf = dot(nh, ray.d) > 0 ? v3(-nh.x, -nh.y, -nh.z) : nh;
    a.P = h.pos; a.d = ray.d;
    a.roughness = m.roughness; a.mat = (int32_t)(h.mf >> 3);
    if constexpr (LM != 0) { if (!(m.roughness < .9)) a.mat = h.tri; }
    return true;
}
}  // namespace gi

// What the kernel reads beside the scene: the probe grid, the chain and the level each material reads, through global memory (small, L2-resident);
// the lightmap instances (LM) also the atlas, the chart and the row that serves each entity, the same way.
struct LitArgs {
    int32_t terms;                                  // GI_BAKED_*
    int32_t n3[3];                                  // nx, ny, nz
    double gmin[3], gmax[3];
    const double* sh;                               // [nz][ny][nx][9][3]
    const double* chain;                            // the whole chain, [texels][3]
    const int32_t* level_of_mat;                    // [n_mat]
    uint32_t face;
    uint32_t level_off[GI_CUBEMAP_MAX_LEVELS];      // texels before level l
    const struct LitLm* lm;                         // gi_render_baked_lightmap_*: read by the LM instances only
    const double* vis;                              // gi_render_baked_visibility_*: the probes' maps [nz][ny][nx][M][M][2], read by the PV instances only
    int32_t vis_size;                               //   M
    double normal_bias, vis_floor;                  //   gi_baked_visibility_params
    const double* rs_probes;                        // gi_render_baked_reflections_*: the set's table [K][10], read by the RS instances only
    const double* rs_chains;                        //   its chains [K][rs_texels][3]
    int32_t rs_n;                                   //   K
    uint32_t rs_texels;                             //   texels of one chain
};
// the lightmap of a call, in device memory (written by k_lm_rows): one pointer among the kernel's arguments, read where the look-up happens
struct LitLm {
    int32_t w, h, filter;                           // the atlas's size, GI_LM_*
    const double* atlas;                            // [h][w][3]
    const double* uv;                               // the chart's coordinates, [n_chart][3][2]
    const int* row_of_ent;                          // [n_tri]: the lowest chart row of the entity, GI_LM_NONE where it has none
};

// row_of_ent of a chart: one lane per chart row, the lowest row index of every entity by a 32-bit atomicMin on a table preset to GI_LM_NONE, as
// k_lm_raster decides a texel's owner -- the minimum does not depend on the order of the atomics.  Rows that name no entity of the scene, or a
// sphere, serve nothing.  Lane 0 also leaves the call's LitLm for k_lit.
__global__ __launch_bounds__(GI_BLOCK) void k_lm_rows(Scene S, int32_t n_chart, const int32_t* ent, int* row_of_ent, LitLm lm, LitLm* lm_out)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j == 0u) *lm_out = lm;
    if (j >= (uint32_t)n_chart) return;
    const int32_t e = ent[j];
    if (e < 0 || e >= S.n_tri || (S.tris[e].flags & 4u)) return;
    atomicMin(row_of_ent + e, (int)j);
}

// One kernel, k_lit<FEAT, WIDE, LM>, of k_ao's shape: one lane per pixel of this rank's rows in the 8x8-tile order of st_pixel_xy, a lane loops over its
// samples; per sample the first hit, then one any-hit walk per light from the last light down until one is visible, then the look-ups.  It keeps its
// twelve f64 sums in registers and stores once.  No queue, no sort, no atomics, nothing of the path pool, no reduction across lanes.
// The three steps of a sample follow one another with little carried across: ray, hit record and entity record are dead when the light loop starts
// (LitHit is what lives on), the walk's state is dead when the look-ups start, so the register need is that of the largest step, not the sum.
// LDS as k_ao's: the records of the octree's top with the whole entities' content boxes, which the any-hit walks read; the closest-hit walk takes the
// tables cut to the leaves through L2 where the two differ.  A light's segment ends at the light, but the boxes are the whole entities'
// (Scene::leaf_boxes), valid for any segment: the answers are those of k_st_shadow's cut boxes.
// LM (gi_render_baked_lightmap_*): a diffuse-lobe hit on an entity with a chart row reads the atlas at the hit's chart coordinate instead of the
// grid; one without a row reads the grid if there is one.  The look-up stands where the grid's does, behind the walks: no LDS, no atomics and no
// step across lanes are added, and the LM = 0 instances carry none of it.
// PV (gi_render_baked_visibility_*): the grid's look-up weights its eight probes by their octahedral depth maps (pv_irradiance, gi_visibility.h)
// instead of interpolating them trilinearly; it stands where the grid's does, reads the maps through global memory as it reads the probes, and
// adds no LDS, no atomics and no step across lanes.  The PV = 0 instances carry none of it; LM and PV are not combined.
// RS (gi_render_baked_reflections_*): the specular term blends the probes of a set whose boxes contain the hit, each cube read at the direction
// from the probe to where the reflection ray leaves its box (rs_specular, gi_reflections.h), instead of reading one chain at R.  It stands where
// step 5 stands, behind the walks.  The loop over the probes has the same trip count and the same table addresses in every lane, so the table's
// rows come through the scalar cache; a chain's texel is a lane's own read through global memory, as the one chain's is.  No LDS, no atomics and
// no step across lanes are added, and the RS = 0 instances carry none of it; RS goes with LM = PV = 0 only.
template <int FEAT, int WIDE, int LM, int PV, int RS>
__global__ __launch_bounds__(GI_LIT_BLOCK) void k_lit(Scene S, Frame F, LitArgs A, uint32_t n_pix, int32_t n, void* out, int out_f64)
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
    V3 sum[4] = {v3(0, 0, 0), v3(0, 0, 0), v3(0, 0, 0), v3(0, 0, 0)};   // beauty, direct, diffuse, specular
    for (int32_t s = 0; s < n; s++, idx += F.he.inc) {
        LitHit a;
        Rng rng;
        if (!lit_first_hit<FEAT, LM>(S, NT, F, F.seed, idx, rng, a)) { sum[0] = sum[0] + ld3(S.ambient); continue; }   // a miss: the ambient term, no share of the three
        V3 direct = v3(0, 0, 0), diffuse = v3(0, 0, 0), specular = v3(0, 0, 0);
        if (A.terms & GI_BAKED_DIRECT) direct = a.color * lit_direct<FEAT | GI_FEAT_FOG>(S, NV, a.P, a.norm, a.roughness, rng);
        if (a.roughness < .9) {             // mirror (< .001: level 0) or glossy (the material's level): specular only
            if (A.terms & GI_BAKED_SPECULAR) {
                const uint32_t l = a.roughness < .001 ? 0u : (uint32_t)A.level_of_mat[a.mat];
                if constexpr (RS != 0)
                    specular = a.color * rs_specular(A.rs_probes, A.rs_chains, A.rs_n, A.rs_texels, A.level_off[l], A.face >> l, a.P, reflect(a.d, a.nf));
                else {
                    const size_t t = (size_t)A.level_off[l] + cube_texel(reflect(a.d, a.nf), A.face >> l);
                    specular = a.color * ld3(A.chain + t * 3);
                }
            }
        } else if (A.terms & GI_BAKED_DIFFUSE) {
            if constexpr (LM != 0) {
                const LitLm& L = *A.lm;
                const int32_t row = L.row_of_ent[a.mat];      // the entity: lit_first_hit
                if (row != GI_LM_NONE) {
                    const LmCoord uv = lm_coord(S.tris[a.mat], a.P, L.uv + (size_t)row * 6);
                    diffuse = a.color * (L.filter == GI_LM_NEAREST ? lm_nearest(L.atlas, L.w, L.h, uv) : lm_bilinear(L.atlas, L.w, L.h, uv));
                } else if (A.sh)
                    diffuse = a.color * grid_irradiance(A.sh, A.n3, A.gmin, A.gmax, a.P, a.nf);
            } else if constexpr (PV != 0)
                diffuse = a.color * pv_irradiance(A.sh, A.vis, A.vis_size, A.n3, A.gmin, A.gmax, a.P, a.nf, A.normal_bias, A.vis_floor);
            else
                diffuse = a.color * grid_irradiance(A.sh, A.n3, A.gmin, A.gmax, a.P, a.nf);
        }
        const V3 beauty = ((direct + diffuse) + specular) + ((A.terms & GI_BAKED_EMISSIVE) ? a.emissive : v3(0, 0, 0));
        sum[0] = sum[0] + beauty; sum[1] = sum[1] + direct; sum[2] = sum[2] + diffuse; sum[3] = sum[3] + specular;
    }
    const size_t o = ((size_t)ly * F.w + x) * 12;
    const double dn = (double)n;
    GI_UNROLL
    for (int k = 0; k < 4; k++) {
        const V3 v = sum[k] / dn;
        if (out_f64) { double* q = (double*)out + o + k * 3; q[0] = v.x; q[1] = v.y; q[2] = v.z; }
        else { float* q = (float*)out + o + k * 3; q[0] = (float)v.x; q[1] = (float)v.y; q[2] = (float)v.z; }
    }
}

namespace {

#define GI_BAKED_ALL_TERMS (GI_BAKED_DIRECT | GI_BAKED_DIFFUSE | GI_BAKED_SPECULAR | GI_BAKED_EMISSIVE)

// false + message when the parameters and pointers are not the header's
bool lit_check(const gi_baked_params* p, const void* sh, const void* chain, std::string& err)
{
    if (!p) { err = "render_baked: null parameters"; return false; }
    if (p->n_samples < 1) { err = "render_baked: n_samples must be at least 1, got " + std::to_string(p->n_samples); return false; }
    if (p->terms == 0 || (p->terms & ~GI_BAKED_ALL_TERMS)) { err = "render_baked: terms must be a non-empty set of GI_BAKED_DIRECT, _DIFFUSE, _SPECULAR and _EMISSIVE, got " + std::to_string(p->terms); return false; }
    if (p->nx < 1 || p->ny < 1 || p->nz < 1) { err = "render_baked: every grid dimension must be at least 1, got " + std::to_string(p->nx) + " x " + std::to_string(p->ny) + " x " + std::to_string(p->nz); return false; }
    if ((unsigned long long)p->nx * (unsigned long long)p->ny > (1ull << 31) || (unsigned long long)p->nx * (unsigned long long)p->ny * (unsigned long long)p->nz > (1ull << 31)) {
        err = "render_baked: more than 2^31 probes";
        return false;
    }
    if (p->terms & GI_BAKED_DIFFUSE) {
        if (!sh) { err = "render_baked: the diffuse term needs the probe grid"; return false; }
        for (int k = 0; k < 3; k++)
            if (!std::isfinite(p->grid_min[k]) || !std::isfinite(p->grid_max[k]) || !(p->grid_max[k] > p->grid_min[k])) { err = "render_baked: the grid box must be finite with grid_max > grid_min on every axis"; return false; }
    }
    if (p->terms & GI_BAKED_SPECULAR) {
        if (!chain) { err = "render_baked: the specular term needs the chain"; return false; }
        if (p->face < 1 || p->face > GI_CM_MAX_FACE) { err = "render_baked: face must be 1 .. " + std::to_string(GI_CM_MAX_FACE) + ", got " + std::to_string(p->face); return false; }
        if (p->levels < 1 || p->levels > GI_CUBEMAP_MAX_LEVELS) { err = "render_baked: levels must be 1 .. " + std::to_string(GI_CUBEMAP_MAX_LEVELS) + ", got " + std::to_string(p->levels); return false; }
        if (p->face & ((1 << (p->levels - 1)) - 1)) { err = "render_baked: " + std::to_string(p->levels) + " levels need a face divisible by " + std::to_string(1 << (p->levels - 1)) + ", got " + std::to_string(p->face); return false; }
        for (int l = 1; l < p->levels; l++)
            if (p->log2_exponent[l] < 0 || p->log2_exponent[l] > 16) { err = "render_baked: log2_exponent[" + std::to_string(l) + "] must be 0 .. 16, got " + std::to_string(p->log2_exponent[l]); return false; }
    }
    return true;
}

// The chain's layout and the level every material reads, into A: face, the texels before each level, and the table [n_mat] in `d_levels` (a pass's
// own, sized on first use and kept), made per call from the roughnesses kept at upload (baked_level_of: no transcendental on the device).  It waits
// for the stream first: an earlier pass on it may still read the table.
int lit_level_table(gi_ctx* c, const gi_baked_params* bp, DevBuf<int32_t>& d_levels, LitArgs& A)
{
    A.face = (uint32_t)bp->face;
    for (int l = 0; l < bp->levels; l++) A.level_off[l] = (uint32_t)cm_texels_before(bp->face, l);
    std::vector<int32_t> levels(c->scene.mat_roughness.size());
    for (size_t m = 0; m < levels.size(); m++) levels[m] = baked_level_of(c->scene.mat_roughness[m], bp->levels, bp->log2_exponent);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (d_levels.n < levels.size()) HIP_TRY(c, d_levels.alloc(levels.size()));
    if (!levels.empty()) HIP_TRY(c, hipMemcpy(d_levels.p, levels.data(), levels.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    A.level_of_mat = d_levels.p;
    return GI_OK;
}

// The pass itself on checked arguments: LitArgs from the parameters, the level table, the one launch.  terms: bp->terms, or fewer bits.  lm: null, or
// a LitArgs whose `lm` points at the call's LitLm, which selects the LM instances, or one whose `vis` points at the probes' maps (with vis_size,
// normal_bias and vis_floor), which selects the PV instances, or one whose `rs_probes` points at a probe set's table (with rs_chains, rs_n and
// rs_texels), which selects the RS instances.
int lit_run(gi_ctx* c, const char* name, const Frame& F, const gi_baked_params* bp, int32_t terms, const double* d_sh, const double* d_chain, const LitArgs* lm, void* d_out, int out_is_f64)
{
    LitArgs A{};
    if (lm) A = *lm;
    A.terms = terms;
    A.n3[0] = bp->nx; A.n3[1] = bp->ny; A.n3[2] = bp->nz;
    for (int k = 0; k < 3; k++) { A.gmin[k] = bp->grid_min[k]; A.gmax[k] = bp->grid_max[k]; }
    A.sh = d_sh; A.chain = d_chain;
    if (terms & GI_BAKED_SPECULAR)
        if (const int rc = lit_level_table(c, bp, c->lit.d_levels, A)) return rc;
    const auto launch = [&](const LitK& k, dim3 grid, dim3 block, uint32_t n_pix) {
        hipLaunchKernelGGL(k.fn, grid, block, k.lds, c->stream, c->S, F, A, n_pix, bp->n_samples, d_out, out_is_f64);
    };
    if (!lm) return pixel_pass(c, c->lit, name, F, bp->n_samples, kLit, GI_LIT_BLOCK, launch);
    if (lm->lm) return pixel_pass(c, c->lit, name, F, bp->n_samples, kLitLm, GI_LIT_BLOCK, launch);
    return lm->rs_probes ? pixel_pass(c, c->lit, name, F, bp->n_samples, kLitRs, GI_LIT_BLOCK, launch) : pixel_pass(c, c->lit, name, F, bp->n_samples, kLitPv, GI_LIT_BLOCK, launch);
}

// ---- gi_render_baked_lightmap_*
// lit_check's message under this entry's name
std::string lit_named(const std::string& err, const char* entry) { return err.compare(0, 13, "render_baked:") == 0 ? std::string(entry) + ":" + err.substr(13) : err; }
std::string lm_named(const std::string& err) { return lit_named(err, "render_baked_lightmap"); }
// false + message when the lightmap's parameters and pointers are not the header's (behind lit_check, which has seen bp)
bool lit_lm_check(const gi_baked_params* bp, const gi_baked_lightmap_params* lp, const void* atlas, const void* ent, const void* uv, std::string& err)
{
    if (!lp) { err = "render_baked_lightmap: null lightmap parameters"; return false; }
    if (lp->width < 1 || lp->width > 8192 || lp->height < 1 || lp->height > 8192) { err = "render_baked_lightmap: width and height must be 1 .. 8192, got " + std::to_string(lp->width) + " x " + std::to_string(lp->height); return false; }
    if (lp->filter != GI_LM_NEAREST && lp->filter != GI_LM_BILINEAR) { err = "render_baked_lightmap: filter must be GI_LM_NEAREST or GI_LM_BILINEAR, got " + std::to_string(lp->filter); return false; }
    if (lp->n_chart < 0) { err = "render_baked_lightmap: n_chart must not be negative, got " + std::to_string(lp->n_chart); return false; }
    if (lp->n_chart > 0 && (bp->terms & GI_BAKED_DIFFUSE) && (!atlas || !ent || !uv)) { err = "render_baked_lightmap: the diffuse term of a chart needs the atlas, ent and uv"; return false; }
    return true;
}
// a chart with rows and the diffuse term: the look-up takes part; else the pass is gi_render_baked_*'s, bit for bit
bool lit_lm_active(const gi_baked_params* bp, const gi_baked_lightmap_params* lp) { return lp->n_chart > 0 && (bp->terms & GI_BAKED_DIFFUSE); }

}  // namespace

extern "C" {

void gi_baked_default_params(gi_baked_params* p)
{
    if (!p) return;
    p->n_samples = 4; p->terms = GI_BAKED_DIRECT | GI_BAKED_EMISSIVE;
    for (int k = 0; k < 3; k++) { p->grid_min[k] = 0.0; p->grid_max[k] = 1.0; }
    p->nx = p->ny = p->nz = 1;
    p->face = 32; p->levels = 1;
    for (int l = 0; l < GI_CUBEMAP_MAX_LEVELS; l++) p->log2_exponent[l] = std::max(0, 16 - 3 * l);
}

int gi_render_baked_device(gi_ctx* c, const gi_render_params* p, const gi_baked_params* bp, const double* d_sh, const double* d_chain, void* d_out, int out_is_f64)
{
    if (!c) return GI_E_INVALID;
    if (!p || !d_out) return fail(c, GI_E_INVALID, "render_baked: null frame parameters or output pointer");
    std::string err;
    if (!lit_check(bp, d_sh, d_chain, err)) return fail(c, GI_E_INVALID, err);
    Frame F;
    if (const int rc = pixel_pass_frame(c, "render_baked", p, F)) return rc;
    return lit_run(c, "render_baked", F, bp, bp->terms, d_sh, d_chain, nullptr, d_out, out_is_f64);
}

int gi_render_baked_host(gi_ctx* c, const gi_render_params* p, const gi_baked_params* bp, const double* sh, const double* chain, void* h_out, int out_is_f64)
{
    if (!c) return GI_E_INVALID;
    if (!p || !h_out) return fail(c, GI_E_INVALID, "render_baked: null frame parameters or output pointer");
    std::string err;
    if (!lit_check(bp, sh, chain, err)) return fail(c, GI_E_INVALID, err);
    if (!c->scene.have_scene) return fail(c, GI_E_STATE, "render_baked: no scene uploaded");
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf<double> d_sh, d_chain;
    if (bp->terms & GI_BAKED_DIFFUSE) HIP_TRY(c, d_sh.upload(sh, (size_t)bp->nx * (size_t)bp->ny * (size_t)bp->nz * 27));
    if (bp->terms & GI_BAKED_SPECULAR) HIP_TRY(c, d_chain.upload(chain, cm_texels_before(bp->face, bp->levels) * 3));
    return pixel_pass_to_host(c, c->lit, "render_baked_host", p, 12, h_out, out_is_f64, nullptr,
                              [&](void* d_out, int32_t*) { return gi_render_baked_device(c, p, bp, d_sh.p, d_chain.p, d_out, out_is_f64); });
}

int gi_last_baked_ms(gi_ctx* c, float* ms) { return pass_ms(c, &gi_ctx::lit, ms); }

void gi_baked_lightmap_default_params(gi_baked_lightmap_params* p)
{
    if (!p) return;
    p->width = 256; p->height = 256; p->filter = GI_LM_BILINEAR; p->n_chart = 0;
}

int gi_render_baked_lightmap_device(gi_ctx* c, const gi_render_params* p, const gi_baked_params* bp, const gi_baked_lightmap_params* lp, const double* d_sh, const double* d_chain,
                                    const double* d_atlas, const int32_t* d_ent, const double* d_uv, void* d_out, int out_is_f64)
{
    if (!c) return GI_E_INVALID;
    if (!p || !d_out) return fail(c, GI_E_INVALID, "render_baked_lightmap: null frame parameters or output pointer");
    std::string err;
    // sh may be null with the diffuse term: hits without a chart row then have no diffuse term (lit_check asks only whether sh is null)
    if (!lit_check(bp, (bp && !d_sh) ? (const void*)bp : (const void*)d_sh, d_chain, err)) return fail(c, GI_E_INVALID, lm_named(err));
    if (!lit_lm_check(bp, lp, d_atlas, d_ent, d_uv, err)) return fail(c, GI_E_INVALID, err);
    Frame F;
    if (const int rc = pixel_pass_frame(c, "render_baked_lightmap", p, F)) return rc;
    if (!lit_lm_active(bp, lp))      // no row serves anything: the LM = 0 instances; without a grid the diffuse term is +0.0 everywhere, as with its bit clear
        return lit_run(c, "render_baked_lightmap", F, bp, d_sh ? bp->terms : (bp->terms & ~GI_BAKED_DIFFUSE), d_sh, d_chain, nullptr, d_out, out_is_f64);
    HIP_TRY(c, hipSetDevice(c->device));
    LitPass& lit = c->lit;
    if (lit.lds_refused < 0) { lit.lds_refused = 0; ask_for_lds(kLit, lit.lds_refused); }       // (pixel_pass would take the LM table's answer for this one)
    if (lit.lm_lds_refused < 0) { lit.lm_lds_refused = 0; ask_for_lds(kLitLm, lit.lm_lds_refused); }
    if (lit.lm_lds_refused) return fail(c, GI_E_HIP, "render_baked_lightmap: the device refused " + std::to_string(lit.lm_lds_refused) + " bytes of dynamic LDS per workgroup");
    // row_of_ent, rebuilt per call on the stream, behind whatever pass still reads the last one
    const size_t n_ent = (size_t)std::max(c->S.n_tri, 0);
    if (lit.d_lm_rows.n < n_ent || !lit.d_lm_rows.p) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, lit.d_lm_rows.alloc(n_ent));
    }
    if (!lit.d_lm.p) HIP_TRY(c, lit.d_lm.alloc(1));
    if (n_ent) HIP_TRY(c, hipMemsetD32Async((hipDeviceptr_t)lit.d_lm_rows.p, GI_LM_NONE, n_ent, c->stream));
    LitLm desc{};
    desc.w = lp->width; desc.h = lp->height; desc.filter = lp->filter;
    desc.atlas = d_atlas; desc.uv = d_uv; desc.row_of_ent = lit.d_lm_rows.p;
    hipLaunchKernelGGL(k_lm_rows, GI_GRID((size_t)lp->n_chart), 0, c->stream, c->S, lp->n_chart, d_ent, lit.d_lm_rows.p, desc, lit.d_lm.p);
    HIP_TRY(c, hipGetLastError());
    LitArgs lm{};
    lm.lm = lit.d_lm.p;
    return lit_run(c, "render_baked_lightmap", F, bp, bp->terms, d_sh, d_chain, &lm, d_out, out_is_f64);
}

int gi_render_baked_lightmap_host(gi_ctx* c, const gi_render_params* p, const gi_baked_params* bp, const gi_baked_lightmap_params* lp, const double* sh, const double* chain,
                                  const void* atlas, int atlas_is_f64, const int32_t* ent, const double* uv, void* h_out, int out_is_f64)
{
    if (!c) return GI_E_INVALID;
    if (!p || !h_out) return fail(c, GI_E_INVALID, "render_baked_lightmap: null frame parameters or output pointer");
    std::string err;
    if (!lit_check(bp, (bp && !sh) ? (const void*)bp : (const void*)sh, chain, err)) return fail(c, GI_E_INVALID, lm_named(err));
    if (!lit_lm_check(bp, lp, atlas, ent, uv, err)) return fail(c, GI_E_INVALID, err);
    if (!c->scene.have_scene) return fail(c, GI_E_STATE, "render_baked_lightmap: no scene uploaded");
    const bool active = lit_lm_active(bp, lp);
    if (active && !lm_chart_ok(c, lp->n_chart, ent, uv, err)) return fail(c, GI_E_INVALID, "render_baked_" + err);      // ("lightmap: chart row ...")
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf<double> d_sh, d_chain, d_atlas, d_uv;
    DevBuf<int32_t> d_ent;
    if ((bp->terms & GI_BAKED_DIFFUSE) && sh) HIP_TRY(c, d_sh.upload(sh, (size_t)bp->nx * (size_t)bp->ny * (size_t)bp->nz * 27));
    if (bp->terms & GI_BAKED_SPECULAR) HIP_TRY(c, d_chain.upload(chain, cm_texels_before(bp->face, bp->levels) * 3));
    if (active) {
        const size_t n = (size_t)lp->width * (size_t)lp->height * 3;
        if (atlas_is_f64) HIP_TRY(c, d_atlas.upload((const double*)atlas, n));
        else {                                                // widened here, exactly: the device reads f64
            std::vector<double> wide(n);
            for (size_t i = 0; i < n; i++) wide[i] = (double)((const float*)atlas)[i];
            HIP_TRY(c, d_atlas.upload(wide));
        }
        HIP_TRY(c, d_ent.upload(ent, (size_t)lp->n_chart)); HIP_TRY(c, d_uv.upload(uv, (size_t)lp->n_chart * 6));
    }
    return pixel_pass_to_host(c, c->lit, "render_baked_lightmap_host", p, 12, h_out, out_is_f64, nullptr, [&](void* d_out, int32_t*) {
        return gi_render_baked_lightmap_device(c, p, bp, lp, d_sh.p, d_chain.p, d_atlas.p, d_ent.p, d_uv.p, d_out, out_is_f64);
    });
}

}  // extern "C"
