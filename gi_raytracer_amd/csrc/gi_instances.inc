// gi_instances.inc -- the instances of the kernels that take dynamic LDS, and the selectors that pick the one a launch runs.  Host code only;
// included by gi_kernels.hip behind gi_context.inc.  Every instance of a family is named once, in its table (FEAT = scene_feat / scene_trace_feat,
// gi_scene.h); stream_grids (gi_stream.inc) and the per-pixel passes walk the same tables when they ask for the LDS.

// The three per-pixel passes' kernels stand with their entries (gi_features.inc, gi_occlusion.inc, gi_baked.inc), behind this file; so does the
// per-texel capture of the probes' visibility maps (gi_visibility.inc).
#ifndef GI_AOV_BLOCK
// One workgroup per CU next to the 160 KB of records and boxes, as k_st_trace -- but of 512 lanes: the lane keeps a pixel's eight sums and the
// frame constants next to the walk, which at the 128 registers of a 1024-lane workgroup spills 408 B per lane (wide triangle instance); at 512
// it fits in 227 without scratch.  Measured on the benchmark frame (caustics 1920x1080, n = 256): 1024 lanes 76.0 ms, 512 lanes 66.5 ms.
#define GI_AOV_BLOCK 512
#endif
#ifndef GI_AO_BLOCK
#define GI_AO_BLOCK 512     // as GI_AOV_BLOCK: one workgroup per CU next to the records, 256 registers per lane
#endif
#ifndef GI_LIT_BLOCK
#define GI_LIT_BLOCK 512    // as GI_AO_BLOCK: the closest-hit walk, then any-hit walks, next to the same records; the look-ups behind them need fewer registers than either
#endif
#ifndef GI_FG_BLOCK
// 256 lanes, not 512: a gather ray's any-hit walks run with the loop's state (O, Nf, the running sum, the first hit's direct term) on top of what
// k_lit holds there, which at the 256 registers of a 512-lane workgroup spills 96 to 224 B per lane more than k_lit does.  At 256 lanes a wave may
// take the whole 512-entry file (256 VGPRs + 52 .. 203 AGPRs) and nothing spills, at one wave per SIMD.  The 512-lane build is the faster one on the
// benchmark frame (DESIGN.md has both sets of figures); -DGI_FG_BLOCK=512 builds it.
#define GI_FG_BLOCK 256
#endif
#ifndef GI_PV_BLOCK
#define GI_PV_BLOCK 512     // as GI_AOV_BLOCK: a closest-hit walk per sample next to the same records, two f64 sums per lane
#endif
template <int FEAT, int WIDE>
__global__ __launch_bounds__(GI_AOV_BLOCK) void k_aov(Scene S, Frame F, uint32_t n_pix, int32_t n, void* out, int out_f64, int32_t* ids);
template <int FEAT, int WIDE>
__global__ __launch_bounds__(GI_AO_BLOCK) void k_ao(Scene S, Frame F, uint32_t n_pix, int32_t n, int32_t n_dirs, double radius, void* out, int out_f64);
struct LitArgs;
template <int FEAT, int WIDE, int LM = 0, int PV = 0, int RS = 0>
__global__ __launch_bounds__(GI_LIT_BLOCK) void k_lit(Scene S, Frame F, LitArgs A, uint32_t n_pix, int32_t n, void* out, int out_f64);

template <int FEAT, int WIDE>
__global__ __launch_bounds__(GI_FG_BLOCK) void k_fg(Scene S, Frame F, LitArgs A, uint32_t n_pix, int32_t n, int32_t n_dirs, void* out, int out_f64, int32_t* ids);

struct PvArgs;
template <int FEAT, int WIDE>
__global__ __launch_bounds__(GI_PV_BLOCK) void k_pv_capture(Scene S, PvArgs A, unsigned long long n_texels, void* out, int out_f64);

static constexpr size_t kLdsNodes = (size_t)GI_LDS_NODES * sizeof(TNode);
static constexpr size_t kLdsFinishCoop = (size_t)GI_FINISH_COOP_LDS_BYTES;   // the one-path-per-group forms of the finisher: 292 records + content boxes + a heap per group
static constexpr size_t kLdsWideBoxes = (size_t)GI_LDS_WIDE_BOXES_BYTES;   // wide records + their content boxes: k_st_trace / k_st_shadow, one 1024-thread workgroup per CU

template <class Fn> struct StKernel { Fn fn; size_t lds; };
using TraceK = StKernel<decltype(&k_st_trace<0, 0>)>;
using ShadeK = StKernel<decltype(&k_st_shade<0, 0, 0>)>;
using ShadowK = StKernel<decltype(&k_st_shadow<0, 0>)>;
using FinishK = StKernel<decltype(&k_st_finish<0, 0, 0>)>;
using AovK = StKernel<decltype(&k_aov<0, 0>)>;
using AoK = StKernel<decltype(&k_ao<0, 0>)>;
using LitK = StKernel<decltype(&k_lit<0, 0>)>;
using FgK = StKernel<decltype(&k_fg<0, 0>)>;
using PvK = StKernel<decltype(&k_pv_capture<0, 0>)>;

static int first_hit_row(int feat, bool wide) { return (feat == 7 ? 2 : feat) * 2 + (wide ? 1 : 0); }   // the first-hit families: FEAT 0, spheres, textures x per-node, wide
static int feat_row(int feat) { return feat == 7 ? 3 : (feat == 3 ? 2 : feat); }                        // the others: the levels 0, spheres, fog, textures

// k_st_trace<FEAT, WIDE>: the first-hit rows; then the counting instance
static constexpr TraceK kTrace[] = {
    {k_st_trace<0, 0>, kLdsNodes}, {k_st_trace<0, 1>, kLdsWideBoxes}, {k_st_trace<GI_FEAT_SPHERES, 0>, kLdsNodes}, {k_st_trace<GI_FEAT_SPHERES, 1>, kLdsWideBoxes},
    {k_st_trace<7, 0>, kLdsNodes}, {k_st_trace<7, 1>, kLdsWideBoxes}, {k_st_trace<0, 1, true>, kLdsWideBoxes},
    // the first-hit rows again for a context with a thin lens (gi_set_lens): the pinhole's instances carry no code for it
    {k_st_trace<0, 0, false, true>, kLdsNodes}, {k_st_trace<0, 1, false, true>, kLdsWideBoxes}, {k_st_trace<GI_FEAT_SPHERES, 0, false, true>, kLdsNodes},
    {k_st_trace<GI_FEAT_SPHERES, 1, false, true>, kLdsWideBoxes}, {k_st_trace<7, 0, false, true>, kLdsNodes}, {k_st_trace<7, 1, false, true>, kLdsWideBoxes}};
static TraceK st_trace(int feat, bool wide, bool counting, bool lens) { return counting ? kTrace[6] : kTrace[(lens ? 7 : 0) + first_hit_row(feat, wide)]; }
// k_st_shade<FEAT, WIDE, DEFER>: FEAT 0, spheres, fog, textures x per-node, wide, wide with the shadow walks put off (one light; several lights)
// (the one-light form stages the trace stage's records and content boxes for the probe of the next ray: its LDS, one 512-thread workgroup per CU as before)
static constexpr ShadeK kShade[] = {
    {k_st_shade<0, 0, 0>, kLdsNodes}, {k_st_shade<0, 1, 0>, kLdsNodes}, {k_st_shade<0, 1, 1>, kLdsWideBoxes}, {k_st_shade<0, 1, 2>, kLdsNodes},
    {k_st_shade<GI_FEAT_SPHERES, 0, 0>, kLdsNodes}, {k_st_shade<GI_FEAT_SPHERES, 1, 0>, kLdsNodes}, {k_st_shade<GI_FEAT_SPHERES, 1, 1>, kLdsWideBoxes}, {k_st_shade<GI_FEAT_SPHERES, 1, 2>, kLdsNodes},
    {k_st_shade<3, 0, 0>, kLdsNodes}, {k_st_shade<3, 1, 0>, kLdsNodes}, {k_st_shade<3, 1, 1>, kLdsWideBoxes}, {k_st_shade<3, 1, 2>, kLdsNodes},
    {k_st_shade<7, 0, 0>, kLdsNodes}, {k_st_shade<7, 1, 0>, kLdsNodes}, {k_st_shade<7, 1, 1>, kLdsWideBoxes}, {k_st_shade<7, 1, 2>, kLdsNodes}};
static ShadeK st_shade(int feat, bool wide, int defer) { return kShade[feat_row(feat) * 4 + (wide ? 1 + defer : 0)]; }
// k_st_shadow<FEAT, MULTI>: FEAT 0, spheres, fog, textures x one light, several lights; then the counting instances (one light, several)
static constexpr ShadowK kShadow[] = {
    {k_st_shadow<0, 0>, kLdsWideBoxes}, {k_st_shadow<0, 1>, kLdsWideBoxes}, {k_st_shadow<GI_FEAT_SPHERES, 0>, kLdsWideBoxes}, {k_st_shadow<GI_FEAT_SPHERES, 1>, kLdsWideBoxes},
    {k_st_shadow<3, 0>, kLdsWideBoxes}, {k_st_shadow<3, 1>, kLdsWideBoxes}, {k_st_shadow<7, 0>, kLdsWideBoxes}, {k_st_shadow<7, 1>, kLdsWideBoxes},
    {k_st_shadow<0, 0, true>, kLdsWideBoxes}, {k_st_shadow<0, 1, true>, kLdsWideBoxes}};
static ShadowK st_shadow(int feat, bool many, bool counting) { return kShadow[(counting ? 4 : feat_row(feat)) * 2 + (many ? 1 : 0)]; }
// k_st_finish<FEAT, WIDE, MODE>: FEAT 0, spheres, fog, textures x per-node, wide: a path per lane, a path per wave, a path per group of 16 lanes
static constexpr FinishK kFinish[] = {
    {k_st_finish<0, 0, 0>, kLdsNodes}, {k_st_finish<0, 1, 0>, kLdsNodes}, {k_st_finish<0, 1, 1>, kLdsFinishCoop}, {k_st_finish<0, 1, 2>, kLdsFinishCoop},
    {k_st_finish<GI_FEAT_SPHERES, 0, 0>, kLdsNodes}, {k_st_finish<GI_FEAT_SPHERES, 1, 0>, kLdsNodes}, {k_st_finish<GI_FEAT_SPHERES, 1, 1>, kLdsFinishCoop}, {k_st_finish<GI_FEAT_SPHERES, 1, 2>, kLdsFinishCoop},
    {k_st_finish<3, 0, 0>, kLdsNodes}, {k_st_finish<3, 1, 0>, kLdsNodes}, {k_st_finish<3, 1, 1>, kLdsFinishCoop}, {k_st_finish<3, 1, 2>, kLdsFinishCoop},
    {k_st_finish<7, 0, 0>, kLdsNodes}, {k_st_finish<7, 1, 0>, kLdsNodes}, {k_st_finish<7, 1, 1>, kLdsFinishCoop}, {k_st_finish<7, 1, 2>, kLdsFinishCoop}};
static FinishK st_finish(int feat, bool wide, int mode) { return kFinish[feat_row(feat) * 4 + (wide ? 1 + mode : 0)]; }
// k_aov<FEAT, WIDE> (the feature pass) and k_ao<FEAT, WIDE> (the occlusion pass): the first-hit rows, with k_st_trace's LDS
static constexpr AovK kAov[] = {
    {k_aov<0, 0>, kLdsNodes}, {k_aov<0, 1>, kLdsWideBoxes}, {k_aov<GI_FEAT_SPHERES, 0>, kLdsNodes}, {k_aov<GI_FEAT_SPHERES, 1>, kLdsWideBoxes},
    {k_aov<7, 0>, kLdsNodes}, {k_aov<7, 1>, kLdsWideBoxes}};
static constexpr AoK kAo[] = {
    {k_ao<0, 0>, kLdsNodes}, {k_ao<0, 1>, kLdsWideBoxes}, {k_ao<GI_FEAT_SPHERES, 0>, kLdsNodes}, {k_ao<GI_FEAT_SPHERES, 1>, kLdsWideBoxes},
    {k_ao<7, 0>, kLdsNodes}, {k_ao<7, 1>, kLdsWideBoxes}};
// k_lit<FEAT, WIDE, LM> (the baked-light pass): the same rows and LDS; then the rows again with the lightmap look-up (gi_render_baked_lightmap_*)
static constexpr LitK kLit[] = {
    {k_lit<0, 0>, kLdsNodes}, {k_lit<0, 1>, kLdsWideBoxes}, {k_lit<GI_FEAT_SPHERES, 0>, kLdsNodes}, {k_lit<GI_FEAT_SPHERES, 1>, kLdsWideBoxes},
    {k_lit<7, 0>, kLdsNodes}, {k_lit<7, 1>, kLdsWideBoxes}};
static constexpr LitK kLitLm[] = {
    {k_lit<0, 0, 1>, kLdsNodes}, {k_lit<0, 1, 1>, kLdsWideBoxes}, {k_lit<GI_FEAT_SPHERES, 0, 1>, kLdsNodes}, {k_lit<GI_FEAT_SPHERES, 1, 1>, kLdsWideBoxes},
    {k_lit<7, 0, 1>, kLdsNodes}, {k_lit<7, 1, 1>, kLdsWideBoxes}};
// and once more with the probes' visibility maps in the grid's look-up (gi_render_baked_visibility_*)
static constexpr LitK kLitPv[] = {
    {k_lit<0, 0, 0, 1>, kLdsNodes}, {k_lit<0, 1, 0, 1>, kLdsWideBoxes}, {k_lit<GI_FEAT_SPHERES, 0, 0, 1>, kLdsNodes}, {k_lit<GI_FEAT_SPHERES, 1, 0, 1>, kLdsWideBoxes},
    {k_lit<7, 0, 0, 1>, kLdsNodes}, {k_lit<7, 1, 0, 1>, kLdsWideBoxes}};
// and with a reflection probe set in the specular term (gi_render_baked_reflections_*)
static constexpr LitK kLitRs[] = {
    {k_lit<0, 0, 0, 0, 1>, kLdsNodes}, {k_lit<0, 1, 0, 0, 1>, kLdsWideBoxes}, {k_lit<GI_FEAT_SPHERES, 0, 0, 0, 1>, kLdsNodes}, {k_lit<GI_FEAT_SPHERES, 1, 0, 0, 1>, kLdsWideBoxes},
    {k_lit<7, 0, 0, 0, 1>, kLdsNodes}, {k_lit<7, 1, 0, 0, 1>, kLdsWideBoxes}};
// k_fg<FEAT, WIDE> (the final-gather pass, gi_render_final_gather_*): kLit's rows and LDS
static constexpr FgK kFg[] = {
    {k_fg<0, 0>, kLdsNodes}, {k_fg<0, 1>, kLdsWideBoxes}, {k_fg<GI_FEAT_SPHERES, 0>, kLdsNodes}, {k_fg<GI_FEAT_SPHERES, 1>, kLdsWideBoxes},
    {k_fg<7, 0>, kLdsNodes}, {k_fg<7, 1>, kLdsWideBoxes}};
// k_pv_capture<FEAT, WIDE> (a probe's visibility map, gi_probe_visibility_*): the first-hit rows, with k_aov's LDS -- its walks are closest-hit walks
static constexpr PvK kPv[] = {
    {k_pv_capture<0, 0>, kLdsNodes}, {k_pv_capture<0, 1>, kLdsWideBoxes}, {k_pv_capture<GI_FEAT_SPHERES, 0>, kLdsNodes}, {k_pv_capture<GI_FEAT_SPHERES, 1>, kLdsWideBoxes},
    {k_pv_capture<7, 0>, kLdsNodes}, {k_pv_capture<7, 1>, kLdsWideBoxes}};
// k_st_gather / k_st_gather_wave<COUNT>: no template argument of the scene's, no dynamic LDS
static auto st_gather(bool counting) { return counting ? k_st_gather<true> : k_st_gather<false>; }
static auto st_gather_wave(bool counting) { return counting ? k_st_gather_wave<true> : k_st_gather_wave<false>; }

// more than 64 KB of dynamic LDS has to be asked for, per kernel (and per device: the attribute belongs to the loaded code object); a refusal
// (a part with less LDS than gfx950's 160 KB per CU) would make every later launch of the kernel fail: it is kept to be reported by name
template <class K, size_t N> static void ask_for_lds(const K (&ks)[N], int& refused)
{
    for (const K& k : ks)
        if (k.lds > 64 * 1024 && hipFuncSetAttribute((const void*)k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.lds) != hipSuccess) refused = (int)k.lds;
}
