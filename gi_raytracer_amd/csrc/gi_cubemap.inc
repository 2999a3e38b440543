// gi_cubemap.inc -- reflection probes (gi_cubemap_*; an addition beside the bakes of gi_bake.inc): a cube map of the radiance seen from a point, and
// the roughness mip chain filtered from it.  Included by gi_kernels.hip behind gi_lightmap.inc: the capture is bake_passes (gi_bake.inc) with a
// source of its own, and the chain is stored by the lightmap's k_lm_store.  The definition is stated in include/gi_hip.h; the per-lane functions,
// cm_coord(), cm_face_dir(), cm_measure(), cm_weight(), cm_box() and cm_ray(), are gi_cubemap.h.

namespace gi {
#include "gi_cubemap.h"
}  // namespace gi

// A capture is a third source of k_bake_gen: point i of the list is texel i of the cube, its rays leave the probe's position through the texel at the
// stream index's jitter.  The chunks, the ranges, the stream passes and the texel fold are the bake's (bake_passes).
struct CubeTexels {
    V3 P;                       // the probe (by value: no table on the device)
    uint32_t face, t0;          // the cube's face size; the chunk's first texel
    struct At { uint32_t t; };
    __device__ At at(uint32_t i) const { At a; a.t = t0 + i; return a; }
    __device__ Ray ray(const Scene& S, const At& a, uint32_t stream) const { return cm_ray(S, P, face, a.t, stream); }
};

// A box level: one lane per texel of the level of face n, from the 2 x 2 block of the level of face 2 n below it.
__global__ __launch_bounds__(GI_BLOCK) void k_cm_box(const double* src, uint32_t n, double* dst)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 6u * n * n) return;
    const CmTexel q = cm_texel(t, n);
    const uint32_t ns = 2u * n;
    const double* r0 = src + ((size_t)(q.f * ns + 2u * q.y) * ns + 2u * q.x) * 3;
    const double* r1 = r0 + (size_t)ns * 3;
    GI_UNROLL
    for (int ch = 0; ch < 3; ch++) dst[(size_t)t * 3 + ch] = cm_box(r0[ch], r0[3 + ch], r1[ch], r1[3 + ch]);
}

// The prefilter's all-pairs sum, the hot path.  A level of face n has 6 n^2 output texels and reads the 6 x 4 n^2 texels of the box level below it.
// One lane owns one PAIR (output texel, source face): blockIdx.y is the source face, the lanes of a workgroup are 256 neighbouring output texels, and
// each lane adds the face's 4 n^2 source texels to its W and A[3] in ascending order -- the header's order whatever the launch; no atomics, no
// reduction across lanes.  The six partial sums of an output texel go to part [6][6 n^2][4], and k_cm_resolve adds them face by face.  The split by
// face is what keeps the small levels parallel: 36 n^2 lanes, not 6 n^2.
// Source texels are staged through LDS in tiles of GI_CM_TILE = 256, one per lane of the workgroup: the lane computes its texel's unit direction and
// measure from the index (a sqrt and two divisions, once per texel and workgroup, against 256 uses) and loads its radiance, 64 bytes a texel.  In the
// inner loop every lane reads tile[j] at the same address: a broadcast, four ds_read_b128 without a bank conflict.
// Sizes.  16 KiB of LDS per workgroup: the 8 workgroups of 4 waves that fill a CU's 32 wave slots take 128 of its 160 KiB.  Per source texel a lane
// issues 5 f64 operations for the cosine, log2_e multiplications, one more for the measure, and 3 multiplications and 4 additions for the sums:
// 13 + log2_e VALU operations (no FMA: the project compiles without contraction, so that the bits are the statement's) against 4 LDS reads, so the
// f64 pipe is the limit, and with W, A[3] and R[3] in 14 VGPRs of state the kernel stays far below the 64 registers that allow 8 waves per SIMD.
// hipcc -Rpass-analysis=kernel-resource-usage, gfx950: 54 VGPRs, 37 SGPRs, 0 bytes of scratch, 16384 bytes of LDS, 8 waves per SIMD.
#define GI_CM_TILE GI_BLOCK
struct alignas(16) CmSrc { double dx, dy, dz, m, l0, l1, l2, pad; };
__global__ __launch_bounds__(GI_BLOCK) void k_cm_filter(const double* src, uint32_t n, int log2_e, double* part)
{
    __shared__ CmSrc tile[GI_CM_TILE];
    const uint32_t n_out = 6u * n * n, ns = 2u * n, per_face = ns * ns;
    const uint32_t o = blockIdx.x * blockDim.x + threadIdx.x, g = blockIdx.y;
    const V3 R = cm_centre_dir(o < n_out ? o : n_out - 1u, n);      // (lanes past the end stage tiles with the others and store nothing)
    double W = 0.0, A0 = 0.0, A1 = 0.0, A2 = 0.0;
    for (uint32_t s0 = 0; s0 < per_face; s0 += GI_CM_TILE) {
        const uint32_t count = per_face - s0 < GI_CM_TILE ? per_face - s0 : GI_CM_TILE;     // uniform over the workgroup
        __syncthreads();                                                                     // every lane is done with the tile before
        if (threadIdx.x < count) {
            const uint32_t s = g * per_face + s0 + threadIdx.x;
            const CmTexel q = cm_texel(s, ns);
            const double a = cm_coord(q.x, 0.5, ns), b = cm_coord(q.y, 0.5, ns);
            const V3 d = cm_unit(cm_face_dir(q.f, a, b));
            const double* l = src + (size_t)s * 3;
            CmSrc t;
            t.dx = d.x; t.dy = d.y; t.dz = d.z; t.m = cm_measure(a, b);
            t.l0 = l[0]; t.l1 = l[1]; t.l2 = l[2]; t.pad = 0.0;
            tile[threadIdx.x] = t;
        }
        __syncthreads();
        for (uint32_t j = 0; j < count; j++) {
            const CmSrc t = tile[j];
            const double w = cm_weight(R, v3(t.dx, t.dy, t.dz), t.m, log2_e);
            W += w;
            A0 += w * t.l0; A1 += w * t.l1; A2 += w * t.l2;
        }
    }
    if (o >= n_out) return;
    double* p = part + ((size_t)g * n_out + o) * 4;
    p[0] = W; p[1] = A0; p[2] = A1; p[3] = A2;
}

// One lane per output texel: the six faces' sums added in the order of the faces, A / W per channel, stored as the level's texel (rounded once for f32).
__global__ __launch_bounds__(GI_BLOCK) void k_cm_resolve(const double* part, uint32_t n_out, void* out, int out_f64)
{
    const uint32_t o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= n_out) return;
    double s[4];
    GI_UNROLL
    for (int k = 0; k < 4; k++) {
        s[k] = part[(size_t)o * 4 + k];
        GI_UNROLL
        for (uint32_t g = 1; g < 6u; g++) s[k] = s[k] + part[((size_t)g * n_out + o) * 4 + k];
    }
    GI_UNROLL
    for (int ch = 0; ch < 3; ch++) {
        const double v = s[1 + ch] / s[0];
        if (out_f64) ((double*)out)[(size_t)o * 3 + ch] = v;
        else ((float*)out)[(size_t)o * 3 + ch] = (float)v;
    }
}

namespace {

#define GI_CM_MAX_FACE 26754      // 6 face^2 <= 2^32: beyond it no stream index is left for a texel

// texels of level l of a chain of face N; of the levels before level l
size_t cm_level_texels(int32_t face, int l) { const size_t n = (size_t)(face >> l); return 6 * n * n; }
size_t cm_texels_before(int32_t face, int l)
{
    size_t t = 0;
    for (int k = 0; k < l; k++) t += cm_level_texels(face, k);
    return t;
}
bool cm_pair_ok(int32_t face, int32_t levels)
{
    return face >= 1 && face <= GI_CM_MAX_FACE && levels >= 1 && levels <= GI_CUBEMAP_MAX_LEVELS && (face & ((1 << (levels - 1)) - 1)) == 0;
}

// false + message when the parameters are not the header's
bool cm_check(const gi_cubemap_params* p, std::string& err)
{
    if (!p) { err = "cubemap: null parameters"; return false; }
    if (p->face < 1) { err = "cubemap: face must be at least 1, got " + std::to_string(p->face); return false; }
    if (p->n_samples < 1) { err = "cubemap: n_samples must be at least 1, got " + std::to_string(p->n_samples); return false; }
    if (p->levels < 1 || p->levels > GI_CUBEMAP_MAX_LEVELS) { err = "cubemap: levels must be 1 .. " + std::to_string(GI_CUBEMAP_MAX_LEVELS) + ", got " + std::to_string(p->levels); return false; }
    if (p->face & ((1 << (p->levels - 1)) - 1)) { err = "cubemap: " + std::to_string(p->levels) + " levels need a face divisible by " + std::to_string(1 << (p->levels - 1)) + ", got " + std::to_string(p->face); return false; }
    for (int l = 1; l < p->levels; l++)
        if (p->log2_exponent[l] < 0 || p->log2_exponent[l] > 16) { err = "cubemap: log2_exponent[" + std::to_string(l) + "] must be 0 .. 16, got " + std::to_string(p->log2_exponent[l]); return false; }
    if (p->face > GI_CM_MAX_FACE || (unsigned long long)p->stream_base + 6ull * (unsigned long long)p->face * (unsigned long long)p->face * (unsigned long long)p->n_samples > (1ull << 32)) {
        err = "cubemap: 6 x " + std::to_string(p->face) + " x " + std::to_string(p->face) + " texels of " + std::to_string(p->n_samples) + " samples from stream_base " + std::to_string(p->stream_base) + " take the stream index beyond 32 bits";
        return false;
    }
    return true;
}
bool cm_pos_ok(const double* pos, std::string& err)
{
    if (std::isfinite(pos[0]) && std::isfinite(pos[1]) && std::isfinite(pos[2])) return true;
    err = "cubemap: the probe has a non-finite position";
    return false;
}

void cm_reset_timers(gi_ctx* c)
{
    c->cm.timer.reset();
    for (EventTimer& t : c->cm.t_stage) t.reset();
}

// elements of the scratch a chain of `levels` needs beside B_0: the box levels 1 .. levels - 2 (level l is filtered from B_(l-1)), [texels][3], and
// the partial sums of the largest filtered level, [6][6 (N / 2)^2][4]
size_t cm_box_elems(int32_t face, int32_t levels) { return levels > 2 ? (cm_texels_before(face, levels - 1) - cm_level_texels(face, 0)) * 3 : 0; }
size_t cm_part_elems(int32_t face, int32_t levels) { return levels > 1 ? cm_level_texels(face, 1) * 6 * 4 : 0; }

// The chain from B_0 on the context's stream: level 0 stored as it is, then per level the box level its source needs (from the second on), the
// all-pairs sums and their resolve.  b0 [6 N^2][3] f64; box, part: cm_box_elems, cm_part_elems; out: the chain, f64 or f32.
void cm_prefilter_launch(gi_ctx* c, const gi_cubemap_params& p, const double* b0, double* box, double* part, void* out, int out_is_f64)
{
    hipStream_t st = c->stream;
    const size_t esz = out_is_f64 ? 8 : 4, t0 = cm_level_texels(p.face, 0);
    hipLaunchKernelGGL(k_lm_store, GI_GRID(t0 * 3), 0, st, b0, t0 * 3, out, out_is_f64);
    const double* below = b0;                         // B_(l-1)
    for (int l = 1; l < p.levels; l++) {
        const uint32_t n = (uint32_t)(p.face >> l);
        if (l >= 2) {                                 // B_(l-1) from B_(l-2)
            double* level = box + (cm_texels_before(p.face, l - 1) - t0) * 3;
            hipLaunchKernelGGL(k_cm_box, GI_GRID(6u * (2u * n) * (2u * n)), 0, st, below, 2u * n, level);
            below = level;
        }
        const uint32_t n_out = 6u * n * n;
        hipLaunchKernelGGL(k_cm_filter, dim3((n_out + GI_BLOCK - 1) / GI_BLOCK, 6), dim3(GI_BLOCK), 0, st, below, n, p.log2_exponent[l], part);
        hipLaunchKernelGGL(k_cm_resolve, GI_GRID(n_out), 0, st, (const double*)part, n_out, (void*)((char*)out + cm_texels_before(p.face, l) * 3 * esz), out_is_f64);
    }
}

// the whole probe: d_out on the device, arguments checked
int cm_run(gi_ctx* c, const double* pos, const gi_cubemap_params& p, void* d_out, int out_is_f64)
{
    HIP_TRY(c, hipSetDevice(c->device));
    CubemapPass& cm = c->cm;
    hipStream_t st = c->stream;
    const uint32_t T = (uint32_t)cm_level_texels(p.face, 0);
    cm_reset_timers(c);
    struct Guard { gi_ctx* c; bool ok = false; ~Guard() { if (!ok) cm_reset_timers(c); } } guard{c};   // a call that fails has no time to report
    HIP_TRY(c, lm_grow(cm.d_b0, (size_t)T * 3)); HIP_TRY(c, lm_grow(cm.d_box, cm_box_elems(p.face, p.levels))); HIP_TRY(c, lm_grow(cm.d_part, cm_part_elems(p.face, p.levels)));
    HIP_TRY(c, cm.timer.begin(st));
    gi_bake_params bp;
    bp.mode = GI_BAKE_TEXEL; bp.n_samples = p.n_samples; bp.stream_base = p.stream_base; bp.seed = p.seed;
    const V3 P = ld3(pos);
    const uint32_t face = (uint32_t)p.face;
    const auto texels = [&](uint32_t i0) { CubeTexels s; s.P = P; s.face = face; s.t0 = i0; return s; };
    if (const int rc = bake_passes(c, T, bp, texels, cm.d_b0.p, 1, cm.t_stage[0])) return rc;
    HIP_TRY(c, cm.t_stage[1].begin(st));
    cm_prefilter_launch(c, p, cm.d_b0.p, cm.d_box.p, cm.d_part.p, d_out, out_is_f64);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, cm.t_stage[1].end(st));
    HIP_TRY(c, cm.timer.end(st));
    guard.ok = true;
    return GI_OK;
}

}  // namespace

extern "C" {

void gi_cubemap_default_params(gi_cubemap_params* p)
{
    if (!p) return;
    p->face = 32; p->n_samples = 64; p->levels = 1;
    p->stream_base = 0u;
    p->seed = 0x9E3779B97F4A7C15ull;
    for (int l = 0; l < GI_CUBEMAP_MAX_LEVELS; l++) p->log2_exponent[l] = std::max(0, 16 - 3 * l);
}

int64_t gi_cubemap_chain_texels(int32_t face, int32_t levels)
{
    return cm_pair_ok(face, levels) ? (int64_t)cm_texels_before(face, levels) : -1;
}

int gi_cubemap_device(gi_ctx* c, const double* pos3, const gi_cubemap_params* p, void* d_out, int out_is_f64)
{
    if (!c) return GI_E_INVALID;
    std::string err;
    if (!cm_check(p, err)) return fail(c, GI_E_INVALID, err);
    if (!pos3 || !d_out) return fail(c, GI_E_INVALID, "cubemap: null position or output pointer");
    if (!c->scene.have_scene) return fail(c, GI_E_STATE, "cubemap: no scene uploaded");
    return cm_run(c, pos3, *p, d_out, out_is_f64);
}

int gi_cubemap_host(gi_ctx* c, const double* pos3, const gi_cubemap_params* p, void* h_out, int out_is_f64)
{
    if (!c) return GI_E_INVALID;
    std::string err;
    if (!cm_check(p, err)) return fail(c, GI_E_INVALID, err);
    if (!pos3 || !h_out) return fail(c, GI_E_INVALID, "cubemap: null position or output pointer");
    if (!cm_pos_ok(pos3, err)) return fail(c, GI_E_INVALID, err);
    if (!c->scene.have_scene) return fail(c, GI_E_STATE, "cubemap: no scene uploaded");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = cm_texels_before(p->face, p->levels) * 3 * (out_is_f64 ? 8 : 4);
    DevBuf<unsigned char> d_out;
    HIP_TRY(c, d_out.alloc(bytes));
    int rc = cm_run(c, pos3, *p, d_out.p, out_is_f64);
    if (rc == GI_OK) rc = finish_to_host(c, "cubemap_host", {{h_out, d_out.p, bytes}});
    else (void)hipStreamSynchronize(c->stream);
    if (rc != GI_OK) cm_reset_timers(c);
    return rc;
}

int gi_last_cubemap_ms(gi_ctx* c, float* ms, float* stages2)
{
    if (!c || !ms) return GI_E_INVALID;
    HIP_TRY(c, c->cm.timer.read(ms));
    for (int k = 0; stages2 && k < 2; k++) HIP_TRY(c, c->cm.t_stage[k].read(stages2 + k));
    return GI_OK;
}

int gi_cubemap_rays(gi_ctx* c, const double* pos3, const gi_cubemap_params* p, double* rays6_out, uint32_t* stream_out)
{
    if (!c) return GI_E_INVALID;
    std::string err;
    if (!cm_check(p, err)) return fail(c, GI_E_INVALID, err);
    if (!pos3 || !rays6_out || !stream_out) return fail(c, GI_E_INVALID, "cubemap_rays: null position or output pointer");
    if (!cm_pos_ok(pos3, err)) return fail(c, GI_E_INVALID, err);
    const size_t n_rays = cm_level_texels(p->face, 0) * (size_t)p->n_samples;
    if (n_rays > 0x7fffffffull) return fail(c, GI_E_INVALID, "cubemap_rays: more than 2^31 - 1 rays");
    Entry e(c, "cubemap_rays");
    double* d_r = e.out(rays6_out, n_rays * 6);
    uint32_t* d_s = e.out(stream_out, n_rays);
    CubeTexels src;
    src.P = ld3(pos3); src.face = (uint32_t)p->face; src.t0 = 0u;
    return e.run([&] { hipLaunchKernelGGL(k_bake_rays<CubeTexels>, GI_GRID(n_rays), 0, c->stream, c->S, src, (uint32_t)n_rays, (uint32_t)p->n_samples, p->stream_base, d_r, d_s); });
}

int gi_cubemap_prefilter(gi_ctx* c, const gi_cubemap_params* p, const double* cube_in, double* chain_out)
{
    if (!c) return GI_E_INVALID;
    std::string err;
    if (!cm_check(p, err)) return fail(c, GI_E_INVALID, err);
    if (!cube_in || !chain_out) return fail(c, GI_E_INVALID, "cubemap_prefilter: null cube or output pointer");
    Entry e(c, "cubemap_prefilter");
    const double* d_b0 = e.in(cube_in, cm_level_texels(p->face, 0) * 3);
    double* d_box = e.scratch<double>(cm_box_elems(p->face, p->levels));
    double* d_part = e.scratch<double>(cm_part_elems(p->face, p->levels));
    double* d_o = e.out(chain_out, cm_texels_before(p->face, p->levels) * 3);
    return e.run([&] { cm_prefilter_launch(c, *p, d_b0, d_box, d_part, (void*)d_o, 1); });
}

}  // extern "C"
