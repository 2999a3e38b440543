// gi_kernels.hip -- the gfx950 kernels of the renderer; the C ABI of include/gi_hip.h is in the .inc files included at the end.
//
// Kernels (all one ray / one pixel per lane, 64-wide waves, scene tables read through L1/L2):
//   k_render     the pixel loop of RayTracer::run with the whole path inside (include/raytracer.h:93-160,167-579)
//   k_trace / k_visible / k_gather / k_radiance   function-level entry points (parity tests, public C++ methods)
//   k_emit       RayTracer::tracePhotons (include/raytracer.h:582-715), one (photon index, light) per lane
// The photon gather's kernels (k_st_gather, k_st_gather_wave, k_gather, ...) are in gi_gather.inc, included behind k_st_compact; what they share
// with the per-lane gather is in gi_gather.h (through gi_device.h).
// This file holds kernels only.  The host side -- the context, the scheduler and the gi_* entry points -- is in the .inc files listed at its end,
// which also hold the kernels of the sort, the photon-map build and the auxiliary passes.  No CPU fallback exists: every entry needs a HIP device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/gi_hip.h"
#include "gi_device.h"
#include "gi_layout.h"

using namespace gi;

#define GI_BLOCK 256

// ================================================================================================= kernels
// A pixel of the adaptive loop between launches (streaming and round-based renderers), as PixelState plus n = samples started this round.
struct PixRec { double color[3], lastCol[3], var; int32_t samps, s, n, pad; };
__device__ __forceinline__ PixelState pixrec_to_state(const PixRec& r)
{
    PixelState ps;
    ps.color = ld3(r.color); ps.lastCol = ld3(r.lastCol); ps.var = r.var; ps.samps = r.samps; ps.s = r.s;
    return ps;
}
__device__ __forceinline__ void state_to_pixrec(const PixelState& ps, PixRec& r)   // leaves r.n and r.pad as they are
{
    r.color[0] = ps.color.x; r.color[1] = ps.color.y; r.color[2] = ps.color.z;
    r.lastCol[0] = ps.lastCol.x; r.lastCol[1] = ps.lastCol.y; r.lastCol[2] = ps.lastCol.z;
    r.var = ps.var; r.samps = ps.samps; r.s = ps.s;
}
// the pixel's colour so far to out (f32 or f64) and its sample count to out_spp (optional), at (x, local row ly)
__device__ __forceinline__ void pixel_write(const Frame& F, int x, int ly, const PixelState& ps, void* out, int out_f64, int32_t* out_spp)
{
    const size_t o = ((size_t)ly * F.w + x);
    if (!out_f64) {
        float* p = (float*)out + o * 3;
        p[0] = (float)ps.color.x; p[1] = (float)ps.color.y; p[2] = (float)ps.color.z;
    } else {
        double* p = (double*)out + o * 3;
        p[0] = ps.color.x; p[1] = ps.color.y; p[2] = ps.color.z;
    }
    if (out_spp) out_spp[o] = ps.s;
}

template <bool COUNT>
__global__ __launch_bounds__(GI_BLOCK) void k_render(Scene S, Frame F, void* out, int out_f64, int32_t* out_spp,
                                                     unsigned int* tile_counter, Counters* counters)
{
    __shared__ float heap[GI_GATHER_K * GI_BLOCK];
    const int tid = threadIdx.x, lane = tid & 63;
    const int tiles_x = (F.w + 7) >> 3, tiles_y = (F.local_rows + 7) >> 3;
    const unsigned int n_tiles = (unsigned int)(tiles_x * tiles_y);
    Counters cnt;
    if (COUNT) memset(&cnt, 0, sizeof cnt);
    for (;;) {
        unsigned int t0 = 0;
        if (lane == 0) t0 = atomicAdd(tile_counter, 1u);   // one tile of 8x8 pixels per wave, dealt dynamically
        const unsigned int tile = (unsigned int)__builtin_amdgcn_readfirstlane((int)t0);
        if (tile >= n_tiles) break;
        const int tx = (int)(tile % (unsigned)tiles_x), ty = (int)(tile / (unsigned)tiles_x);
        const int x = tx * 8 + (lane & 7), ly = ty * 8 + (lane >> 3);
        if (x < F.w && ly < F.local_rows) {
            const int y = global_row(F, ly);
            PixelState ps;
            pixel_begin(ps);
            while (pixel_wants_sample(ps, F)) {
                uint32_t idx;
                Ray ray = primary_ray(S, F, ps.s, x, y, idx);
                V3 L = radiance_path(S, ray, idx, F.seed, heap + tid, GI_BLOCK, COUNT ? &cnt : nullptr);
                pixel_add_sample(ps, F, L);
            }
            pixel_write(F, x, ly, ps, out, out_f64, out_spp);
        }
    }
    if (COUNT) {
        atomicAdd(&counters->v_trace, cnt.v_trace); atomicAdd(&counters->v_shadow, cnt.v_shadow);
        atomicAdd(&counters->tri, cnt.tri); atomicAdd(&counters->shaded, cnt.shaded);
        atomicAdd(&counters->pcand, cnt.pcand); atomicAdd(&counters->traces, cnt.traces);
        atomicAdd(&counters->shadows, cnt.shadows); atomicAdd(&counters->gathers, cnt.gathers);
    }
}

// ================================================================================================= octree top in LDS
// The traversal kernels of the streaming pipeline copy the first n_l node records (breadth-first order = the top levels of
// the octree, which every ray visits) into LDS once per workgroup and read them from there; deeper nodes come from L1/L2.
extern __shared__ __align__(128) unsigned char gi_dyn_lds[];
#define GI_LDS_NODES 512                      // 64 KB of 128-byte records
struct LdsNodes {
    static constexpr bool kWide = false;
    const TNode* g;
    int32_t n_l;
    __device__ __forceinline__ void fetch(int32_t i, int oct, NodeView& v) const
    {
        if (i < n_l) {
            const TNode* l = reinterpret_cast<const TNode*>(gi_dyn_lds);
            const TNode& n = l[i];
            v.bmin[0] = n.bmin[0]; v.bmin[1] = n.bmin[1]; v.bmin[2] = n.bmin[2];
            v.bmax[0] = n.bmax[0]; v.bmax[1] = n.bmax[1]; v.bmax[2] = n.bmax[2];
            v.first_ref = n.first_ref; v.n_ref = n.n_ref;
            v.hit = n.link[oct].hit; v.skip = n.link[oct].skip;
        } else {
            const TNode& n = g[i];
            v.bmin[0] = n.bmin[0]; v.bmin[1] = n.bmin[1]; v.bmin[2] = n.bmin[2];
            v.bmax[0] = n.bmax[0]; v.bmax[1] = n.bmax[1]; v.bmax[2] = n.bmax[2];
            v.first_ref = n.first_ref; v.n_ref = n.n_ref;
            v.hit = n.link[oct].hit; v.skip = n.link[oct].skip;
        }
    }
    __device__ __forceinline__ int32_t leaf_id(int32_t i) const { return g[i].leaf_id; }
};
__device__ __forceinline__ LdsNodes stage_nodes_in_lds(const Scene& S)
{
    LdsNodes N;
    N.g = S.tnodes;
    N.n_l = S.n_node < GI_LDS_NODES ? S.n_node : GI_LDS_NODES;
    const uint4* src = reinterpret_cast<const uint4*>(S.tnodes);
    uint4* dst = reinterpret_cast<uint4*>(gi_dyn_lds);
    for (int i = threadIdx.x; i < N.n_l * 8; i += blockDim.x) dst[i] = src[i];
    __syncthreads();
    return N;
}

// the same for the wide records (gi_scene.h: WNode): 292 of them = every inner node of the BASELINE scenes
#define GI_LDS_WNODES 292                     // 64 KB of 224-byte records
// LDS layout "records + content boxes": cap records, 16 bytes of counters, the records' content boxes (192 bytes each), their flag words.
// The kernels that own a CU with one 1024-thread workgroup (k_st_trace, k_st_shadow) use nearly all of its 160 KB: 384 records; the one-path-per-
// group forms of the finisher 292 (and 4 KB of heaps behind them).
#define GI_LDS_WNODES_BIG 384
#define GI_LDS_CNT_OFF(cap) ((cap) * 224)
#define GI_LDS_CBOX_OFF(cap) (GI_LDS_CNT_OFF(cap) + 16)
#define GI_LDS_CUSE_OFF(cap) (GI_LDS_CBOX_OFF(cap) + (cap) * 192)
#define GI_LDS_BOXES_BYTES(cap) (GI_LDS_CUSE_OFF(cap) + (cap) * 4)
#define GI_LDS_BIG_CNT_OFF GI_LDS_CNT_OFF(GI_LDS_WNODES_BIG)
#define GI_LDS_WIDE_BOXES_BYTES GI_LDS_BOXES_BYTES(GI_LDS_WNODES_BIG)
template <bool COUNT>
struct LdsWideT {
    static constexpr bool kWide = true;
    static constexpr bool kCoop = false;
    static constexpr bool kCount = COUNT;
    // executed-work counters of this lane (gi_set_counters(ctx, 2)); an instance that does not count never touches them, and they are gone
    mutable WalkCnt wc = {0, 0, 0, 0, 0, 0, 0};
    __device__ __forceinline__ void tick_walk() const { if constexpr (COUNT) wc.walks++; }
    __device__ __forceinline__ void tick_node(uint32_t exists) const { if constexpr (COUNT) { wc.nodes++; wc.child_boxes += (uint32_t)__builtin_popcount(exists & 0xffu); } }
    __device__ __forceinline__ void tick_cull(uint32_t n) const { if constexpr (COUNT) wc.cull_tests += n; }
    __device__ __forceinline__ void tick_leaf() const { if constexpr (COUNT) wc.leaves++; }
    __device__ __forceinline__ void tick_tri() const { if constexpr (COUNT) wc.tris++; }
    __device__ __forceinline__ void tick_ebox(uint32_t n) const { if constexpr (COUNT) wc.ent_boxes += n; }
    const WNode* g;
    const float* cboxes;      // content boxes of the children (gi_walk.h: content_cull), read through L1 / L2; null = no culling
    const uint32_t* cuse;
    int32_t n_l;
    int32_t n_lc = 0;         // records whose content boxes are staged in LDS too
    uint32_t box_off = 0, use_off = 0;   // where (GI_LDS_CBOX_OFF / GI_LDS_CUSE_OFF of the kernel's record count)
#ifdef GI_EXP_DIV
    mutable uint32_t ds[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // lane / wave counts of: node steps, leaves, triangle tests (scalar path), triangle tests (per-lane path)
#endif
    template <class F> __device__ __forceinline__ auto with(int32_t i, F&& f) const
    {
        if (i < n_l) return f(reinterpret_cast<const WNode*>(gi_dyn_lds) + i);
        return f(g + i);
    }
    // the content boxes of a record's children: every turn of a walk reads them right after the record -- from L2 that is the longest wait of the turn
    __device__ __forceinline__ uint32_t cull(int32_t node, uint32_t m, const Ray& r, const WRay& wr) const
    {
        if (!cboxes || wr.plain) return m;
        uint32_t nt = 0;
        uint32_t* const ntp = COUNT ? &nt : nullptr;
        const uint32_t res = node < n_lc ? content_cull(reinterpret_cast<const float*>(gi_dyn_lds + box_off), reinterpret_cast<const uint32_t*>(gi_dyn_lds + use_off), node, m, r, wr, ntp)
                                         : content_cull(cboxes, cuse, node, m, r, wr, ntp);
        tick_cull(nt);
        return res;
    }
    // the tables cull() reads, for callers that test a record's children side by side (gi_walk.h: walk_hits of the one-ray-per-group walks)
    __device__ __forceinline__ const float* cbox_table(int32_t node) const { return !cboxes ? nullptr : (node < n_lc ? reinterpret_cast<const float*>(gi_dyn_lds + box_off) : cboxes); }
    __device__ __forceinline__ uint32_t cuse_of(int32_t node) const { return node < n_lc ? reinterpret_cast<const uint32_t*>(gi_dyn_lds + use_off)[node] : cuse[node]; }
};
typedef LdsWideT<false> LdsWide;
#ifdef GI_EXP_DIV
__device__ unsigned long long g_div[64 * 16 * 2];   // [workgroup & 63][kernel][counter]
template <class LW> __device__ __forceinline__ void div_flush(const LW& N, int kernel)
{
    for (int k = 0; k < 8; k++) {
        unsigned long long v = N.ds[k];
        for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
        if ((threadIdx.x & 63u) == 0) atomicAdd(&g_div[((blockIdx.x & 63u) * 2 + kernel) * 16 + k], v);
    }
    unsigned long long one = 1;
    for (int o = 32; o; o >>= 1) one += __shfl_xor(one, o);
    if ((threadIdx.x & 63u) == 0) atomicAdd(&g_div[((blockIdx.x & 63u) * 2 + kernel) * 16 + 8], one);
}
extern "C" int gi_debug_div(unsigned long long* out, int reset)
{
    static unsigned long long h[64 * 16 * 2];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_div), sizeof(h)) != hipSuccess) return -1;
    for (int i = 0; i < 32; i++) out[i] = 0;
    for (int b = 0; b < 64; b++) for (int i = 0; i < 32; i++) out[i] += h[b * 32 + i];
    if (reset) { static unsigned long long z[64 * 16 * 2]; if (hipMemcpyToSymbol(HIP_SYMBOL(g_div), z, sizeof(z)) != hipSuccess) return -1; }
    return 0;
}
#endif
template <int G> struct LdsWideCoop : LdsWide { static constexpr bool kCoop = true; static constexpr int kGroup = G; };   // the same records, one ray per group of G lanes (gi_walk.h: trace_wide_coop)
template <bool COUNT = false>
__device__ __forceinline__ LdsWideT<COUNT> stage_wide_in_lds(const Scene& S, bool with_boxes = false, int boxes_cap = GI_LDS_WNODES_BIG, int tables = 0)
{
    // tables: whose content boxes -- 0 the whole entities' (any walk), 1 the closest-hit walk's, 2 those for segments that end at a light
    LdsWideT<COUNT> N;
    N.g = S.wnodes;
    N.cboxes = tables == 1 ? S.tcboxes : (tables == 2 ? S.scboxes : S.cboxes); N.cuse = tables == 1 ? S.tcuse : (tables == 2 ? S.scuse : S.cuse);
    const int cap = with_boxes ? boxes_cap : GI_LDS_WNODES;
    N.box_off = GI_LDS_CBOX_OFF(cap); N.use_off = GI_LDS_CUSE_OFF(cap);
    N.n_l = S.n_wnode < cap ? S.n_wnode : cap;
    const uint4* src = reinterpret_cast<const uint4*>(S.wnodes);
    uint4* dst = reinterpret_cast<uint4*>(gi_dyn_lds);
    for (int i = threadIdx.x; i < N.n_l * (int)(sizeof(WNode) / 16); i += blockDim.x) dst[i] = src[i];
    if (with_boxes && N.cboxes) {
        N.n_lc = N.n_l;
        const uint4* bsrc = reinterpret_cast<const uint4*>(N.cboxes);
        uint4* bdst = reinterpret_cast<uint4*>(gi_dyn_lds + N.box_off);
        for (int i = threadIdx.x; i < N.n_lc * 12; i += blockDim.x) bdst[i] = bsrc[i];   // 8 children x 6 floats = 12 x 16 bytes per record
        uint32_t* udst = reinterpret_cast<uint32_t*>(gi_dyn_lds + N.use_off);
        for (int i = threadIdx.x; i < N.n_lc; i += blockDim.x) udst[i] = N.cuse[i];
    }
    __syncthreads();
    return N;
}
template <int WIDE, bool COUNT = false> struct LdsSrc;
template <bool COUNT> struct LdsSrc<0, COUNT> { typedef LdsNodes type; static __device__ __forceinline__ LdsNodes stage(const Scene& S) { return stage_nodes_in_lds(S); }
                         static __device__ __forceinline__ LdsNodes stage_with_boxes(const Scene& S) { return stage_nodes_in_lds(S); }
                         static __device__ __forceinline__ LdsNodes stage_for_trace(const Scene& S) { return stage_nodes_in_lds(S); } };
template <bool COUNT> struct LdsSrc<1, COUNT> { typedef LdsWideT<COUNT> type; static __device__ __forceinline__ type stage(const Scene& S) { return stage_wide_in_lds<COUNT>(S); }
                         static __device__ __forceinline__ type stage_with_boxes(const Scene& S) { return stage_wide_in_lds<COUNT>(S, true); }
                         static __device__ __forceinline__ type stage_for_trace(const Scene& S) { return stage_wide_in_lds<COUNT>(S, true, GI_LDS_WNODES_BIG, 1); } };   // the closest-hit walk's own content boxes
// what the streaming kernels executed in one frame (gi_get_stream_counters): per-lane WalkCnt sums of k_st_trace and k_st_shadow, the rays handed
// to each, the gather's queries and the candidates they scanned
struct StreamCounters { unsigned long long trace[7], trace_rays, shadow[7], shadow_rays, gather_queries, gather_cand; };
__device__ __forceinline__ void flush_u64(unsigned long long* dst, unsigned long long v)
{
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63u) == 0u && v) atomicAdd(dst, v);
}
__device__ __forceinline__ void flush_walk_cnt(unsigned long long* dst6, const WalkCnt& w)
{
    flush_u64(dst6 + 0, w.walks); flush_u64(dst6 + 1, w.nodes); flush_u64(dst6 + 2, w.child_boxes);
    flush_u64(dst6 + 3, w.cull_tests); flush_u64(dst6 + 4, w.leaves); flush_u64(dst6 + 5, w.tris); flush_u64(dst6 + 6, w.ent_boxes);
}

// ================================================================================================= path pool
// The streaming passes run the same per-path stage_* code as the megakernel, so both give the same numbers.
// The streaming pipeline's paths in flight: ONE ARRAY PER GROUP OF FIELDS that a stage reads or writes together, instead of one 224-byte PathRec per
// path.  A stage wants 40 - 160 bytes of a path; out of records it moved whole DRAM pages for them (exp/aos_bench.hip: the shade stage's
// read-104-write-172 pattern costs 48 ms per 477 M records as 224-byte structures, 24 ms as field arrays).  pool[slot] gives a PathRef -- the field
// names of PathRec as references -- so the stage functions (templates on the path type) read and write exactly the fields they did.
struct alignas(16) PoolRay  { double o[3], d[3]; uint32_t stream; int32_t depth; uint32_t pad_[2]; };   // 64 B: all a new path consists of, all the trace stage reads
struct alignas(16) PoolHit  { double hpos[3], hu, hv; int32_t htri; uint32_t mf; };                     // 48 B: what the trace stage leaves for the shade stage
struct alignas(16) PoolThru { double T[3], contrib[3]; };                                               // 48 B
struct alignas(16) PoolGath { double gdir[3], gcoef[3]; };                                              // 48 B: the pending photon gather (and minUV between trace and shade)
struct PathRef {
    double (&o)[3]; double (&d)[3]; uint32_t& stream; int32_t& depth; int32_t& htri; uint32_t& pad;
    double (&T)[3]; double (&contrib)[3]; double (&gdir)[3]; double (&gcoef)[3]; double (&hpos)[3]; double& hu; double& hv; double (&L)[3];
};
#define GI_POOL_BYTES_PER_SLOT (sizeof(PoolRay) + sizeof(PoolHit) + sizeof(PoolThru) + sizeof(PoolGath) + 24)
static_assert(GI_POOL_BYTES_PER_SLOT == kPoolRecordBytes, "the pool budget (gi_layout.h: plan_pool) counts this record");
struct PathPool {
    PoolRay* ray; PoolHit* hit; PoolThru* thru; PoolGath* gath; double* L;
    __device__ __forceinline__ PathRef operator[](size_t s) const
    {
        return PathRef{ray[s].o, ray[s].d, ray[s].stream, ray[s].depth, hit[s].htri, hit[s].mf, thru[s].T, thru[s].contrib, gath[s].gdir, gath[s].gcoef,
                       hit[s].hpos, hit[s].hu, hit[s].hv, *reinterpret_cast<double (*)[3]>(L + s * 3)};
    }
    __device__ __forceinline__ PathRec load(size_t s) const     // a copy in registers (finisher)
    {
        PathRec p;
        const PathRef r = (*this)[s];
        for (int k = 0; k < 3; k++) { p.o[k] = r.o[k]; p.d[k] = r.d[k]; p.T[k] = r.T[k]; p.contrib[k] = r.contrib[k]; p.gdir[k] = r.gdir[k]; p.gcoef[k] = r.gcoef[k]; p.hpos[k] = r.hpos[k]; p.L[k] = r.L[k]; }
        p.stream = r.stream; p.depth = r.depth; p.htri = r.htri; p.pad = r.pad; p.hu = r.hu; p.hv = r.hv;
        return p;
    }
    __device__ __forceinline__ void store(size_t s, const PathRec& p) const
    {
        const PathRef r = (*this)[s];
        for (int k = 0; k < 3; k++) { r.o[k] = p.o[k]; r.d[k] = p.d[k]; r.T[k] = p.T[k]; r.contrib[k] = p.contrib[k]; r.gdir[k] = p.gdir[k]; r.gcoef[k] = p.gcoef[k]; r.hpos[k] = p.hpos[k]; r.L[k] = p.L[k]; }
        r.stream = p.stream; r.depth = p.depth; r.htri = p.htri; r.pad = p.pad; r.hu = p.hu; r.hv = p.hv;
    }
};
__device__ __forceinline__ void pool_begin(const PathPool& pool, size_t slot, const Ray& ray, uint32_t sample)   // a new path: one 64-byte store (path_begin_lean)
{
    PoolRay r;
    r.o[0] = ray.o.x; r.o[1] = ray.o.y; r.o[2] = ray.o.z;
    r.d[0] = ray.d.x; r.d[1] = ray.d.y; r.d[2] = ray.d.z;
    r.stream = sample; r.depth = 0; r.pad_[0] = 0u; r.pad_[1] = 0u;
    pool.ray[slot] = r;
}
__device__ __forceinline__ uint32_t wave_append(unsigned int* counter, bool pred)
{
    const unsigned long long mask = __ballot(pred);
    if (mask == 0ull) return 0u;
    const int lane = (int)(threadIdx.x & 63u);
    const int leader = __ffsll((long long)mask) - 1;
    unsigned int base = 0;
    if (lane == leader) base = atomicAdd(counter, (unsigned int)__popcll(mask));
    base = (unsigned int)__shfl((int)base, leader);
    return base + (unsigned int)__popcll(mask & ((1ull << lane) - 1ull));
}

// record of the rounds schedule -> (x, local row): padded 8x8 tiles, so that the 64 lanes of a wave start neighbouring pixels; false for a padding record
__device__ __forceinline__ bool tile_pixel_xy(const Frame& F, uint32_t i, int& x, int& ly)
{
    const int tiles_x = (F.w + 7) >> 3;
    const uint32_t tile = i >> 6, t = i & 63u;
    x = (int)(tile % (uint32_t)tiles_x) * 8 + (int)(t & 7u);
    ly = (int)(tile / (uint32_t)tiles_x) * 8 + (int)(t >> 3);
    return x < F.w && ly < F.local_rows;
}

// v-th pixel of the local frame in 8x8-tile order, partial tiles at the right / bottom edge included (no padding pixels)
__device__ __forceinline__ void st_pixel_xy(const Frame& F, uint32_t v, int& x, int& ly)
{
    const uint32_t w = (uint32_t)F.w, rows = (uint32_t)F.local_rows;
    const uint32_t tiles_x = (w + 7u) >> 3, rows_full = rows >> 3;
    uint32_t r = v / (w * 8u);
    if (r > rows_full) r = rows_full;
    const uint32_t hr = r < rows_full ? 8u : (rows & 7u);
    const uint32_t rem = v - r * w * 8u;
    uint32_t tile = rem / (8u * hr);
    uint32_t tw = 8u;
    if (tile >= tiles_x - 1u) { tile = tiles_x - 1u; tw = w - 8u * (tiles_x - 1u); }
    const uint32_t t = rem - tile * 8u * hr;
    x = (int)(tile * 8u + t % tw);
    ly = (int)(r * 8u + t / tw);
}

// every pixel's state before its first sample (render_streaming, render_adaptive)
__global__ __launch_bounds__(GI_BLOCK) void k_pix_init(PixRec* pix, uint32_t n_pix)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_pix; i += gridDim.x * blockDim.x) {
        PixelState ps;
        pixel_begin(ps);
        PixRec r;
        state_to_pixrec(ps, r);
        r.n = 0; r.pad = 0;
        pix[i] = r;
    }
}

// Which sample a slot of the path pool carries.  The table slot_sample[slot] says so in general (slots are handed on from path to path).  When the
// pool holds every sample of a chunk at once, the trace stage's first pass gives item i slot i and sample sample0 + i and no slot is ever reissued:
// the table would be the identity plus sample0, so the host passes no table (nullptr, wave-uniform) and nobody writes or reads one (stream_samples).
__device__ __forceinline__ unsigned long long sample_of(const unsigned long long* slot_sample, unsigned long long sample0, uint32_t slot)
{
    return slot_sample ? slot_sample[slot] : sample0 + slot;
}

// Adaptive rounds on the streaming machinery (render_adaptive): the paths of a round are started here, compacted into q_new, and then
// go through the k_st_* passes; a finished path leaves its radiance in lbuf[slot] (slot_sample[slot] = slot), which the accumulate
// step folds into the pixel in sample order.
__global__ __launch_bounds__(GI_BLOCK) void k_ad_gen(Scene S, Frame F, PixRec* pix, PathPool pool, unsigned long long* slot_sample, uint32_t n_pix, int B,
                                                    uint32_t* q_new, unsigned int* n_new)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_round = (n_pix + 63u) & ~63u;
    for (uint32_t i0 = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < n_round; i0 += gridDim.x * blockDim.x) {
        const uint32_t i = i0 + lane;
        int x = 0, ly = 0, n = 0, s0 = 0;
        const bool inside = i < n_pix && tile_pixel_xy(F, i, x, ly);
        if (inside) {
            const int s = pix[i].s, samps = pix[i].samps;
            if (s < F.max_samples && samps < F.min_samples) {
                // min - samps samples are certain (each adds 1 to samps or subtracts 1, include/raytracer.h:143-147).  Past those the
                // pixel may stop at any sample, but which one is decided by the radiances in sample order alone: starting up to B
                // samples and folding them until the rule says stop (k_ad_accum) takes the same samples in the same order; the
                // surplus is discarded.  A handful of rounds instead of one per sample of a borderline pixel.
                // At least the certain ones, at most 8 on speculation -- but a pixel that comes back (the noisy few per cent) and could be
                // finished for good in this round gets everything it may still take: a round costs its tail (some 25 ms on a 1080p frame)
                // whatever its size, the surplus samples of those pixels cost next to nothing.
                const int rem = F.max_samples - s;
                n = min(min(B, rem), (s >= F.min_samples && rem <= B) ? rem : max(F.min_samples - samps, 8));
                s0 = s;
            }
            pix[i].n = n;
        }
        const int y = inside ? global_row(F, ly) : 0;
        for (int k = 0; k < B; k++) {                       // wave-uniform trip count: the appends below are collective
            const bool start = k < n;
            const uint32_t slot = i * (uint32_t)B + (uint32_t)k;
            if (start) {
                uint32_t idx;
                Ray ray = primary_ray(S, F, s0 + k, x, y, idx);
                pool_begin(pool, slot, ray, idx);
                slot_sample[slot] = slot;
            }
            const uint32_t at = wave_append(n_new, start);
            if (start) q_new[at] = slot;
        }
    }
}
__global__ __launch_bounds__(GI_BLOCK) void k_ad_accum(Frame F, PixRec* pix, const double* lbuf, uint32_t n_pix, int B, void* out, int out_f64,
                                                      int32_t* out_spp, unsigned int* n_wanting)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_round = (n_pix + 63u) & ~63u;
    for (uint32_t i0 = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < n_round; i0 += gridDim.x * blockDim.x) {
        const uint32_t i = i0 + lane;
        bool wants = false;
        int x, ly;
        if (i < n_pix && tile_pixel_xy(F, i, x, ly)) {
            PixRec r = pix[i];
            PixelState ps = pixrec_to_state(r);
            for (int k = 0; k < r.n && pixel_wants_sample(ps, F); k++) pixel_add_sample(ps, F, ld3(lbuf + ((size_t)i * B + k) * 3));
            state_to_pixrec(ps, r);
            r.n = 0;
            pix[i] = r;
            wants = pixel_wants_sample(ps, F);
            pixel_write(F, x, ly, ps, out, out_f64, out_spp);
        }
        (void)wave_append(n_wanting, wants);
    }
}

// ------------------------------------------------------------------------------------------------- streaming variant (fixed spp)
// When min_samples == max_samples every pixel takes exactly spp samples, so samples can be started in any order as long as
// they are folded into the running mean in sample order.  Path slots are refilled with the next unstarted sample as soon as
// their path ends (path regeneration): every pass works on a full pool and the straggler tail is paid once per frame, not
// once per round.  Finished paths write their radiance to Lbuf[sample]; k_st_accum folds Lbuf per pixel in sample order.
// sample id = s * n_pix + i  (i = 8x8-tile-ordered pixel index): consecutive ids are neighbouring pixels of one sample index.
struct StreamCtl {
    unsigned long long next_sample;   // next sample id to start
    unsigned int n_new, n_cont, n_shade, n_gather, n_free, n_free_trace;
};
// Queue appends.  One atomic per wave per loop turn on ONE counter is what these kernels used to do -- and a returning atomic on a single
// address completes every ~11 ns on this part (exp/atomic_bench.hip: 8.2 M of them take 93 ms), so the 8 M waves of a pass could not finish
// faster than that whatever else they did.  Now every workgroup appends to a counter of its own (the same 11 ns, but only its 8-16 waves
// contend) and writes into a segment of its own in a staging queue: the segment of workgroup b starts where the items of workgroups
// 0 .. b-1 would end if every one of them produced an entry (seg_start: pure arithmetic on the grid-stride loop), so segments can never
// overlap.  k_st_compact then closes the gaps -- a streaming copy of a few bytes per entry -- and leaves the total in StreamCtl.
#define GI_CNT_STRIDE 32   // counters 128 bytes apart
#define GI_MAX_PRODUCER_BLOCKS 2048
enum { QC_SHADE = 0, QC_CONT = 1, QC_GATHER = 2, QC_FREE = 3, QC_KINDS = 4 };
__device__ __forceinline__ unsigned int* blk_counter(unsigned int* bc, int kind) { return bc + ((size_t)kind * GI_MAX_PRODUCER_BLOCKS + blockIdx.x) * GI_CNT_STRIDE; }
// items the grid-stride loop `for (i0 = b * bs; i0 < n_in; i0 += grid * bs)` gives to workgroups 0 .. b-1, every chunk counted as full
__host__ __device__ __forceinline__ uint32_t seg_start(uint32_t b, uint32_t n_in, uint32_t grid, uint32_t bs)
{
    const uint32_t n_chunks = (n_in + bs - 1) / bs, full = n_chunks / grid, extra = n_chunks % grid;
    const uint32_t lo = b < extra ? b : extra;
    return (lo * (full + 1) + (b - lo) * full) * bs;
}
// The u-th item of this workgroup's share, in its own numbering (what its LDS counter hands out), as an index into the input queue: the workgroup's
// chunks of cs items are those of the grid-stride loop above, gridDim.x chunks apart.  One contract, three parties: seg_start counts these same chunks
// (as full) to place the workgroup's output segment, and k_st_compact reads the segments back through segs[] -- all must agree on cs and the grid.
__device__ __forceinline__ uint32_t chunk_item(uint32_t u, uint32_t cs) { return ((u / cs) * gridDim.x + blockIdx.x) * cs + u % cs; }

// a finished path gives its slot back (its radiance is already in the per-sample buffer: the stages accumulate there)
__device__ __forceinline__ void st_release(uint32_t slot, uint32_t* q_free, unsigned int* n_free, bool finished)
{
    const uint32_t at = wave_append(n_free, finished);
    if (finished) q_free[at] = slot;
}

// items are dealt to the workgroups of the wide instances in chunks (multiples of 64); measured on the benchmark frame: chunks of the workgroup's
// size are best (64: -5 %, 4 workgroup sizes: -8 %, 16: -26 %)
#ifndef GI_TRACE_CHUNK
#define GI_TRACE_CHUNK 1024
#endif
#ifndef GI_SHADE_CHUNK
#define GI_SHADE_CHUNK 512
#endif
#ifndef GI_GATHER_CHUNK
#define GI_GATHER_CHUNK 256
#endif
#ifndef GI_TRACE_BLOCK
#define GI_TRACE_BLOCK 1024
#endif
#ifndef GI_SHADOW_BLOCK
#define GI_SHADOW_BLOCK 1024
#endif
#ifndef GI_SHADOW_LEAF_MIN
#define GI_SHADOW_LEAF_MIN 16   // lanes of a wave that must stand on a leaf before k_st_shadow tests leaves (or nobody is left walking)
#endif
#define GI_SHADE_BLOCK 512
// New samples are started inside the trace kernel (path regeneration fused into the first trace of the path): item i < g.n_gen takes the
// i-th free slot and sample id g.id_base + i, builds its primary ray in registers and traces it at once -- a primary ray that misses
// never exists in memory (its radiance goes straight to lbuf and the slot straight back to the free list), one that hits is stored
// together with its hit.  Sample ids are consecutive per lane = neighbouring pixels of one 8x8 tile, so these waves are coherent.
// What a new path of pixel p needs before its ray can be made -- the pixel's place in the frame (st_pixel_xy: four divisions by run-time numbers) and
// the Halton index of its first sample (halton_index: a 64-bit remainder) -- is the same for all the samples of the pixel: one table per frame instead
// of ~300 instructions per primary ray.
__global__ void k_pixel_table(Frame F, uint32_t n_pix, uint32_t* out);
struct GenArgs {
    Frame F;
    const uint32_t* q_free;           // free slots to fill (nullptr: slots 0 .. n_gen - 1)
    uint32_t n_gen, n_pix;
    unsigned long long id_base, sample_begin;
    int s_begin;
    const uint32_t* pixtab;           // per pixel of this rank, tile order: the Halton index of its sample 0 (k_pixel_table)
    double inv_n_pix;
};
__global__ void k_pixel_table(Frame F, uint32_t n_pix, uint32_t* out)
{
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n_pix; p += gridDim.x * blockDim.x) {
        int x, ly;
        st_pixel_xy(F, p, x, ly);
        const int y = global_row(F, ly);
        out[p] = halton_index(F.he, 0u, (uint32_t)x, (uint32_t)y);
    }
}
// Wide-record instances keep the lanes of a wave on DIFFERENT rays: a lane whose walk is over waits until `refill_min` lanes of its wave
// are idle, then the idle lanes write their results and take the next items of the workgroup's share of the queue (an LDS counter), while
// the others walk on -- a wave no longer runs at the pace of its longest ray with the other lanes switched off (closed scenes: a third
// of the lanes were active per leaf step).  Waves of new paths (neighbouring pixels, leaves shared through the scalar cache) stay in
// lockstep: refill_min = 64 for them.  The workgroup's items are those of the grid-stride loop, so seg_start still bounds its output.
// The refill step of those waves (k_st_trace, k_st_shadow), by all 64 lanes once the kernel has decided to refill: the idle lanes (~busy) take the next items of the
// workgroup's share with one LDS atomic.  base: the first of them, wave-uniform; u: this lane's (chunk_item's numbering; idle lanes only, check it against total).
struct HandOut { uint32_t base, u; };
__device__ __forceinline__ HandOut hand_out(unsigned long long busy, unsigned int* s_next, uint32_t total, uint32_t lane, bool& more)
{
    const unsigned long long want = ~busy;
    const uint32_t nw = (uint32_t)__popcll(want);
    const int leader = __ffsll((long long)want) - 1;
    unsigned int base = 0;
    if ((int)lane == leader) base = atomicAdd(s_next, nw);
    base = (unsigned int)__shfl((int)base, leader);
    more = base + nw < total;
    return HandOut{base, base + (uint32_t)__popcll(want & ((1ull << lane) - 1ull))};
}
template <int FEAT, int WIDE, bool COUNT = false, bool LENS = false>   // LENS: new paths start on the thin lens (launched only when the context has one)
__global__ __launch_bounds__(GI_TRACE_BLOCK) void k_st_trace(Scene S, uint64_t seed, PathPool pool, unsigned long long* slot_sample, unsigned long long sample0,
                                                       GenArgs g, const uint32_t* q_a, uint32_t n_a, const uint32_t* q_b, uint32_t n_b, unsigned int* bc, uint32_t* segs,
                                                       uint32_t* q_shade, uint32_t* q_free, double* lbuf, uint32_t refill_min, StreamCounters* sc)
{
    static_assert(!COUNT || WIDE != 0, "the executed-work counters belong to the wide walk");
    // wide instances: next unfetched item of this workgroup, in its own numbering; lives in the 128 bytes the 292 wide records leave of the 64 KB
    static_assert(sizeof(WNode) == 224 && GI_LDS_WIDE_BOXES_BYTES <= 160 * 1024, "LDS layout of the wide trace / shadow kernels");
    unsigned int* const s_next = reinterpret_cast<unsigned int*>(gi_dyn_lds + GI_LDS_BIG_CNT_OFF);
    if (WIDE != 0 && threadIdx.x == 0) *s_next = 0u;
    const typename LdsSrc<WIDE, COUNT>::type N = LdsSrc<WIDE, COUNT>::stage_for_trace(S);   // ends with a barrier
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_in = g.n_gen + n_a + n_b;
    uint32_t n_rays = 0;   // COUNT: items this lane took
    const uint32_t cs = WIDE != 0 ? (uint32_t)GI_TRACE_CHUNK : blockDim.x;
    const uint32_t seg = seg_start(blockIdx.x, n_in, gridDim.x, cs);   // this workgroup's segment of the staging queues
    if (threadIdx.x == 0) segs[blockIdx.x] = seg;
    unsigned int* const c_shade = blk_counter(bc, QC_SHADE);
    unsigned int* const c_free = blk_counter(bc, QC_FREE);
    // one item: a new path (sample id -> primary ray) or a continuing one (ray from its record)
    auto fetch = [&](uint32_t i, uint32_t& slot, Ray& ray, uint32_t& stream, int32_t& depth) {
        if (i < g.n_gen) {
            slot = g.q_free ? g.q_free[i] : i;
            const unsigned long long id = g.id_base + i;
            // ids of one chunk span less than 2^32 (the radiance buffer bounds the chunk): 32-bit division instead of 64-bit
            const uint32_t rel = (uint32_t)(id - g.sample_begin);
            uint32_t srel = (uint32_t)((double)rel * g.inv_n_pix);               // rel / n_pix: the quotient of the doubles, put right by one step either way
            if ((unsigned long long)srel * g.n_pix > rel) srel--;
            else if ((unsigned long long)(srel + 1u) * g.n_pix <= rel) srel++;
            stream = g.pixtab[rel - srel * g.n_pix] + (uint32_t)(g.s_begin + (int)srel) * g.F.he.inc;        // halton_index(he, s, x, y) = its value for s = 0 + s * inc
            ray = primary_ray_at<LENS || COUNT>(S, g.F, stream);
            depth = 0;
        } else {
            slot = i - g.n_gen < n_a ? q_a[i - g.n_gen] : q_b[i - g.n_gen - n_a];
            const PoolRay& p = pool.ray[slot];
            ray = make_ray_exact(ld3(p.o), ld3(p.d));
            stream = p.stream; depth = p.depth;
        }
    };
    // what a finished walk leaves behind: the hit in the record (a new path's record is created here), or the end of the path
    auto retire = [&](uint32_t i, uint32_t slot, const Ray& ray, uint32_t stream, int32_t depth, bool hit, const HitRec& h) {
        const bool gen = i < g.n_gen;
        if (hit) {
            PoolHit p;                                    // put together in registers, stored whole
            if (gen) { pool_begin(pool, slot, ray, stream); if (slot_sample) slot_sample[slot] = g.id_base + i; }
            if constexpr (WIDE != 0) {
                // the walk carries only WHICH entity it hit: hit point and barycentrics are computed again here, by the same test with the same
                // operands -- ten registers less to hold through the walk (the kernel runs at the 128 its four waves per SIMD leave it)
                double ru = 0, rv = 0;
                V3 rp = v3(0, 0, 0);
                const TriGeom& tg = S.tris[h.tri];
                const uint32_t mf = ((uint32_t)tg.mat << 3) | tg.flags;      // = LeafTri::matflags of every reference to it
                ent_hit<FEAT>(tg, mf, ray, ru, rv, rp);
                p.hpos[0] = rp.x; p.hpos[1] = rp.y; p.hpos[2] = rp.z;
                p.hu = ru; p.hv = rv; p.htri = h.tri; p.mf = mf;
            } else {
            p.hpos[0] = h.pos.x; p.hpos[1] = h.pos.y; p.hpos[2] = h.pos.z;
            p.hu = h.u; p.hv = h.v; p.htri = h.tri; p.mf = h.mf;
            }
            pool.hit[slot] = p;
            if (FEAT & GI_FEAT_TEX) { pool.gath[slot].gdir[0] = h.tu; pool.gath[slot].gdir[1] = h.tv; }   // minUV rides in the (idle between gather and shade) gather fields
        } else if (depth <= GI_MAX_DEPTH) {
            // the path ends here with a miss: L += T * ambient (stage_trace_nodes), on the per-sample radiance buffer where the path's L lives.
            // A path at depth 0 writes (L = 0, T = 1 by definition); a deeper one adds -- and when the scene has no ambient light there is nothing
            // to add (L + T * 0 = L: L is a sum of non-negative terms and photon terms, never -0), so the record's tail, the sample id and
            // the buffer are not touched at all: this is what 96 % of the benchmark's reflected rays do.
            const V3 amb = ld3(S.ambient);
            if (depth == 0) {   // generated here, or handed in by the adaptive loop's generator (k_ad_gen)
                const V3 L = v3(0, 0, 0) + v3(1, 1, 1) * amb;
                const unsigned long long id = gen ? g.id_base + i : sample_of(slot_sample, sample0, slot);
                double* o = lbuf + (id - sample0) * 3;
                o[0] = L.x; o[1] = L.y; o[2] = L.z;
            } else if (amb.x != 0.0 || amb.y != 0.0 || amb.z != 0.0) {
                double* o = lbuf + (sample_of(slot_sample, sample0, slot) - sample0) * 3;
                const V3 L = ld3(o) + ld3(pool.thru[slot].T) * amb;
                o[0] = L.x; o[1] = L.y; o[2] = L.z;
            }
        }
    };
    if constexpr (WIDE != 0) {
        const uint32_t bs = cs;
        const uint32_t total = seg_start(blockIdx.x + 1, n_in, gridDim.x, bs) - seg;   // this workgroup's chunks, counted as full
        bool walking = false, pend = false;
        uint32_t item = 0, slot = 0, stream = 0;
        int32_t depth = 0;
        Ray ray = make_ray_exact(v3(0, 0, 0), v3(1, 0, 0));
        TraceWalk t;
        t.intersected = false;
        HitRec h;
        bool more = true;            // wave-uniform: the workgroup may still have items
        uint32_t thr = 64u;          // wave-uniform: idle lanes that trigger a refill
        for (;;) {
            const unsigned long long busy = __ballot(walking);
            if (busy == 0ull || (more && 64u - (uint32_t)__popcll(busy) >= thr)) {
                const bool hit = pend && t.intersected, fin = pend && !t.intersected;
                if (pend) retire(item, slot, ray, stream, depth, hit, h);
                const uint32_t at = wave_append(c_shade, hit);
                if (hit) q_shade[seg + at] = slot;
                if (q_free) {        // (a kernel argument: null when nothing will read this pass's free list, stream_passes)
                    const uint32_t af = wave_append(c_free, fin);
                    if (fin) q_free[seg + af] = slot;
                }
                pend = false;
                if (more) {
                    const HandOut f = hand_out(busy, s_next, total, lane, more);
                    // first item this fetch hands out: new paths run in lockstep, continuing ones refill
                    thr = chunk_item(f.base, bs) < g.n_gen ? 64u : refill_min;
                    if (!walking) {
                        const uint32_t i = chunk_item(f.u, bs);
                        if (f.u < total && i < n_in) {
                            item = i;
                            if constexpr (COUNT) n_rays++;
                            fetch(i, slot, ray, stream, depth);
                            t.intersected = false;
                            pend = true;          // over already (past MAX_DEPTH radiance() returns 0; a ray that misses the scene's box) unless the walk starts
                            if (depth <= GI_MAX_DEPTH && trace_wide_begin<FEAT>(S, N, ray, t)) { walking = true; pend = false; }
                        }
                    }
                }
                if (__ballot(walking || pend) == 0ull) break;
            }
            if (walking) {
                Rng rng = rng_make(seed, stream);      // only an entity with an alpha test draws: built where it is used, not held through the walk
                rng.depth = (uint32_t)depth;
                if (!trace_wide_step<FEAT>(S, N, ray, rng, P_TRACE_ALPHA, t, h)) { walking = false; pend = true; }
            }
        }
    } else {
        for (uint32_t i0 = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < n_in; i0 += gridDim.x * blockDim.x) {
            const uint32_t i = i0 + lane;
            bool hit = false, fin = false;
            uint32_t slot = 0;
            if (i < n_in) {
                Ray ray;
                uint32_t stream;
                int32_t depth = 0;
                fetch(i, slot, ray, stream, depth);
                HitRec h;
                if (depth <= GI_MAX_DEPTH) {            // radiance() returns 0 past MAX_DEPTH
                    Rng rng = rng_make(seed, stream);
                    rng.depth = (uint32_t)depth;
                    hit = trace_nodes<FEAT>(S, N, ray, rng, P_TRACE_ALPHA, h, nullptr);
                }
                fin = !hit;
                retire(i, slot, ray, stream, depth, hit, h);
            }
            const uint32_t at = wave_append(c_shade, hit);
            if (hit) q_shade[seg + at] = slot;
            if (q_free) {
                const uint32_t af = wave_append(c_free, fin);
                if (fin) q_free[seg + af] = slot;
            }
        }
    }
#ifdef GI_EXP_DIV
    if constexpr (WIDE != 0) div_flush(N, 0);
#endif
    if constexpr (COUNT) { flush_walk_cnt(sc->trace, N.wc); flush_u64(&sc->trace_rays, n_rays); }
}

__global__ void k_iota(uint32_t* v, uint32_t n) { for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) v[i] = i; }

// the walk-free instance fits its registers at 2 waves per SIMD without a spill and runs fastest that way (round 2, records: 4 waves 260 B of scratch per
// lane, 144 ms on the benchmark; 3 waves 128 ms; 2 waves 128 ms.  Round 3, field arrays, the path held in registers: 229 VGPRs, 58 ms at 2 waves; 3 waves
// spill 212 B: 65 ms)
#ifndef GI_DEFER_WAVES
#define GI_DEFER_WAVES 2
#endif
template <int FEAT, int WIDE, int DEFER>
__global__ __launch_bounds__(GI_SHADE_BLOCK, DEFER ? GI_DEFER_WAVES : 4) void k_st_shade(Scene S, uint64_t seed, PathPool pool, const unsigned long long* slot_sample, unsigned long long sample0,
                                                       const uint32_t* q_shade, const StreamCtl* ctl, unsigned int* bc, uint32_t* segs, uint32_t* q_cont, uint32_t* k_cont, uint32_t* q_gather, double* g_pos,
                                                       uint32_t* q_free, double* lbuf, ShadowQ* shq, const uint32_t* q_orig, uint32_t early_turns)
{
    // the waves of a workgroup take its items 64 at a time from a counter in LDS (in the 128 bytes the wide records leave free) instead of
    // a fixed share each: a wave that drew cheap items takes more of them
    unsigned int* const s_next = reinterpret_cast<unsigned int*>(gi_dyn_lds + (DEFER == 1 ? (size_t)GI_LDS_BIG_CNT_OFF : (size_t)GI_LDS_WNODES * sizeof(WNode)));
    if (WIDE != 0 && threadIdx.x == 0) *s_next = 0u;
    typename LdsSrc<WIDE>::type N;
    // early_turns != 0 (stream_passes): the next ray of a vertex is walked for up to that many turns (ray_leaves_scene, gi_walk.h); one that leaves
    // the scene without meeting a leaf ends its path here.  The walk is the trace stage's, over the trace stage's tables: NP is staged as k_st_trace stages N.
    // One-light instance only (DEFER 1): the several-lights instances have no registers to spare for a walk, and are always handed 0
    typename LdsSrc<WIDE>::type NP;
    if constexpr (DEFER != 0) {   // no shadow walk in this instance: the records stay where they are unless the probe wants them
        N.g = S.wnodes; N.cboxes = S.cboxes; N.cuse = S.cuse; N.n_l = 0;
        if (DEFER == 1 && early_turns != 0u) NP = LdsSrc<WIDE>::stage_for_trace(S);   // ends with a barrier
        else { NP = N; __syncthreads(); }
    } else {
        N = LdsSrc<WIDE>::stage(S);   // ends with a barrier
        NP = N;
    }
    const uint32_t n_in = ctl->n_shade;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t cs = WIDE != 0 ? (uint32_t)GI_SHADE_CHUNK : blockDim.x;
    const uint32_t seg = seg_start(blockIdx.x, n_in, gridDim.x, cs);   // this workgroup's segment of the staging queues (k_st_trace)
    if (threadIdx.x == 0) segs[blockIdx.x] = seg;
    unsigned int* const c_cont = blk_counter(bc, QC_CONT);
    unsigned int* const c_gather = blk_counter(bc, QC_GATHER);
    unsigned int* const c_free = blk_counter(bc, QC_FREE);
    const uint32_t total = seg_start(blockIdx.x + 1, n_in, gridDim.x, cs) - seg;   // this workgroup's chunks of the grid-stride loop, counted as full
    for (uint32_t w = threadIdx.x >> 6;; w += blockDim.x >> 6) {
        uint32_t u = w * 64u;
        if (WIDE != 0) {
            unsigned int b = 0;
            if (lane == 0) b = atomicAdd(s_next, 64u);
            u = (uint32_t)__shfl((int)b, 0);
        }
        if (u >= total) break;
        const uint32_t i = chunk_item(u, cs) + lane;
        int fl = 0;
        bool valid = i < n_in;
        uint32_t slot = 0;
        ShadeOut so;
        so.key = 0; so.gpos = v3(0, 0, 0);
        if (valid) {
            slot = q_shade[i];
            if constexpr (DEFER != 0) {
                const int nl = DEFER == 2 ? S.n_light : 1;          // one query per light, the queries of item i side by side
                ShadowQ* const e = shq + (size_t)(q_orig ? q_orig[i] : i) * (size_t)nl;   // q_orig: the item's place in the queue the shadow kernel follows (the trace stage's order)
                // the path in registers: its arrays are read up front, whole records at a time (the loads of one vertex in flight together), and
                // written back as whole records -- only those the vertex changed, and nothing at all for a path that ends here
                PathRec p;
                {
                    const PoolRay r = pool.ray[slot];
                    const PoolHit h = pool.hit[slot];
                    for (int k = 0; k < 3; k++) { p.o[k] = r.o[k]; p.d[k] = r.d[k]; p.hpos[k] = h.hpos[k]; }
                    p.stream = r.stream; p.depth = r.depth; p.htri = h.htri; p.pad = h.mf; p.hu = h.hu; p.hv = h.hv;
                    if (r.depth != 0) { const PoolThru t = pool.thru[slot]; for (int k = 0; k < 3; k++) { p.T[k] = t.T[k]; p.contrib[k] = t.contrib[k]; } }
                    if (FEAT & GI_FEAT_TEX) { p.gdir[0] = pool.gath[slot].gdir[0]; p.gdir[1] = pool.gath[slot].gdir[1]; }
                }
                const V3 hp0 = ld3(p.hpos);
                p.L[0] = NAN;                                       // (written only for an emitting surface: its A0, a finite number)
                ShadowQ ql;                                         // one light: the query is put together in registers too and stored whole
                ql.pad = 0u;
                if constexpr (DEFER == 1) fl = stage_shade_nodes<FEAT, typename LdsSrc<WIDE>::type, DEFER>(S, N, p, seed, nullptr, &so, nullptr, &ql);
                else
                fl = stage_shade_nodes<FEAT, typename LdsSrc<WIDE>::type, DEFER>(S, N, p, seed, nullptr, &so, nullptr, e);
                // what does not depend on the probe goes out first (its registers are free for the walk): the shadow query, the gather query, A0
                if constexpr (DEFER == 1) { ql.idx = (uint32_t)(sample_of(slot_sample, sample0, slot) - sample0); ql.slot = slot; *e = ql; }
                else
                for (int li = 0; li < nl; li++) { e[li].idx = (uint32_t)(sample_of(slot_sample, sample0, slot) - sample0); e[li].slot = slot; }
                if (fl != 0) {
                    if (fl & ST_GATHER) {
                        PoolGath gq;
                        for (int k = 0; k < 3; k++) { gq.gdir[k] = p.gdir[k]; gq.gcoef[k] = p.gcoef[k]; }
                        pool.gath[slot] = gq;
                    }
                    if (p.L[0] == p.L[0]) { double* Lp = pool.L + (size_t)slot * 3; Lp[0] = p.L[0]; Lp[1] = p.L[1]; Lp[2] = p.L[2]; }   // A0 of an emitting surface waits there for k_st_shadow
                    // the next ray as the trace stage would read it back; "leaves" = its walk ends without a leaf: the miss adds nothing (no ambient
                    // light, stream_passes), so the path ends here -- no ray, no throughput, no queue entry, no key
                    if (DEFER == 1 && early_turns != 0u && (fl & ST_CONTINUE) && ray_leaves_scene(S, NP, make_ray_exact(ld3(p.o), ld3(p.d)), (int)early_turns)) fl &= ~ST_CONTINUE;
                    if (early_turns == 0u || (fl & ST_CONTINUE)) {
                        PoolRay r;
                        for (int k = 0; k < 3; k++) { r.o[k] = p.o[k]; r.d[k] = p.d[k]; }
                        r.stream = p.stream; r.depth = p.depth; r.pad_[0] = 0u; r.pad_[1] = 0u;
                        pool.ray[slot] = r;
                        PoolThru t;
                        for (int k = 0; k < 3; k++) { t.T[k] = p.T[k]; t.contrib[k] = p.contrib[k]; }
                        pool.thru[slot] = t;
                    }
                }
                if ((FEAT & GI_FEAT_FOG) && (p.hpos[0] != hp0.x || p.hpos[1] != hp0.y || p.hpos[2] != hp0.z)) {   // the segment ended in the medium: the gather of this vertex uses the scatter point
                    PoolHit& h = pool.hit[slot];
                    h.hpos[0] = p.hpos[0]; h.hpos[1] = p.hpos[1]; h.hpos[2] = p.hpos[2];
                }
            } else {
                PathRef pr = pool[slot];
                fl = stage_shade_nodes<FEAT>(S, N, pr, seed, nullptr, &so, lbuf + (sample_of(slot_sample, sample0, slot) - sample0) * 3);
            }
        }
        // a path with a pending gather stays alive one more pass even when it may not continue: the trace stage retires it.  With the probe on it
        // is released here: the gather adds to lbuf[slot_sample[slot]] and reads the slot's hit and gather fields, and the free list of this pass is
        // first read by the trace kernel of the next one, which the stream runs after this pass's shadow and gather kernels
        const bool cont = valid && (fl & (early_turns != 0u ? ST_CONTINUE : (ST_CONTINUE | ST_GATHER))) != 0;
        const uint32_t a = wave_append(c_cont, cont);
        if (cont) { q_cont[seg + a] = slot; k_cont[seg + a] = so.key; }   // the key of the next ray, from the registers that just held it
        const uint32_t g = wave_append(c_gather, (fl & ST_GATHER) != 0);
        if (fl & ST_GATHER) {
            // the gather query's position goes into the queue as well: the key kernel then reads 24 consecutive bytes per query
            // instead of one scattered sector of the path pool (that read alone kept it at HBM speed)
            q_gather[seg + g] = slot;
            g_pos[(size_t)(seg + g) * 3] = so.gpos.x; g_pos[(size_t)(seg + g) * 3 + 1] = so.gpos.y; g_pos[(size_t)(seg + g) * 3 + 2] = so.gpos.z;
        }
        if (q_free) st_release(slot, q_free + seg, c_free, valid && !cont);   // null: nothing will read this pass's free list (stream_passes)
    }
#ifdef GI_EXP_DIV
    if constexpr (WIDE != 0) div_flush(N, 1);
#endif
}

// The shadow queries the shade stage put off (ShadowQ, entry i = item i of the shade queue): RayTracer::visible towards the scene's one
// light, then L += A where the light is visible.  Lanes work like k_st_trace's: whoever has his answer waits until `refill_min` lanes of
// the wave are idle, then they write their results and take the next queries of the workgroup's share.  Inside the shade kernel these walks
// ran with 15-40 % of the lanes (a wave waited for its longest segment, under the register pressure of the whole shade stage).
// MULTI: several lights -- the reference keeps the share of the LAST visible light of a vertex, so a lane asks the item's queries from the last light
// down and stops at the first visible one (the medium's answer is then needed at the end of each walk, not only when the lane retires).
template <int FEAT, int MULTI, bool COUNT = false>
__global__ __launch_bounds__(GI_SHADOW_BLOCK) void k_st_shadow(Scene S, uint64_t seed, PathPool pool, const ShadowQ* shq, const StreamCtl* ctl, double* lbuf, uint32_t refill_min, StreamCounters* sc)
{
    const uint32_t nl = MULTI ? (uint32_t)S.n_light : 1u;
    uint32_t li = 0;   // the light this lane's walk is about
    unsigned int* const s_next = reinterpret_cast<unsigned int*>(gi_dyn_lds + GI_LDS_BIG_CNT_OFF);
    if (threadIdx.x == 0) *s_next = 0u;
    const LdsWideT<COUNT> N = stage_wide_in_lds<COUNT>(S, true, GI_LDS_WNODES_BIG, 2);   // ends with a barrier; every segment of this kernel ends at a light
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_in = ctl->n_shade, bs = (uint32_t)GI_TRACE_CHUNK;
    uint32_t n_rays = 0;   // COUNT: shadow segments this lane walked
    const uint32_t total = seg_start(blockIdx.x + 1, n_in, gridDim.x, bs) - seg_start(blockIdx.x, n_in, gridDim.x, bs);
    bool walking = false, pend = false, blocked = false;
    uint32_t item = 0;
    Ray ray = make_ray_exact(v3(0, 0, 0), v3(1, 0, 0));
    double mt = 0;
    Rng rng = rng_make(seed, 0);
    VisWalk v;
    bool at_leaf = false;
    int32_t lnode = 0, first = 0, cnt = 0;
    int lslot = 0;
    const uint32_t leaf_min = GI_SHADOW_LEAF_MIN;
    bool more = true;   // wave-uniform
    for (;;) {
        const unsigned long long busy = __ballot(walking);
        if (busy == 0ull || (more && 64u - (uint32_t)__popcll(busy) >= refill_min)) {
            if (pend) {
                const ShadowQ& e0 = shq[(size_t)item * nl];          // the item's first query carries what belongs to the vertex
                const ShadowQ& e = shq[(size_t)item * nl + li];      // the query of the light that won (or of light 0 when none did)
                const bool vis = !blocked && (MULTI ? true : visible_through_fog<FEAT>(S, ray, mt, rng, 0u));
                double* o = lbuf + (size_t)e.idx * 3;
                if (e.depth == 0 || vis || e0.live == 2u) {
                    // L += T * (color * i + emissive): i = the light's share when it is visible (A), else 0 (A0: zero unless the surface emits,
                    // and then L + 0 = L is not worth a write -- except at depth 0, where L = 0 + ... starts the sum)
                    const V3 add = vis ? ld3(e.A) : (e0.live == 2u ? ld3(pool.L + (size_t)e.slot * 3) : v3(0, 0, 0));
                    const V3 L = (e.depth == 0 ? v3(0, 0, 0) : ld3(o)) + add;
                    o[0] = L.x; o[1] = L.y; o[2] = L.z;
                }
                pend = false;
            }
            if (more) {
                const HandOut f = hand_out(busy, s_next, total, lane, more);
                if (!walking) {
                    const uint32_t i = chunk_item(f.u, bs);
                    if (f.u < total && i < n_in && shq[(size_t)i * nl].live) {
                        li = nl - 1u;
                        const ShadowQ& e = shq[(size_t)i * nl + li];
                        item = i;
                        if constexpr (COUNT) n_rays++;
                        const V3 dir = ld3(e.dir);
                        ray = make_ray(ld3(e.o), dir);
                        mt = len2(dir);
                        rng = rng_make(seed, e.stream);
                        rng.depth = (uint32_t)e.depth;
                        blocked = false;
                        pend = true;      // answered already when the segment misses the scene's box
                        if (visible_wide_begin<FEAT>(S, N, ray, mt, v)) { walking = true; pend = false; at_leaf = false; }
                        else if constexpr (MULTI != 0) blocked = !visible_through_fog<FEAT>(S, ray, mt, rng, li);
                    }
                }
            }
            if (__ballot(walking || pend) == 0ull) break;
        }
        // One turn of the walk for every lane that is between leaves; a lane that reaches a leaf waits there until `leaf_min` lanes stand on
        // one (or nobody is left walking), then those test their leaves' triangles together.  A shadow segment takes some ten turns per leaf
        // it meets: run as "walk to the next leaf, test it" per lane, the turns of a wave ran at the pace of its slowest lane.
        if (walking && !at_leaf) {
            const int r = wwalk_turn(N, v.k, ray, v.wr, 0.0, v.tmax, lnode, lslot, first, cnt);
            if (r == WALK_LEAF) at_leaf = true;
            else if (r == WALK_END) {
                walking = false; pend = true; blocked = false;
                if constexpr (MULTI != 0) blocked = !visible_through_fog<FEAT>(S, ray, mt, rng, li);
            }
        }
        const unsigned long long lf = __ballot(walking && at_leaf);
        if (lf != 0ull && ((uint32_t)__popcll(lf) >= leaf_min || __ballot(walking && !at_leaf) == 0ull)) {
            if (walking && at_leaf) {
                at_leaf = false;
                if (visible_leaf_blocks<FEAT>(S, N, ray, mt, rng, li, lnode, lslot, first, cnt, S.shadow_boxes)) { walking = false; pend = true; blocked = true; }
            }
        }
        if constexpr (MULTI != 0) {   // this light is hidden: on to the one before it, in the same lane
            while (pend && blocked && li > 0u) {
                li--;
                if constexpr (COUNT) n_rays++;
                const ShadowQ& e = shq[(size_t)item * nl + li];
                const V3 dir = ld3(e.dir);
                ray = make_ray(ld3(e.o), dir);
                mt = len2(dir);
                blocked = false;
                at_leaf = false;
                if (visible_wide_begin<FEAT>(S, N, ray, mt, v)) { walking = true; pend = false; }
                else blocked = !visible_through_fog<FEAT>(S, ray, mt, rng, li);   // the segment misses the scene's box: only the medium can hide the light
            }
        }
    }
#ifdef GI_EXP_DIV
    div_flush(N, 1);
#endif
    if constexpr (COUNT) { flush_walk_cnt(sc->shadow, N.wc); flush_u64(&sc->shadow_rays, n_rays); }
}

// Closes the gaps between the workgroups' segments of up to three staging queues (one launch per producer kernel).  Stream k copies
// width[k] 4-byte words per entry from src[k] to dst[k]; entry t of the dense queue is entry (t - prefix[r]) of segment r.  Every
// workgroup recomputes the prefix sums of the (at most 2048) per-workgroup counts in LDS; workgroup 0 leaves the totals in StreamCtl.
// The queue of gather queries is not copied but turned into the input of its sort: (key = photon-map leaf that contains the query's
// position, value = slot) -- PhotonMap::Node::getBounds' descent (gather_find_leaf) runs here, on positions read in queue order.
// Gather queries are sorted by the leaf of the photon octree they fall in; only leaves that have candidate photons matter (a query anywhere else
// adds nothing), so the sort key is the leaf's rank among those -- 15 bits for the 200 000-photon map of the benchmark (27 k such leaves of 72 k
// nodes: two 8-bit digit passes of the radix sort instead of three) -- and every other query gets the one key past them.  One workgroup, at upload.
__global__ __launch_bounds__(1024) void k_pleaf_rank(const PNode* nodes, int32_t n, int32_t* rank, int32_t* inv, int32_t* n_out)
{
    __shared__ int32_t part[1024];
    __shared__ int32_t base;
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    for (int32_t i0 = 0; i0 < n; i0 += 1024) {
        const int32_t i = i0 + (int32_t)threadIdx.x;
        const int32_t f = (i < n && nodes[i].first_child < 0 && nodes[i].u.lf.nb_photons > 0) ? 1 : 0;
        part[threadIdx.x] = f;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {   // inclusive prefix sums
            const int32_t v = threadIdx.x >= (unsigned)o ? part[threadIdx.x - o] : 0;
            __syncthreads();
            part[threadIdx.x] += v;
            __syncthreads();
        }
        if (i < n) {
            const int32_t r = base + part[threadIdx.x] - 1;
            rank[i] = f ? r : -1;
            if (f) inv[r] = i;
        }
        __syncthreads();
        if (threadIdx.x == 1023) base += part[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) *n_out = base;
}
// The candidate lists written out (k_st_gather stages a leaf's candidates 64 at a time, one per lane: a lane that has to find "candidate number k" by
// walking the leaf's range list reads its range records one after the other; k_st_gather_wave deals a leaf's candidates to the lanes of a wave).
__global__ __launch_bounds__(256) void k_pcand_count(const PNode* nodes, const int32_t* inv, int32_t n_pleaf, uint32_t* cnt)
{
    const int32_t r = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (r <= n_pleaf) cnt[r] = r < n_pleaf ? (uint32_t)nodes[inv[r]].u.lf.nb_photons : 0u;
}
__global__ __launch_bounds__(256) void k_pcand_fill(const PNode* nodes, const PRange* pranges, const double* ph_pos, const double* ph_dircol, const int32_t* inv, int32_t n_pleaf, const uint32_t* off,
                                                   double* out_pos, double* out_dc)
{
    // a wave per leaf: its ranges one after the other, a range's photons across the lanes
    const int32_t wave = (int32_t)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = (int32_t)(threadIdx.x & 63u), n_waves = (int32_t)((gridDim.x * blockDim.x) >> 6);
    for (int32_t r = wave; r < n_pleaf; r += n_waves) {
        const PNode& lf = nodes[inv[r]];
        const PRange* ranges = pranges + lf.nb_off;
        uint32_t at = off[r];
        for (int32_t k = 0; k < lf.u.lf.nb_cnt; k++) {
            const PRange rg = ranges[k];
            for (int32_t j = lane; j < rg.count; j += 64) {          // the photon itself, not its index: one read less between a leaf and its candidates
                const size_t src = (size_t)(rg.first + j), dst = (size_t)at + (size_t)j;
                for (int k = 0; k < 3; k++) out_pos[dst * 3 + k] = ph_pos[src * 3 + k];
                for (int k = 0; k < 6; k++) out_dc[dst * 6 + k] = ph_dircol[src * 6 + k];
            }
            at += (uint32_t)rg.count;
        }
    }
}
__global__ __launch_bounds__(256) void k_pdescent(const PNode* nodes, int32_t n, PDescent* out)
{
    const int32_t i = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    PDescent d;
    d.mid[0] = nodes[i].mid[0]; d.mid[1] = nodes[i].mid[1]; d.mid[2] = nodes[i].mid[2];
    d.first_child = nodes[i].first_child; d.pad = 0;
    out[i] = d;
}
// The jump table of gather_find_leaf_fast: for every cell of a grid of GI_PJUMP_N^3 cells over the map's box the node GI_PJUMP_BITS levels down (or the leaf above that) on the way of
// the cell's centre.  *bad is raised when a split plane met on the way is not the grid's plane of that level to within 1e-12 of the extent (the reference
// computes "the middle" in three ways that differ in the last bit, no more): the table is then not used.
__global__ __launch_bounds__(256) void k_pjump(const PDescent* pd, const double* bmin3, const double* cell3, double eps, int32_t* out, int* bad)
{
    const int32_t i = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= GI_PJUMP_N * GI_PJUMP_N * GI_PJUMP_N) return;
    const int cell[3] = {i & (GI_PJUMP_N - 1), i >> (2 * GI_PJUMP_BITS), (i >> GI_PJUMP_BITS) & (GI_PJUMP_N - 1)};       // x fastest, then z, then y
    int32_t node = 0;
    for (int level = 0; level < GI_PJUMP_BITS; level++) {
        const PDescent nd = pd[node];
        if (nd.first_child < 0) break;
        int k = 0;
        for (int ax = 0; ax < 3; ax++) {
            const int top = cell[ax] >> (GI_PJUMP_BITS - 1 - level);                                        // the cell's index among this level's 2^(level+1) halves
            const double plane = bmin3[ax] + (double)(((top >> 1) * 2 + 1) << (GI_PJUMP_BITS - 1 - level)) * cell3[ax];   // the grid's middle of the node's interval
            if (!(fabs(nd.mid[ax] - plane) <= eps)) *bad = 1;
            if (top & 1) k |= ax == 0 ? 1 : (ax == 2 ? 2 : 4);
        }
        node = nd.first_child + k;
    }
    out[i] = node;
}
struct CompactStream { const uint32_t* src; uint32_t* dst; int width; };
struct CompactJob {
    CompactStream st[5];    // streams of queue A (e.g. slot + key), then queue B, queue C: n_streams[q] streams each
    int n_streams[3];
    int kind[3];            // QC_* counter of each queue, -1 = unused
    int total_field[3];     // which StreamCtl field receives the total: 0 n_shade, 1 n_cont, 2 n_gather, 3 n_free (+ base), 4 n_free_trace
    int free_base_from_trace;   // queue with total_field 3 appends behind ctl->n_free_trace
    int gather_queue;       // index of the queue whose streams are (slot, position): dst of stream 0 = values, dst of stream 1 = keys; -1 = none
};
__global__ __launch_bounds__(256) void k_st_compact(Scene S, CompactJob job, const unsigned int* bc, const uint32_t* segs, uint32_t n_blocks, StreamCtl* ctl)
{
    __shared__ uint32_t prefix[GI_MAX_PRODUCER_BLOCKS + 1];
    __shared__ uint32_t part[256];
    int stream0 = 0;
    for (int q = 0; q < 3; q++) {
        if (job.kind[q] < 0) { stream0 += job.n_streams[q]; continue; }   // an unused queue still owns its streams: the next queue's begin behind them
        const unsigned int* cnt = bc + (size_t)job.kind[q] * GI_MAX_PRODUCER_BLOCKS * GI_CNT_STRIDE;
        // exclusive prefix sums of the per-workgroup counts: thread t owns counts [t * per, t * per + per)
        const uint32_t per = (n_blocks + 255u) / 256u;
        __syncthreads();
        {
            uint32_t acc = 0;
            for (uint32_t k = 0; k < per; k++) { const uint32_t b = threadIdx.x * per + k; if (b < n_blocks) acc += cnt[(size_t)b * GI_CNT_STRIDE]; }
            part[threadIdx.x] = acc;
        }
        __syncthreads();
        if (threadIdx.x == 0) { uint32_t acc = 0; for (int t = 0; t < 256; t++) { const uint32_t v = part[t]; part[t] = acc; acc += v; } prefix[n_blocks] = acc; }
        __syncthreads();
        {
            uint32_t acc = part[threadIdx.x];
            for (uint32_t k = 0; k < per; k++) { const uint32_t b = threadIdx.x * per + k; if (b < n_blocks) { prefix[b] = acc; acc += cnt[(size_t)b * GI_CNT_STRIDE]; } }
        }
        __syncthreads();
        const uint32_t total = prefix[n_blocks];
        const uint32_t base = (job.total_field[q] == 3 && job.free_base_from_trace) ? ctl->n_free_trace : 0u;
        // Every workgroup copies one contiguous run of output positions, a multiple of the workgroup's size long; a thread's positions are 256 apart.
        // Its producer segment lo (largest r with prefix[r] <= t) is searched for once; from one position to the next it stays, or moves on by the
        // one comparison below -- and only a thread that steps over the end of a segment searches again, in what lies ahead.
        const unsigned long long run = (((unsigned long long)total + gridDim.x - 1u) / gridDim.x + 255ull) & ~255ull;   // (64 bits: total may be close to 2^32)
        const uint32_t t_begin = (uint32_t)(blockIdx.x * run < total ? blockIdx.x * run : total);
        const uint32_t t_end = (uint32_t)(t_begin + run < total ? t_begin + run : total);
        uint32_t lo = 0, seg_end = 0, seg_off = 0;                  // prefix[lo + 1]; segs[lo] - prefix[lo] (mod 2^32): from = t + seg_off
        for (uint32_t t = t_begin + threadIdx.x; t < t_end; t += blockDim.x) {
            if (t >= seg_end) {
                uint32_t hi = n_blocks;
                while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (prefix[mid] <= t) lo = mid; else hi = mid; }
                seg_end = prefix[lo + 1];
                seg_off = segs[lo] - prefix[lo];
            }
            const size_t from = (size_t)(uint32_t)(t + seg_off), to = (size_t)base + t;
            if (q == job.gather_queue) {
                const CompactStream& sl = job.st[stream0];
                const double* pos = reinterpret_cast<const double*>(job.st[stream0 + 1].src) + from * 3;
                const uint32_t key = gather_key(S, v3(pos[0], pos[1], pos[2]));
                sl.dst[to] = sl.src[from];
                job.st[stream0 + 1].dst[to] = key;
                continue;
            }
            for (int k = 0; k < job.n_streams[q]; k++) {
                const CompactStream& cs = job.st[stream0 + k];
                for (int w = 0; w < cs.width; w++) cs.dst[to * cs.width + w] = cs.src[from * cs.width + w];
            }
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            switch (job.total_field[q]) {
            case 0: ctl->n_shade = total; break;
            case 1: ctl->n_cont = total; break;
            case 2: ctl->n_gather = total; break;
            case 3: ctl->n_free = base + total; break;
            default: ctl->n_free_trace = total; break;
            }
        }
        stream0 += job.n_streams[q];
    }
}

// ================================================================================================= photon gather
#include "gi_gather.inc"   // gather_wave, k_st_gather, k_st_gather_wave, finish_gathers, k_gather and the debug kernels (the selection itself: gi_gather.h)

// the last stragglers of a chunk (paths bouncing between specular surfaces up to MAX_DEPTH), finished without one nearly
// empty pass per remaining depth.  A wave's bounce costs what its most divergent lanes cost (one depth-65 path alone in a
// wave: ~150 us per bounce; 15 unrelated ones sharing a wave: ~730 us), and the tail of a frame is one dependent chain of
// such bounces, so the finisher runs in stages: stage k gives each wave `lanes` paths (lanes 0..lanes-1, the rest idle),
// advances them at most `max_bounces` vertices, and hands the survivors to stage k+1, which spreads them thinner.  The
// survivor count stays on the device (n_in_dev): no host round trip between stages.
#define GI_FINISH_BLOCK 512   // 8 waves: with 64 KB of heaps and 64 KB of octree records one block fills a CU, at the 2 waves per SIMD the registers allow
// Three forms of a stage, one kernel each: MODE 0 a path per lane (heaps of 32 keys per lane: 64 KB, and the 292 records), MODE 1 a path per wave,
// MODE 2 a path per group of 16 lanes -- the latter two keep the records' content boxes in LDS as well (a lone path's bounce is a chain of dependent
// reads, and the boxes were the one left in L2 on every turn) and one heap per GROUP (its lanes carry the same path and would fill 16 or 64 identical
// heaps).  Which form a stage runs depends on how many paths reach it -- a count that stays on the device -- so all three are launched and two return at once.
#define GI_FINISH_COOP_RECORDS GI_LDS_WNODES
#define GI_FINISH_COOP_HEAP_OFF ((GI_LDS_BOXES_BYTES(GI_FINISH_COOP_RECORDS) + 15) & ~15)
#define GI_FINISH_COOP_LDS_BYTES (GI_FINISH_COOP_HEAP_OFF + (GI_FINISH_BLOCK / 16) * GI_GATHER_K * 4)
__device__ __forceinline__ int finish_mode(int wide, int lanes, uint32_t n_in, uint32_t n_waves, uint32_t coop_factor)
{
    // coop_factor: low half = paths per group-of-16 slot up to which a stage runs one path per group, high half = paths per resident wave up to which it
    // runs one path per WAVE (the wave's lanes walk the nodes together, test a leaf's entities side by side and take a gather candidate each)
    if (!wide || lanes > 0) return 0;
    if (n_in <= (coop_factor >> 16) * n_waves) return 1;
    if (n_in <= (coop_factor & 0xffffu) * 4u * n_waves) return 2;
    return 0;
}
template <int FEAT, int WIDE, int MODE>
__global__ __launch_bounds__(GI_FINISH_BLOCK) void k_st_finish(Scene S, uint64_t seed, PathPool pool, const unsigned long long* slot_sample, unsigned long long sample0,
                                                        const uint32_t* q_in, const unsigned int* n_in_dev, uint32_t n_in_host, int lanes, int max_bounces,
                                                        uint32_t* q_out, unsigned int* n_out, double* lbuf, uint32_t coop_factor)
{
    const uint32_t n_in = n_in_dev ? *n_in_dev : n_in_host;
    const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;
    if (finish_mode(WIDE, lanes, n_in, n_waves, coop_factor) != MODE) return;   // uniform over the grid
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if constexpr (WIDE != 0 && MODE != 0) {
        constexpr uint32_t G = MODE == 1 ? 64u : 16u, per_wave = 64u / G;
        const LdsWide N = stage_wide_in_lds(S, true, GI_FINISH_COOP_RECORDS);   // ends with a barrier
        LdsWideCoop<(int)G> NC;
        NC.g = N.g; NC.n_l = N.n_l; NC.cboxes = N.cboxes; NC.cuse = N.cuse; NC.n_lc = N.n_lc; NC.box_off = N.box_off; NC.use_off = N.use_off;
        float* const heap = reinterpret_cast<float*>(gi_dyn_lds + GI_FINISH_COOP_HEAP_OFF) + threadIdx.x / G;   // one heap per group, element i at heap[i * groups]
        const int heap_stride = (int)(GI_FINISH_BLOCK / G);
        const uint32_t grp = lane / G;
        // every lane of the wave stays in the loops (a group without a path idles): a pending photon gather is served by the WHOLE wave, one query at a
        // time -- its lanes take a candidate each (gather_wave: gather_in_leaf's sums to the last bit).  A group's or lane's own walk through its leaf's
        // candidates is a chain of dependent reads that the stage's other paths all wait for (0.5 - 1 ms per vertex of a stage, whatever its size).
        for (uint32_t i0 = wave * per_wave; i0 < n_in; i0 += n_waves * per_wave) {
            const uint32_t i = i0 + grp;
            const bool have = i < n_in;
            const uint32_t slot = have ? q_in[i] : 0u;
            PathRec p;
            double* const Lb = lbuf + (have ? (sample_of(slot_sample, sample0, slot) - sample0) * 3 : 0ull);   // the path's radiance so far; kept in registers while this stage works on it
            if (have) { p = pool.load(slot); p.L[0] = Lb[0]; p.L[1] = Lb[1]; p.L[2] = Lb[2]; }
            bool alive = have, running = have;
            for (int b = 0;;) {
                int fl = 0;
                if (running) {
                    if (!stage_trace_nodes<FEAT>(S, NC, p, seed, nullptr)) { alive = false; running = false; }
                    if (running) fl = stage_shade_nodes<FEAT>(S, NC, p, seed, nullptr);
                }
                finish_gathers(S, p, running && (fl & ST_GATHER) != 0, G, heap, heap_stride, lane);
                if (running && !(fl & ST_CONTINUE)) { alive = false; running = false; }
                if (++b >= max_bounces) running = false;
                if (__ballot(running) == 0ull) break;
            }
            if (have && (lane & (G - 1u)) == 0u) {
                Lb[0] = p.L[0]; Lb[1] = p.L[1]; Lb[2] = p.L[2];
                if (alive) {
                    pool.store(slot, p);
                    q_out[atomicAdd(n_out, 1u)] = slot;
                }
            }
        }
    } else {
        __shared__ float heap[GI_GATHER_K * GI_FINISH_BLOCK];
        const typename LdsSrc<WIDE>::type N = LdsSrc<WIDE>::stage(S);   // a lone path's bounce is a chain of dependent node reads: LDS, not L2
        if (lanes <= 0) lanes = (int)min(64u, max(1u, (n_in + n_waves - 1) / n_waves));   // spread the paths evenly over the resident waves
        for (uint32_t i0 = wave * lanes; i0 < n_in; i0 += n_waves * lanes) {
            const uint32_t i = i0 + lane;
            const bool have = lane < (uint32_t)lanes && i < n_in;
            const uint32_t slot = have ? q_in[i] : 0u;
            PathRec p;
            double* const Lb = lbuf + (have ? (sample_of(slot_sample, sample0, slot) - sample0) * 3 : 0ull);
            if (have) { p = pool.load(slot); p.L[0] = Lb[0]; p.L[1] = Lb[1]; p.L[2] = Lb[2]; }
            bool alive = have, running = have;
            for (int b = 0;;) {
                int fl = 0;
                if (running) {
                    if (!stage_trace_nodes<FEAT>(S, N, p, seed, nullptr)) { alive = false; running = false; }
                    else fl = stage_shade_nodes<FEAT>(S, N, p, seed, nullptr);
                }
                finish_gathers(S, p, running && (fl & ST_GATHER) != 0, 1u, heap + threadIdx.x, GI_FINISH_BLOCK, lane);
                if (running && !(fl & ST_CONTINUE)) { alive = false; running = false; }
                if (++b >= max_bounces) running = false;
                if (__ballot(running) == 0ull) break;
            }
            if (have) {
                Lb[0] = p.L[0]; Lb[1] = p.L[1]; Lb[2] = p.L[2];
                if (alive) {
                    pool.store(slot, p);
                    q_out[atomicAdd(n_out, 1u)] = slot;
                }
            }
        }
    }
}

// fold samples [s0, s0 + ns) of every pixel into its running mean, in sample order (include/raytracer.h:131-147)
__global__ __launch_bounds__(GI_BLOCK) void k_st_accum(Frame F, PixRec* pix, const double* lbuf, uint32_t n_pix, int ns, void* out, int out_f64, int32_t* out_spp)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_pix; i += gridDim.x * blockDim.x) {
        int x, ly;
        st_pixel_xy(F, i, x, ly);
        PixRec r = pix[i];
        PixelState ps = pixrec_to_state(r);
        for (int k = 0; k < ns; k++) {
            const double* l = lbuf + ((size_t)k * n_pix + i) * 3;
            pixel_add_sample(ps, F, v3(l[0], l[1], l[2]));
        }
        state_to_pixrec(ps, r);
        pix[i] = r;
        pixel_write(F, x, ly, ps, out, out_f64, out_spp);
    }
}

// Progressive sessions (gi_progressive_*): the frame as the pixel records hold it, nothing folded.  One lane per record, consecutive lanes read
// consecutive 72-byte records; tiled = 0: the records are in st_pixel_xy order (fixed schedule), 1: in padded 8x8 tiles (rounds, tile_pixel_xy),
// whose padding records have no pixel.
__global__ __launch_bounds__(GI_BLOCK) void k_pix_resolve(Frame F, const PixRec* pix, uint32_t n_rec, int tiled, void* out, int out_f64, int32_t* out_spp)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_rec; i += gridDim.x * blockDim.x) {
        int x, ly;
        if (tiled) { if (!tile_pixel_xy(F, i, x, ly)) continue; }
        else st_pixel_xy(F, i, x, ly);
        const PixRec r = pix[i];
        pixel_write(F, x, ly, pixrec_to_state(r), out, out_f64, out_spp);
    }
}
// gi_progressive_status: how many pixels pixel_wants_sample holds for under F (the session's own max_samples); one count per wave, as k_ad_accum
__global__ __launch_bounds__(GI_BLOCK) void k_pix_wanting(Frame F, const PixRec* pix, uint32_t n_rec, int tiled, unsigned int* n_wanting)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_round = (n_rec + 63u) & ~63u;
    for (uint32_t i0 = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < n_round; i0 += gridDim.x * blockDim.x) {
        const uint32_t i = i0 + lane;
        int x, ly;
        bool wants = false;
        if (i < n_rec && (!tiled || tile_pixel_xy(F, i, x, ly))) {
            const int2 ss = *reinterpret_cast<const int2*>(&pix[i].samps);   // samps and s, adjacent and 8-byte aligned in the 72-byte record
            PixelState ps;
            ps.samps = ss.x; ps.s = ss.y;                                      // the two fields the rule reads
            wants = pixel_wants_sample(ps, F);
        }
        (void)wave_append(n_wanting, wants);
    }
}

__global__ __launch_bounds__(GI_BLOCK) void k_trace(Scene S, int n, const double* rays, int32_t* hit, int32_t* ent, double* res)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* r = rays + (size_t)i * 6;
    Ray ray = make_ray_exact(v3(r[0], r[1], r[2]), v3(r[3], r[4], r[5]));
    Rng rng = rng_make(0, (uint32_t)i);
    HitRec h;
    bool ok = trace(S, ray, rng, P_TRACE_ALPHA, h, nullptr);
    hit[i] = ok ? 1 : 0;
    ent[i] = ok ? h.tri : -1;
    double* o = res + (size_t)i * 8;
    if (ok) {
        V3 nn = shading_normal(S, h);
        o[0] = h.pos.x; o[1] = h.pos.y; o[2] = h.pos.z; o[3] = nn.x; o[4] = nn.y; o[5] = nn.z; o[6] = h.u; o[7] = h.v;
    } else
        for (int k = 0; k < 8; k++) o[k] = 0;
}

__global__ __launch_bounds__(GI_BLOCK) void k_visible(Scene S, int n, const double* q, int32_t* vis)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* p = q + (size_t)i * 6;
    V3 o = v3(p[0], p[1], p[2]), t = v3(p[3], p[4], p[5]);
    V3 ld = t - o;
    double maxt = len2(ld);
    Ray sr = make_ray(o, ld);
    Rng rng = rng_make(0, (uint32_t)i);
    vis[i] = visible(S, sr, maxt, rng, 0, nullptr) ? 1 : 0;
}

__global__ __launch_bounds__(GI_BLOCK) void k_visible_rays(Scene S, int n, const double* rays, const double* mt, int32_t* vis)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* r = rays + (size_t)i * 6;
    Ray sr = make_ray_exact(v3(r[0], r[1], r[2]), v3(r[3], r[4], r[5]));
    Rng rng = rng_make(0, (uint32_t)i);
    vis[i] = visible(S, sr, mt[i], rng, 0, nullptr) ? 1 : 0;
}

// gi_debug_walk: caller rays through the walk forms the passes run, with k_trace's / k_visible_rays' keys (rng_make(0, i), P_TRACE_ALPHA, light 0) and
// k_trace's output.  FORM 0: a ray per lane over the records and content boxes k_st_trace (closest hit) / a shadow kernel without lights to end at
// (any hit) stages; FORM 1, 2: a ray per wave / per group of 16 lanes over what k_st_finish stages (ray i = group i, every lane of the group holds
// it, the first writes).  lds = 0: the same source with nothing staged (n_l = n_lc = 0), every record and box from global memory.
#define GI_DEBUG_WALK_BLOCK 256
template <int FEAT, int FORM, bool ANY>
__global__ __launch_bounds__(GI_DEBUG_WALK_BLOCK) void k_debug_walk(Scene S, int n, const double* rays, const double* mt, int lds, int32_t* hit, int32_t* ent, double* res)
{
    constexpr uint32_t G = FORM == 1 ? 64u : (FORM == 2 ? 16u : 1u);
    typedef typename std::conditional<FORM == 0, LdsWide, LdsWideCoop<FORM == 2 ? 16 : 64>>::type Src;
    const LdsWide L = FORM == 0 ? stage_wide_in_lds(S, true, GI_LDS_WNODES_BIG, ANY ? 0 : 1) : stage_wide_in_lds(S, true, GI_FINISH_COOP_RECORDS);   // ends with a barrier
    Src N;
    N.g = L.g; N.cboxes = L.cboxes; N.cuse = L.cuse; N.box_off = L.box_off; N.use_off = L.use_off;
    N.n_l = lds ? L.n_l : 0; N.n_lc = lds ? L.n_lc : 0;
    const uint32_t n_groups = gridDim.x * blockDim.x / G;
    for (uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) / G; i < (uint32_t)n; i += n_groups) {   // uniform over a group: its lanes stay together
        const double* r = rays + (size_t)i * 6;
        const Ray ray = make_ray_exact(v3(r[0], r[1], r[2]), v3(r[3], r[4], r[5]));
        const Rng rng = rng_make(0, i);
        const bool writes = (threadIdx.x & (G - 1u)) == 0u;
        if constexpr (ANY) {
            const bool vis = visible_nodes<FEAT>(S, N, ray, mt[i], rng, 0, nullptr);
            if (writes) hit[i] = vis ? 1 : 0;
        } else {
            HitRec h;
            h.tu = 0; h.tv = 0;
            const bool ok = trace_nodes<FEAT>(S, N, ray, rng, P_TRACE_ALPHA, h, nullptr);
            if (!writes) continue;
            hit[i] = ok ? 1 : 0;
            ent[i] = ok ? h.tri : -1;
            double* o = res + (size_t)i * 8;
            if (ok) {
                const V3 nn = shading_normal(S, h);
                o[0] = h.pos.x; o[1] = h.pos.y; o[2] = h.pos.z; o[3] = nn.x; o[4] = nn.y; o[5] = nn.z; o[6] = h.u; o[7] = h.v;
            } else
                for (int k = 0; k < 8; k++) o[k] = 0;
        }
    }
}

__global__ __launch_bounds__(GI_BLOCK) void k_radiance(Scene S, int n, const double* rays, const uint32_t* stream, uint64_t seed, double* out3)
{
    __shared__ float heap[GI_GATHER_K * GI_BLOCK];
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* r = rays + (size_t)i * 6;
    Ray ray = make_ray_exact(v3(r[0], r[1], r[2]), v3(r[3], r[4], r[5]));
    V3 L = radiance_path(S, ray, stream[i], seed, heap + threadIdx.x, GI_BLOCK, nullptr);
    out3[(size_t)i * 3] = L.x; out3[(size_t)i * 3 + 1] = L.y; out3[(size_t)i * 3 + 2] = L.z;
}

__global__ __launch_bounds__(GI_BLOCK) void k_emit(Scene S, int count, int max_depth, uint64_t seed, PhotonOut* out, int32_t* stored, int32_t* tries)
{
    int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count * S.n_light) return;
    int i = j / S.n_light, li = j % S.n_light;
    PhotonOut po;
    int32_t t = 0;
    bool ok = emit_photon(S, i, li, count, max_depth, seed, po, t);
    stored[j] = ok ? 1 : 0;
    tries[j] = t;
    if (ok) out[j] = po;
}

__global__ __launch_bounds__(GI_BLOCK) void k_leaf_order(Scene S, int n, const double* rays, int cap, int32_t* leaf_out, int32_t* n_out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* r = rays + (size_t)i * 6;
    n_out[i] = leaf_order(S, make_ray_exact(v3(r[0], r[1], r[2]), v3(r[3], r[4], r[5])), cap, leaf_out + (size_t)i * cap);
}
__global__ __launch_bounds__(GI_BLOCK) void k_kat(int what, int n, const double* in, int in_stride, double* out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double a[9], o[3];
    for (int k = 0; k < 9; k++) a[k] = k < in_stride ? in[(size_t)i * in_stride + k] : 0.0;
    kat_eval(what, a, o);
    for (int k = 0; k < 3; k++) out[(size_t)i * 3 + k] = o[k];
}

__global__ void k_halton(Scene S, int n, const uint32_t* dim, const uint32_t* index, float* out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = halton_sample(S, dim[i], index[i]);
}
__global__ void k_halton_index(HaltonEnumD he, int n, const uint32_t* sxy, uint32_t* out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = halton_index(he, sxy[i * 3], sxy[i * 3 + 1], sxy[i * 3 + 2]);
}

// ================================================================================================= host side, and the kernels that stand with it
#include "gi_context.inc"        // gi_ctx and its parts: scene, photon map, tuning, stage clock, stream workspaces, auxiliary passes
#include "gi_instances.inc"      // the kernel instances with dynamic LDS, their tables and selectors
#include "gi_sort.inc"           // the radix sort of the queues: kernels and rs_sort_pairs
#include "gi_photon_build.inc"   // the photon map built on the device: kernels and build_photon_map_on_device
#include "gi_stream.inc"         // the scheduler: stream_samples, run_rounds, stream_passes
#include "gi_api.inc"            // create / destroy, uploads, setters, the frame, its timers and counters
#include "gi_progressive.inc"    // progressive sessions (gi_progressive_*)
#include "gi_denoise.inc"        // the a-trous denoiser: kernels and gi_denoise_*
#include "gi_upsample.inc"       // the guided upsampler: kernel and gi_upsample_*
#include "gi_features.inc"       // first-hit feature buffers: k_aov and gi_render_features_*; the host frame of the per-pixel passes
#include "gi_occlusion.inc"      // ambient occlusion: k_ao and gi_render_occlusion_*
#include "gi_entries.inc"        // function-level entries (parity tests, public C++ methods) and the debug entries
#include "gi_lens.inc"           // the thin lens: gi_set_lens, its vertex table, gi_debug_primary_rays, gi_focus_distance
#include "gi_bake.inc"           // light baking: k_bake_gen, k_bake_fold and gi_bake_*
#include "gi_lightmap.inc"       // lightmap atlases: k_lm_raster, k_lm_point, the rank, k_lm_scatter, k_lm_dilate and gi_lightmap_*
#include "gi_group.inc"          // one frame over several devices (gi_group_*)
