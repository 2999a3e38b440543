// gi_kernels.hip -- gfx950 kernels + the C ABI of include/gi_hip.h.
//
// Kernels (all one ray / one pixel per lane, 64-wide waves, scene tables read through L1/L2):
//   k_render     the pixel loop of RayTracer::run with the whole path inside (include/raytracer.h:93-160,167-579)
//   k_trace / k_visible / k_gather / k_radiance   function-level entry points (parity tests, public C++ methods)
//   k_emit       RayTracer::tracePhotons (include/raytracer.h:582-715), one (photon index, light) per lane
// Host side of this file: device layouts (8 direction-ordered copies of the octree, leaf-ordered photons, Halton tables)
// and the gi_* entry points.  No CPU fallback exists: every entry needs a HIP device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
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
#ifndef GI_EXP_SHADE
#define GI_EXP_SHADE 0
#endif

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

// the same for the wide records (gi_device.h: WNode): 292 of them = every inner node of the BASELINE scenes
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
    const float* cboxes;      // content boxes of the children (gi_device.h: content_cull), read through L1 / L2; null = no culling
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
    // the tables cull() reads, for callers that test a record's children side by side (gi_device.h: walk_hits of the one-ray-per-group walks)
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
template <int G> struct LdsWideCoop : LdsWide { static constexpr bool kCoop = true; static constexpr int kGroup = G; };   // the same records, one ray per group of G lanes (gi_device.h: trace_wide_coop)
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
static PathPool make_path_pool(void* base, size_t n)
{
    PathPool P;
    char* b = static_cast<char*>(base);
    P.ray = reinterpret_cast<PoolRay*>(b); b += n * sizeof(PoolRay);
    P.hit = reinterpret_cast<PoolHit*>(b); b += n * sizeof(PoolHit);
    P.thru = reinterpret_cast<PoolThru*>(b); b += n * sizeof(PoolThru);
    P.gath = reinterpret_cast<PoolGath*>(b); b += n * sizeof(PoolGath);
    P.L = reinterpret_cast<double*>(b);
    return P;
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

// pixel index -> (x, local row): 8x8 tiles so that the 64 lanes of a wave start neighbouring pixels
__device__ __forceinline__ bool wf_pixel_xy(const Frame& F, uint32_t i, int& x, int& ly)
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
        const bool inside = i < n_pix && wf_pixel_xy(F, i, x, ly);
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
        if (i < n_pix && wf_pixel_xy(F, i, x, ly)) {
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
template <int FEAT, int WIDE, bool COUNT = false>
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
            ray = primary_ray_at(S, g.F, stream);
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
                    const unsigned long long want = ~busy;
                    const uint32_t nw = (uint32_t)__popcll(want);
                    unsigned int base = 0;
                    if (lane == (uint32_t)(__ffsll((long long)want) - 1)) base = atomicAdd(s_next, nw);
                    base = (unsigned int)__shfl((int)base, __ffsll((long long)want) - 1);
                    more = base + nw < total;
                    // first item this fetch hands out: new paths run in lockstep, continuing ones refill
                    const uint32_t i_first = ((base / bs) * gridDim.x + blockIdx.x) * bs + base % bs;
                    thr = i_first < g.n_gen ? 64u : refill_min;
                    if (!walking) {
                        const uint32_t u = base + (uint32_t)__popcll(want & ((1ull << lane) - 1ull));
                        const uint32_t i = ((u / bs) * gridDim.x + blockIdx.x) * bs + u % bs;
                        if (u < total && i < n_in) {
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
    // early_turns != 0 (stream_passes): the next ray of a vertex is walked for up to that many turns (ray_leaves_scene, gi_device.h); one that leaves
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
        const uint32_t i = ((u / cs) * gridDim.x + blockIdx.x) * cs + u % cs + lane;
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
                const unsigned long long want = ~busy;
                const uint32_t nw = (uint32_t)__popcll(want);
                const int leader = __ffsll((long long)want) - 1;
                unsigned int base = 0;
                if ((int)lane == leader) base = atomicAdd(s_next, nw);
                base = (unsigned int)__shfl((int)base, leader);
                more = base + nw < total;
                if (!walking) {
                    const uint32_t u = base + (uint32_t)__popcll(want & ((1ull << lane) - 1ull));
                    const uint32_t i = ((u / bs) * gridDim.x + blockIdx.x) * bs + u % bs;
                    if (u < total && i < n_in && shq[(size_t)i * nl].live) {
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
__global__ void k_find_leaves(Scene S, int32_t n, const double* pos, int32_t* fast, int32_t* full)   // gi_debug_find_leaves
{
    for (int32_t i = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x); i < n; i += (int32_t)(gridDim.x * blockDim.x)) {
        const V3 p = v3(pos[(size_t)i * 3], pos[(size_t)i * 3 + 1], pos[(size_t)i * 3 + 2]);
        fast[i] = S.pdescent ? gather_find_leaf_fast(S, p) : -2;
        full[i] = gather_find_leaf(S, p);
    }
}
// The sort key of a gather query (k_st_compact's gather queue, gi_debug_gather_pass): the rank of the photon-map leaf around the position among the
// leaves with candidates; n_pleaf, the key past the last leaf, when there is nothing to gather (outside the map, a leaf without candidates)
__device__ __forceinline__ uint32_t gather_key(const Scene& S, V3 pos)
{
    int32_t leaf = S.pdescent ? gather_find_leaf_fast(S, pos) : -2;
    if (leaf == -2) leaf = gather_find_leaf(S, pos);
    const int32_t rank = leaf < 0 ? -1 : S.pleaf_rank[leaf];
    return rank < 0 ? (uint32_t)S.n_pleaf : (uint32_t)rank;
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

// Gather queries are sorted by the photon-map leaf that contains them (keys from k_st_compact): queries of one leaf share their candidate
// photons, so the lanes of a wave read the same photons and run loops of equal length.
// Queries arrive sorted by leaf, and a leaf typically serves thousands of queries per pass, so most waves hold 64 queries of ONE
// leaf: such a wave copies the leaf's candidate photons into LDS once (64 at a time, one photon per lane, coalesced) and every lane
// scans them from there -- a broadcast LDS read per candidate instead of an L2 round trip per lane.  Waves that straddle a leaf
// boundary take the per-lane walk.  Both run g_key / g_acc / g_end, i.e. the same arithmetic in the same order.
#define GI_GCHUNK 64
#ifndef GI_GATHER_WAVES
#define GI_GATHER_WAVES 4      // waves per SIMD the gather kernel is compiled for (launch bound)
#endif
// Pass 1 of the cooperative path keeps a lane's 32 smallest keys sorted in registers and folds the candidates in 32 at a time
// (ksel_tau, gi_device.h): 18 branch-free instructions per candidate; the LDS heap costs ~55, because with 64 lanes some lane always has
// to sift, so the wave pays a full sift for nearly every candidate.  The result (tau = 32nd smallest float key) is the same number.
static_assert(GI_GCHUNK == 64, "ksel_tau stages the candidates 64 at a time");
template <bool COUNT>
__global__ __launch_bounds__(GI_BLOCK, GI_GATHER_WAVES) void k_st_gather(Scene S, PathPool pool, const uint32_t* keys, const uint32_t* vals, uint32_t n_in,
                                                                         const unsigned long long* slot_sample, unsigned long long sample0, double* lbuf, StreamCounters* sc)
{
    unsigned long long n_q = 0, n_c = 0;   // COUNT: queries of this lane, candidates they scanned (a leaf's whole candidate list per query, as PhotonMap::getInRange returns it)
    // 8 KB of LDS per wave: the staged candidates of the cooperative path (64 x 9 doubles) or the float heaps of the per-lane walk (32 x 64),
    // never both at once -- a wave is in one of the two, and the tie pass runs after the last candidate was read
    __shared__ __align__(16) float lds[GI_GATHER_K * GI_BLOCK];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    float* const heap = lds + wave * (GI_GATHER_K * 64) + lane;                       // element i of this lane's heap at heap[i * 64]
    double (*const cand)[9] = reinterpret_cast<double (*)[9]>(lds + wave * (GI_GATHER_K * 64));   // cand[k] = staged candidate k of this wave
    // the waves of a workgroup draw its chunks of the grid-stride loop 64 queries at a time (k_st_shade): leaves differ in candidates
    __shared__ unsigned int s_next;
    if (threadIdx.x == 0) s_next = 0u;
    __syncthreads();
    const uint32_t cs = (uint32_t)GI_GATHER_CHUNK;
    const uint32_t total = seg_start(blockIdx.x + 1, n_in, gridDim.x, cs) - seg_start(blockIdx.x, n_in, gridDim.x, cs);
    for (;;) {
        unsigned int u = 0;
        if (lane == 0) u = atomicAdd(&s_next, 64u);
        u = (unsigned int)__shfl((int)u, 0);
        if (u >= total) break;
        const uint32_t i = ((u / cs) * gridDim.x + blockIdx.x) * cs + u % cs + lane;
        const bool valid = i < n_in;
        const uint32_t rank = valid ? keys[i] : 0xffffffffu;                       // rank of the query's leaf among the leaves with candidates
        const bool has_leaf = valid && rank < (uint32_t)S.n_pleaf;
        const uint32_t leaf = has_leaf ? (uint32_t)S.prank_leaf[rank] : 0xffffffffu;
        const uint32_t leaf0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)leaf);
        const bool uniform = __ballot(valid && leaf != leaf0) == 0ull && leaf0 < (uint32_t)S.n_pnode;
        if constexpr (COUNT) { if (valid) n_q++; }
        if (!uniform) {
            if (has_leaf) {
                if constexpr (COUNT) n_c += (unsigned long long)S.pnodes[leaf].u.lf.nb_photons;
                PathRef pr = pool[vals[i]];
                stage_gather_in_leaf(S, pr, (int32_t)leaf, heap, 64, lbuf + (sample_of(slot_sample, sample0, vals[i]) - sample0) * 3);
            }
            continue;
        }
        const uint32_t rank0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)rank);
        const PNode& lf = S.pnodes[leaf0];
        const int ncand = lf.u.lf.nb_photons;
        if constexpr (COUNT) { if (valid) n_c += (unsigned long long)ncand; }
        if (ncand == 0) continue;
        const PRange* ranges = S.pranges + lf.nb_off;
        GatherAcc a;
        const uint32_t gslot = valid ? vals[i] : 0u;
        g_begin(a, valid ? ld3(pool.hit[gslot].hpos) : v3(0, 0, 0), valid ? ld3(pool.gath[gslot].gdir) : v3(0, 0, 0), heap, 64, ncand);
        // the leaf's candidates as one sequence (its ranges back to back, the order gather_in_leaf visits them), 64 per step: candidates
        // [c0, c0 + m) into cand[0, m), positions only or (all9) positions, directions and colours
        auto stage = [&](int32_t c0, int32_t m, bool all9) {
            __builtin_amdgcn_wave_barrier();
            if ((int32_t)lane < m) {
                const double* pp;
                const double* dc;
                if (S.pcand) {
                    const size_t at = (size_t)S.pcand_off[rank0] + (size_t)(c0 + (int32_t)lane);
                    pp = S.pcand + at * 3; dc = S.pcand_dc + at * 6;
                } else {
                    int32_t off = c0 + (int32_t)lane, r = 0;
                    while (off >= ranges[r].count) { off -= ranges[r].count; r++; }   // r < n_ranges: off < ncand = sum of the counts
                    const size_t ph = (size_t)(ranges[r].first + off);
                    pp = S.ph_pos + ph * 3; dc = S.ph_dircol + ph * 6;
                }
                cand[lane][0] = pp[0]; cand[lane][1] = pp[1]; cand[lane][2] = pp[2];
                if (all9)
                    for (int k = 0; k < 6; k++) cand[lane][3 + k] = dc[k];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        };
        // pass 1 runs the chunks from the last to the first and stages chunk 0 whole, so pass 2 (chunks in candidate order) finds it in LDS
        a.tau = ksel_tau(ncand, [&](int32_t c0, int32_t m) { stage(c0, m, c0 == 0); }, [&](int32_t k) {
            const double* q = cand[k];
            return (float)len2(v3(q[0], q[1], q[2]) - a.pos);   // same expression as g_key
        });
        for (int32_t c0 = 0; c0 < ncand; c0 += GI_GCHUNK) {
            const int32_t m = min((int32_t)GI_GCHUNK, ncand - c0);
            if (c0 != 0) stage(c0, m, true);
            if (valid) {
                // g_acc per candidate, with the rare case set aside: a candidate whose key EQUALS tau (the 32nd smallest itself; one per
                // query, more only when float keys tie) is some lane's business for nearly every candidate of the wave, so its branch --
                // a sum of its own, a count, a running maximum -- would run for nearly every candidate.  The loop only notes where such
                // candidates are; they are added afterwards, in candidate order, by the same g_acc.
                int n_eq = 0;
                int32_t k_eq = 0;
                for (int32_t k = 0; k < m; k++) {
                    const double* q = cand[k];
                    const double d2 = len2(v3(q[0], q[1], q[2]) - a.pos);
                    const float key = (float)d2;
                    if (key < a.tau) {
                        const V3 contrib = v3(q[6], q[7], q[8]) * dot(v3(q[3], q[4], q[5]), a.dir);
                        a.s_lt = a.s_lt + contrib; a.c_lt++;
                    } else if (key == a.tau) {
                        if (n_eq == 0) k_eq = k;
                        n_eq++;
                    }
                }
                if (n_eq == 1) {
                    const double* q = cand[k_eq];
                    g_acc(a, v3(q[0], q[1], q[2]), q + 3);
                } else if (n_eq > 1) {     // float keys tie at tau: walk on from the first of them
                    for (int32_t k = k_eq; n_eq > 0 && k < m; k++) {
                        const double* q = cand[k];
                        if ((float)len2(v3(q[0], q[1], q[2]) - a.pos) == a.tau) { g_acc(a, v3(q[0], q[1], q[2]), q + 3); n_eq--; }
                    }
                }
            }
        }
        if (valid) {
            V3 caustic;
            if (!g_end(a, caustic)) caustic = gather_in_leaf(S, (int32_t)leaf0, a.pos, a.dir, heap, 64, nullptr, nullptr);   // float-key tie: exact pass
            double* Lp = lbuf + (sample_of(slot_sample, sample0, vals[i]) - sample0) * 3;   // the path's radiance lives in the per-sample buffer
            V3 L = ld3(Lp) + ld3(pool.gath[gslot].gcoef) * caustic;
            Lp[0] = L.x; Lp[1] = L.y; Lp[2] = L.z;
        }
    }
    if constexpr (COUNT) { flush_u64(&sc->gather_queries, n_q); flush_u64(&sc->gather_cand, n_c); }
}

// A query per WAVE, for the passes with few queries.  Late passes hold a handful of queries per photon-map leaf: a wave of k_st_gather then either serves
// sixty leaves one after the other with one or two lanes at work, or lets every lane walk its own leaf -- either way the pass lasts as long as some
// five thousand candidate steps of one wave (1.2 - 1.6 ms on the benchmark frame, whatever the number of queries).  Here the lanes take a CANDIDATE
// each: 64 keys per step, the 32 smallest kept across the lanes (a bitonic sort of the 64 new keys through lane exchanges, the smaller half against
// the best so far, a bitonic merge: ~110 instructions per 64 candidates instead of 18 per candidate and query), tau read off lane K - 1; the second
// pass computes every lane's contribution and adds those below tau in CANDIDATE ORDER (a lane at a time, read off by v_readlane), so the sums are the
// sums of g_acc to the last bit; the tie group (keys equal to tau) likewise; float-key ties across rank 32 go to lane 0's gather_in_leaf, as everywhere.
__device__ __forceinline__ double wave_read(double v, int src_lane)      // src_lane is wave-uniform
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src_lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), src_lane);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ V3 gather_wave(const Scene& S, int32_t leaf, uint32_t rank, V3 pos, V3 dir, float* heap32, uint32_t lane, int* n_cand_out)
{
    const PNode& lf = S.pnodes[leaf];
    const int ncand = lf.u.lf.nb_photons;
    if (n_cand_out) *n_cand_out = ncand;
    V3 res = v3(0, 0, 0);
    if (ncand == 0) return res;
    const size_t cbase = (size_t)S.pcand_off[rank];
    const int K = ncand < GI_GATHER_K ? ncand : GI_GATHER_K;
    // pass 1: the K-th smallest float key.  lane j < 32 holds the j-th smallest so far
    float best = INFINITY;
    for (int32_t c0 = 0; c0 < ncand; c0 += 64) {
        const int32_t c = c0 + (int32_t)lane;
        float key = INFINITY;
        if (c < ncand) {
            const double* pp = S.pcand + (cbase + (size_t)c) * 3;
            key = (float)len2(v3(pp[0], pp[1], pp[2]) - pos);            // the expression of g_key
        }
#pragma unroll
        for (int k = 2; k <= 64; k <<= 1)
#pragma unroll
            for (int j = k >> 1; j > 0; j >>= 1) {
                const float o = __shfl_xor(key, j);
                const bool keep_min = ((lane & (uint32_t)j) == 0u) == ((lane & (uint32_t)k) == 0u);   // ascending blocks where bit k is clear (k = 64: everywhere)
                key = keep_min ? fminf(key, o) : fmaxf(key, o);
            }
        const float r = __shfl(key, (int)((31u - lane) & 63u));         // the 32 smallest new keys, descending over lanes 0 .. 31
        float m = lane < 32u ? fminf(best, r) : INFINITY;               // the 32 smallest of both, a bitonic sequence
#pragma unroll
        for (int j = 16; j > 0; j >>= 1) {
            const float o = __shfl_xor(m, j);
            m = (lane & (uint32_t)j) == 0u ? fminf(m, o) : fmaxf(m, o);
        }
        best = lane < 32u ? m : INFINITY;
    }
    const float tau = __shfl(best, K - 1);
    // pass 2: g_acc over the candidates, in their order
    V3 s_lt = v3(0, 0, 0), s_eq = v3(0, 0, 0);
    int c_lt = 0, c_eq = 0;
    double r_eq = 0;
    for (int32_t c0 = 0; c0 < ncand; c0 += 64) {
        const int32_t c = c0 + (int32_t)lane;
        bool lt = false, eq = false;
        double d2 = 0;
        V3 contrib = v3(0, 0, 0);
        if (c < ncand) {
            const double* pp = S.pcand + (cbase + (size_t)c) * 3;
            d2 = len2(v3(pp[0], pp[1], pp[2]) - pos);
            const float key = (float)d2;
            lt = key < tau; eq = key == tau;
            if (lt || eq) {
                const double* dc = S.pcand_dc + (cbase + (size_t)c) * 6;
                contrib = v3(dc[3], dc[4], dc[5]) * dot(v3(dc[0], dc[1], dc[2]), dir);
            }
        }
        unsigned long long mlt = __ballot(lt), meq = __ballot(eq);
        c_lt += (int)__popcll(mlt); c_eq += (int)__popcll(meq);
        while (mlt != 0ull) {
            const int b = __ffsll((long long)mlt) - 1;
            mlt &= mlt - 1ull;
            s_lt = s_lt + v3(wave_read(contrib.x, b), wave_read(contrib.y, b), wave_read(contrib.z, b));
        }
        while (meq != 0ull) {
            const int b = __ffsll((long long)meq) - 1;
            meq &= meq - 1ull;
            s_eq = s_eq + v3(wave_read(contrib.x, b), wave_read(contrib.y, b), wave_read(contrib.z, b));
            const double de = wave_read(d2, b);
            r_eq = de > r_eq ? de : r_eq;
        }
    }
    const int need = K - c_lt;       // g_end
    if (c_eq > need) {               // float keys tie across rank 32: the exact pass, by one lane
        if (lane == 0u) res = gather_in_leaf(S, leaf, pos, dir, heap32, 1, nullptr, nullptr);
        res = v3(wave_read(res.x, 0), wave_read(res.y, 0), wave_read(res.z, 0));
        return res;
    }
    return (s_lt + s_eq) / (GI_PI * r_eq);
}
#define GI_GW_BLOCK 256      // four waves: a wave per SIMD and workgroup, five workgroups per CU at 87 registers
template <bool COUNT>
__global__ __launch_bounds__(GI_GW_BLOCK) void k_st_gather_wave(Scene S, PathPool pool, const uint32_t* keys, const uint32_t* vals, uint32_t n_in,
                                                            const unsigned long long* slot_sample, unsigned long long sample0, double* lbuf, StreamCounters* sc)
{
    __shared__ float heaps[(GI_GW_BLOCK / 64) * GI_GATHER_K];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;
    unsigned long long n_q = 0, n_c = 0;
    for (uint32_t q = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; q < n_in; q += n_waves) {
        const uint32_t rank = (uint32_t)__builtin_amdgcn_readfirstlane((int)keys[q]);
        if constexpr (COUNT) n_q++;
        if (rank >= (uint32_t)S.n_pleaf) continue;
        const int32_t leaf = __builtin_amdgcn_readfirstlane(S.prank_leaf[rank]);
        const uint32_t slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)vals[q]);
        int nc = 0;
        const V3 caustic = gather_wave(S, leaf, rank, ld3(pool.hit[slot].hpos), ld3(pool.gath[slot].gdir), heaps + wave * GI_GATHER_K, lane, &nc);
        if constexpr (COUNT) n_c += (unsigned long long)nc;
        if (lane == 0u && nc > 0) {
            double* Lp = lbuf + (sample_of(slot_sample, sample0, slot) - sample0) * 3;   // the path's radiance lives in the per-sample buffer
            const V3 L = ld3(Lp) + ld3(pool.gath[slot].gcoef) * caustic;
            Lp[0] = L.x; Lp[1] = L.y; Lp[2] = L.z;
        }
    }
    if constexpr (COUNT) { if (lane != 0u) { n_q = 0; n_c = 0; } flush_u64(&sc->gather_queries, n_q); flush_u64(&sc->gather_cand, n_c); }
}
// gi_debug_gather_pass: query i in slot i of a pool of n (position, direction, factor 1, sample i) and its key as k_st_compact computes it
__global__ __launch_bounds__(256) void k_gather_pass_prep(Scene S, PathPool pool, int32_t n, const double* q6, unsigned long long* slot_sample, uint32_t* keys, uint32_t* vals)
{
    const int32_t i = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const double* q = q6 + (size_t)i * 6;
    for (int k = 0; k < 3; k++) { pool.hit[i].hpos[k] = q[k]; pool.gath[i].gdir[k] = q[3 + k]; pool.gath[i].gcoef[k] = 1.0; }
    slot_sample[i] = (unsigned long long)i;
    keys[i] = gather_key(S, v3(q[0], q[1], q[2]));
    vals[i] = (uint32_t)i;
}

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
// The photon gathers the paths of a finisher wave have pending after a vertex (`pending`: this lane's -- or, with G lanes per path, this group's --
// path has one).  Up to GI_FIN_WAVE_GATHERS of them are served by the whole wave one after the other (gather_wave); more than that (a stage that still
// holds a path in most lanes), or no written-out candidate lists, and every path walks its own leaf as before (stage_gather).  Called by all 64 lanes.
#ifndef GI_FIN_WAVE_GATHERS
#define GI_FIN_WAVE_GATHERS 24
#endif
__device__ __forceinline__ void finish_gathers(const Scene& S, PathRec& p, bool pending, uint32_t G, float* heap, int heap_stride, float* heap32, uint32_t lane)
{
    unsigned long long pend = __ballot(pending && (lane & (G - 1u)) == 0u);
    if (pend == 0ull) return;
    if (!S.pcand || (uint32_t)__popcll(pend) > (uint32_t)GI_FIN_WAVE_GATHERS) {
        if (pending) stage_gather(S, p, heap, heap_stride, nullptr);
        return;
    }
    while (pend != 0ull) {
        const int src = __ffsll((long long)pend) - 1;
        pend &= pend - 1ull;
        const V3 gp = v3(wave_read(p.hpos[0], src), wave_read(p.hpos[1], src), wave_read(p.hpos[2], src));
        const V3 gd = v3(wave_read(p.gdir[0], src), wave_read(p.gdir[1], src), wave_read(p.gdir[2], src));
        int32_t leaf = S.pdescent ? gather_find_leaf_fast(S, gp) : -2;      // the descent k_st_compact keys the queries of a pass with
        if (leaf == -2) leaf = gather_find_leaf(S, gp);
        V3 caustic = v3(0, 0, 0);
        if (leaf >= 0) {
            const int32_t rank = S.pleaf_rank[leaf];
            if (rank >= 0) caustic = gather_wave(S, leaf, (uint32_t)rank, gp, gd, heap32, lane, nullptr);
        }
        if (lane / G == (uint32_t)src / G) {                                  // stage_gather, on the path's own lanes
            const V3 L = ld3(p.L) + ld3(p.gcoef) * caustic;
            p.L[0] = L.x; p.L[1] = L.y; p.L[2] = L.z;
        }
    }
}
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
        float* const heap32 = reinterpret_cast<float*>(gi_dyn_lds + GI_FINISH_COOP_HEAP_OFF) + (threadIdx.x >> 6) * GI_GATHER_K;
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
                finish_gathers(S, p, running && (fl & ST_GATHER) != 0, G, heap, heap_stride, heap32, lane);
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
                finish_gathers(S, p, running && (fl & ST_GATHER) != 0, 1u, heap + threadIdx.x, GI_FINISH_BLOCK, heap + (threadIdx.x & ~63u), lane);   // (heap32: row 0 of this wave's own lanes 0 .. 31)
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
// consecutive 72-byte records; tiled = 0: the records are in st_pixel_xy order (fixed schedule), 1: in padded 8x8 tiles (rounds, wf_pixel_xy),
// whose padding records have no pixel.
__global__ __launch_bounds__(GI_BLOCK) void k_pix_resolve(Frame F, const PixRec* pix, uint32_t n_rec, int tiled, void* out, int out_f64, int32_t* out_spp)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_rec; i += gridDim.x * blockDim.x) {
        int x, ly;
        if (tiled) { if (!wf_pixel_xy(F, i, x, ly)) continue; }
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
        if (i < n_rec && (!tiled || wf_pixel_xy(F, i, x, ly))) {
            const int2 ss = *reinterpret_cast<const int2*>(&pix[i].samps);   // samps and s, adjacent and 8-byte aligned in the 72-byte record
            PixelState ps;
            ps.samps = ss.x; ps.s = ss.y;                                      // the two fields the rule reads
            wants = pixel_wants_sample(ps, F);
        }
        (void)wave_append(n_wanting, wants);
    }
}

// First-hit feature buffers (gi_render_features_*; gi_device.h: aov_sample): one lane per pixel of this rank's rows in the 8x8-tile order of
// st_pixel_xy, so a wave is a tile and all its lanes are on the same sample index s -- rays as coherent as the new paths of k_st_trace, on the same
// records in LDS and the same wave-uniform leaves.  A lane loops over s (Halton index of sample s = that of sample 0 + s * inc), keeps its eight
// sums in registers and writes once: no queue, no sort, no per-sample buffer, no atomics, and nothing of the path pool.
// out [local_rows][w][8] = albedo rgb, normal xyz, depth, coverage: the f64 sums in ascending s, divided once by n.  ids [local_rows][w][2]
// (optional) = entity and material of sample 0's hit, -1 on a miss.
#ifndef GI_AOV_BLOCK
// One workgroup per CU next to the 160 KB of records and boxes, as k_st_trace -- but of 512 lanes: the lane keeps a pixel's eight sums and the
// frame constants next to the walk, which at the 128 registers of a 1024-lane workgroup spills 408 B per lane (wide triangle instance); at 512
// it fits in 227 without scratch.  Measured on the benchmark frame (caustics 1920x1080, n = 256): 1024 lanes 76.0 ms, 512 lanes 66.5 ms.
#define GI_AOV_BLOCK 512
#endif
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

__global__ __launch_bounds__(GI_BLOCK) void k_gather(Scene S, int n, const double* q, double* res3, int32_t* n_cand)
{
    __shared__ float heap[GI_GATHER_K * GI_BLOCK];
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* p = q + (size_t)i * 6;
    int nc = 0;
    V3 r = gather(S, v3(p[0], p[1], p[2]), v3(p[3], p[4], p[5]), heap + threadIdx.x, GI_BLOCK, &nc, nullptr);
    res3[(size_t)i * 3] = r.x; res3[(size_t)i * 3 + 1] = r.y; res3[(size_t)i * 3 + 2] = r.z;
    if (n_cand) n_cand[i] = nc;
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

// ================================================================================================= host side
#include "gi_scratch.h"   // DevBuf, EventTimer, finish_to_host

#include "gi_stream.inc"   // StreamGrids, StreamWork, STG_*: what the context holds of the scheduler

struct gi_ctx {
    int device = 0;
    StreamGrids grids;                // launch grids of the streaming kernels on this context's device
    hipStream_t stream = nullptr;
    std::string err;
    bool have_scene = false;
    Scene S{};
    DevBuf<TNode> d_tnodes;
    DevBuf<WNode> d_wnodes;
    DevBuf<TexD> d_texs;
    DevBuf<TriUV> d_tri_uv;
    DevBuf<unsigned char> d_tex_pixels;
    DevBuf<double> d_tex_lut;
    DevBuf<int32_t> d_wleaf_id;
    DevBuf<float> d_cboxes;           // content boxes of the wide records' children
    DevBuf<uint32_t> d_cuse;
    SceneSwitches sw;                 // gi_set_wide_nodes, gi_set_content_culling, gi_set_entity_boxes, GI_CLIP_BOXES, GI_WALK_CUT (apply_switches)
    bool flat_candidates = true;      // GI_FLAT_CANDIDATES=0: k_st_gather finds a leaf's k-th candidate through its range list, no k_st_gather_wave
    DevBuf<uint32_t> d_pcand_off;
    DevBuf<double> d_pcand, d_pcand_dc;
    uint32_t gather_wave_below = 200000u;    // GI_GATHER_WAVE_BELOW: gather passes with fewer queries give every query a wave (k_st_gather_wave)
    bool descent_jump = true;         // GI_DESCENT_JUMP=0: the fast descent of the gather keys starts at the root
    DevBuf<int32_t> d_pjump;          // its jump table (gi_device.h: gather_find_leaf_fast)
    DevBuf<double> d_pjump_aux;
    bool sort_cont = true;            // GI_SORT_CONT=0: continuing rays stay in queue order
    bool sort_shade = true;           // GI_SORT_SHADE=0: the shade stage takes a pass of continuing rays in the order the trace stage left them
    int sort_shade_lo = 5;            // GI_SORT_SHADE_LO: lowest slot bit that sort looks at (32 neighbouring records = 7 KB stay in the trace stage's order)
    int sort_lo_bit = 0;              // GI_SORT_LO_BIT: lowest key bit the sort of the continuing rays looks at (27-bit key: octant, 18 Morton bits, 6 direction bits)
    uint32_t refill_min = 32;         // GI_REFILL_MIN: idle lanes of a wave that make k_st_trace hand out new rays (64: lockstep waves)
    bool pn_planes_ok = false;        // the uploaded photon octree qualifies for the one-record-per-level descent
    int32_t n_prange = 0;             // entries of d_pranges in use
    DevBuf<int32_t> d_refs;
    DevBuf<LeafTri> d_leaf_tris;
    DevBuf<double> d_leaf_boxes;          // every leaf reference's own box (gi_device.h: entity_survivors)
    DevBuf<double> d_trace_boxes;         // the closest-hit walk's boxes (gi_device.h: trace_wide_step)
    DevBuf<float> d_tcboxes;              // and the content boxes made of them
    DevBuf<uint32_t> d_tcuse;
    bool lights_clear = false;            // of the scene last uploaded: no entity within a light's radius + the shadow bias of it (gi_layout.h)
    double cut_margin = -1;               // of the scene last uploaded
    bool scene_clipped = false;           // its trace boxes differ from the whole ones
    DevBuf<TriGeom> d_tris;
    DevBuf<TriShade> d_shade;
    DevBuf<Mat> d_mats;
    DevBuf<LightD> d_lights;
    DevBuf<FogD> d_fogs;
    DevBuf<double> d_fog_grid;
    DevBuf<PNode> d_pnodes;
    DevBuf<PRange> d_pranges;
    DevBuf<int32_t> d_pleaf_rank, d_prank_leaf, d_n_pleaf;
    DevBuf<PDescent> d_pdescent;
    bool pdescent_ready = false, pjump_ready = false;   // d_pdescent / d_pjump hold the tables of the current photon map (apply_switches)
    bool fast_descent = true;         // GI_FAST_DESCENT=0: every gather query walks the full photon-octree records
    DevBuf<double> d_ph_pos, d_ph_dircol;
    DevBuf<HaltonDim> d_hdims;
    DevBuf<uint16_t> d_htable;
    DevBuf<unsigned int> d_tile_counter;
    DevBuf<Counters> d_counters;
    // wavefront pipeline workspaces (grown on demand, kept between frames)
    DevBuf<uint32_t> d_pixtab;               // k_pixel_table of the frame being rendered
    DevBuf<unsigned char> d_spool;        // paths of the streaming pipeline: field arrays (PathPool), GI_POOL_BYTES_PER_SLOT each
    size_t spool_slots = 0;
    DevBuf<PixRec> d_pix;
    // a progressive session (gi_progressive_*): the pixel records it owns between steps -- everything else a step uses is the shared scratch above and below
    struct Progressive {
        bool open = false;
        gi_render_params rp{};
        Frame F{};                    // make_frame(rp): max_samples is the session's own
        int schedule = 0;             // 0: refill pipeline, records in st_pixel_xy order; 1: synchronous rounds, records in padded 8x8 tiles (wf_pixel_xy)
        int32_t sample_end = 0;       // E: every pixel has been offered samples [0, E)
        uint32_t n_rec = 0;
        DevBuf<PixRec> pix;
    } prog;
    DevBuf<unsigned int> d_wfcnt;    // rounds (render_adaptive): [0] paths started by k_ad_gen, [1] pixels still wanting samples
    unsigned int* h_wfcnt = nullptr;  // pinned host mirror of d_wfcnt
    DevBuf<double> d_lbuf;            // streaming variant: per-sample radiance of the current chunk
    DevBuf<unsigned long long> d_slot_sample;
    StreamWork work;                     // queues, keys and scratch of the stream passes (gi_stream.inc)
    DevBuf<StreamCtl> d_ctl;
    DevBuf<ShadowQ> d_shq;               // shadow queries the shade stage put off (one light, wide records): entry i belongs to item i of the shade queue
    bool defer_shadows = true;           // GI_DEFER_SHADOWS=0: the shade kernel walks its shadow segments itself
    DevBuf<unsigned int> d_blkcnt;       // per-workgroup append counters [QC_KINDS][GI_MAX_PRODUCER_BLOCKS], 128 bytes apart
    DevBuf<uint32_t> d_segs;             // segment start of every producer workgroup
    DevBuf<uint32_t> d_rs_hist;          // gi_sort.inc: [digit][workgroup] counters of a radix pass
    bool rs_attr_set = false;
    StreamCtl* h_ctl = nullptr;
    size_t lbuf_bytes_max = (size_t)16 << 30;
    // per-stage device time of the last streaming frame (HIP events around every launch, same stream)
    std::vector<hipEvent_t> ev_pool;
    std::vector<int> ev_stage;        // stage id of event pair k (events 2k, 2k+1)
    size_t ev_used = 0;
    bool stage_timing = true;
    float stage_ms[STG_COUNT_MAX] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    int render_mode = 0;              // 0 streaming passes (fixed spp) or rounds (adaptive), 1 megakernel, 2 synchronous rounds always (gi_set_render_mode)
    size_t pool_slots_max = (size_t)1 << 30;    // upper bound on paths in flight; the actual pool is also bounded by free HBM (render_streaming)
    uint32_t finish_threshold = 1u << 17;   // GI_FINISH_THRESHOLD: paths left when the finisher takes over
    bool sample_identity = true;      // GI_SAMPLE_IDENTITY=0: the stream passes always keep the slot -> sample table, also where it would be the identity (stream_samples)
    bool keep_free_list = false;      // GI_KEEP_FREE_LIST=1: the stream passes write the free list in every pass, also where nothing will read it (stream_passes)
    bool early_miss = true;           // GI_EARLY_MISS: the deferred shade kernel ends a path whose next ray leaves the scene without meeting a leaf (stream_passes)
    uint32_t early_turns = 4;         // GI_EARLY_MISS_TURNS: turns of the walk that probe may take before it gives the ray to the trace stage
    uint32_t wave_factor = 0;         // GI_WAVE_FACTOR: finisher stages with at most this many paths per resident wave run one path per wave; 0 = by the size of the frame (stream_passes)
    uint32_t coop_factor = 4;         // finisher stages with at most 4 x coop_factor x (resident waves) paths run one path per group of 16 lanes (at most 2 x: one per wave)
    // finisher stages {paths per wave (0: spread evenly over the resident waves), max vertices}; the last stage runs to MAX_DEPTH.
    // Measured on the default frame (tools/stripe_probe.py): one full-wave stage 60 ms, this plan 51 ms; on 1/8 of the rows 40 -> 30 ms.
    std::vector<std::pair<int, int>> finish_plan = {{0, 1}, {0, 1}, {0, 1}, {0, 1}, {0, 2}, {0, 2}, {0, 4}, {0, 8}, {0, GI_MAX_DEPTH + 1}};
    DevBuf<unsigned int> d_fin_cnt;
    EventTimer t_frame;               // around the kernels of the last gi_render_* / gi_progressive_step_* call
    int last_launches = 0;
    EventTimer t_feat;                // the feature pass (gi_render_features_*) keeps its own: it leaves the frame's times (t_frame, ev_pool) alone
    int aov_lds_refused = -1;         // -1: the k_aov instances were not asked for their LDS yet; else as StreamGrids::lds_refused
    // the denoiser (gi_denoise_*, gi_denoise.inc): a timer of its own again, and its scratch -- the guide records [h][w][8] and two colour
    // buffers [h][w][3], f64, sized on first use and kept
    EventTimer t_dn;
    DevBuf<double> d_dn_guides, d_dn_a, d_dn_b;
    // the guided upsampler (gi_upsample_*, gi_upsample.inc): a timer of its own; its low frame is packed into the denoiser's scratch (dn_reserve)
    EventTimer t_up;
    // the occlusion pass (gi_render_occlusion_*, gi_occlusion.inc): a timer of its own, and the answer of its kernels' LDS request (as aov_lds_refused)
    EventTimer t_ao;
    int ao_lds_refused = -1;
    bool count_enabled = false;       // gi_set_counters(ctx, 1): the megakernel counts the reference's visits (per-node walk)
    bool count_stream = false;        // gi_set_counters(ctx, 2): the streaming kernels count what they execute (StreamCounters)
    DevBuf<StreamCounters> d_stream_cnt;
    unsigned long long stream_shaded = 0;   // shaded hits of the last counted frame (sum of the shade queues' lengths)
    Counters last_counters{};
    int n_cu = 256;
};

namespace {

int fail(gi_ctx* c, int code, const std::string& msg)
{
    if (c) c->err = msg;
    return code;
}
#define HIP_TRY(c, expr)                                                                                     \
    do {                                                                                                     \
        hipError_t e__ = (expr);                                                                             \
        if (e__ != hipSuccess) return fail((c), GI_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e__)); \
    } while (0)

// The photon map's box: the caller's, or the scene's
void frame_box(const gi_ctx* c, const double* box6, double* out)
{
    for (int k = 0; k < 3; k++) { out[k] = box6 ? box6[k] : c->S.root_bmin[k]; out[3 + k] = box6 ? box6[3 + k] : c->S.root_bmax[k]; }
}

// A frame of npix pixels that `render(d_out, d_spp)` leaves in scratch of this call, copied to the caller's arrays (gi_render_host, gi_progressive_step_host)
template <class Render>
int frame_to_host(gi_ctx* c, const char* what, size_t npix, void* h_out, int out_is_f64, int32_t* h_spp, Render render)
{
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = npix * 3 * (out_is_f64 ? 8 : 4);
    DevBuf<unsigned char> d_out;
    DevBuf<int32_t> d_spp;
    HIP_TRY(c, d_out.alloc(bytes));
    if (h_spp) HIP_TRY(c, d_spp.alloc(npix));
    const int rc = render((void*)d_out.p, d_spp.p);
    return rc != GI_OK ? rc : finish_to_host(c, what, {{h_out, d_out.p, bytes}, to_host(h_spp, d_spp, npix)});
}

// The device side of a function-level entry (gi_entries.inc), after its argument and state checks.  in() uploads a caller's array, out() allocates a
// result and notes where it goes (h == nullptr: an optional output nobody asked for -- the kernel still writes it), scratch() is memory of this
// call alone; each takes the element count, once.  run(launch) launches (unless a buffer failed), asks for the launch's status, waits for the
// stream and copies the results back in the order of the out() calls.  launch returns nothing, or a failure it has recorded with fail().
struct Entry {
    gi_ctx* c;
    const char* what;
    hipError_t e;
    DevBuf<unsigned char> buf[16];
    ToHost outs[6];
    int n_buf = 0, n_out = 0;
    Entry(gi_ctx* c_, const char* what_) : c(c_), what(what_), e(hipSetDevice(c_->device)) {}
    template <class T> T* scratch(size_t count)
    {
        if (e == hipSuccess) e = n_buf < 16 ? buf[n_buf].alloc(count * sizeof(T)) : hipErrorOutOfMemory;
        return e == hipSuccess ? reinterpret_cast<T*>(buf[n_buf++].p) : nullptr;
    }
    template <class T> const T* in(const T* h, size_t count)
    {
        if (e == hipSuccess) e = n_buf < 16 ? buf[n_buf].upload(reinterpret_cast<const unsigned char*>(h), count * sizeof(T)) : hipErrorOutOfMemory;
        return e == hipSuccess ? reinterpret_cast<const T*>(buf[n_buf++].p) : nullptr;
    }
    template <class T> T* out(T* h, size_t count)
    {
        T* d = scratch<T>(count);
        if (d && n_out == 6) e = hipErrorOutOfMemory;
        if (e == hipSuccess) outs[n_out++] = ToHost{h, d, count * sizeof(T)};
        return d;
    }
    template <class Launch> int run(Launch launch)
    {
        if (e == hipSuccess) {
            if constexpr (std::is_void<decltype(launch())>::value) launch();
            else if (const int rc = launch()) return rc;
            e = hipGetLastError();
        }
        if (e != hipSuccess) return fail(c, GI_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
        return finish_to_host(c, what, outs, (size_t)n_out);
    }
};

}  // namespace

__global__ __launch_bounds__(1024) void k_rs_scan(uint32_t* ghist, uint32_t total);   // gi_sort.inc
// The Scene fields that follow the context's switches, from the uploaded tables and the switches alone (gi_layout.h: apply_scene_switches, which
// the CPU suite's emulator calls too).  Every upload, every change of the photon map and every gi_set_* of a switch ends here, and nothing else
// assigns these fields.
static void apply_switches(gi_ctx* c)
{
    SceneTables T;
    T.wnodes = c->d_wnodes.p; T.cboxes = c->d_cboxes.p; T.n_cboxes = c->d_cboxes.n;
    T.leaf_boxes = c->d_leaf_boxes.p; T.trace_boxes = c->d_trace_boxes.p;
    T.tcboxes = c->d_tcboxes.p; T.n_tcboxes = c->d_tcboxes.n; T.tcuse = c->d_tcuse.p;
    T.cut_margin = c->cut_margin; T.clipped = c->scene_clipped; T.lights_clear = c->lights_clear;
    T.pn_planes_ok = c->pn_planes_ok;
    T.pdescent = c->pdescent_ready ? c->d_pdescent.p : nullptr;   // (build_photon_tables)
    T.pjump = c->pjump_ready ? c->d_pjump.p : nullptr;
    apply_scene_switches(c->S, T, c->sw);
}

// The tables derived from the photon map c->S points at: the sort key of the gather queries (k_pleaf_rank), the leaves' candidate lists and, for a
// map that qualifies whatever the switches are now, the split records of the fast descent and its jump table (apply_switches decides on their use)
static int build_photon_tables(gi_ctx* c)
{
    Scene& S = c->S;
    S.pleaf_rank = nullptr; S.prank_leaf = nullptr; S.n_pleaf = 0; S.pcand_off = nullptr; S.pcand = nullptr; S.pcand_dc = nullptr;
    c->pdescent_ready = false; c->pjump_ready = false;
    if (S.n_pnode <= 0) return GI_OK;
    if (c->d_pleaf_rank.n < (size_t)S.n_pnode) { HIP_TRY(c, c->d_pleaf_rank.alloc((size_t)S.n_pnode)); HIP_TRY(c, c->d_prank_leaf.alloc((size_t)S.n_pnode)); }
    if (!c->d_n_pleaf.p) HIP_TRY(c, c->d_n_pleaf.alloc(1));
    hipLaunchKernelGGL(k_pleaf_rank, dim3(1), dim3(1024), 0, c->stream, S.pnodes, S.n_pnode, c->d_pleaf_rank.p, c->d_prank_leaf.p, c->d_n_pleaf.p);
    HIP_TRY(c, hipGetLastError());
    int32_t n = 0;
    HIP_TRY(c, hipMemcpyAsync(&n, c->d_n_pleaf.p, sizeof n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    S.pleaf_rank = c->d_pleaf_rank.p; S.prank_leaf = c->d_prank_leaf.p; S.n_pleaf = n;
    S.pcand_off = nullptr; S.pcand = nullptr; S.pcand_dc = nullptr;
    if (c->flat_candidates && n > 0) {
        if (c->d_pcand_off.n < (size_t)n + 1) HIP_TRY(c, c->d_pcand_off.alloc((size_t)n + 1));
        hipLaunchKernelGGL(k_pcand_count, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, c->stream, S.pnodes, c->d_prank_leaf.p, n, c->d_pcand_off.p);
        hipLaunchKernelGGL(k_rs_scan, dim3(1), dim3(1024), 0, c->stream, c->d_pcand_off.p, (uint32_t)n + 1u);
        HIP_TRY(c, hipGetLastError());
        uint32_t total = 0;
        HIP_TRY(c, hipMemcpyAsync(&total, c->d_pcand_off.p + n, sizeof total, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (total > 0 && total < 0x7fffffffu) {
            if (c->d_pcand.n < (size_t)total * 3) { HIP_TRY(c, c->d_pcand.alloc((size_t)total * 3)); HIP_TRY(c, c->d_pcand_dc.alloc((size_t)total * 6)); }
            hipLaunchKernelGGL(k_pcand_fill, dim3(1024), dim3(256), 0, c->stream, S.pnodes, S.pranges, S.ph_pos, S.ph_dircol, c->d_prank_leaf.p, n, c->d_pcand_off.p, c->d_pcand.p, c->d_pcand_dc.p);
            HIP_TRY(c, hipGetLastError());
            S.pcand_off = c->d_pcand_off.p; S.pcand = c->d_pcand.p; S.pcand_dc = c->d_pcand_dc.p;
        }
    }
    // the split records of the descent and the map's own box (gather_find_leaf_fast); the one-record-per-level layout only (children from the parent's planes)
    if (c->fast_descent && c->pn_planes_ok) {
        if (c->d_pdescent.n < (size_t)S.n_pnode) HIP_TRY(c, c->d_pdescent.alloc((size_t)S.n_pnode));
        hipLaunchKernelGGL(k_pdescent, dim3((unsigned)((S.n_pnode + 255) / 256)), dim3(256), 0, c->stream, S.pnodes, S.n_pnode, c->d_pdescent.p);
        HIP_TRY(c, hipGetLastError());
        PNode root;
        HIP_TRY(c, hipMemcpyAsync(&root, S.pnodes, sizeof(PNode), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (int k = 0; k < 3; k++) { S.pmap_bmin[k] = root.bmin[k]; S.pmap_bmax[k] = root.bmax[k]; }
        c->pdescent_ready = true;
        if (c->descent_jump) {
            double ext = 0.0, host[7];
            for (int k = 0; k < 3; k++) { ext = std::max(ext, root.bmax[k] - root.bmin[k]); S.pjump_cell[k] = (root.bmax[k] - root.bmin[k]) / (double)GI_PJUMP_N; S.pjump_inv[k] = (double)GI_PJUMP_N / (root.bmax[k] - root.bmin[k]); }
            bool ok = ext > 0.0;
            for (int k = 0; k < 3; k++) { host[k] = root.bmin[k]; host[3 + k] = S.pjump_cell[k]; if (!(S.pjump_cell[k] > 0.0) || !std::isfinite(S.pjump_inv[k])) ok = false; }
            if (ok) {
                if (c->d_pjump.n < (size_t)GI_PJUMP_N * GI_PJUMP_N * GI_PJUMP_N) HIP_TRY(c, c->d_pjump.alloc((size_t)GI_PJUMP_N * GI_PJUMP_N * GI_PJUMP_N));
                if (c->d_pjump_aux.n < 8) HIP_TRY(c, c->d_pjump_aux.alloc(8));
                host[6] = 0.0;                                                    // (as an int: the "bad" flag)
                HIP_TRY(c, hipMemcpyAsync(c->d_pjump_aux.p, host, sizeof host, hipMemcpyHostToDevice, c->stream));
                hipLaunchKernelGGL(k_pjump, dim3((unsigned)((GI_PJUMP_N * GI_PJUMP_N * GI_PJUMP_N + 255) / 256)), dim3(256), 0, c->stream, c->d_pdescent.p, c->d_pjump_aux.p, c->d_pjump_aux.p + 3, 1e-12 * ext, c->d_pjump.p, reinterpret_cast<int*>(c->d_pjump_aux.p + 6));
                HIP_TRY(c, hipGetLastError());
                int bad = 1;
                HIP_TRY(c, hipMemcpyAsync(&bad, c->d_pjump_aux.p + 6, sizeof bad, hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(c, hipStreamSynchronize(c->stream));
                c->pjump_ready = !bad;
            }
        }
    }
    return GI_OK;
}

// A photon map now in d_pnodes / d_pranges / d_ph_pos / d_ph_dircol (gi_upload_photons, build_photon_map_on_device): the scene reads it from there
static int install_photon_map(gi_ctx* c, int32_t n_node, int32_t n_photon, int32_t n_prange, bool planes_ok)
{
    Scene& S = c->S;
    S.pnodes = c->d_pnodes.p; S.pranges = c->d_pranges.p; S.ph_pos = c->d_ph_pos.p; S.ph_dircol = c->d_ph_dircol.p;
    S.n_pnode = n_node; S.n_photon = n_photon;
    c->n_prange = n_prange;
    c->pn_planes_ok = planes_ok;
    const int rc = build_photon_tables(c);
    apply_switches(c);
    return rc;
}

// no photon map (a fresh PhotonMap): gather queries find nothing
static void clear_photon_map(gi_ctx* c)
{
    Scene& S = c->S;
    S.pnodes = nullptr; S.ph_pos = nullptr; S.ph_dircol = nullptr; S.n_pnode = 0; S.n_photon = 0; S.n_pleaf = 0;
    c->pdescent_ready = false; c->pjump_ready = false;
    apply_switches(c);
}

#include "gi_sort.inc"
#include "gi_photon_build.inc"
#include "gi_denoise.inc"
#include "gi_upsample.inc"
#include "gi_occlusion.inc"

static constexpr size_t kLdsNodes = (size_t)GI_LDS_NODES * sizeof(TNode);
static constexpr size_t kLdsFinishCoop = (size_t)GI_FINISH_COOP_LDS_BYTES;   // the one-path-per-group forms of the finisher: 292 records + content boxes + a heap per group
static constexpr size_t kLdsWideBoxes = (size_t)GI_LDS_WIDE_BOXES_BYTES;   // wide records + their content boxes: k_st_trace / k_st_shadow, one 1024-thread workgroup per CU

// The instances of the k_st_* kernels with their dynamic LDS: every instance of a family is named once, in its table; its selector picks the
// instance a launch runs (FEAT = scene_feat / scene_trace_feat, gi_device.h), and stream_grids walks the same tables.
template <class Fn> struct StKernel { Fn fn; size_t lds; };
using TraceK = StKernel<decltype(&k_st_trace<0, 0>)>;
using ShadeK = StKernel<decltype(&k_st_shade<0, 0, 0>)>;
using ShadowK = StKernel<decltype(&k_st_shadow<0, 0>)>;
using FinishK = StKernel<decltype(&k_st_finish<0, 0, 0>)>;
// k_st_trace<FEAT, WIDE>: FEAT 0, spheres, textures x per-node, wide; then the counting instance
static constexpr TraceK kTrace[] = {
    {k_st_trace<0, 0>, kLdsNodes}, {k_st_trace<0, 1>, kLdsWideBoxes}, {k_st_trace<GI_FEAT_SPHERES, 0>, kLdsNodes}, {k_st_trace<GI_FEAT_SPHERES, 1>, kLdsWideBoxes},
    {k_st_trace<7, 0>, kLdsNodes}, {k_st_trace<7, 1>, kLdsWideBoxes}, {k_st_trace<0, 1, true>, kLdsWideBoxes}};
static TraceK st_trace(int feat, bool wide, bool counting) { return counting ? kTrace[6] : kTrace[(feat == 7 ? 2 : feat) * 2 + (wide ? 1 : 0)]; }
// k_st_shade<FEAT, WIDE, DEFER>: FEAT 0, spheres, fog, textures x per-node, wide, wide with the shadow walks put off (one light; several lights)
// (the one-light form stages the trace stage's records and content boxes for the probe of the next ray: its LDS, one 512-thread workgroup per CU as before)
static constexpr ShadeK kShade[] = {
    {k_st_shade<0, 0, 0>, kLdsNodes}, {k_st_shade<0, 1, 0>, kLdsNodes}, {k_st_shade<0, 1, 1>, kLdsWideBoxes}, {k_st_shade<0, 1, 2>, kLdsNodes},
    {k_st_shade<GI_FEAT_SPHERES, 0, 0>, kLdsNodes}, {k_st_shade<GI_FEAT_SPHERES, 1, 0>, kLdsNodes}, {k_st_shade<GI_FEAT_SPHERES, 1, 1>, kLdsWideBoxes}, {k_st_shade<GI_FEAT_SPHERES, 1, 2>, kLdsNodes},
    {k_st_shade<3, 0, 0>, kLdsNodes}, {k_st_shade<3, 1, 0>, kLdsNodes}, {k_st_shade<3, 1, 1>, kLdsWideBoxes}, {k_st_shade<3, 1, 2>, kLdsNodes},
    {k_st_shade<7, 0, 0>, kLdsNodes}, {k_st_shade<7, 1, 0>, kLdsNodes}, {k_st_shade<7, 1, 1>, kLdsWideBoxes}, {k_st_shade<7, 1, 2>, kLdsNodes}};
static int feat_row(int feat) { return feat == 7 ? 3 : (feat == 3 ? 2 : feat); }   // the levels 0, spheres, fog, textures
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
// k_aov<FEAT, WIDE> (the feature pass): FEAT 0, spheres, textures x per-node, wide -- the rows of kTrace, with the same LDS
using AovK = StKernel<decltype(&k_aov<0, 0>)>;
static constexpr AovK kAov[] = {
    {k_aov<0, 0>, kLdsNodes}, {k_aov<0, 1>, kLdsWideBoxes}, {k_aov<GI_FEAT_SPHERES, 0>, kLdsNodes}, {k_aov<GI_FEAT_SPHERES, 1>, kLdsWideBoxes},
    {k_aov<7, 0>, kLdsNodes}, {k_aov<7, 1>, kLdsWideBoxes}};
static AovK aov_kernel(int feat, bool wide) { return kAov[(feat == 7 ? 2 : feat) * 2 + (wide ? 1 : 0)]; }
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

extern "C" {

int gi_create(gi_ctx** out, int device_ordinal)
{
    if (!out) return GI_E_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return GI_E_NO_DEVICE;
    if (device_ordinal < 0 || device_ordinal >= n) return GI_E_INVALID;
    if (hipSetDevice(device_ordinal) != hipSuccess) return GI_E_NO_DEVICE;
    gi_ctx* c = new gi_ctx();
    c->device = device_ordinal;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_ordinal) == hipSuccess) c->n_cu = prop.multiProcessorCount;
    std::vector<HaltonDim> dims;
    std::vector<uint16_t> table;
    build_halton_tables(dims, table);
    if (c->d_hdims.upload(dims) != hipSuccess || c->d_htable.upload(table) != hipSuccess || c->d_tile_counter.alloc(1) != hipSuccess ||
        c->d_counters.alloc(1) != hipSuccess) {
        delete c;
        return GI_E_HIP;
    }
    c->S.hdims = c->d_hdims.p;
    c->S.htable = c->d_htable.p;
    if (const char* e = getenv("GI_LBUF_MAX_BYTES")) c->lbuf_bytes_max = (size_t)strtoull(e, nullptr, 0);   // per-sample radiance buffer: frames beyond it run in sample chunks
    if (const char* e = getenv("GI_COOP_FACTOR")) c->coop_factor = (uint32_t)strtoul(e, nullptr, 0);
    if (const char* e = getenv("GI_WAVE_FACTOR")) c->wave_factor = std::min<uint32_t>((uint32_t)strtoul(e, nullptr, 0), 0xffffu);
    if (const char* e = getenv("GI_EARLY_MISS")) c->early_miss = atoi(e) != 0;
    if (const char* e = getenv("GI_EARLY_MISS_TURNS")) c->early_turns = (uint32_t)std::min(64, std::max(1, atoi(e)));
    if (const char* e = getenv("GI_SAMPLE_IDENTITY")) c->sample_identity = atoi(e) != 0;
    if (const char* e = getenv("GI_KEEP_FREE_LIST")) c->keep_free_list = atoi(e) != 0;
    if (const char* e = getenv("GI_SORT_CONT")) c->sort_cont = atoi(e) != 0;
    if (const char* e = getenv("GI_DESCENT_JUMP")) c->descent_jump = atoi(e) != 0;
    if (const char* e = getenv("GI_FLAT_CANDIDATES")) c->flat_candidates = atoi(e) != 0;
    if (const char* e = getenv("GI_GATHER_WAVE_BELOW")) c->gather_wave_below = (uint32_t)strtoul(e, nullptr, 10);
    if (const char* e = getenv("GI_SORT_SHADE")) c->sort_shade = atoi(e) != 0;
    if (const char* e = getenv("GI_SORT_SHADE_LO")) c->sort_shade_lo = std::max(0, atoi(e));
    if (const char* e = getenv("GI_SORT_LO_BIT")) c->sort_lo_bit = std::min(26, std::max(0, atoi(e)));
    if (const char* e = getenv("GI_DEFER_SHADOWS")) c->defer_shadows = atoi(e) != 0;
    if (const char* e = getenv("GI_FAST_DESCENT")) c->fast_descent = atoi(e) != 0;
    if (const char* e = getenv("GI_ENTITY_BOXES")) c->sw.entity_boxes = atoi(e) != 0;
    if (const char* e = getenv("GI_CLIP_BOXES")) c->sw.clip_boxes = atoi(e) != 0;
    if (const char* e = getenv("GI_WALK_CUT")) c->sw.walk_cut = atoi(e) != 0;
    if (const char* e = getenv("GI_REFILL_MIN")) c->refill_min = (uint32_t)std::min(64, std::max(1, atoi(e)));
    if (const char* e = getenv("GI_FINISH_THRESHOLD")) c->finish_threshold = (uint32_t)strtoul(e, nullptr, 0);   // tuning knobs
    if (const char* e = getenv("GI_FINISH_PLAN")) {   // "lanes:vertices,lanes:vertices,..."
        std::vector<std::pair<int, int>> plan;
        for (const char* q = e; *q;) {
            int l = 0, b = 0, used = 0;
            if (sscanf(q, "%d:%d%n", &l, &b, &used) != 2 || l < 0 || l > 64 || b < 1) { plan.clear(); break; }
            plan.push_back({l, b});
            q += used;
            if (*q == ',') q++;
        }
        if (!plan.empty()) c->finish_plan = plan;
    }
    *out = c;
    return GI_OK;
}

void gi_destroy(gi_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
    if (c->h_wfcnt) (void)hipHostFree(c->h_wfcnt);
    if (c->h_ctl) (void)hipHostFree(c->h_ctl);
    for (EventTimer* t : {&c->t_frame, &c->t_feat, &c->t_dn, &c->t_up, &c->t_ao}) t->destroy();
    delete c;
}

const char* gi_last_error(const gi_ctx* c) { return c ? c->err.c_str() : "null context"; }

int gi_set_stream(gi_ctx* c, void* s)
{
    if (!c) return GI_E_INVALID;
    c->stream = (hipStream_t)s;
    return GI_OK;
}

int gi_upload_scene(gi_ctx* c, const gi_scene_desc* d)
{
    if (!c) return GI_E_INVALID;
    c->prog.open = false;   // a progressive session belongs to the scene and photon map it began on
    HostScene H;
    std::string err;
    if (!layout_scene(d, H, err)) return fail(c, GI_E_INVALID, err);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, c->d_tnodes.upload(H.tnodes));
    HIP_TRY(c, c->d_wnodes.upload(H.wnodes));
    HIP_TRY(c, c->d_wleaf_id.upload(H.wleaf_id));
    HIP_TRY(c, c->d_cboxes.upload(H.cboxes));
    HIP_TRY(c, c->d_cuse.upload(H.cuse));
    HIP_TRY(c, c->d_texs.upload(H.texs));
    HIP_TRY(c, c->d_tri_uv.upload(H.tri_uv));
    HIP_TRY(c, c->d_tex_pixels.upload(H.tex_pixels));
    HIP_TRY(c, c->d_tex_lut.upload(H.tex_lut));
    HIP_TRY(c, c->d_refs.upload(H.refs));
    HIP_TRY(c, c->d_leaf_tris.upload(H.leaf_tris));
    HIP_TRY(c, c->d_leaf_boxes.upload(H.leaf_boxes));
    HIP_TRY(c, c->d_trace_boxes.upload(H.trace_boxes));
    HIP_TRY(c, c->d_tcboxes.upload(H.tcboxes));
    HIP_TRY(c, c->d_tcuse.upload(H.tcuse));
    c->cut_margin = H.cut_margin;
    c->scene_clipped = H.clipped;
    c->lights_clear = H.lights_clear;
    HIP_TRY(c, c->d_tris.upload(H.tris));
    HIP_TRY(c, c->d_shade.upload(H.shade));
    HIP_TRY(c, c->d_mats.upload(H.mats));
    HIP_TRY(c, c->d_lights.upload(H.lights));
    HIP_TRY(c, c->d_fogs.upload(H.fogs));
    HIP_TRY(c, c->d_fog_grid.upload(H.fog_grid));
    Scene& S = c->S;
    S.tnodes = c->d_tnodes.p; S.leaf_refs = c->d_refs.p; S.leaf_tris = c->d_leaf_tris.p; S.tris = c->d_tris.p; S.shade = c->d_shade.p;
    S.mats = c->d_mats.p; S.lights = c->d_lights.p;
    S.n_node = H.n_node; S.n_tri = H.n_tri; S.n_light = H.n_light;
    for (int k = 0; k < 3; k++) { S.root_bmin[k] = H.tnodes[0].bmin[k]; S.root_bmax[k] = H.tnodes[0].bmax[k]; }
    S.n_wnode = (int32_t)H.wnodes.size();
    S.wleaf_id = c->d_wleaf_id.p;
    S.cuse = c->d_cuse.p;
    S.tri_uv = c->d_tri_uv.p; S.texs = c->d_texs.p; S.tex_pixels = c->d_tex_pixels.p; S.tex_lut = c->d_tex_lut.p; S.n_tex = H.n_tex();
    S.has_spheres = 0;
    S.fogs = c->d_fogs.p; S.fog_grid = c->d_fog_grid.p; S.n_fog = H.n_fog();
    for (const TriGeom& g : H.tris) if (g.flags & 4u) S.has_spheres = 1;
    for (int k = 0; k < 3; k++) S.ambient[k] = H.ambient[k];
    // the photon map stays as it is: the reference keeps a valid map when the scene is edited and rebuilt (include/raytracer.h:56-72);
    // RayTracer::setScene, which allocates a fresh PhotonMap (include/raytracer.h:38), is gi_upload_scene + gi_clear_photons
    c->have_scene = true;
    apply_switches(c);
    return GI_OK;
}

int gi_clear_photons(gi_ctx* c)
{
    if (!c) return GI_E_INVALID;
    c->prog.open = false;
    clear_photon_map(c);
    return GI_OK;
}

int gi_upload_photons(gi_ctx* c, const gi_photon_map_desc* d)
{
    if (!c || !d) return GI_E_INVALID;
    c->prog.open = false;
    if (!c->have_scene) return fail(c, GI_E_STATE, "upload_photons: no scene");
    HostPhotons H;
    std::string err;
    if (!layout_photons(d, H, err)) return fail(c, GI_E_INVALID, err);
    HIP_TRY(c, hipSetDevice(c->device));
    if (H.n_node == 0) {
        clear_photon_map(c);
        return GI_OK;
    }
    HIP_TRY(c, c->d_pnodes.upload(H.nodes));
    HIP_TRY(c, c->d_pranges.upload(H.ranges));
    HIP_TRY(c, c->d_ph_pos.upload(H.pos));
    HIP_TRY(c, c->d_ph_dircol.upload(H.dircol));
    return install_photon_map(c, H.n_node, H.n_photon, (int32_t)H.ranges.size(), H.planes_ok);
}

int gi_local_rows(const gi_render_params* p) { return local_rows(p); }

#include "gi_stream.inc"   // the scheduler: stream_samples, run_rounds, stream_passes and what the render entries below choose between

int gi_render_device(gi_ctx* c, const gi_render_params* p, void* d_out, int out_is_f64, int32_t* d_spp, volatile const int* cancel)
{
    if (!c || !d_out) return GI_E_INVALID;
    if (!c->have_scene) return fail(c, GI_E_STATE, "render: no scene uploaded");
    Frame F;
    std::string ferr;
    if (!make_frame(p, F, ferr)) return fail(c, GI_E_INVALID, ferr);
    if (cancel && *cancel) return fail(c, GI_E_CANCELLED, "render: cancelled");
    HIP_TRY(c, hipSetDevice(c->device));
    c->t_frame.reset(); c->last_launches = 0;
    if (F.local_rows == 0) return GI_OK;
    if (c->render_mode == 1 || c->count_enabled) return render_megakernel(c, F, d_out, out_is_f64, d_spp);
    if (c->count_stream && !uses_refill_schedule(c, F))
        return fail(c, GI_E_STATE, "render: the streaming work counters (gi_set_counters 2) belong to fixed-sample-count frames of the wavefront pipeline");
    if (uses_refill_schedule(c, F)) return render_streaming(c, F, d_out, out_is_f64, d_spp, cancel);
    return render_adaptive(c, F, d_out, out_is_f64, d_spp, cancel);
}

int gi_set_wide_nodes(gi_ctx* c, int enable)
{
    if (!c) return GI_E_INVALID;
    c->sw.wide = enable != 0;
    apply_switches(c);
    return (c->S.wnodes ? 1 : 0) | (c->S.pn_planes ? 2 : 0);
}

int gi_set_content_culling(gi_ctx* c, int enable)
{
    if (!c) return GI_E_INVALID;
    c->sw.cull = enable != 0;
    apply_switches(c);
    return c->S.cboxes ? 1 : 0;
}

int gi_set_entity_boxes(gi_ctx* c, int enable)
{
    if (!c) return GI_E_INVALID;
    c->sw.entity_boxes = enable != 0;
    apply_switches(c);
    return c->S.leaf_boxes ? 1 : 0;
}

int gi_set_render_mode(gi_ctx* c, int mode)
{
    if (!c || mode < 0 || mode > 2) return GI_E_INVALID;
    c->render_mode = mode;
    return GI_OK;
}

int gi_set_pool_slots(gi_ctx* c, int64_t slots)
{
    if (!c || slots < 64) return GI_E_INVALID;
    c->pool_slots_max = (size_t)slots;
    return GI_OK;
}

int gi_last_render_ms(gi_ctx* c, float* ms, int32_t* n_launches)
{
    if (!c) return GI_E_INVALID;
    float frame_ms = 0;
    HIP_TRY(c, c->t_frame.read(&frame_ms));
    for (int k = 0; k < STG_COUNT_MAX; k++) c->stage_ms[k] = 0;
    const bool debug_stages = getenv("GI_DEBUG_STAGES") != nullptr;   // read at every call
    for (size_t k = 0; k + 1 < c->ev_used + 1 && k / 2 < c->ev_stage.size() && k + 1 < c->ev_pool.size() && k < c->ev_used; k += 2) {
        float t = 0;
        if (hipEventElapsedTime(&t, c->ev_pool[k], c->ev_pool[k + 1]) == hipSuccess) c->stage_ms[c->ev_stage[k / 2]] += t;
        if (debug_stages) fprintf(stderr, "[stage] %d %.3f ms\n", c->ev_stage[k / 2], t);
    }
    if (ms) *ms = frame_ms;
    if (n_launches) *n_launches = c->last_launches;
    return GI_OK;
}

int gi_last_stage_ms(gi_ctx* c, float* out8)
{
    if (!c || !out8) return GI_E_INVALID;
    int rc = gi_last_render_ms(c, nullptr, nullptr);
    if (rc) return rc;
    for (int k = 0; k < 8; k++) out8[k] = c->stage_ms[k];
    out8[STG_SHADE] += c->stage_ms[STG_SHADOW];   // the shade stage of the 8-entry form includes the shadow walks it put off
    return GI_OK;
}

int gi_last_kernel_ms(gi_ctx* c, float* out10)
{
    if (!c || !out10) return GI_E_INVALID;
    int rc = gi_last_render_ms(c, nullptr, nullptr);
    if (rc) return rc;
    for (int k = 0; k < STG_COUNT_MAX; k++) out10[k] = c->stage_ms[k];
    return GI_OK;
}

int gi_set_counters(gi_ctx* c, int enable)
{
    if (!c || enable < 0 || enable > 2) return GI_E_INVALID;
    c->count_enabled = enable == 1;
    c->count_stream = enable == 2;
    return GI_OK;
}
int gi_get_stream_counters(gi_ctx* c, int64_t* out17 /* [19] */)
{
    if (!c || !out17) return GI_E_INVALID;
    if (!c->d_stream_cnt.p) return fail(c, GI_E_STATE, "stream counters: no counted frame was rendered (gi_set_counters(ctx, 2), fixed sample count)");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    StreamCounters h;
    HIP_TRY(c, hipMemcpy(&h, c->d_stream_cnt.p, sizeof h, hipMemcpyDeviceToHost));
    for (int k = 0; k < 6; k++) { out17[k] = (int64_t)h.trace[k]; out17[7 + k] = (int64_t)h.shadow[k]; }
    out17[6] = (int64_t)h.trace_rays; out17[13] = (int64_t)h.shadow_rays;
    out17[14] = (int64_t)h.gather_queries; out17[15] = (int64_t)h.gather_cand; out17[16] = (int64_t)c->stream_shaded;
    out17[17] = (int64_t)h.trace[6]; out17[18] = (int64_t)h.shadow[6];
    return GI_OK;
}
int gi_get_counters(gi_ctx* c, int64_t* out8)
{
    if (!c || !out8) return GI_E_INVALID;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    Counters h;
    HIP_TRY(c, hipMemcpy(&h, c->d_counters.p, sizeof h, hipMemcpyDeviceToHost));
    out8[0] = (int64_t)h.v_trace; out8[1] = (int64_t)h.v_shadow; out8[2] = (int64_t)h.tri; out8[3] = (int64_t)h.shaded;
    out8[4] = (int64_t)h.pcand; out8[5] = (int64_t)h.traces; out8[6] = (int64_t)h.shadows; out8[7] = (int64_t)h.gathers;
    return GI_OK;
}

int gi_render_host(gi_ctx* c, const gi_render_params* p, void* h_out, int out_is_f64, int32_t* h_spp, volatile const int* cancel)
{
    if (!c || !h_out || !p) return GI_E_INVALID;
    const size_t npix = (size_t)gi_local_rows(p) * (size_t)std::max(p->width, 0);
    if (npix == 0) return GI_OK;
    return frame_to_host(c, "render_host", npix, h_out, out_is_f64, h_spp,
                         [&](void* d_out, int32_t* d_spp) { return gi_render_device(c, p, d_out, out_is_f64, d_spp, cancel); });
}

#include "gi_progressive.inc"

// ---- first-hit feature buffers (an addition: the reference renders radiance only; the values are those RayTracer::radiance holds after trace()
// of the primary ray, include/raytracer.h:186-210)
int gi_render_features_device(gi_ctx* c, const gi_render_params* p, int32_t n_samples, void* d_out, int out_is_f64, int32_t* d_ids)
{
    if (!c) return GI_E_INVALID;
    c->t_feat.reset();
    if (!d_out) return GI_E_INVALID;
    if (!c->have_scene) return fail(c, GI_E_STATE, "render_features: no scene uploaded");
    Frame F;
    std::string ferr;
    if (!make_frame(p, F, ferr)) return fail(c, GI_E_INVALID, ferr);
    if (n_samples < 1) return fail(c, GI_E_INVALID, "render_features: n_samples must be at least 1");
    // Halton index of sample s = (offset of the pixel < inc) + s * inc, in 32 bits as in the beauty pass
    if ((unsigned long long)n_samples * F.he.inc > (1ull << 32))
        return fail(c, GI_E_INVALID, "render_features: n_samples = " + std::to_string(n_samples) + " takes the Halton index of a " + std::to_string(F.w) + " x " + std::to_string(F.h) +
                                     " frame beyond 32 bits (at most " + std::to_string((1ull << 32) / F.he.inc) + ")");
    HIP_TRY(c, hipSetDevice(c->device));
    if (F.local_rows == 0) return GI_OK;
    if (c->aov_lds_refused < 0) { c->aov_lds_refused = 0; ask_for_lds(kAov, c->aov_lds_refused); }
    if (c->aov_lds_refused) return fail(c, GI_E_HIP, "render_features: the device refused " + std::to_string(c->aov_lds_refused) + " bytes of dynamic LDS per workgroup");
    const uint32_t n_pix = (uint32_t)F.w * (uint32_t)F.local_rows;
    const AovK k = aov_kernel(scene_trace_feat(c->S), c->S.wnodes != nullptr);
    HIP_TRY(c, c->t_feat.begin(c->stream));
    hipLaunchKernelGGL(k.fn, dim3((n_pix + GI_AOV_BLOCK - 1) / GI_AOV_BLOCK), dim3(GI_AOV_BLOCK), k.lds, c->stream, c->S, F, n_pix, n_samples, d_out, out_is_f64, d_ids);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, c->t_feat.end(c->stream));
    return GI_OK;
}

int gi_render_features_host(gi_ctx* c, const gi_render_params* p, int32_t n_samples, void* h_out, int out_is_f64, int32_t* h_ids)
{
    if (!c) return GI_E_INVALID;
    c->t_feat.reset();
    if (!h_out || !p) return GI_E_INVALID;
    const size_t npix = (size_t)gi_local_rows(p) * (size_t)std::max(p->width, 0);
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = npix * 8 * (out_is_f64 ? 8 : 4);
    DevBuf<unsigned char> d_out;
    DevBuf<int32_t> d_ids;
    HIP_TRY(c, d_out.alloc(bytes));
    if (h_ids) HIP_TRY(c, d_ids.alloc(npix * 2));
    const int rc = gi_render_features_device(c, p, n_samples, d_out.p, out_is_f64, d_ids.p);
    return rc != GI_OK ? rc : finish_to_host(c, "render_features_host", {{h_out, d_out.p, bytes}, to_host(h_ids, d_ids, npix * 2)}, &c->t_feat);
}

int gi_last_features_ms(gi_ctx* c, float* ms)
{
    if (!c || !ms) return GI_E_INVALID;
    HIP_TRY(c, c->t_feat.read(ms));
    return GI_OK;
}

#include "gi_entries.inc"

#include "gi_group.inc"

}  // extern "C"
