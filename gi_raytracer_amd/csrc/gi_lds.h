// gi_lds.h -- the octree top in LDS (LdsNodes, LdsWideT, LdsWideCoop, stage_*_in_lds, LdsSrc) and the executed-work counters of the streaming
// kernels (StreamCounters, flush_*).  Device side only, but for the read-out of the GI_EXP_DIV experiment, which stands beside the counters it reads.
// Needs gi_device.h (TNode, WNode, NodeView, content_cull, WalkCnt); included by gi_kernels.hip ahead of every kernel that walks the octree.
//
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
