// gi_stages.inc -- the stage kernels of the streaming pipeline and what they share: StreamCtl, the per-workgroup queue appends (seg_start, chunk_item),
// GenArgs, hand_out, k_st_trace, k_iota, k_st_shade, k_st_shadow, k_st_compact, the photon gather and k_st_finish.  Kernels only: the scheduler that
// launches them is gi_stream.inc, behind the context and the instance tables.  Needs gi_lds.h and gi_pool.h; included by gi_kernels.hip.  It
// includes gi_gather.inc itself, between the compaction (which keys the gather's queries) and the finisher (which calls finish_gathers).
//
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
struct GenArgs {
    Frame F;
    const uint32_t* q_free;           // free slots to fill (nullptr: slots 0 .. n_gen - 1)
    uint32_t n_gen, n_pix;
    unsigned long long id_base, sample_begin;
    int s_begin;
    const uint32_t* pixtab;           // per pixel of this rank, tile order: the Halton index of its sample 0 (k_pixel_table)
    double inv_n_pix;
};
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
