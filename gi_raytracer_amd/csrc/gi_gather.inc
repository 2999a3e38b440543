// gi_gather.inc -- the photon gather's wave-level forms and its kernels.  Included by gi_stages.inc behind PathPool, sample_of, chunk_item and
// k_st_compact (which keys the queries: gather_key).  The selection they share with the per-lane form -- key, contribution, the two sums, the
// end rule, the exact pass -- and the one result write are in gi_gather.h; here is only how each form brings a leaf's candidates to them:
//   k_st_gather        a wave of 64 queries, served leaf by leaf: a leaf's candidates staged in LDS, 64 at a time, for the lanes whose query lies in it
//                      (a wave that spans more than GI_GATHER_RUNS leaves, or a map without written-out candidate lists: gather_in_leaf per lane)
//   gather_wave        a wave per query, a candidate per lane: k_st_gather_wave (late passes) and finish_gathers (the finisher)
//   k_gather           gather() per lane, the function-level entry (parity tests, samplePhotons)

// Gather queries are sorted by the photon-map leaf that contains them (keys from k_st_compact): queries of one leaf share their candidate
// photons and stand side by side in a wave.  In a large pass a leaf serves thousands of queries, so most waves hold 64 queries of ONE leaf:
// such a wave copies the leaf's candidate photons into LDS once (64 at a time, one photon per lane, coalesced) and every lane scans them
// from there -- a broadcast LDS read per candidate instead of an L2 round trip per lane.  A wave that holds the queries of several leaves
// (the tail of a large pass; nearly every wave of a pass of a few hundred thousand to a few million queries, where a leaf serves tens) does
// the same once per leaf, one run of lanes after the other: all 64 lanes stage and select, the lanes of the run take the sums.  That is more
// instructions than a walk per lane, but no chain of dependent L2 reads: the per-lane walk makes two passes of 70 to 120 candidates, four
// loads at a time, and such a pass holds too few waves to hide them.  Every path fills a GatherAcc through the steps of gi_gather.h, i.e.
// the same arithmetic in the same order.
#define GI_GCHUNK 64
#ifndef GI_GATHER_WAVES
#define GI_GATHER_WAVES 4      // waves per SIMD the gather kernel is compiled for (launch bound)
#endif
// Pass 1 of the cooperative path keeps a lane's 32 smallest keys sorted in registers and folds the candidates in 32 at a time
// (ksel_tau, gi_gather.h): 18 branch-free instructions per candidate; the LDS heap costs ~55, because with 64 lanes some lane always has
// to sift, so the wave pays a full sift for nearly every candidate.  The result (tau = 32nd smallest float key) is the same number.
static_assert(GI_GCHUNK == 64, "ksel_tau stages the candidates 64 at a time");
// A wave whose queries lie in up to GI_GATHER_RUNS leaves takes them one leaf after the other through the cooperative path; with more leaves than
// that the 64 lanes idle through too many selections that are not theirs, and every lane walks its own leaf (gather_in_leaf).
#ifndef GI_GATHER_RUNS
#define GI_GATHER_RUNS 16
#endif
template <bool COUNT>
__global__ __launch_bounds__(GI_BLOCK, GI_GATHER_WAVES) void k_st_gather(Scene S, PathPool pool, const uint32_t* keys, const uint32_t* vals, uint32_t n_in,
                                                                         const unsigned long long* slot_sample, unsigned long long sample0, double* lbuf, StreamCounters* sc)
{
    unsigned long long n_q = 0, n_c = 0;   // COUNT: queries of this lane, candidates they scanned (a leaf's whole candidate list per query, as PhotonMap::getInRange returns it)
    // 8 KB of LDS per wave: the staged candidates of the cooperative path (64 x 9 doubles) or the float heaps of the per-lane walk (32 x 64),
    // never both at once -- a wave is in one of the two
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
        const uint32_t i = chunk_item(u, cs) + lane;
        const bool valid = i < n_in;
        const uint32_t rank = valid ? keys[i] : 0xffffffffu;                       // rank of the query's leaf among the leaves with candidates
        const bool has_leaf = valid && rank < (uint32_t)S.n_pleaf;
        const uint32_t leaf = has_leaf ? (uint32_t)S.prank_leaf[rank] : 0xffffffffu;
        if constexpr (COUNT) { if (valid) n_q++; }
        // the runs of the wave: lanes of one leaf stand side by side (the queries are in leaf order), so a run starts where a lane's leaf is not its left
        // neighbour's.  (Queries in another order -- gi_debug_gather_pass, sort = 0 -- give more starts than leaves, which only moves the limit.)
        unsigned long long todo = __ballot(has_leaf);                              // lanes whose query is still to be served
        if (todo == 0ull) continue;
        const uint32_t left = (uint32_t)__shfl_up((int)leaf, 1);
        const int n_runs = __popcll(__ballot(has_leaf && (lane == 0u || leaf != left)));
        const uint32_t gslot = valid ? vals[i] : 0u;
        if (n_runs > 1 && (!S.pcand || n_runs > GI_GATHER_RUNS)) {
            if (has_leaf) {
                if constexpr (COUNT) n_c += (unsigned long long)S.pnodes[leaf].u.lf.nb_photons;
                PathRef pr = pool[gslot];
                stage_gather_in_leaf(S, pr, (int32_t)leaf, heap, 64, lbuf + (sample_of(slot_sample, sample0, gslot) - sample0) * 3);
            }
            continue;
        }
        const V3 qpos = valid ? ld3(pool.hit[gslot].hpos) : v3(0, 0, 0), qdir = valid ? ld3(pool.gath[gslot].gdir) : v3(0, 0, 0);
        // The cooperative gather of the queries of ONE leaf (leaf0, of rank rank0; both wave-uniform): `mine` = this lane holds one of them.  All 64 lanes
        // stage and run the selection (the barriers in stage are wave barriers); only the lanes with a query take sums and write a result.
        auto gather_leaf = [&](uint32_t leaf0, uint32_t rank0, bool mine) {
            const PNode& lf = S.pnodes[leaf0];
            const int ncand = lf.u.lf.nb_photons;
            if constexpr (COUNT) { if (mine) n_c += (unsigned long long)ncand; }
            if (ncand == 0) return;
            const PRange* ranges = S.pranges + lf.nb_off;
            GatherAcc a;
            g_begin(a, qpos, qdir, heap, 64, ncand);
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
            a.tau = ksel_tau(ncand, [&](int32_t c0, int32_t m) { stage(c0, m, c0 == 0); }, [&](int32_t k) { return (float)g_d2(a, ld3(cand[k])); });
            for (int32_t c0 = 0; c0 < ncand; c0 += GI_GCHUNK) {
                const int32_t m = min((int32_t)GI_GCHUNK, ncand - c0);
                if (c0 != 0) stage(c0, m, true);
                if (mine) {
                    // g_acc per candidate, with the rare case set aside: a candidate whose key EQUALS tau (the 32nd smallest itself; one per
                    // query, more only when float keys tie) is some lane's business for nearly every candidate of the wave, so its branch --
                    // a sum of its own, a count, a running maximum -- would run for nearly every candidate.  The loop takes the below-tau half
                    // and only notes where such candidates are; they are added afterwards, in candidate order, by g_acc itself.
                    int n_eq = 0;
                    int32_t k_eq = 0;
                    for (int32_t k = 0; k < m; k++) {
                        const double* q = cand[k];
                        const float key = (float)g_d2(a, ld3(q));
                        if (key < a.tau) g_add_lt(a, g_contrib(a, q + 3));
                        else if (key == a.tau) {
                            if (n_eq == 0) k_eq = k;
                            n_eq++;
                        }
                    }
                    if (n_eq == 1) g_acc(a, ld3(cand[k_eq]), cand[k_eq] + 3);
                    else if (n_eq > 1) {       // float keys tie at tau: walk on from the first of them
                        for (int32_t k = k_eq; n_eq > 0 && k < m; k++) {
                            const double* q = cand[k];
                            if ((float)g_d2(a, ld3(q)) == a.tau) { g_acc(a, ld3(q), q + 3); n_eq--; }
                        }
                    }
                }
            }
            if (mine) {
                V3 caustic;
                if (!g_end(a, caustic)) caustic = g_exact(S, (int32_t)leaf0, a);   // float keys tie across rank 32
                gather_add(lbuf + (sample_of(slot_sample, sample0, gslot) - sample0) * 3, pool.gath[gslot].gcoef, caustic);   // the path's radiance lives in the per-sample buffer
            }
        };
        // one run per turn, the leftmost lane not yet served names it; a wave of one leaf (nearly all of a large pass) makes one turn.  todo is wave-uniform
        do {
            const int src = __ffsll((long long)todo) - 1;
            const uint32_t leaf0 = (uint32_t)__builtin_amdgcn_readlane((int)leaf, src), rank0 = (uint32_t)__builtin_amdgcn_readlane((int)rank, src);
            const bool mine = leaf == leaf0;                                        // (a lane without a leaf holds 0xffffffff)
            todo &= ~__ballot(mine);
            gather_leaf(leaf0, rank0, mine);
        } while (todo != 0ull);
    }
    if constexpr (COUNT) { flush_u64(&sc->gather_queries, n_q); flush_u64(&sc->gather_cand, n_c); }
}

// A query per WAVE, for the passes with few queries.  Late passes hold a handful of queries per photon-map leaf: a wave of k_st_gather then spans
// more leaves than it serves one after the other (GI_GATHER_RUNS) and lets every lane walk its own leaf, which lasts as long as some five thousand
// candidate steps of one wave (1.2 - 1.6 ms on the benchmark frame, whatever the number of queries).  Passes whose waves still fit the runs take
// 1.6 ms at 2.0 M queries, 1.0 at 1.0 M, 0.9 at 520 k, 0.7 at 337 k and 0.6 at 214 k; below GI_GATHER_WAVE_BELOW queries (200 000: 0.5 ms) this
// form takes over.  Here the lanes take a CANDIDATE
// each: 64 keys per step, the 32 smallest kept across the lanes (a bitonic sort of the 64 new keys through lane exchanges, the smaller half against
// the best so far, a bitonic merge: ~110 instructions per 64 candidates instead of 18 per candidate and query), tau read off lane K - 1; the second
// pass computes every lane's contribution and adds those below tau in CANDIDATE ORDER (a lane at a time, read off by v_readlane, through g_add_lt), so
// the sums are the sums of g_acc to the last bit; the tie group (keys equal to tau) likewise; float-key ties across rank 32 go to lane 0's g_exact.
__device__ __forceinline__ double wave_read(double v, int src_lane)      // src_lane is wave-uniform
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src_lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), src_lane);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ V3 wave_read(V3 v, int src_lane) { return v3(wave_read(v.x, src_lane), wave_read(v.y, src_lane), wave_read(v.z, src_lane)); }
__device__ __forceinline__ V3 gather_wave(const Scene& S, int32_t leaf, uint32_t rank, V3 pos, V3 dir, uint32_t lane, int* n_cand_out)
{
    const int ncand = S.pnodes[leaf].u.lf.nb_photons;
    if (n_cand_out) *n_cand_out = ncand;
    V3 res = v3(0, 0, 0);
    if (ncand == 0) return res;
    const size_t cbase = (size_t)S.pcand_off[rank];
    GatherAcc a;           // wave-uniform: every lane holds the query's sums
    g_begin(a, pos, dir, nullptr, 0, ncand);
    // pass 1: the K-th smallest float key.  lane j < 32 holds the j-th smallest so far
    float best = INFINITY;
    for (int32_t c0 = 0; c0 < ncand; c0 += 64) {
        const int32_t c = c0 + (int32_t)lane;
        float key = INFINITY;
        if (c < ncand) key = (float)g_d2(a, ld3(S.pcand + (cbase + (size_t)c) * 3));
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
    a.tau = __shfl(best, g_k(a) - 1);
    // pass 2: every lane its candidate's contribution; the wave adds them in candidate order
    for (int32_t c0 = 0; c0 < ncand; c0 += 64) {
        const int32_t c = c0 + (int32_t)lane;
        bool lt = false, eq = false;
        double d2 = 0;
        V3 contrib = v3(0, 0, 0);
        if (c < ncand) {
            d2 = g_d2(a, ld3(S.pcand + (cbase + (size_t)c) * 3));
            const float key = (float)d2;
            lt = key < a.tau; eq = key == a.tau;
            if (lt || eq) contrib = g_contrib(a, S.pcand_dc + (cbase + (size_t)c) * 6);
        }
        unsigned long long mlt = __ballot(lt), meq = __ballot(eq);
        while (mlt != 0ull) {
            const int b = __ffsll((long long)mlt) - 1;
            mlt &= mlt - 1ull;
            g_add_lt(a, wave_read(contrib, b));
        }
        while (meq != 0ull) {
            const int b = __ffsll((long long)meq) - 1;
            meq &= meq - 1ull;
            g_add_eq(a, wave_read(contrib, b), wave_read(d2, b));
        }
    }
    if (!g_end(a, res)) {            // float keys tie across rank 32: the exact pass, by one lane
        if (lane == 0u) res = g_exact(S, leaf, a);
        res = wave_read(res, 0);
    }
    return res;
}
#define GI_GW_BLOCK 256      // four waves: a wave per SIMD and workgroup, five workgroups per CU at 87 registers
template <bool COUNT>
__global__ __launch_bounds__(GI_GW_BLOCK) void k_st_gather_wave(Scene S, PathPool pool, const uint32_t* keys, const uint32_t* vals, uint32_t n_in,
                                                            const unsigned long long* slot_sample, unsigned long long sample0, double* lbuf, StreamCounters* sc)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;
    unsigned long long n_q = 0, n_c = 0;
    for (uint32_t q = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; q < n_in; q += n_waves) {
        const uint32_t rank = (uint32_t)__builtin_amdgcn_readfirstlane((int)keys[q]);
        if constexpr (COUNT) n_q++;
        if (rank >= (uint32_t)S.n_pleaf) continue;
        const int32_t leaf = __builtin_amdgcn_readfirstlane(S.prank_leaf[rank]);
        const uint32_t slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)vals[q]);
        int nc = 0;
        const V3 caustic = gather_wave(S, leaf, rank, ld3(pool.hit[slot].hpos), ld3(pool.gath[slot].gdir), lane, &nc);
        if constexpr (COUNT) n_c += (unsigned long long)nc;
        if (lane == 0u && nc > 0) gather_add(lbuf + (sample_of(slot_sample, sample0, slot) - sample0) * 3, pool.gath[slot].gcoef, caustic);   // the path's radiance lives in the per-sample buffer
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

// The photon gathers the paths of a finisher wave (k_st_finish) have pending after a vertex (`pending`: this lane's -- or, with G lanes per path, this
// group's -- path has one).  Up to GI_FIN_WAVE_GATHERS of them are served by the whole wave one after the other (gather_wave); more than that (a stage that
// still holds a path in most lanes), or no written-out candidate lists, and every path walks its own leaf with its own heap (stage_gather).  Called by all 64 lanes.
#ifndef GI_FIN_WAVE_GATHERS
#define GI_FIN_WAVE_GATHERS 24
#endif
__device__ __forceinline__ void finish_gathers(const Scene& S, PathRec& p, bool pending, uint32_t G, float* heap, int heap_stride, uint32_t lane)
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
        const V3 gp = wave_read(ld3(p.hpos), src), gd = wave_read(ld3(p.gdir), src);
        const int32_t leaf = gather_leaf_of(S, gp);                            // the descent k_st_compact keys the queries of a pass with
        V3 caustic = v3(0, 0, 0);
        if (leaf >= 0) {
            const int32_t rank = S.pleaf_rank[leaf];
            if (rank >= 0) caustic = gather_wave(S, leaf, (uint32_t)rank, gp, gd, lane, nullptr);
        }
        if (lane / G == (uint32_t)src / G) gather_add(p.L, p.gcoef, caustic);   // stage_gather, on the path's own lanes
    }
}

// ---- function-level entries (parity tests, public C++ methods)
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
// gi_debug_find_leaves: the two descents gather_leaf_of is made of, side by side (fast: -2 where the quick one declines or has no tables)
__global__ void k_find_leaves(Scene S, int32_t n, const double* pos, int32_t* fast, int32_t* full)
{
    for (int32_t i = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x); i < n; i += (int32_t)(gridDim.x * blockDim.x)) {
        const V3 p = ld3(pos + (size_t)i * 3);
        fast[i] = gather_find_leaf_fast(S, p);
        full[i] = gather_find_leaf(S, p);
    }
}
