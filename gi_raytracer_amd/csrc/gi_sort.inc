// gi_sort.inc -- the pipeline's own radix sort of (32-bit key, 32-bit value) pairs (included by gi_kernels.hip).
//
// What is sorted: the gather queries of a pass by the rank of their photon-map leaf (<= 17 bits) and the continuing rays by their 27-bit coherence
// key -- up to 531 M pairs each on the benchmark frame.  A least-significant-digit radix sort with digits of up to 9 bits (27 bits = three passes,
// 15 bits = two), every pass stable.  Laid out for one MI355X: a pass is three launches over a PERSISTENT grid of one 1 024-thread workgroup per CU,
// every workgroup owning one contiguous chunk of the input --
//   k_rs_hist     the chunk's digit histogram (512 counters in LDS), written bin-major: 256 x 512 counters per pass instead of one row per tile;
//   k_rs_scan     one workgroup: exclusive prefix sums over the 131 072 (bin, workgroup) counters = where every workgroup's share of a bin starts;
//   k_rs_scatter  the chunk again, 8 192 pairs (64 KB of LDS) at a time: every wave ranks its 512 consecutive elements by digit with ballots (no
//                 atomics: the rank of an element among the equal digits before it is a popcount), the tile is staged in LDS in digit order and
//                 written out as runs of consecutive addresses per digit (16 pairs = 128 bytes on average), the workgroup's bin cursors move on.
// Traffic per pass: 4 bytes per pair for the histogram, 8 read + 8 written for the scatter.
// Measured (round 3, MI355X, benchmark frame, all sorts of a frame): 17.1 ms against 22.0 ms with rocPRIM's one-sweep sort behind
// hipcub::DeviceRadixSort, which rounds 1 and 2 used (the frames are the same either way -- the order of a queue is a schedule, not arithmetic):
// three 9-bit passes instead of four 8-bit ones for the 27-bit key, the next tile's 16 loads in flight while a tile is ranked (k_rs_scatter moves
// its 16 bytes per pair at 2.9 TB/s, k_rs_hist -- 16-byte loads, one LDS atomic per run of equal digits -- its 4 at 2.2).  First version, without
// the prefetch, with one LDS atomic per key and a strided scan: 25.7 ms.  The teapot frame 118 against 151 ms; frames of many small passes (the
// closed box: 22 sorts of 16 M pairs and fewer) 6.0 against 5.1 ms -- three launches per digit pass have a floor of ~60 us.
#define GI_RS_BLOCK 1024
#define GI_RS_ITEMS 8                                   // per thread and tile
#define GI_RS_TILE (GI_RS_BLOCK * GI_RS_ITEMS)          // 8 192 pairs
#define GI_RS_MAXBINS 512
#define GI_RS_LDS_BYTES (GI_RS_TILE * 8 + 16 * GI_RS_MAXBINS * 4 + 3 * GI_RS_MAXBINS * 4)

// the chunk of workgroup b: whole tiles, the last workgroups may get none
__device__ __forceinline__ void rs_chunk(uint32_t n, uint32_t& begin, uint32_t& end)
{
    const uint32_t tiles = (n + GI_RS_TILE - 1) / GI_RS_TILE, per = (tiles + gridDim.x - 1) / gridDim.x;
    const unsigned long long b0 = (unsigned long long)blockIdx.x * per * GI_RS_TILE, e0 = b0 + (unsigned long long)per * GI_RS_TILE;
    begin = (uint32_t)(b0 < n ? b0 : n);
    end = (uint32_t)(e0 < n ? e0 : n);
}

// the lanes of the wave that hold the same digit as this one (valid lanes only)
__device__ __forceinline__ unsigned long long rs_same_digit(uint32_t d, int bits, bool valid)
{
    unsigned long long same = __ballot(valid);
    for (int b = 0; b < bits; b++) {
        const bool bit = (d >> b) & 1u;
        const unsigned long long bal = __ballot(bit);
        same &= bit ? bal : ~bal;
    }
    return same;
}

__global__ __launch_bounds__(GI_RS_BLOCK) void k_rs_hist(const uint32_t* keys, const uint32_t* n_dev, uint32_t n_host, int shift, int bits, uint32_t* ghist)
{
    __shared__ unsigned int hist[GI_RS_MAXBINS];
    const uint32_t n = n_dev ? *n_dev : n_host, nb = 1u << bits, mask = nb - 1u;
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (uint32_t i = threadIdx.x; i < nb; i += blockDim.x) hist[i] = 0u;
    __syncthreads();
    uint32_t begin, end;
    rs_chunk(n, begin, end);
    // neighbouring keys are often equal (queries of one photon-map leaf, rays of one cell): a lane adds the length of the run of equal digits that
    // starts at it (runs inside its own four keys first, then across the lanes of the wave), not one per key; 16 keys (four 16-byte loads) in flight
    // per lane.  chunks start at multiples of the tile size, so the 16-byte loads are aligned.
    const uint4* const k4 = reinterpret_cast<const uint4*>(keys);
    for (uint32_t w0 = begin + (threadIdx.x & ~63u) * 4u; w0 < end; w0 += blockDim.x * 16u) {      // (wave-uniform trip count: the ballots below see every lane)
        const uint32_t i0 = w0 + lane * 4u;
        uint4 q[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const uint32_t i = i0 + (uint32_t)r * blockDim.x * 4u;
            if (i + 3u < end) q[r] = k4[i >> 2];
            else { q[r].x = i < end ? keys[i] : 0u; q[r].y = i + 1u < end ? keys[i + 1u] : 0u; q[r].z = i + 2u < end ? keys[i + 2u] : 0u; q[r].w = 0u; }
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const uint32_t i = i0 + (uint32_t)r * blockDim.x * 4u;
            const uint32_t kk[4] = {q[r].x, q[r].y, q[r].z, q[r].w};
            uint32_t run_d = 0, run_n = 0;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                if (i + (uint32_t)e >= end) break;
                const uint32_t d = (kk[e] >> shift) & mask;
                if (run_n && d == run_d) run_n++;
                else { if (run_n) atomicAdd(&hist[run_d], run_n); run_d = d; run_n = 1u; }
            }
            // the lane's last run may go on in the next lanes' first keys only when they hold nothing else: merge whole-lane runs
            const bool whole = run_n == 4u && ((kk[0] >> shift) & mask) == run_d;
            const uint32_t prev_d = (uint32_t)__shfl_up((int)run_d, 1);
            const bool prev_whole = (bool)__shfl_up((int)whole, 1) && lane != 0u;
            const bool head = !(whole && prev_whole && prev_d == run_d);                 // a lane whose four keys continue the previous lane's whole-lane run is not a head
            const unsigned long long heads = __ballot(head || !whole);
            if (run_n) {
                if (whole && head) {
                    // count the whole lanes that follow with the same digit
                    const unsigned long long stop = heads >> (lane + 1u);
                    const uint32_t follow = lane == 63u ? 0u : (stop ? (uint32_t)__builtin_ctzll(stop) : 63u - lane);
                    atomicAdd(&hist[run_d], 4u * (1u + follow));
                } else if (!whole) atomicAdd(&hist[run_d], run_n);
            }
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < nb; i += blockDim.x) ghist[(size_t)i * gridDim.x + blockIdx.x] = hist[i];
}

// exclusive prefix sums over ghist[bin][workgroup] in that order (one workgroup; any total -- the sort's is at most 512 x 2 048 counters, the
// lightmap's rank passes one count per 256 texels, up to 262 145), 8 192 counters at a time through LDS so that the global reads and writes are coalesced
__global__ __launch_bounds__(1024) void k_rs_scan(uint32_t* ghist, uint32_t total)
{
    __shared__ uint32_t buf[8192];
    __shared__ uint32_t part[1024];
    __shared__ uint32_t carry;
    if (threadIdx.x == 0) carry = 0u;
    __syncthreads();
    for (uint32_t c0 = 0; c0 < total; c0 += 8192u) {
        for (uint32_t i = threadIdx.x; i < 8192u; i += 1024u) buf[i] = c0 + i < total ? ghist[c0 + i] : 0u;
        __syncthreads();
        uint32_t acc = 0;
        for (uint32_t k = 0; k < 8u; k++) acc += buf[threadIdx.x * 8u + k];
        part[threadIdx.x] = acc;
        __syncthreads();
        for (uint32_t o = 1; o < 1024u; o <<= 1) {
            const uint32_t v = threadIdx.x >= o ? part[threadIdx.x - o] : 0u;
            __syncthreads();
            part[threadIdx.x] += v;
            __syncthreads();
        }
        uint32_t run = carry + part[threadIdx.x] - acc;     // exclusive
        for (uint32_t k = 0; k < 8u; k++) { const uint32_t v = buf[threadIdx.x * 8u + k]; buf[threadIdx.x * 8u + k] = run; run += v; }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < 8192u; i += 1024u) if (c0 + i < total) ghist[c0 + i] = buf[i];
        if (threadIdx.x == 1023u) carry = run;
        __syncthreads();
    }
}

__global__ __launch_bounds__(GI_RS_BLOCK) void k_rs_scatter(const uint32_t* keys_in, const uint32_t* vals_in, uint32_t* keys_out, uint32_t* vals_out,
                                                            const uint32_t* n_dev, uint32_t n_host, int shift, int bits, const uint32_t* gbase_all)
{
    uint32_t* const stage_k = reinterpret_cast<uint32_t*>(gi_dyn_lds);                     // [8192]
    uint32_t* const stage_v = stage_k + GI_RS_TILE;                                        // [8192]
    uint32_t* const wavecnt = stage_v + GI_RS_TILE;                                        // [16 waves][512]: per wave, elements of a digit so far in the tile
    uint32_t* const tile_first = wavecnt + 16 * GI_RS_MAXBINS;                             // [512] first staged position of a digit in this tile
    uint32_t* const tile_cnt = tile_first + GI_RS_MAXBINS;                                 // [512]
    uint32_t* const gbase = tile_cnt + GI_RS_MAXBINS;                                      // [512] where this workgroup's next element of a digit goes
    __shared__ uint32_t wsum[8];
    const uint32_t n = n_dev ? *n_dev : n_host, nb = 1u << bits, mask = nb - 1u;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (uint32_t i = threadIdx.x; i < nb; i += blockDim.x) gbase[i] = gbase_all[(size_t)i * gridDim.x + blockIdx.x];
    uint32_t begin, end;
    rs_chunk(n, begin, end);
    // wave w owns elements [t0 + 512 w, t0 + 512 w + 512) of a tile, 64 at a time, in order; the next tile's are requested while this one is ranked
    uint32_t key[GI_RS_ITEMS], val[GI_RS_ITEMS], nkey[GI_RS_ITEMS], nval[GI_RS_ITEMS];
    auto load_tile = [&](uint32_t t0, uint32_t (&k)[GI_RS_ITEMS], uint32_t (&v)[GI_RS_ITEMS]) {
#pragma unroll
        for (int r = 0; r < GI_RS_ITEMS; r++) {
            const uint32_t e = t0 + wave * (64u * GI_RS_ITEMS) + (uint32_t)r * 64u + lane;
            k[r] = e < end ? keys_in[e] : 0u;
            v[r] = e < end ? vals_in[e] : 0u;
        }
    };
    if (begin < end) load_tile(begin, key, val);
    uint4* const wz = reinterpret_cast<uint4*>(wavecnt);
    for (uint32_t t0 = begin; t0 < end; t0 += GI_RS_TILE) {
        for (uint32_t i = threadIdx.x; i < 16u * GI_RS_MAXBINS / 4u; i += blockDim.x) wz[i] = make_uint4(0u, 0u, 0u, 0u);
        if (t0 + GI_RS_TILE < end) load_tile(t0 + GI_RS_TILE, nkey, nval);
        __syncthreads();
        // ---- rank
        uint32_t dr[GI_RS_ITEMS];      // digit | rank within the wave's segment << 16 | valid << 31
        uint32_t* const mycnt = wavecnt + wave * GI_RS_MAXBINS;
#pragma unroll
        for (int r = 0; r < GI_RS_ITEMS; r++) {
            const uint32_t e = t0 + wave * (64u * GI_RS_ITEMS) + (uint32_t)r * 64u + lane;
            const bool valid = e < end;
            const uint32_t d = (key[r] >> shift) & mask;
            const unsigned long long same = rs_same_digit(d, bits, valid);
            const uint32_t before = valid ? mycnt[d] : 0u;                  // (every lane of a digit group reads the same counter before its leader moves it)
            const uint32_t rank = before + (uint32_t)__popcll(same & lt);
            __builtin_amdgcn_wave_barrier();
            if (valid && (same & lt) == 0ull) mycnt[d] = before + (uint32_t)__popcll(same);   // the group's first lane: one writer per counter
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            dr[r] = d | (rank << 16) | (valid ? 0x80000000u : 0u);
        }
        __syncthreads();
        // ---- per digit: where each wave's elements start inside the digit's run, the digit's count in the tile, and its first staged position
        // (exclusive prefix sums over the <= 512 counts: a wave scan per 64 digits, the waves' totals through LDS)
        uint32_t cnt_d = 0, incl = 0;
        if (threadIdx.x < nb) {
            uint32_t acc = 0;
            for (uint32_t w = 0; w < 16u; w++) { const uint32_t v = wavecnt[w * GI_RS_MAXBINS + threadIdx.x]; wavecnt[w * GI_RS_MAXBINS + threadIdx.x] = acc; acc += v; }
            cnt_d = acc;
        }
        if (wave < 8u) {
            incl = cnt_d;
            for (uint32_t o = 1; o < 64u; o <<= 1) { const uint32_t v = (uint32_t)__shfl_up((int)incl, o); if (lane >= o) incl += v; }
            if (lane == 63u) wsum[wave] = incl;
        }
        __syncthreads();
        if (threadIdx.x < nb) {
            uint32_t off = 0;
            for (uint32_t w = 0; w < wave; w++) off += wsum[w];
            tile_cnt[threadIdx.x] = cnt_d;
            tile_first[threadIdx.x] = off + incl - cnt_d;
        }
        __syncthreads();
        // ---- stage in digit order
#pragma unroll
        for (int r = 0; r < GI_RS_ITEMS; r++) {
            if (dr[r] & 0x80000000u) {
                const uint32_t d = dr[r] & 0xffffu, rank = (dr[r] >> 16) & 0x7fffu;
                const uint32_t pos = tile_first[d] + wavecnt[wave * GI_RS_MAXBINS + d] + rank;
                stage_k[pos] = key[r];
                stage_v[pos] = val[r];
            }
        }
        __syncthreads();
        // ---- write out: consecutive staged elements of a digit go to consecutive addresses
        const uint32_t n_tile = end - t0 < GI_RS_TILE ? end - t0 : GI_RS_TILE;
        for (uint32_t j = threadIdx.x; j < n_tile; j += blockDim.x) {
            const uint32_t k = stage_k[j], d = (k >> shift) & mask;
            const uint32_t at = gbase[d] + (j - tile_first[d]);
            keys_out[at] = k;
            vals_out[at] = stage_v[j];
        }
        __syncthreads();
        if (threadIdx.x < nb) gbase[threadIdx.x] += tile_cnt[threadIdx.x];
#pragma unroll
        for (int r = 0; r < GI_RS_ITEMS; r++) { key[r] = nkey[r]; val[r] = nval[r]; }
        // (the barrier at the top of the next tile orders the cursors' update before their next use)
    }
}

// Sort n pairs by bits [begin_bit, end_bit) of the key, stable.  keys_in / vals_in are left as they are; the result is in keys_out / vals_out;
// tmp_keys / tmp_vals hold n entries each.  n_dev (optional) = the count in device memory: n is then only the bound the grid is sized for.
static int rs_sort_pairs(gi_ctx* c, const uint32_t* keys_in, uint32_t* keys_out, const uint32_t* vals_in, uint32_t* vals_out, uint32_t* tmp_keys, uint32_t* tmp_vals,
                         uint32_t n, const uint32_t* n_dev, int begin_bit, int end_bit, uint32_t* ghist)
{
    hipStream_t st = c->stream;
    const int total_bits = std::max(end_bit - begin_bit, 1);
    const int passes = (total_bits + 8) / 9;
    // one workgroup per CU, fewer when the input has fewer tiles than that (the last passes of a frame sort a few thousand pairs)
    const int grid = (int)std::max<uint32_t>(1u, std::min<uint32_t>((uint32_t)std::min(c->n_cu, GI_MAX_PRODUCER_BLOCKS), (n + GI_RS_TILE - 1) / GI_RS_TILE));
    if (!c->st.rs_attr_set) { HIP_TRY(c, hipFuncSetAttribute((const void*)k_rs_scatter, hipFuncAttributeMaxDynamicSharedMemorySize, (int)GI_RS_LDS_BYTES)); c->st.rs_attr_set = true; }
    const uint32_t* src_k = keys_in;
    const uint32_t* src_v = vals_in;
    int shift = begin_bit;
    for (int p = 0; p < passes; p++) {
        const int bits = (total_bits - (shift - begin_bit) + (passes - p) - 1) / (passes - p);      // the remaining bits spread evenly: 27 = 9 + 9 + 9, 15 = 8 + 7
        // ping-pong so that the last pass lands in the caller's output: passes - p odd -> out, even -> tmp
        uint32_t* dst_k = ((passes - p) & 1) ? keys_out : tmp_keys;
        uint32_t* dst_v = ((passes - p) & 1) ? vals_out : tmp_vals;
        hipLaunchKernelGGL(k_rs_hist, dim3(grid), dim3(GI_RS_BLOCK), 0, st, src_k, n_dev, n, shift, bits, ghist);
        hipLaunchKernelGGL(k_rs_scan, dim3(1), dim3(1024), 0, st, ghist, (uint32_t)((1u << bits) * grid));
        hipLaunchKernelGGL(k_rs_scatter, dim3(grid), dim3(GI_RS_BLOCK), GI_RS_LDS_BYTES, st, src_k, src_v, dst_k, dst_v, n_dev, n, shift, bits, ghist);
        src_k = dst_k; src_v = dst_v;
        shift += bits;
    }
    HIP_TRY(c, hipGetLastError());
    return GI_OK;
}
