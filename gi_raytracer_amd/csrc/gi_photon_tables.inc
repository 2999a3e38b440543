// gi_photon_tables.inc -- the kernels that derive the gather's tables from an uploaded photon map: leaf ranks, candidate lists, the descent
// records and the jump table.  Kernels only: their launches are the steps of install_photon_map (gi_context.inc: build_photon_*), which the upload
// and the device build both end with, so the kernels stand ahead of gi_context.inc and not in gi_photon_build.inc behind it.  Needs gi_device.h (PNode, PRange, PDescent); included by gi_kernels.hip.

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
