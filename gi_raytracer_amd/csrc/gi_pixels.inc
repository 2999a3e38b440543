// gi_pixels.inc -- everything that reads or writes the per-pixel records: PixRec and its conversions, the two record orders (tile_pixel_xy,
// st_pixel_xy), the megakernel k_render, and the kernels that start (k_pix_init, k_ad_gen, k_pixel_table), fold (k_ad_accum, k_st_accum) and read
// out (k_pix_resolve, k_pix_wanting) a frame's records.  Kernels only: the schedules that launch them are in gi_stream.inc, gi_api.inc and
// gi_progressive.inc, behind the context.  Needs gi_device.h (PixelState, Frame, primary_ray, radiance_path) and gi_pool.h (k_ad_gen starts
// paths in the pool); included by gi_kernels.hip.

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

// The trace stage starts new samples itself (gi_stages.inc: GenArgs).  What a new path of pixel p needs before its ray can be made -- the pixel's place in the frame (st_pixel_xy: four divisions by run-time numbers) and
// the Halton index of its first sample (halton_index: a 64-bit remainder) -- is the same for all the samples of the pixel: one table per frame instead
// of ~300 instructions per primary ray.
__global__ void k_pixel_table(Frame F, uint32_t n_pix, uint32_t* out)
{
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n_pix; p += gridDim.x * blockDim.x) {
        int x, ly;
        st_pixel_xy(F, p, x, ly);
        const int y = global_row(F, ly);
        out[p] = halton_index(F.he, 0u, (uint32_t)x, (uint32_t)y);
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
