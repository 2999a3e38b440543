// gi_bake.inc -- light baking (gi_bake_*; an addition: everything else the project renders starts at the camera).  Included by gi_kernels.hip behind
// gi_entries.inc, whose Entry the two check entries use.  The definition is stated in include/gi_hip.h; the per-lane functions, bake_point(),
// bake_ray() and sh9_basis(), stand first with GI_BAKE_MODE_*, in namespace gi beside the functions of gi_device.h they call.

namespace gi {
// ------------------------------------------------------------------------------------------------ light baking (an addition: the reference starts every path at the camera)
// gi_hip.h: gi_bake_*.  A bake's ray: sample `stream` of a point takes Halton dimensions 0 and 1 at that index for its direction -- the two a
// primary ray takes for its place in the pixel -- and the rest of the index (dimensions 2 + 2d, 3 + 2d, the counter RNG) drives the path as a
// primary ray's would.  A texel's rays leave the surface in the lobe of the diffuse bounce (stage_shade: hemi_cos_n(norm, sx, sy, 2)) from the
// point lifted by the shadow bias; a probe's go anywhere on the sphere from the point itself.
#define GI_BAKE_MODE_TEXEL 0
#define GI_BAKE_MODE_SH9 1
struct BakePoint { V3 o, n; };          // where the point's rays start, and the unit normal (texel; 0 for a probe)
GI_HD BakePoint bake_point(int mode, const double* p)   // p: a row of `points`, [6] = position, normal (texel) or [3] = position (probe)
{
    BakePoint b;
    if (mode == GI_BAKE_MODE_TEXEL) {
        const V3 N = ld3(p + 3);
        b.n = N / sqrt((N.x * N.x + N.y * N.y) + N.z * N.z);
        b.o = ld3(p) + GI_SHADOW_BIAS * b.n;
    } else {
        b.n = v3(0, 0, 0);
        b.o = ld3(p);
    }
    return b;
}
GI_HD Ray bake_ray(const Scene& S, int mode, const BakePoint& b, uint32_t stream)
{
    const float u = halton_sample(S, 0, stream);
    const float v = halton_sample(S, 1, stream);
    return make_ray(b.o, mode == GI_BAKE_MODE_TEXEL ? hemi_cos_n(b.n, u, v, 2) : random_unit_vec((double)u, (double)v));
}
// the real spherical harmonics of bands 0 to 2 at the unit direction d, in the header's order and with its literals; IEEE operations only
GI_HD void sh9_basis(V3 d, double* Y)
{
    const double x = d.x, y = d.y, z = d.z;
    Y[0] = 0.28209479177387814;
    Y[1] = 0.4886025119029199 * y;
    Y[2] = 0.4886025119029199 * z;
    Y[3] = 0.4886025119029199 * x;
    Y[4] = 1.0925484305920792 * (x * y);
    Y[5] = 1.0925484305920792 * (y * z);
    Y[6] = 0.31539156525252005 * (3.0 * (z * z) - 1.0);
    Y[7] = 1.0925484305920792 * (x * z);
    Y[8] = 0.5462742152960396 * (x * x - y * y);
}
}  // namespace gi

// A bake is a second generator and a second fold around the stream passes (gi_stream.inc), as an adaptive round is k_ad_gen and k_ad_accum around
// them: k_bake_gen prepares the paths of a chunk of points and a range of samples in work.q_new, stream_passes runs them with a RoundRefill, and
// k_bake_fold adds what they left in lbuf to the points' sums.  No k_st_* kernel knows of it.  The generator is a template over where its rays
// come from (BakePoints here, the cube texels of gi_cubemap.inc), and bake_passes is the loop both share.
//
// Slots.  Sample k of point i of the chunk (both counted from the chunk's start) takes slot k * n_chunk_points + i -- the layout of the frame's
// sample id = s * n_pix + i: the lanes of a wave start neighbouring points of one k, and the fold's lanes (one per point) read lbuf side by side.
// Chunks.  The pool holds `slots` paths (bake_plan: gi_set_pool_slots and free memory, as plan_pool); a chunk is as many points as fit with one
// sample each, and the samples of a chunk run in ranges of as many k as fit.  The fold of a range continues the sums of the range before in
// ascending k (f64, [terms][points] of the chunk), so neither split can show in the result.
struct BakeGen {
    int32_t n_samples;
    uint32_t n_chunk_points, k_begin, k_count;
    uint32_t stream0;           // stream_base + (chunk's first point) * n_samples
};
// Where a generator's rays come from: at(i) is what point i of the chunk holds for all its samples, ray() the ray of one of them.  A bake reads a
// point list; a cube capture (gi_cubemap.inc: CubeTexels) numbers the texels of its cube.
struct BakePoints {
    const double* points;       // rows of the chunk's first point on
    int32_t mode;
    typedef BakePoint At;
    __device__ BakePoint at(uint32_t i) const { return bake_point(mode, points + (size_t)i * (mode == GI_BAKE_MODE_TEXEL ? 6 : 3)); }
    __device__ Ray ray(const Scene& S, const BakePoint& b, uint32_t stream) const { return bake_ray(S, mode, b, stream); }
};
template <class Src>
__global__ __launch_bounds__(GI_BLOCK) void k_bake_gen(Scene S, Src src, BakeGen g, PathPool pool, unsigned long long* slot_sample, double* dirs, uint32_t* q_new, unsigned int* n_new)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_round = (g.n_chunk_points + 63u) & ~63u;
    for (uint32_t i0 = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < n_round; i0 += gridDim.x * blockDim.x) {
        const uint32_t i = i0 + lane;
        const bool start = i < g.n_chunk_points;
        typename Src::At b{};
        if (start) b = src.at(i);
        for (uint32_t k = 0; k < g.k_count; k++) {          // wave-uniform trip count: the appends below are collective
            const uint32_t slot = k * g.n_chunk_points + i;
            if (start) {
                const uint32_t stream = g.stream0 + i * (uint32_t)g.n_samples + (g.k_begin + k);
                const Ray ray = src.ray(S, b, stream);
                pool_begin(pool, slot, ray, stream);
                slot_sample[slot] = slot;
                if (dirs) { double* d = dirs + (size_t)slot * 3; d[0] = ray.d.x; d[1] = ray.d.y; d[2] = ray.d.z; }   // what the path record holds: the fold reads it here
            }
            const uint32_t at = wave_append(n_new, start);
            if (start) q_new[at] = slot;
        }
    }
}

// the rays k_bake_gen makes, sample by sample (gi_bake_rays, gi_cubemap_rays): ray j = sample j % n_samples of point j / n_samples
template <class Src>
__global__ __launch_bounds__(GI_BLOCK) void k_bake_rays(Scene S, Src src, uint32_t n_rays, uint32_t n_samples, uint32_t stream_base, double* rays, uint32_t* streams)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_rays) return;
    const uint32_t stream = stream_base + j;
    const Ray r = src.ray(S, src.at(j / n_samples), stream);
    double* o = rays + (size_t)j * 6;
    o[0] = r.o.x; o[1] = r.o.y; o[2] = r.o.z; o[3] = r.d.x; o[4] = r.d.y; o[5] = r.d.z;
    streams[j] = stream;
}

// One lane per point of the chunk: samples k = 0 .. k_count-1 of the range in ascending order, no reduction across lanes, so the order of the
// additions is the header's whatever the launch.  sums [terms][n_chunk_points]: read unless this is the point's first range, written unless it is
// the last, which scales and stores out (the chunk's first row on).  27 f64 accumulators and 9 basis values per lane (MODE 1): 94 VGPRs, no scratch,
// five waves per SIMD at 256 lanes per workgroup (MODE 0: 20 VGPRs); no LDS.
template <int MODE>
__global__ __launch_bounds__(GI_BLOCK) void k_bake_fold(const double* lbuf, const double* dirs, uint32_t n_chunk_points, uint32_t k_count, double* sums, int first, int last,
                                                         double n_samples, void* out, int out_f64)
{
    constexpr int TERMS = MODE == GI_BAKE_MODE_SH9 ? 27 : 3;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_chunk_points) return;
    double acc[TERMS];
    GI_UNROLL
    for (int t = 0; t < TERMS; t++) acc[t] = first ? 0.0 : sums[(size_t)t * n_chunk_points + i];
    for (uint32_t k = 0; k < k_count; k++) {
        const size_t slot = (size_t)k * n_chunk_points + i;
        const double* l = lbuf + slot * 3;
        const double L[3] = {l[0], l[1], l[2]};
        if constexpr (MODE == GI_BAKE_MODE_SH9) {
            double Y[9];
            sh9_basis(ld3(dirs + slot * 3), Y);
            GI_UNROLL
            for (int j = 0; j < 9; j++) {
                GI_UNROLL
                for (int ch = 0; ch < 3; ch++) acc[j * 3 + ch] += L[ch] * Y[j];
            }
        } else {
            GI_UNROLL
            for (int ch = 0; ch < 3; ch++) acc[ch] += L[ch];
        }
    }
    if (!last) {
        GI_UNROLL
        for (int t = 0; t < TERMS; t++) sums[(size_t)t * n_chunk_points + i] = acc[t];
        return;
    }
    GI_UNROLL
    for (int t = 0; t < TERMS; t++) {
        const double v = MODE == GI_BAKE_MODE_SH9 ? (acc[t] * 12.566370614359172) / n_samples : acc[t] / n_samples;
        if (out_f64) ((double*)out)[(size_t)i * TERMS + t] = v;
        else ((float*)out)[(size_t)i * TERMS + t] = (float)v;
    }
}

namespace {

static_assert(GI_BAKE_TEXEL == GI_BAKE_MODE_TEXEL && GI_BAKE_SH9 == GI_BAKE_MODE_SH9, "the header's modes are the device functions'");
int bake_terms(int mode) { return mode == GI_BAKE_MODE_SH9 ? 27 : 3; }
int bake_row(int mode) { return mode == GI_BAKE_MODE_TEXEL ? 6 : 3; }

// false + message when parameters and point count are not the header's
bool bake_check(const gi_bake_params* p, int32_t n_points, std::string& err)
{
    if (!p) { err = "bake: null parameters"; return false; }
    if (p->mode != GI_BAKE_TEXEL && p->mode != GI_BAKE_SH9) { err = "bake: mode must be GI_BAKE_TEXEL (0) or GI_BAKE_SH9 (1), got " + std::to_string(p->mode); return false; }
    if (p->n_samples < 1) { err = "bake: n_samples must be at least 1, got " + std::to_string(p->n_samples); return false; }
    if (n_points < 0) { err = "bake: n_points must not be negative, got " + std::to_string(n_points); return false; }
    if ((unsigned long long)p->stream_base + (unsigned long long)n_points * (unsigned long long)p->n_samples > (1ull << 32)) {
        err = "bake: " + std::to_string(n_points) + " points of " + std::to_string(p->n_samples) + " samples from stream_base " + std::to_string(p->stream_base) + " take the stream index beyond 32 bits";
        return false;
    }
    return true;
}
// the host entries look at the points: every position finite, every normal finite and not 0 0 0
bool bake_points_ok(int mode, const double* points, int32_t n_points, std::string& err)
{
    const int row = bake_row(mode);
    for (int32_t i = 0; i < n_points; i++) {
        const double* p = points + (size_t)i * row;
        bool ok = true;
        for (int k = 0; k < row; k++) ok = ok && std::isfinite(p[k]);
        if (ok && mode == GI_BAKE_TEXEL) { const double n2 = (p[3] * p[3] + p[4] * p[4]) + p[5] * p[5]; ok = n2 > 0.0 && std::isfinite(n2); }
        if (!ok) { err = "bake: point " + std::to_string(i) + " has a non-finite position or a non-finite or zero normal"; return false; }
    }
    return true;
}

// How a bake of n_points x n_samples is cut: points per chunk, samples per range; their product is the pool.  budget: paths that may be in flight.
struct BakePlan { uint32_t chunk_points, range_k; };
BakePlan bake_plan(size_t budget, uint32_t n_points, uint32_t n_samples)
{
    BakePlan pl;
    budget = std::max<size_t>(budget, 1);
    pl.chunk_points = (uint32_t)std::min<size_t>(n_points, budget);
    pl.range_k = (uint32_t)std::max<size_t>(1, std::min<size_t>(n_samples, budget / pl.chunk_points));
    return pl;
}

// k_bake_fold of the mode over the np points of a chunk, one lane per point (the bake's ranges and gi_bake_fold's)
void launch_bake_fold(int mode, hipStream_t st, const double* lbuf, const double* dirs, uint32_t np, uint32_t nk, double* sums, int first, int last, double n_samples, void* out, int out_f64)
{
    const auto fold = mode == GI_BAKE_SH9 ? k_bake_fold<GI_BAKE_MODE_SH9> : k_bake_fold<GI_BAKE_MODE_TEXEL>;
    hipLaunchKernelGGL(fold, GI_GRID(np), 0, st, lbuf, dirs, np, nk, sums, first, last, n_samples, out, out_f64);
}

// the stream passes run on the frame's stage clock and, when asked, its work counters: a bake switches both off for its own passes and puts them back
struct BakeQuiet {
    gi_ctx* c;
    bool timing, counting;
    explicit BakeQuiet(gi_ctx* c_) : c(c_), timing(c_->clock.stage_timing), counting(c_->count_stream) { c->clock.stage_timing = false; c->count_stream = false; }
    ~BakeQuiet() { c->clock.stage_timing = timing; c->count_stream = counting; }
};

// What every pass that feeds the stream passes from a generator shares: n_points points of bp.n_samples samples cut into chunks and ranges, k_bake_gen
// on the chunk's source, the stream passes with a RoundRefill, the fold of bp.mode into d_out (on the device).  source(i0): the Src of the chunk
// whose first point is i0.  tm: the events around it.  Arguments checked.
template <class Source>
int bake_passes(gi_ctx* c, uint32_t n_points, const gi_bake_params& bp, Source source, void* d_out, int out_is_f64, EventTimer& tm)
{
    using Src = decltype(source(0u));
    HIP_TRY(c, hipSetDevice(c->device));
    const uint32_t n_samples = (uint32_t)bp.n_samples;
    const int n_shadow = defers_shadows(c) ? c->S.n_light : 0;
    // paths in flight: gi_set_pool_slots, and what 90 % of the free memory (plus what the context holds and would re-use) has room for -- per slot the
    // budget of plan_pool, its radiance (lbuf) and its direction
    size_t budget = std::min<size_t>(c->tune.pool_slots_max, 0xfffffff0ull);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
        const size_t held = c->st.held_bytes() + c->bake.d_dirs.n * 8;
        const size_t per_slot = kPoolRecordBytes + kBudgetWorkBytes + sizeof(ShadowQ) * (size_t)n_shadow + 24 + 24;
        budget = std::min(budget, std::max<size_t>(64, (size_t)((double)(free_b + held) * 0.90) / per_slot));
    }
    const BakePlan pl = bake_plan(budget, n_points, n_samples);
    const size_t slots = (size_t)pl.chunk_points * pl.range_k;
    const int terms = bake_terms(bp.mode);
    if (const int rc = stream_alloc(c, (uint32_t)slots, true)) return rc;   // k_bake_gen names every path's place in the radiance buffer
    if (c->st.d_lbuf.n < slots * 3) HIP_TRY(c, c->st.d_lbuf.alloc(slots * 3));
    if (bp.mode == GI_BAKE_SH9 && c->bake.d_dirs.n < slots * 3) HIP_TRY(c, c->bake.d_dirs.alloc(slots * 3));
    if (pl.range_k < n_samples && c->bake.d_sums.n < (size_t)terms * pl.chunk_points) HIP_TRY(c, c->bake.d_sums.alloc((size_t)terms * pl.chunk_points));
    if (!c->st.d_wfcnt.p) HIP_TRY(c, c->st.d_wfcnt.alloc(2));
    const bool debug_wf = debug_wf_on();
    if (debug_wf) fprintf(stderr, "[bake] %u points x %u samples: chunks of %u points, ranges of %u samples\n", n_points, n_samples, pl.chunk_points, pl.range_k);
    // the passes take the seed from a frame, and the size of the finisher's share from its extent: a frame of one row of this chunk's points
    Frame F;
    memset(&F, 0, sizeof F);
    F.seed = bp.seed; F.h = 1; F.local_rows = 1; F.stripe_h = 1; F.stripe_world = 1;
    BakeQuiet quiet(c);
    hipStream_t st = c->stream;
    double* const dirs = bp.mode == GI_BAKE_SH9 ? c->bake.d_dirs.p : nullptr;
    const size_t out_row = (size_t)terms * (out_is_f64 ? 8 : 4);
    int launches = 0;
    HIP_TRY(c, tm.begin(st));
    for (uint32_t i0 = 0; i0 < n_points; i0 += pl.chunk_points) {
        const uint32_t np = std::min(pl.chunk_points, n_points - i0);
        F.w = (int32_t)np;
        for (uint32_t k0 = 0; k0 < n_samples; k0 += pl.range_k) {
            const uint32_t nk = std::min(pl.range_k, n_samples - k0);
            F.min_samples = F.max_samples = (int32_t)nk;
            BakeGen g;
            g.n_samples = bp.n_samples;
            g.n_chunk_points = np; g.k_begin = k0; g.k_count = nk;
            g.stream0 = bp.stream_base + i0 * n_samples;
            HIP_TRY(c, hipMemsetAsync(c->st.d_wfcnt.p, 0, 2 * sizeof(unsigned int), st));
            hipLaunchKernelGGL(k_bake_gen<Src>, dim3(std::min<uint32_t>((np + GI_BLOCK - 1) / GI_BLOCK, (uint32_t)(4 * c->n_cu))), dim3(GI_BLOCK), 0, st, c->S, source(i0), g,
                               make_path_pool(c->st.d_spool.p, c->st.spool_slots), c->st.d_slot_sample.p, dirs, c->st.work.q_new.p, c->st.d_wfcnt.p);
            HIP_TRY(c, hipGetLastError());
            RoundRefill refill(F, np * nk);      // every sample of the range starts: the count needs no read-back
            if (const int rc = stream_passes(c, F, c->st.d_slot_sample.p, 0ull, c->st.d_lbuf.p, 0u, refill, debug_wf, nullptr, launches)) { tm.reset(); return rc; }
            const int first = k0 == 0, last = k0 + nk == n_samples;
            void* const out = (char*)d_out + (size_t)i0 * out_row;
            launch_bake_fold(bp.mode, st, c->st.d_lbuf.p, dirs, np, nk, c->bake.d_sums.p, first, last, (double)bp.n_samples, out, out_is_f64);
            HIP_TRY(c, hipGetLastError());
        }
    }
    HIP_TRY(c, tm.end(st));
    return GI_OK;
}

// the bake itself: d_points and d_out on the device, arguments checked.  timer: the events around it -- the bake's own, or those of a pass that
// bakes as one of its stages (gi_lightmap.inc) and leaves gi_last_bake_ms alone
int bake_run(gi_ctx* c, const double* d_points, uint32_t n_points, const gi_bake_params& bp, void* d_out, int out_is_f64, EventTimer* timer = nullptr)
{
    const auto rows = [&](uint32_t i0) { BakePoints s; s.points = d_points + (size_t)i0 * bake_row(bp.mode); s.mode = bp.mode; return s; };
    return bake_passes(c, n_points, bp, rows, d_out, out_is_f64, timer ? *timer : c->bake.timer);
}

}  // namespace

extern "C" {

void gi_bake_default_params(gi_bake_params* p)
{
    if (!p) return;
    p->mode = GI_BAKE_SH9; p->n_samples = 256;
    p->stream_base = 0u;
    p->seed = 0x9E3779B97F4A7C15ull;
}

int gi_bake_device(gi_ctx* c, const double* d_points, int32_t n_points, const gi_bake_params* bp, void* d_out, int out_is_f64)
{
    if (!c) return GI_E_INVALID;
    c->bake.timer.reset();
    std::string err;
    if (!bake_check(bp, n_points, err)) return fail(c, GI_E_INVALID, err);
    if (n_points && (!d_points || !d_out)) return fail(c, GI_E_INVALID, "bake: null points or output pointer");
    if (!c->scene.have_scene) return fail(c, GI_E_STATE, "bake: no scene uploaded");
    if (n_points == 0) return GI_OK;
    return bake_run(c, d_points, (uint32_t)n_points, *bp, d_out, out_is_f64);
}

int gi_bake_host(gi_ctx* c, const double* points, int32_t n_points, const gi_bake_params* bp, void* h_out, int out_is_f64)
{
    if (!c) return GI_E_INVALID;
    c->bake.timer.reset();
    std::string err;
    if (!bake_check(bp, n_points, err)) return fail(c, GI_E_INVALID, err);
    if (n_points && (!points || !h_out)) return fail(c, GI_E_INVALID, "bake: null points or output pointer");
    if (!bake_points_ok(bp->mode, points, n_points, err)) return fail(c, GI_E_INVALID, err);
    if (!c->scene.have_scene) return fail(c, GI_E_STATE, "bake: no scene uploaded");
    if (n_points == 0) return GI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t N = (size_t)n_points, bytes = N * bake_terms(bp->mode) * (out_is_f64 ? 8 : 4);
    DevBuf<double> d_points;
    DevBuf<unsigned char> d_out;
    HIP_TRY(c, d_points.upload(points, N * bake_row(bp->mode)));
    HIP_TRY(c, d_out.alloc(bytes));
    const int rc = bake_run(c, d_points.p, (uint32_t)n_points, *bp, d_out.p, out_is_f64);
    return rc != GI_OK ? rc : finish_to_host(c, "bake_host", {{h_out, d_out.p, bytes}}, &c->bake.timer);
}

int gi_last_bake_ms(gi_ctx* c, float* ms) { return pass_ms(c, &gi_ctx::bake, ms); }

int gi_bake_rays(gi_ctx* c, const double* points, int32_t n_points, const gi_bake_params* bp, double* rays6_out, uint32_t* stream_out)
{
    if (!c) return GI_E_INVALID;
    std::string err;
    if (!bake_check(bp, n_points, err)) return fail(c, GI_E_INVALID, err);
    if (n_points && (!points || !rays6_out || !stream_out)) return fail(c, GI_E_INVALID, "bake_rays: null points or output pointer");
    if (!bake_points_ok(bp->mode, points, n_points, err)) return fail(c, GI_E_INVALID, err);
    const size_t n_rays = (size_t)n_points * (size_t)bp->n_samples;
    if (n_rays > 0x7fffffffull) return fail(c, GI_E_INVALID, "bake_rays: more than 2^31 - 1 rays");
    if (n_rays == 0) return GI_OK;
    Entry e(c, "bake_rays");
    const double* d_p = e.in(points, (size_t)n_points * bake_row(bp->mode));
    double* d_r = e.out(rays6_out, n_rays * 6);
    uint32_t* d_s = e.out(stream_out, n_rays);
    BakePoints src;
    src.points = d_p; src.mode = bp->mode;
    return e.run([&] { hipLaunchKernelGGL(k_bake_rays<BakePoints>, GI_GRID(n_rays), 0, c->stream, c->S, src, (uint32_t)n_rays, (uint32_t)bp->n_samples, bp->stream_base, d_r, d_s); });
}

int gi_bake_fold(gi_ctx* c, int32_t mode, int32_t n_points, int32_t n_samples, const double* dirs3, const double* L3, double* out)
{
    if (!c) return GI_E_INVALID;
    if ((mode != GI_BAKE_TEXEL && mode != GI_BAKE_SH9) || n_points < 0 || n_samples < 1) return fail(c, GI_E_INVALID, "bake_fold: mode 0 or 1, n_points >= 0, n_samples >= 1");
    if (n_points && (!L3 || !out || (mode == GI_BAKE_SH9 && !dirs3))) return fail(c, GI_E_INVALID, "bake_fold: null pointer");
    if (n_points == 0) return GI_OK;
    // the caller's [point][sample] rows in the bake's slot order, k * n_points + i, in ranges of at most 16 samples: the sums go through memory
    // between ranges as they do in a bake whose samples do not fit the pool
    const uint32_t np = (uint32_t)n_points, ns = (uint32_t)n_samples, range = 16;
    const size_t n = (size_t)np * ns;
    const int terms = bake_terms(mode);
    std::vector<double> hl(n * 3), hd(mode == GI_BAKE_SH9 ? n * 3 : 0);
    for (uint32_t i = 0; i < np; i++)
        for (uint32_t k = 0; k < ns; k++)
            for (int x = 0; x < 3; x++) {
                hl[((size_t)k * np + i) * 3 + x] = L3[((size_t)i * ns + k) * 3 + x];
                if (mode == GI_BAKE_SH9) hd[((size_t)k * np + i) * 3 + x] = dirs3[((size_t)i * ns + k) * 3 + x];
            }
    Entry e(c, "bake_fold");
    const double* d_l = e.in(hl.data(), n * 3);
    const double* d_d = mode == GI_BAKE_SH9 ? e.in(hd.data(), n * 3) : nullptr;
    double* d_sums = e.scratch<double>((size_t)terms * np);
    double* d_o = e.out(out, (size_t)np * terms);
    return e.run([&] {
        for (uint32_t k0 = 0; k0 < ns; k0 += range) {
            const uint32_t nk = std::min(range, ns - k0);
            const int first = k0 == 0, last = k0 + nk == ns;
            const double* l = d_l + (size_t)k0 * np * 3;
            const double* d = d_d ? d_d + (size_t)k0 * np * 3 : nullptr;
            launch_bake_fold(mode, c->stream, l, d, np, nk, d_sums, first, last, (double)n_samples, (void*)d_o, 1);
        }
    });
}

}  // extern "C"
