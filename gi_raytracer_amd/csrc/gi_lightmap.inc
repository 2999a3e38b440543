// gi_lightmap.inc -- lightmap atlases (gi_lightmap_*; an addition around the bake of gi_bake.inc).  Included by gi_kernels.hip behind gi_bake.inc, whose
// bake_run is the middle stage.  The definition is stated in include/gi_hip.h; the per-lane functions, lm_edge(), lm_covers(), lm_point() and their
// kin, stand first, in namespace gi beside the types of gi_device.h they use.

namespace gi {
// ------------------------------------------------------------------------------------------------ lightmap atlases (an addition, around the bake)
// gi_hip.h: gi_lightmap_*.  A chart row maps a triangle entity to three chart coordinates; a texel whose centre the row covers takes its point from
// the entity at the centre's barycentrics.  IEEE + - * / only, in the header's order, so that with -ffp-contract=off the texel table equals the
// tests' numpy statement bit for bit.  uv: a row of the chart, [3][2] = the coordinates of the entity's vertices 0, 1, 2.
GI_HD double lm_edge(double ax, double ay, double bx, double by, double px, double py) { return (bx - ax) * (py - ay) - (by - ay) * (px - ax); }
GI_HD bool lm_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }
struct LmEdges { double area, e0, e1, e2; };
GI_HD double lm_area(const double* uv) { return lm_edge(uv[0], uv[1], uv[2], uv[3], uv[4], uv[5]); }
GI_HD LmEdges lm_edges(const double* uv, double pu, double pv)
{
    LmEdges e;
    e.area = lm_area(uv);
    e.e0 = lm_edge(uv[2], uv[3], uv[4], uv[5], pu, pv);
    e.e1 = lm_edge(uv[4], uv[5], uv[0], uv[1], pu, pv);
    e.e2 = lm_edge(uv[0], uv[1], uv[2], uv[3], pu, pv);
    return e;
}
// the row's chart box: the smallest and largest of its three coordinates, per axis (plain comparisons)
struct LmBox { double ulo, uhi, vlo, vhi; };
GI_HD double lm_min3(double a, double b, double c) { const double m = b < a ? b : a; return c < m ? c : m; }
GI_HD double lm_max3(double a, double b, double c) { const double m = b > a ? b : a; return c > m ? c : m; }
GI_HD LmBox lm_box(const double* uv)
{
    LmBox b;
    b.ulo = lm_min3(uv[0], uv[2], uv[4]); b.uhi = lm_max3(uv[0], uv[2], uv[4]);
    b.vlo = lm_min3(uv[1], uv[3], uv[5]); b.vhi = lm_max3(uv[1], uv[3], uv[5]);
    return b;
}
// A row covers the centre iff the centre lies in the row's chart box (inclusive) AND the edge test passes: edges inclusive, either winding; a row of
// area 0 or of a non-finite area covers nothing (a NaN edge value fails every comparison).  The box is part of the definition: where the three
// vertices are collinear up to rounding, the edge values round to 0 or to the area's sign all along the line extended, and the box ends the row.
GI_HD bool lm_covers(const LmBox& b, const LmEdges& e, double pu, double pv)
{
    if (!lm_finite(e.area) || e.area == 0.0) return false;
    if (!(pu >= b.ulo && pu <= b.uhi && pv >= b.vlo && pv <= b.vhi)) return false;
    return e.area > 0.0 ? (e.e0 >= 0.0 && e.e1 >= 0.0 && e.e2 >= 0.0) : (e.e0 <= 0.0 && e.e1 <= 0.0 && e.e2 <= 0.0);
}
GI_HD double lm_centre(int32_t i, int32_t n) { return ((double)i + 0.5) / (double)n; }
// the texel's point on the entity and its normal (shading_normal's expression for a triangle); ok: the normal is finite and not 0 0 0
struct LmPoint { V3 P, N; bool ok; };
GI_HD LmPoint lm_point(const TriGeom& g, const TriShade& sh, const LmEdges& e, int flip)
{
    LmPoint q;
    const double b1 = e.e1 / e.area, b2 = e.e2 / e.area;
    q.P = (ld3(g.p0) + b1 * ld3(g.e1)) + b2 * ld3(g.e2);
    q.N = (g.flags & 1u) ? ((1 - b1 - b2) * ld3(sh.n0) + b1 * ld3(sh.n1)) + b2 * ld3(sh.n2) : ld3(sh.fnorm);
    if (flip) q.N = v3(-q.N.x, -q.N.y, -q.N.z);
    q.ok = lm_finite(q.N.x) && lm_finite(q.N.y) && lm_finite(q.N.z) && !(q.N.x == 0.0 && q.N.y == 0.0 && q.N.z == 0.0);
    return q;
}
}  // namespace gi

// One call is three stages on the context's stream, T = width x height texels:
//   raster + rank    k_lm_raster decides every texel's owner row, k_lm_point makes the owned texels' points and counts the valid ones per workgroup,
//                    k_rs_scan (gi_sort.inc) turns the counts into offsets, k_lm_compact writes the texel table in ascending texel order.  One 4-byte
//                    read-back (n_covered) sizes the bake.
//   bake             bake_run on the table, GI_BAKE_TEXEL, with the lightmap's timer: gi_last_bake_ms keeps its value.
//   scatter + dilate k_lm_scatter puts the rows back by rank, k_lm_dilate ping-pongs `dilate` times, k_lm_store rounds once into the caller's atlas.
//
// k_lm_raster: a WAVE per chart row, the lanes striding over the texels of the row's chart box, and gridDim.y waves sharing a box (wave s takes the
// box texels s * 64 + lane, then gridDim.y * 64 further on).  Chart triangles differ in area by orders of magnitude: a lane per row would leave one
// lane with a quarter of the atlas; the other way, flattening (row, box texel) pairs by a prefix sum over the box areas, loads lanes evenly but costs
// a scan, a binary search per lane and a read-back or a second launch -- more than the rasteriser itself on the charts a lightmap has (thousands of
// rows, boxes of tens to thousands of texels).  A wave that finds nothing left of a small box ends after reading 48 bytes.  The range of texels a
// row tests is only a short cut: the chart box is part of the coverage test itself (lm_covers), so the owners are the definition's whatever the
// range, and the definition does not depend on the size of the coordinates.  Owners are decided by a
// 32-bit atomicMin of the row index on a table that starts at 0x7fffffff: the minimum does not depend on the order of the atomics.
// Resource usage (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): DESIGN.md section 4 quotes it; no scratch, no LDS.
#define GI_LM_NONE 0x7fffffff
#define GI_LM_BOX_EXACT 1048576.0   // chart coordinates up to this size: the range of texels k_lm_raster tests is computed; beyond it, the whole atlas

__global__ __launch_bounds__(GI_BLOCK) void k_lm_raster(int32_t n_chart, const double* uv, int32_t w, int32_t h, int* own)
{
    const uint32_t lane = threadIdx.x & 63u, wpb = blockDim.x >> 6;
    const double W = (double)w, H = (double)h;
    for (uint32_t j = blockIdx.x * wpb + (threadIdx.x >> 6); j < (uint32_t)n_chart; j += gridDim.x * wpb) {
        const double* t = uv + (size_t)j * 6;
        const double area = lm_area(t);
        if (!lm_finite(area) || area == 0.0) continue;
        // The texels to test: those whose centres can lie in the row's chart box (lm_covers asks that of every centre, so this range only saves
        // work).  x0 = floor(ulo W - 0.5) - 1: a centre with (x + 0.5) / W >= ulo has x >= ulo W - 0.5 up to the rounding of the product and the
        // quotient, below 2^-18 texels for coordinates up to 2^20 -- the one texel of padding is never used up.  Larger coordinates: every texel.
        const LmBox box = lm_box(t);
        const double ulo = box.ulo, uhi = box.uhi, vlo = box.vlo, vhi = box.vhi;
        const bool exact = fmax(fmax(fabs(ulo), fabs(uhi)), fmax(fabs(vlo), fabs(vhi))) <= GI_LM_BOX_EXACT;
        const int32_t x0 = exact ? (int32_t)fmin(fmax(floor(ulo * W - 0.5) - 1.0, 0.0), W) : 0;
        const int32_t x1 = exact ? (int32_t)fmin(fmax(ceil(uhi * W - 0.5) + 1.0, -1.0), W - 1.0) : w - 1;
        const int32_t y0 = exact ? (int32_t)fmin(fmax(floor(vlo * H - 0.5) - 1.0, 0.0), H) : 0;
        const int32_t y1 = exact ? (int32_t)fmin(fmax(ceil(vhi * H - 0.5) + 1.0, -1.0), H - 1.0) : h - 1;
        if (x1 < x0 || y1 < y0) continue;
        const uint32_t bw = (uint32_t)(x1 - x0 + 1), count = bw * (uint32_t)(y1 - y0 + 1);   // at most 8192 x 8192
        for (uint32_t i = blockIdx.y * 64u + lane; i < count; i += gridDim.y * 64u) {
            const int32_t x = x0 + (int32_t)(i % bw), y = y0 + (int32_t)(i / bw);
            const double pu = lm_centre(x, w), pv = lm_centre(y, h);
            if (!lm_covers(box, lm_edges(t, pu, pv), pu, pv)) continue;
            int* const o = own + ((size_t)y * (size_t)w + (size_t)x);
            // (the table only ever falls: a stale value read here costs an atomic, never an owner)
            if (__hip_atomic_load(o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > (int)j) atomicMin(o, (int)j);
        }
    }
}

// One lane per texel: e1, e2 and the area once more for the owner row, the point and the normal, and own[t] = the row where they are valid, else -1.
// blk[workgroup] = its valid texels (ballot, one LDS atomic per wave).  ent is clamped to the entity tables.
__global__ __launch_bounds__(GI_BLOCK) void k_lm_point(Scene S, const int32_t* ent, const double* uv, int32_t w, int32_t h, uint32_t T, int flip, int* own, double* pn6, uint32_t* blk)
{
    __shared__ unsigned int cnt;
    if (threadIdx.x == 0) cnt = 0u;
    __syncthreads();
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    bool valid = false;
    if (t < T) {
        const int j = own[t];
        if (j != GI_LM_NONE && S.n_tri > 0) {
            const int32_t x = (int32_t)(t % (uint32_t)w), y = (int32_t)(t / (uint32_t)w);
            const int32_t e = min(max(ent[j], 0), S.n_tri - 1);
            const LmPoint q = lm_point(S.tris[e], S.shade[e], lm_edges(uv + (size_t)j * 6, lm_centre(x, w), lm_centre(y, h)), flip);
            valid = q.ok;
            if (valid) {
                double* o = pn6 + (size_t)t * 6;
                o[0] = q.P.x; o[1] = q.P.y; o[2] = q.P.z; o[3] = q.N.x; o[4] = q.N.y; o[5] = q.N.z;
            }
        }
        own[t] = valid ? j : -1;
    }
    const unsigned long long m = __ballot(valid);
    if ((threadIdx.x & 63u) == 0u && m) atomicAdd(&cnt, (unsigned int)__popcll(m));
    __syncthreads();
    if (threadIdx.x == 0) blk[blockIdx.x] = cnt;
}

// The rank of a covered texel = covered texels before it: its workgroup's offset (blk, scanned), the waves before its own, the lanes before it.
// rank[t] = that, or 0xffffffff; rows below `cap` of the table are written.
__global__ __launch_bounds__(GI_BLOCK) void k_lm_compact(const int* own, const double* pn6, const uint32_t* blk, uint32_t T, uint32_t* rank, double* points6, int32_t* texel, uint32_t cap)
{
    __shared__ uint32_t wcnt[GI_BLOCK / 64];
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const bool valid = t < T && own[t] >= 0;
    const unsigned long long m = __ballot(valid);
    if (lane == 0u) wcnt[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t r = blk[blockIdx.x] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    for (uint32_t k = 0; k < wave; k++) r += wcnt[k];
    if (t < T) rank[t] = valid ? r : 0xffffffffu;
    if (valid && r < cap) {
        const double* s = pn6 + (size_t)t * 6;
        double* o = points6 + (size_t)r * 6;
        GI_UNROLL
        for (int k = 0; k < 6; k++) o[k] = s[k];
        texel[r] = (int32_t)t;
    }
}

// a covered texel takes its bake row and is filled; every other texel holds 0 0 0
__global__ __launch_bounds__(GI_BLOCK) void k_lm_scatter(const uint32_t* rank, const double* rows3, uint32_t T, double* val, unsigned char* fill)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const uint32_t r = rank[t];
    const bool f = r != 0xffffffffu;
    double* o = val + (size_t)t * 3;
    const double* s = rows3 + (size_t)(f ? r : 0u) * 3;
    o[0] = f ? s[0] : 0.0; o[1] = f ? s[1] : 0.0; o[2] = f ? s[2] : 0.0;
    fill[t] = f ? 1 : 0;
}

// One dilation pass, one lane per texel: a filled texel keeps its value; an unfilled one with filled 8-neighbours takes their sum, from +0.0 in the
// header's order (rows top to bottom, left to right), divided by their count, and is filled in the output.  Reads only the pass's input.
__global__ __launch_bounds__(GI_BLOCK) void k_lm_dilate(int32_t w, int32_t h, const double* vin, const unsigned char* fin, double* vout, unsigned char* fout)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (uint32_t)w * (uint32_t)h) return;
    const int32_t x = (int32_t)(t % (uint32_t)w), y = (int32_t)(t / (uint32_t)w);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    int n = 0;
    const bool own = fin[t] != 0;
    if (own) { s0 = vin[(size_t)t * 3]; s1 = vin[(size_t)t * 3 + 1]; s2 = vin[(size_t)t * 3 + 2]; }
    else {
        GI_UNROLL
        for (int dy = -1; dy <= 1; dy++) {
            GI_UNROLL
            for (int dx = -1; dx <= 1; dx++) {
                if (dx == 0 && dy == 0) continue;
                const int32_t xx = x + dx, yy = y + dy;
                if (xx < 0 || xx >= w || yy < 0 || yy >= h) continue;
                const size_t q = (size_t)yy * (size_t)w + (size_t)xx;
                if (!fin[q]) continue;
                s0 += vin[q * 3]; s1 += vin[q * 3 + 1]; s2 += vin[q * 3 + 2];
                n++;
            }
        }
        if (n) { const double d = (double)n; s0 = s0 / d; s1 = s1 / d; s2 = s2 / d; }
    }
    vout[(size_t)t * 3] = s0; vout[(size_t)t * 3 + 1] = s1; vout[(size_t)t * 3 + 2] = s2;
    fout[t] = own || n ? 1 : 0;
}

// the atlas to the caller: f64 as it is, or rounded once to f32
__global__ __launch_bounds__(GI_BLOCK) void k_lm_store(const double* val, size_t n, void* out, int out_f64)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (out_f64) ((double*)out)[i] = val[i];
    else ((float*)out)[i] = (float)val[i];
}

namespace {

// false + message when the parameters and the chart's length are not the header's
bool lm_check(const gi_lightmap_params* p, int32_t n_chart, std::string& err)
{
    if (!p) { err = "lightmap: null parameters"; return false; }
    if (p->width < 1 || p->width > 8192 || p->height < 1 || p->height > 8192) { err = "lightmap: width and height must be 1 .. 8192, got " + std::to_string(p->width) + " x " + std::to_string(p->height); return false; }
    if (p->n_samples < 1) { err = "lightmap: n_samples must be at least 1, got " + std::to_string(p->n_samples); return false; }
    if (p->dilate < 0 || p->dilate > 64) { err = "lightmap: dilate must be 0 .. 64, got " + std::to_string(p->dilate); return false; }
    if (p->flip != 0 && p->flip != 1) { err = "lightmap: flip must be 0 or 1, got " + std::to_string(p->flip); return false; }
    if (n_chart < 0) { err = "lightmap: n_chart must not be negative, got " + std::to_string(n_chart); return false; }
    // every texel may be covered: the bake's check for that many points
    if ((unsigned long long)p->stream_base + (unsigned long long)p->width * (unsigned long long)p->height * (unsigned long long)p->n_samples > (1ull << 32)) {
        err = "lightmap: " + std::to_string(p->width) + " x " + std::to_string(p->height) + " texels of " + std::to_string(p->n_samples) + " samples from stream_base " + std::to_string(p->stream_base) + " can take the stream index beyond 32 bits";
        return false;
    }
    return true;
}
// the host entries look at the chart: every entity a triangle of the scene, every coordinate finite
bool lm_chart_ok(const gi_ctx* c, int32_t n_chart, const int32_t* ent, const double* uv, std::string& err)
{
    const std::vector<uint32_t>& flags = c->scene.tri_flags;
    for (int32_t j = 0; j < n_chart; j++) {
        if (ent[j] < 0 || (size_t)ent[j] >= flags.size()) { err = "lightmap: chart row " + std::to_string(j) + " names entity " + std::to_string(ent[j]) + ", the scene has " + std::to_string(flags.size()); return false; }
        if (flags[(size_t)ent[j]] & 4u) { err = "lightmap: chart row " + std::to_string(j) + " names entity " + std::to_string(ent[j]) + ", a sphere"; return false; }
        for (int k = 0; k < 6; k++)
            if (!std::isfinite(uv[(size_t)j * 6 + k])) { err = "lightmap: chart row " + std::to_string(j) + " has a non-finite coordinate"; return false; }
    }
    return true;
}

void lm_reset_timers(gi_ctx* c)
{
    c->lm.timer.reset();
    for (EventTimer& t : c->lm.t_stage) t.reset();
}
template <class T> hipError_t lm_grow(DevBuf<T>& b, size_t n) { return b.n < n ? b.alloc(n) : hipSuccess; }
// The pass's scratch is sized on first use and kept (LightmapPass): 58 bytes per texel (owner 4, rank 4, points / dilation buffers 48, filled flags 2;
// a count per 256 texels on top) and 76 per covered texel (table row 48, texel 4, bake row 24) -- 61 MB + 80 MB at 1024 x 1024 all covered,
// 3.9 GB + 5.1 GB at 8192 x 8192.  What is kept is memory the bake's pool cannot have.  The host entries, which have waited for the stream anyway, give the scratch of an
// atlas above GI_LM_KEEP_TEXELS back when they return; gi_lightmap_device is asynchronous and keeps it until a host entry or gi_destroy frees it.
#define GI_LM_KEEP_TEXELS ((size_t)1 << 22)
void lm_release_large(gi_ctx* c, size_t T)
{
    if (T <= GI_LM_KEEP_TEXELS) return;
    LightmapPass& lm = c->lm;
    lm.d_own.release(); lm.d_texel.release(); lm.d_rank.release(); lm.d_blk.release();
    lm.d_work.release(); lm.d_points.release(); lm.d_rows.release(); lm.d_fill.release();
}

// Stage 1, arguments checked, chart on the device: owners in lm.d_own [T] (-1 where not covered), ranks in lm.d_rank [T], the texel table in
// lm.d_points [n_cov][6] and lm.d_texel [n_cov].  Waits for the stream once, to read n_cov.
int lm_texel_table(gi_ctx* c, const gi_lightmap_params& p, int32_t n_chart, const int32_t* d_ent, const double* d_uv, uint32_t& n_cov)
{
    LightmapPass& lm = c->lm;
    hipStream_t st = c->stream;
    const uint32_t T = (uint32_t)p.width * (uint32_t)p.height, nb = (T + GI_BLOCK - 1) / GI_BLOCK;
    HIP_TRY(c, lm_grow(lm.d_own, T)); HIP_TRY(c, lm_grow(lm.d_rank, T)); HIP_TRY(c, lm_grow(lm.d_blk, (size_t)nb + 1)); HIP_TRY(c, lm_grow(lm.d_work, (size_t)T * 6));
    HIP_TRY(c, hipMemsetD32Async((hipDeviceptr_t)lm.d_own.p, GI_LM_NONE, T, st));
    HIP_TRY(c, hipMemsetAsync(lm.d_blk.p + nb, 0, sizeof(uint32_t), st));
    if (n_chart > 0) {
        const uint32_t gx = std::min<uint32_t>(((uint32_t)n_chart + GI_BLOCK / 64 - 1) / (GI_BLOCK / 64), 1u << 16);
        const uint32_t gy = std::min<uint32_t>(std::max<uint32_t>(T / 4096u, 1u), 64u);
        hipLaunchKernelGGL(k_lm_raster, dim3(gx, gy), dim3(GI_BLOCK), 0, st, n_chart, d_uv, p.width, p.height, lm.d_own.p);
    }
    hipLaunchKernelGGL(k_lm_point, dim3(nb), dim3(GI_BLOCK), 0, st, c->S, d_ent, d_uv, p.width, p.height, T, p.flip, lm.d_own.p, lm.d_work.p, lm.d_blk.p);
    hipLaunchKernelGGL(k_rs_scan, dim3(1), dim3(1024), 0, st, lm.d_blk.p, nb + 1u);   // exclusive prefix sums in place (gi_sort.inc): entry nb = the total
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(&n_cov, lm.d_blk.p + nb, sizeof n_cov, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (n_cov > T) return fail(c, GI_E_HIP, "lightmap: the rank counted more covered texels than the atlas has");
    HIP_TRY(c, lm_grow(lm.d_points, (size_t)n_cov * 6)); HIP_TRY(c, lm_grow(lm.d_texel, n_cov));
    hipLaunchKernelGGL(k_lm_compact, dim3(nb), dim3(GI_BLOCK), 0, st, lm.d_own.p, lm.d_work.p, lm.d_blk.p, T, lm.d_rank.p, lm.d_points.p, lm.d_texel.p, n_cov);
    HIP_TRY(c, hipGetLastError());
    return GI_OK;
}

// `passes` dilation passes from (va, fa), ping-pong with (vb, fb); result: the buffer that holds the last pass's output
void lm_dilate_passes(gi_ctx* c, int32_t w, int32_t h, int32_t passes, double* va, unsigned char* fa, double* vb, unsigned char* fb, const double*& result)
{
    const uint32_t T = (uint32_t)w * (uint32_t)h;
    for (int32_t k = 0; k < passes; k++) {
        hipLaunchKernelGGL(k_lm_dilate, GI_GRID(T), 0, c->stream, w, h, va, fa, vb, fb);
        std::swap(va, vb); std::swap(fa, fb);
    }
    result = va;
}

// the whole lightmap: chart, atlas and owner on the device, arguments checked
int lm_run(gi_ctx* c, const gi_lightmap_params& p, int32_t n_chart, const int32_t* d_ent, const double* d_uv, void* d_atlas, int out_is_f64, int32_t* d_owner, uint32_t& n_cov)
{
    HIP_TRY(c, hipSetDevice(c->device));
    LightmapPass& lm = c->lm;
    hipStream_t st = c->stream;
    const uint32_t T = (uint32_t)p.width * (uint32_t)p.height;
    lm_reset_timers(c);
    struct Guard { gi_ctx* c; bool ok = false; ~Guard() { if (!ok) lm_reset_timers(c); } } guard{c};   // a call that fails has no time to report
    HIP_TRY(c, lm.timer.begin(st));
    HIP_TRY(c, lm.t_stage[0].begin(st));
    if (const int rc = lm_texel_table(c, p, n_chart, d_ent, d_uv, n_cov)) return rc;
    HIP_TRY(c, lm.t_stage[0].end(st));
    if (n_cov) {
        HIP_TRY(c, lm_grow(lm.d_rows, (size_t)n_cov * 3));
        gi_bake_params bp;
        bp.mode = GI_BAKE_TEXEL; bp.n_samples = p.n_samples; bp.stream_base = p.stream_base; bp.seed = p.seed;
        if (const int rc = bake_run(c, lm.d_points.p, n_cov, bp, lm.d_rows.p, 1, &lm.t_stage[1])) return rc;
    }
    HIP_TRY(c, lm.t_stage[2].begin(st));
    HIP_TRY(c, lm_grow(lm.d_fill, (size_t)T * 2));
    double* const va = lm.d_work.p;                       // the points are in the table by now: their buffer is the two dilation buffers
    hipLaunchKernelGGL(k_lm_scatter, GI_GRID(T), 0, st, lm.d_rank.p, lm.d_rows.p, T, va, lm.d_fill.p);
    const double* result = va;
    lm_dilate_passes(c, p.width, p.height, p.dilate, va, lm.d_fill.p, va + (size_t)T * 3, lm.d_fill.p + T, result);
    hipLaunchKernelGGL(k_lm_store, GI_GRID((size_t)T * 3), 0, st, result, (size_t)T * 3, d_atlas, out_is_f64);
    HIP_TRY(c, hipGetLastError());
    if (d_owner) HIP_TRY(c, hipMemcpyAsync(d_owner, lm.d_own.p, (size_t)T * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    HIP_TRY(c, lm.t_stage[2].end(st));
    HIP_TRY(c, lm.timer.end(st));
    guard.ok = true;
    return GI_OK;
}

}  // namespace

extern "C" {

void gi_lightmap_default_params(gi_lightmap_params* p)
{
    if (!p) return;
    p->width = 256; p->height = 256; p->n_samples = 256; p->dilate = 2; p->flip = 0;
    p->stream_base = 0u;
    p->seed = 0x9E3779B97F4A7C15ull;
}

int gi_lightmap_device(gi_ctx* c, const gi_lightmap_params* p, int32_t n_chart, const int32_t* d_ent, const double* d_uv, void* d_atlas, int out_is_f64, int32_t* d_owner, int32_t* n_covered)
{
    if (!c) return GI_E_INVALID;
    std::string err;
    if (!lm_check(p, n_chart, err)) return fail(c, GI_E_INVALID, err);
    if (!d_atlas || (n_chart && (!d_ent || !d_uv))) return fail(c, GI_E_INVALID, "lightmap: null chart or atlas pointer");
    if (!c->scene.have_scene) return fail(c, GI_E_STATE, "lightmap: no scene uploaded");
    uint32_t n_cov = 0;
    const int rc = lm_run(c, *p, n_chart, d_ent, d_uv, d_atlas, out_is_f64, d_owner, n_cov);
    if (rc == GI_OK && n_covered) *n_covered = (int32_t)n_cov;
    return rc;
}

int gi_lightmap_host(gi_ctx* c, const gi_lightmap_params* p, int32_t n_chart, const int32_t* ent, const double* uv, void* h_atlas, int out_is_f64, int32_t* h_owner, int32_t* n_covered)
{
    if (!c) return GI_E_INVALID;
    std::string err;
    if (!lm_check(p, n_chart, err)) return fail(c, GI_E_INVALID, err);
    if (!h_atlas || (n_chart && (!ent || !uv))) return fail(c, GI_E_INVALID, "lightmap: null chart or atlas pointer");
    if (!c->scene.have_scene) return fail(c, GI_E_STATE, "lightmap: no scene uploaded");
    if (!lm_chart_ok(c, n_chart, ent, uv, err)) return fail(c, GI_E_INVALID, err);
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t T = (size_t)p->width * (size_t)p->height, bytes = T * 3 * (out_is_f64 ? 8 : 4);
    DevBuf<int32_t> d_ent, d_owner;
    DevBuf<double> d_uv;
    DevBuf<unsigned char> d_atlas;
    HIP_TRY(c, d_ent.upload(ent, (size_t)n_chart)); HIP_TRY(c, d_uv.upload(uv, (size_t)n_chart * 6));
    HIP_TRY(c, d_atlas.alloc(bytes));
    if (h_owner) HIP_TRY(c, d_owner.alloc(T));
    uint32_t n_cov = 0;
    int rc = lm_run(c, *p, n_chart, d_ent.p, d_uv.p, d_atlas.p, out_is_f64, h_owner ? d_owner.p : nullptr, n_cov);
    if (rc == GI_OK) rc = finish_to_host(c, "lightmap_host", {{h_atlas, d_atlas.p, bytes}, {h_owner, d_owner.p, T * sizeof(int32_t)}});
    else (void)hipStreamSynchronize(c->stream);
    lm_release_large(c, T);
    if (rc != GI_OK) { lm_reset_timers(c); return rc; }
    if (n_covered) *n_covered = (int32_t)n_cov;
    return GI_OK;
}

int gi_last_lightmap_ms(gi_ctx* c, float* ms, float* stages3)
{
    if (!c || !ms) return GI_E_INVALID;
    HIP_TRY(c, c->lm.timer.read(ms));
    for (int k = 0; stages3 && k < 3; k++) HIP_TRY(c, c->lm.t_stage[k].read(stages3 + k));
    return GI_OK;
}

int gi_lightmap_texels(gi_ctx* c, const gi_lightmap_params* p, int32_t n_chart, const int32_t* ent, const double* uv, int32_t* owner, int32_t* n_covered, double* points6, int32_t* texel, int32_t cap)
{
    if (!c) return GI_E_INVALID;
    std::string err;
    if (!lm_check(p, n_chart, err)) return fail(c, GI_E_INVALID, err);
    if (cap < 0 || !owner || !n_covered || (cap && (!points6 || !texel)) || (n_chart && (!ent || !uv))) return fail(c, GI_E_INVALID, "lightmap_texels: null pointer or negative capacity");
    if (!c->scene.have_scene) return fail(c, GI_E_STATE, "lightmap_texels: no scene uploaded");
    if (!lm_chart_ok(c, n_chart, ent, uv, err)) return fail(c, GI_E_INVALID, err);
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t T = (size_t)p->width * (size_t)p->height;
    DevBuf<int32_t> d_ent;
    DevBuf<double> d_uv;
    HIP_TRY(c, d_ent.upload(ent, (size_t)n_chart)); HIP_TRY(c, d_uv.upload(uv, (size_t)n_chart * 6));
    uint32_t n_cov = 0;
    if (const int rc = lm_texel_table(c, *p, n_chart, d_ent.p, d_uv.p, n_cov)) { (void)hipStreamSynchronize(c->stream); lm_release_large(c, T); return rc; }
    const bool fits = n_cov <= (uint32_t)cap;
    int rc = finish_to_host(c, "lightmap_texels", {{owner, c->lm.d_own.p, T * sizeof(int32_t)}, {fits ? points6 : nullptr, c->lm.d_points.p, (size_t)n_cov * 48}, {fits ? texel : nullptr, c->lm.d_texel.p, (size_t)n_cov * sizeof(int32_t)}});
    lm_release_large(c, T);
    if (rc != GI_OK) return rc;
    *n_covered = (int32_t)n_cov;
    if (!fits) return fail(c, GI_E_INVALID, "lightmap_texels: " + std::to_string(n_cov) + " covered texels, capacity " + std::to_string(cap));
    return GI_OK;
}

int gi_lightmap_dilate(gi_ctx* c, int32_t width, int32_t height, int32_t passes, const double* values3, const int32_t* filled, double* out3)
{
    if (!c) return GI_E_INVALID;
    if (width < 1 || width > 8192 || height < 1 || height > 8192 || passes < 0 || passes > 64) return fail(c, GI_E_INVALID, "lightmap_dilate: width and height 1 .. 8192, passes 0 .. 64");
    if (!values3 || !filled || !out3) return fail(c, GI_E_INVALID, "lightmap_dilate: null pointer");
    const size_t T = (size_t)width * (size_t)height;
    std::vector<double> hv(T * 3);
    std::vector<unsigned char> hf(T);
    for (size_t t = 0; t < T; t++) {                 // what k_lm_scatter leaves: an unfilled texel holds 0 0 0
        hf[t] = filled[t] != 0;
        for (int k = 0; k < 3; k++) hv[t * 3 + k] = hf[t] ? values3[t * 3 + k] : 0.0;
    }
    Entry e(c, "lightmap_dilate");
    double* d_va = const_cast<double*>(e.in(hv.data(), T * 3));
    unsigned char* d_fa = const_cast<unsigned char*>(e.in(hf.data(), T));
    double* d_vb = e.scratch<double>(T * 3);
    unsigned char* d_fb = e.scratch<unsigned char>(T);
    double* d_o = e.out(out3, T * 3);
    return e.run([&] {
        const double* result = d_va;
        lm_dilate_passes(c, width, height, passes, d_va, d_fa, d_vb, d_fb, result);
        hipLaunchKernelGGL(k_lm_store, GI_GRID(T * 3), 0, c->stream, result, T * 3, (void*)d_o, 1);
    });
}

}  // extern "C"
