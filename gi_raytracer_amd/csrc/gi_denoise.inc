// gi_denoise.inc -- the edge-avoiding a-trous denoiser (gi_denoise_*; an addition: the reference has no denoiser).  Included by gi_kernels.hip
// after the context and its helpers.  The formula is stated in include/gi_hip.h; the per-tap functions (dn_tap_weight(), and up_tap_weight()
// of the upsampler) stand first with DnPix, DnInv and the GI_DN_* constants, in namespace gi as the kernels' parameter types were.

namespace gi {
// ------------------------------------------------------------------------------------------------ a-trous denoiser (an addition: the reference has no denoiser)
// One tap of the edge-avoiding a-trous filter (gi_hip.h: gi_denoise_*; Dammertz et al. 2010 with Tukey's biweight as the edge-stopping function).
// IEEE operations only, in the order the header states, so that with -ffp-contract=off the result equals the tests' numpy statement bit for bit.
struct DnPix { V3 c, n, a; double z, cov; };     // what a tap reads of a pixel: demodulated colour, normal, albedo, depth, coverage
struct DnInv { double c, n, z, a; };             // 4^level / sigma_color^2, 1 / sigma_normal^2, 1 / sigma_depth^2, 1 / sigma_albedo^2 (0 = term off)
#define GI_DN_ALBEDO_FLOOR 1e-3
#define GI_DN_DC_EPS 1e-12
GI_HD double dn_sq3(V3 v) { return (v.x * v.x + v.y * v.y) + v.z * v.z; }
GI_HD bool dn_finite(V3 c) { return fabs(c.x) <= 1.7976931348623157e308 && fabs(c.y) <= 1.7976931348623157e308 && fabs(c.z) <= 1.7976931348623157e308; }
GI_HD double dn_modulation(double albedo, int demodulate) { return demodulate ? (albedo > GI_DN_ALBEDO_FLOOR ? albedo : GI_DN_ALBEDO_FLOOR) : 1.0; }
// The three guide terms of a tap, shared by both filters' weights: squared normal difference, squared relative depth difference (0 unless
// z_p + z_q > 0), squared albedo difference plus squared coverage difference.
struct GuideDiff { double dn, dz, da; };
GI_HD GuideDiff guide_diff(const DnPix& p, const DnPix& q)
{
    GuideDiff g;
    g.dn = dn_sq3(p.n - q.n);
    const double dcov = p.cov - q.cov;
    g.da = dn_sq3(p.a - q.a) + dcov * dcov;
    const double zs = p.z + q.z;
    g.dz = 0.0;
    if (zs > 0.0) { const double r = (p.z - q.z) / zs; g.dz = r * r; }
    return g;
}
// weight of tap q for the centre p: hh = h[dy] h[dx]; p_c2 = |c_p|^2; p_ok = the centre's colour is finite (else the colour term is 0).
// The caller skips taps outside the frame and taps whose colour is not finite.
GI_HD double dn_tap_weight(const DnPix& p, double p_c2, bool p_ok, const DnPix& q, const DnInv& inv, double hh)
{
    const double dc = p_ok ? dn_sq3(p.c - q.c) / (p_c2 + (dn_sq3(q.c) + GI_DN_DC_EPS)) : 0.0;
    const GuideDiff g = guide_diff(p, q);
    const double d = ((dc * inv.c + g.dn * inv.n) + g.dz * inv.z) + g.da * inv.a;
    const double t = d < 1.0 ? 1.0 - d : 0.0;      // 1 - min(d, 1); a NaN d counts as 1
    return hh * (t * t);
}
// The guided upsampler's tap (gi_hip.h: gi_upsample_*): p = the full pixel's guide, q = a low pixel's; the denoiser's dn, dz and da without its
// colour term, d = (dn inv_n + dz inv_z) + da inv_a (inv.c is not read); hh = ty tx, the tent.
GI_HD double up_tap_weight(const DnPix& p, const DnPix& q, const DnInv& inv, double hh)
{
    const GuideDiff g = guide_diff(p, q);
    const double d = (g.dn * inv.n + g.dz * inv.z) + g.da * inv.a;
    const double e = d < 1.0 ? 1.0 - d : 0.0;      // 1 - min(d, 1); a NaN d counts as 1
    return hh * (e * e);
}
}  // namespace gi

// Three kernels, all on the context's stream, no atomics, no host sync between them:
//   k_dn_pack   widens colour and features to f64, demodulates, and writes the two things a tap reads: the colour [h][w][3] (changes per
//               level) and the level-invariant guide record [h][w][8] (albedo, normal, depth, coverage: 64 B, one half cache line);
//   k_dn_level  one level, one lane per pixel, 25 taps from LDS.  A level of step s is a dense 5 x 5 filter on each of the s^2 interleaved
//               sub-lattices x = ox + s lx, y = oy + s ly, so a workgroup takes a 32 x 16 tile of ONE sub-lattice with a halo of two lattice
//               cells: 36 x 20 = 720 cells whatever s is.  The cells sit in LDS as a GuideTile, so the 32 lanes of a row read 32 consecutive
//               doubles per ds_read_b64: no bank conflicts.  The last level multiplies by the modulation and stores in the caller's type;
//   k_dn_copy   iterations = 0: out = colour, converted.
// What this file shares with the guided upsampler (gi_upsample.inc), each written once here: on the device GuideTile (the LDS tile: its size, its
// two staging loops, its cell reader), TapSum (the weighted sum over the taps) and dn_store3 (three values in the caller's type), beside k_dn_pack
// and guide_diff() above; on the host filter_size_check / filter_sigma_check and the two refusals behind them, dn_inv and dn_reserve.
// The host-pointer forms are an Entry with the pass's timer and the timer reads are pass_ms (both gi_context.inc).
// Workgroups that share a neighbourhood run next to each other: the sub-lattice index is the fastest part of blockIdx.x, so at large steps the
// s^2 workgroups that read one region of the frame (each a 1/s^2 sample of its cache lines) are in flight together and the lines come from L2.
#define GI_DN_TX 32
#define GI_DN_TY 16
#define GI_DN_HX (GI_DN_TX + 4)
#define GI_DN_HY (GI_DN_TY + 4)
#define GI_DN_PLANE 724                         // plane stride in doubles, for 36 x 20 = 720 cells (GuideTile: = 4 mod 16)
#define GI_DN_BLOCK (GI_DN_TX * GI_DN_TY)       // 512
#define GI_DN_MAX_ITERATIONS 8

struct DnGrid { int32_t w, h, log2s, tiles_x; };

template <class T> __device__ __forceinline__ double dn_widen(const void* p, size_t i) { return (double)((const T*)p)[i]; }
__device__ __forceinline__ double dn_load(const void* p, int is_f64, size_t i) { return is_f64 ? dn_widen<double>(p, i) : dn_widen<float>(p, i); }
__device__ __forceinline__ void dn_store(void* p, int is_f64, size_t i, double v)
{
    if (is_f64) ((double*)p)[i] = v;
    else ((float*)p)[i] = (float)v;
}

// one lane per feature value e = pixel * 8 + k: guides[e] = the value in f64; the lanes of the three albedo channels also write the pixel's
// demodulated colour channel
__global__ __launch_bounds__(256) void k_dn_pack(size_t n_pix, const void* color, int color_f64, const void* feat, int feat_f64, int demodulate, double* c, double* guides)
{
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_pix * 8) return;
    const double f = dn_load(feat, feat_f64, e);
    guides[e] = f;
    const int k = (int)(e & 7);
    if (k < 3) {
        const size_t o = (e >> 3) * 3 + k;
        c[o] = dn_load(color, color_f64, o) / dn_modulation(f, demodulate);
    }
}

__global__ __launch_bounds__(256) void k_dn_copy(size_t n, const void* color, int color_f64, void* out, int out_f64)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dn_store(out, out_f64, i, dn_load(color, color_f64, i));
}

// The LDS tile both image filters take their taps from: HX x HY cells (a workgroup's pixels and their halo) as 11 planes of doubles (structure
// of arrays): colour 0..2, then the guide record -- albedo 3..5, normal 6..8, depth 9, coverage 10.  PLANE is the plane stride in doubles, = 4 mod
// 16, so that the loader's 8 components of a cell fall on different banks (2-way at worst).
template <int HX, int HY, int PLANE>
struct GuideTile {
    static constexpr int CELLS = HX * HY, DOUBLES = 11 * PLANE;
    // Stages the tile from colour [h][w][3] and guides [h][w][8] (f64) with the GI_DN_BLOCK lanes of the workgroup and ends with a barrier.
    // pixel_of_cell(cx, cy, x, y) names the frame pixel of halo cell (cx, cy).  A cell outside the frame gets a NaN colour, so the test that skips
    // non-finite input skips it, and zero guides.  Colour goes double by double, the guides in 4 pairs of doubles per cell (16-byte loads).
    template <class PixelOfCell>
    static __device__ __forceinline__ void fill(double* lds, const double* __restrict__ colour, const double* __restrict__ guides, int w, int h, PixelOfCell pixel_of_cell)
    {
        for (int idx = threadIdx.x; idx < CELLS * 3; idx += GI_DN_BLOCK) {
            const int cell = idx / 3, k = idx - cell * 3;
            int x, y;
            pixel_of_cell(cell % HX, cell / HX, x, y);
            const bool in = x >= 0 && x < w && y >= 0 && y < h;
            lds[k * PLANE + cell] = in ? colour[((size_t)y * w + x) * 3 + k] : __builtin_nan("");
        }
        for (int idx = threadIdx.x; idx < CELLS * 4; idx += GI_DN_BLOCK) {
            const int cell = idx >> 2, k = (idx & 3) * 2;
            int x, y;
            pixel_of_cell(cell % HX, cell / HX, x, y);
            double2 v = make_double2(0.0, 0.0);
            if (x >= 0 && x < w && y >= 0 && y < h) v = *(const double2*)(guides + ((size_t)y * w + x) * 8 + k);
            lds[(3 + k) * PLANE + cell] = v.x;
            lds[(4 + k) * PLANE + cell] = v.y;
        }
        __syncthreads();
    }
    static __device__ __forceinline__ DnPix cell(const double* lds, int i)
    {
        DnPix q;
        q.c = v3(lds[i], lds[PLANE + i], lds[2 * PLANE + i]);
        q.a = v3(lds[3 * PLANE + i], lds[4 * PLANE + i], lds[5 * PLANE + i]);
        q.n = v3(lds[6 * PLANE + i], lds[7 * PLANE + i], lds[8 * PLANE + i]);
        q.z = lds[9 * PLANE + i];
        q.cov = lds[10 * PLANE + i];
        return q;
    }
};

// The weighted colour sum of a pixel's taps.  A skipped tap (ok false, wq 0) still adds an exact 0.0, never 0 * its NaN.
struct TapSum {
    V3 num = v3(0, 0, 0);
    double den = 0.0;
    __device__ __forceinline__ void add(const DnPix& q, double wq, bool ok)
    {
        num.x += wq * (ok ? q.c.x : 0.0);
        num.y += wq * (ok ? q.c.y : 0.0);
        num.z += wq * (ok ? q.c.z : 0.0);
        den += wq;
    }
    __device__ __forceinline__ V3 mean() const { return v3(num.x / den, num.y / den, num.z / den); }   // for den > 0
};

__device__ __forceinline__ void dn_store3(void* p, int is_f64, size_t o, V3 v)
{
    dn_store(p, is_f64, o, v.x);
    dn_store(p, is_f64, o + 1, v.y);
    dn_store(p, is_f64, o + 2, v.z);
}

using DnTile = GuideTile<GI_DN_HX, GI_DN_HY, GI_DN_PLANE>;

// src, dst: [h][w][3] f64 demodulated colour; guides [h][w][8] f64.  last: dst is not written; out (type out_f64) gets colour * modulation.
__global__ __launch_bounds__(GI_DN_BLOCK) void k_dn_level(DnGrid G, DnInv inv, const double* __restrict__ src, const double* __restrict__ guides, double* __restrict__ dst,
                                                          int last, int demodulate, void* out, int out_f64)
{
    __shared__ double lds[DnTile::DOUBLES];
    const int s = 1 << G.log2s;
    const uint32_t sub = blockIdx.x & (uint32_t)(s * s - 1);
    const uint32_t tile = blockIdx.x >> (2 * G.log2s);
    const int ox = (int)(sub & (uint32_t)(s - 1)), oy = (int)(sub >> G.log2s);
    const int lx0 = (int)(tile % (uint32_t)G.tiles_x) * GI_DN_TX - 2, ly0 = (int)(tile / (uint32_t)G.tiles_x) * GI_DN_TY - 2;   // lattice cell of halo cell (0, 0)
    DnTile::fill(lds, src, guides, G.w, G.h, [=](int cx, int cy, int& x, int& y) { x = ox + s * (lx0 + cx); y = oy + s * (ly0 + cy); });
    const int tx = threadIdx.x & (GI_DN_TX - 1), ty = threadIdx.x / GI_DN_TX;
    const int x = ox + s * (lx0 + 2 + tx), y = oy + s * (ly0 + 2 + ty);
    if (x >= G.w || y >= G.h) return;
    const DnPix p = DnTile::cell(lds, (ty + 2) * GI_DN_HX + tx + 2);
    const bool p_ok = dn_finite(p.c);
    const double p_c2 = dn_sq3(p.c);
    const double h5[5] = {1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0};
    TapSum sum;
#pragma unroll
    for (int dy = 0; dy < 5; dy++) {
#pragma unroll
        for (int dx = 0; dx < 5; dx++) {
            const DnPix q = DnTile::cell(lds, (ty + dy) * GI_DN_HX + tx + dx);
            const bool ok = dn_finite(q.c);        // outside the frame (NaN from the loader) or a non-finite input: skipped
            sum.add(q, ok ? dn_tap_weight(p, p_c2, p_ok, q, inv, h5[dy] * h5[dx]) : 0.0, ok);
        }
    }
    const V3 r = sum.den > 0.0 ? sum.mean() : v3(0, 0, 0);
    const size_t o = ((size_t)y * G.w + x) * 3;
    if (last) dn_store3(out, out_f64, o, v3(r.x * dn_modulation(p.a.x, demodulate), r.y * dn_modulation(p.a.y, demodulate), r.z * dn_modulation(p.a.z, demodulate)));
    else dn_store3(dst, 1, o, r);
}

namespace {

// ---- what the entries of an image filter `name` ("denoise", "upsample") refuse in the same words.  A *_check gives false + message when the
// parameters are not the header's; the two refusals below it come behind that check, the pixel limit in the device form only.
bool filter_size_check(const char* name, int w, int h, std::string& err)
{
    if (w >= 1 && h >= 1) return true;
    err = std::string(name) + ": width and height must be at least 1, got " + std::to_string(w) + " x " + std::to_string(h);
    return false;
}
bool filter_sigma_check(const char* name, const char* const* names, const double* values, int n, std::string& err)
{
    for (int k = 0; k < n; k++)
        if (!(values[k] >= 0.0)) { err = std::string(name) + ": " + names[k] + " must be >= 0 (0 switches the term off), got " + std::to_string(values[k]); return false; }
    return true;
}
int filter_null_pointer(gi_ctx* c, const char* name) { return fail(c, GI_E_INVALID, std::string(name) + ": null colour, feature or output pointer"); }
int filter_pixel_limit(gi_ctx* c, const char* name, size_t n_pix)
{
    return n_pix > ((size_t)1 << 28) ? fail(c, GI_E_INVALID, std::string(name) + ": frames beyond 2^28 pixels are not supported") : GI_OK;
}

bool dn_check(const gi_denoise_params* p, std::string& err)
{
    if (!p) { err = "denoise: null parameters"; return false; }
    if (!filter_size_check("denoise", p->width, p->height, err)) return false;
    if (p->iterations < 0 || p->iterations > GI_DN_MAX_ITERATIONS) { err = "denoise: iterations must be 0 .. " + std::to_string(GI_DN_MAX_ITERATIONS) + ", got " + std::to_string(p->iterations); return false; }
    const double sg[4] = {p->sigma_color, p->sigma_normal, p->sigma_depth, p->sigma_albedo};
    const char* names[4] = {"sigma_color", "sigma_normal", "sigma_depth", "sigma_albedo"};
    return filter_sigma_check("denoise", names, sg, 4, err);
}

double dn_inv(double sigma, double scale) { return sigma != 0.0 ? scale / (sigma * sigma) : 0.0; }

// The context's scratch for a frame of n_pix pixels: the guide records and the two colour buffers, always sized together, on first use and kept; a
// larger frame replaces them (after the stream has drained: an earlier pass may still read them).  The upsampler packs its low frame here too.
int dn_reserve(gi_ctx* c, size_t n_pix)
{
    if (c->dn.d_guides.n >= n_pix * 8) return GI_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    hipError_t e = c->dn.d_guides.alloc(n_pix * 8);
    if (e == hipSuccess) e = c->dn.d_a.alloc(n_pix * 3);
    if (e == hipSuccess) e = c->dn.d_b.alloc(n_pix * 3);
    if (e != hipSuccess) {                      // none of the three is kept: the size of the guide records stands for all of them
        c->dn.d_guides.release(); c->dn.d_a.release(); c->dn.d_b.release();
        return fail(c, GI_E_HIP, std::string("denoiser scratch: ") + hipGetErrorString(e));
    }
    return GI_OK;
}

}  // namespace

extern "C" {

void gi_denoise_default_params(gi_denoise_params* p)
{
    if (!p) return;
    p->width = 0; p->height = 0;
    p->iterations = 5; p->demodulate = 1;
    p->sigma_color = 1.0; p->sigma_normal = 0.5; p->sigma_depth = 0.1; p->sigma_albedo = 0.25;
}

int gi_denoise_device(gi_ctx* c, const gi_denoise_params* p, const void* d_color, int color_is_f64, const void* d_features, int features_is_f64, void* d_out, int out_is_f64)
{
    if (!c) return GI_E_INVALID;
    c->dn.timer.reset();
    std::string err;
    if (!dn_check(p, err)) return fail(c, GI_E_INVALID, err);
    if (!d_color || !d_features || !d_out) return filter_null_pointer(c, "denoise");
    const size_t n_pix = (size_t)p->width * (size_t)p->height;
    if (const int rc = filter_pixel_limit(c, "denoise", n_pix)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const int it = p->iterations;
    if (it > 0) {
        const int rc = dn_reserve(c, n_pix);
        if (rc != GI_OK) return rc;
    }
    HIP_TRY(c, c->dn.timer.begin(c->stream));
    if (it == 0) {
        if (d_out != d_color || (out_is_f64 != 0) != (color_is_f64 != 0))
            hipLaunchKernelGGL(k_dn_copy, dim3((unsigned)((n_pix * 3 + 255) / 256)), dim3(256), 0, c->stream, n_pix * 3, d_color, color_is_f64, d_out, out_is_f64);
    } else {
        const int demod = p->demodulate != 0;
        hipLaunchKernelGGL(k_dn_pack, dim3((unsigned)((n_pix * 8 + 255) / 256)), dim3(256), 0, c->stream, n_pix, d_color, color_is_f64, d_features, features_is_f64, demod,
                           c->dn.d_a.p, c->dn.d_guides.p);
        double* src = c->dn.d_a.p;
        double* dst = c->dn.d_b.p;
        for (int i = 0; i < it; i++) {
            const int s = 1 << i;
            DnGrid G;
            G.w = p->width; G.h = p->height; G.log2s = i;
            const int lw = (p->width + s - 1) / s, lh = (p->height + s - 1) / s;       // the largest sub-lattice (ox = oy = 0)
            G.tiles_x = (lw + GI_DN_TX - 1) / GI_DN_TX;
            const int tiles_y = (lh + GI_DN_TY - 1) / GI_DN_TY;
            DnInv inv;
            inv.c = dn_inv(p->sigma_color, (double)(1u << (2 * i)));                   // the colour sigma halves per level
            inv.n = dn_inv(p->sigma_normal, 1.0); inv.z = dn_inv(p->sigma_depth, 1.0); inv.a = dn_inv(p->sigma_albedo, 1.0);
            const size_t blocks = (size_t)G.tiles_x * tiles_y * s * s;
            hipLaunchKernelGGL(k_dn_level, dim3((unsigned)blocks), dim3(GI_DN_BLOCK), 0, c->stream, G, inv, src, c->dn.d_guides.p, dst, i == it - 1 ? 1 : 0, demod, d_out, out_is_f64);
            std::swap(src, dst);
        }
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, c->dn.timer.end(c->stream));
    return GI_OK;
}

int gi_denoise_host(gi_ctx* c, const gi_denoise_params* p, const void* h_color, int color_is_f64, const void* h_features, int features_is_f64, void* h_out, int out_is_f64)
{
    if (!c) return GI_E_INVALID;
    c->dn.timer.reset();
    std::string err;
    if (!dn_check(p, err)) return fail(c, GI_E_INVALID, err);
    if (!h_color || !h_features || !h_out) return filter_null_pointer(c, "denoise");
    const size_t n_pix = (size_t)p->width * (size_t)p->height;
    Entry e(c, "denoise_host", &c->dn.timer);
    const unsigned char* d_color = e.in((const unsigned char*)h_color, n_pix * 3 * (color_is_f64 ? 8 : 4));
    const unsigned char* d_feat = e.in((const unsigned char*)h_features, n_pix * 8 * (features_is_f64 ? 8 : 4));
    unsigned char* d_out = e.out((unsigned char*)h_out, n_pix * 3 * (out_is_f64 ? 8 : 4));
    return e.run([&] { return gi_denoise_device(c, p, d_color, color_is_f64, d_feat, features_is_f64, d_out, out_is_f64); });
}

int gi_last_denoise_ms(gi_ctx* c, float* ms) { return pass_ms(c, &gi_ctx::dn, ms); }

}  // extern "C"
