// gi_upsample.inc -- the guided (joint-bilateral) upsampler (gi_upsample_*; an addition: the reference has none).  Included by gi_kernels.hip after
// gi_denoise.inc, whose pack kernel, LDS tile (GuideTile), tap sum, typed store, parameter checks and scratch it uses (listed there).  The formula
// is stated in include/gi_hip.h; the per-tap function, up_tap_weight(), stands in gi_denoise.inc with the guide types it shares with the
// denoiser's (DnPix, DnInv, GuideDiff), so this file has to be included after that one -- the order gi_kernels.hip has.
//
// Two kernels on the context's stream, no atomics, no host sync between them:
//   k_dn_pack    on the LOW frame: widens and demodulates its colour and widens its guide records into the denoiser's scratch (f64);
//   k_up_sample  one lane per FULL pixel; a workgroup takes a 32 x 16 tile of full pixels.  The taps of pixel x are the low columns X0(x) - 1 ..
//                X0(x) + 2 with X0(x) = floor((2x + 1 - S) / 2S), and X0(x0 + 31) - X0(x0) <= ceil(31 / S) <= 16, so the tile's low-size footprint is
//                at most 20 x 12 cells (S = 2; fewer for larger S, the rest of the 240 cells are loaded and not read).  The cells sit in LDS as a
//                GuideTile, as in k_dn_level: the 32 lanes of a tile row read at most 32 / S + 1 different, consecutive doubles per ds_read_b64 --
//                neighbours share a cell, which is a broadcast, not a conflict.  After the barrier each lane reads its own full-size guide record
//                (32 or 64 B; consecutive lanes read consecutive records) straight from global memory, runs the 16 taps out of LDS and stores once
//                in the caller's type.
#define GI_UP_TX 32
#define GI_UP_TY 16
#define GI_UP_HX (GI_UP_TX / 2 + 4)             // 20: the S = 2 footprint
#define GI_UP_HY (GI_UP_TY / 2 + 4)             // 12
#define GI_UP_PLANE 244                         // plane stride in doubles, for 20 x 12 = 240 cells (GuideTile: = 4 mod 16)
#define GI_UP_BLOCK (GI_UP_TX * GI_UP_TY)       // 512
#define GI_UP_MIN_FACTOR 2
#define GI_UP_MAX_FACTOR 8

struct UpGrid { int32_t w, h, wl, hl, S, tiles_x; };

__device__ __forceinline__ int up_floor_div(int a, int b) { const int q = a / b; return (a % b < 0) ? q - 1 : q; }   // b > 0

using UpTile = GuideTile<GI_UP_HX, GI_UP_HY, GI_UP_PLANE>;
static_assert(GI_UP_BLOCK == GI_DN_BLOCK, "GuideTile::fill strides by the denoiser's workgroup size");

// lc [hl][wl][3] f64 demodulated low colour and lg [hl][wl][8] f64 low guides (k_dn_pack's output); feat [h][w][8] and out [h][w][3] in the caller's types
__global__ __launch_bounds__(GI_UP_BLOCK) void k_up_sample(UpGrid G, DnInv inv, const double* __restrict__ lc, const double* __restrict__ lg, const void* __restrict__ feat, int feat_f64,
                                                           int demodulate, void* __restrict__ out, int out_f64)
{
    __shared__ double lds[UpTile::DOUBLES];
    const int S2 = 2 * G.S, S4 = 4 * G.S;
    const int fx0 = (int)(blockIdx.x % (uint32_t)G.tiles_x) * GI_UP_TX, fy0 = (int)(blockIdx.x / (uint32_t)G.tiles_x) * GI_UP_TY;
    const int lx0 = up_floor_div(2 * fx0 + 1 - G.S, S2) - 1, ly0 = up_floor_div(2 * fy0 + 1 - G.S, S2) - 1;     // low pixel of halo cell (0, 0)
    UpTile::fill(lds, lc, lg, G.wl, G.hl, [=](int cx, int cy, int& X, int& Y) { X = lx0 + cx; Y = ly0 + cy; });
    const int x = fx0 + (int)(threadIdx.x & (GI_UP_TX - 1)), y = fy0 + (int)(threadIdx.x / GI_UP_TX);
    if (x >= G.w || y >= G.h) return;
    const size_t pix = (size_t)y * G.w + x;
    double g[8];
    if (((uintptr_t)feat & 15) == 0) {             // whole records in 16-byte loads (every allocation is aligned so; a caller's offset view may not be)
        if (feat_f64) {
#pragma unroll
            for (int k = 0; k < 4; k++) { const double2 v = ((const double2*)feat)[pix * 4 + k]; g[2 * k] = v.x; g[2 * k + 1] = v.y; }
        } else {
#pragma unroll
            for (int k = 0; k < 2; k++) { const float4 v = ((const float4*)feat)[pix * 2 + k]; g[4 * k] = (double)v.x; g[4 * k + 1] = (double)v.y; g[4 * k + 2] = (double)v.z; g[4 * k + 3] = (double)v.w; }
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; k++) g[k] = dn_load(feat, feat_f64, pix * 8 + k);
    }
    DnPix p;
    p.c = v3(0, 0, 0);
    p.a = v3(g[0], g[1], g[2]); p.n = v3(g[3], g[4], g[5]); p.z = g[6]; p.cov = g[7];
    const int Nx = 2 * x + 1 - G.S, Ny = 2 * y + 1 - G.S;
    const int X0 = up_floor_div(Nx, S2), Y0 = up_floor_div(Ny, S2);
    const int cx = X0 - 1 - lx0, cy = Y0 - 1 - ly0;      // halo cell of the first tap: 0 <= cx <= GI_UP_HX - 4, 0 <= cy <= GI_UP_HY - 4
    const double r4 = (double)S4;
    double tx[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int nx = abs(S2 * (X0 - 1 + i) - Nx);
        tx[i] = nx < S4 ? (double)(S4 - nx) / r4 : 0.0;
    }
    TapSum sum;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int ny = abs(S2 * (Y0 - 1 + j) - Ny);
        const double ty = ny < S4 ? (double)(S4 - ny) / r4 : 0.0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const DnPix q = UpTile::cell(lds, (cy + j) * GI_UP_HX + cx + i);
            const bool ok = dn_finite(q.c);        // outside the low frame (NaN from the loader) or a non-finite input: skipped
            sum.add(q, ok ? up_tap_weight(p, q, inv, ty * tx[i]) : 0.0, ok);
        }
    }
    const V3 mf = v3(dn_modulation(p.a.x, demodulate), dn_modulation(p.a.y, demodulate), dn_modulation(p.a.z, demodulate));
    V3 r = v3(0, 0, 0);
    if (sum.den > 0.0) {
        r = sum.mean() * mf;
    } else {
        // every tap rejected: the nearest low pixel.  x / S is X0 or X0 + 1, so it is one of the taps' cells; it lies inside the low frame, so a NaN there is the input's
        const int Xn = min(x / G.S, G.wl - 1), Yn = min(y / G.S, G.hl - 1);
        const DnPix q = UpTile::cell(lds, (Yn - ly0) * GI_UP_HX + (Xn - lx0));
        if (dn_finite(q.c)) r = q.c * mf;
    }
    dn_store3(out, out_f64, pix * 3, r);
}

namespace {

// false + message when the parameters are not the header's
bool up_check(const gi_upsample_params* p, std::string& err)
{
    if (!p) { err = "upsample: null parameters"; return false; }
    if (!filter_size_check("upsample", p->width, p->height, err)) return false;
    if (p->factor < GI_UP_MIN_FACTOR || p->factor > GI_UP_MAX_FACTOR) {
        err = "upsample: factor must be " + std::to_string(GI_UP_MIN_FACTOR) + " .. " + std::to_string(GI_UP_MAX_FACTOR) + ", got " + std::to_string(p->factor);
        return false;
    }
    const int wl = (p->width + p->factor - 1) / p->factor, hl = (p->height + p->factor - 1) / p->factor;
    if (p->low_width != wl || p->low_height != hl) {
        err = "upsample: the low frame of a " + std::to_string(p->width) + " x " + std::to_string(p->height) + " frame at factor " + std::to_string(p->factor) + " is low_width x low_height = " +
              std::to_string(wl) + " x " + std::to_string(hl) + " (the ceilings), got " + std::to_string(p->low_width) + " x " + std::to_string(p->low_height);
        return false;
    }
    const double sg[3] = {p->sigma_normal, p->sigma_depth, p->sigma_albedo};
    const char* names[3] = {"sigma_normal", "sigma_depth", "sigma_albedo"};
    return filter_sigma_check("upsample", names, sg, 3, err);
}

}  // namespace

extern "C" {

void gi_upsample_default_params(gi_upsample_params* p)
{
    if (!p) return;
    p->width = 0; p->height = 0; p->low_width = 0; p->low_height = 0; p->factor = 0;
    p->demodulate = 1;
    p->sigma_normal = 0.5; p->sigma_depth = 0.1; p->sigma_albedo = 0.0;
}

int gi_upsample_device(gi_ctx* c, const gi_upsample_params* p, const void* d_low_color, int low_color_is_f64, const void* d_low_features, int low_features_is_f64,
                       const void* d_features, int features_is_f64, void* d_out, int out_is_f64)
{
    if (!c) return GI_E_INVALID;
    c->up.timer.reset();
    std::string err;
    if (!up_check(p, err)) return fail(c, GI_E_INVALID, err);
    if (!d_low_color || !d_low_features || !d_features || !d_out) return filter_null_pointer(c, "upsample");
    const size_t n_pix = (size_t)p->width * (size_t)p->height, n_low = (size_t)p->low_width * (size_t)p->low_height;
    if (const int rc = filter_pixel_limit(c, "upsample", n_pix)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const int rc = dn_reserve(c, n_low);
    if (rc != GI_OK) return rc;
    HIP_TRY(c, c->up.timer.begin(c->stream));
    const int demod = p->demodulate != 0;
    hipLaunchKernelGGL(k_dn_pack, dim3((unsigned)((n_low * 8 + 255) / 256)), dim3(256), 0, c->stream, n_low, d_low_color, low_color_is_f64, d_low_features, low_features_is_f64, demod,
                       c->dn.d_a.p, c->dn.d_guides.p);
    UpGrid G;
    G.w = p->width; G.h = p->height; G.wl = p->low_width; G.hl = p->low_height; G.S = p->factor;
    G.tiles_x = (p->width + GI_UP_TX - 1) / GI_UP_TX;
    const int tiles_y = (p->height + GI_UP_TY - 1) / GI_UP_TY;
    DnInv inv;
    inv.c = 0.0; inv.n = dn_inv(p->sigma_normal, 1.0); inv.z = dn_inv(p->sigma_depth, 1.0); inv.a = dn_inv(p->sigma_albedo, 1.0);
    hipLaunchKernelGGL(k_up_sample, dim3((unsigned)((size_t)G.tiles_x * tiles_y)), dim3(GI_UP_BLOCK), 0, c->stream, G, inv, c->dn.d_a.p, c->dn.d_guides.p, d_features, features_is_f64,
                       demod, d_out, out_is_f64);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, c->up.timer.end(c->stream));
    return GI_OK;
}

int gi_upsample_host(gi_ctx* c, const gi_upsample_params* p, const void* h_low_color, int low_color_is_f64, const void* h_low_features, int low_features_is_f64,
                     const void* h_features, int features_is_f64, void* h_out, int out_is_f64)
{
    if (!c) return GI_E_INVALID;
    c->up.timer.reset();
    std::string err;
    if (!up_check(p, err)) return fail(c, GI_E_INVALID, err);
    if (!h_low_color || !h_low_features || !h_features || !h_out) return filter_null_pointer(c, "upsample");
    const size_t n_pix = (size_t)p->width * (size_t)p->height, n_low = (size_t)p->low_width * (size_t)p->low_height;
    Entry e(c, "upsample_host", &c->up.timer);
    const unsigned char* d_color = e.in((const unsigned char*)h_low_color, n_low * 3 * (low_color_is_f64 ? 8 : 4));
    const unsigned char* d_low = e.in((const unsigned char*)h_low_features, n_low * 8 * (low_features_is_f64 ? 8 : 4));
    const unsigned char* d_feat = e.in((const unsigned char*)h_features, n_pix * 8 * (features_is_f64 ? 8 : 4));
    unsigned char* d_out = e.out((unsigned char*)h_out, n_pix * 3 * (out_is_f64 ? 8 : 4));
    return e.run([&] { return gi_upsample_device(c, p, d_color, low_color_is_f64, d_low, low_features_is_f64, d_feat, features_is_f64, d_out, out_is_f64); });
}

int gi_last_upsample_ms(gi_ctx* c, float* ms) { return pass_ms(c, &gi_ctx::up, ms); }

}  // extern "C"
