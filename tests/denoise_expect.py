"""Expectation of the edge-avoiding a-trous denoiser (gi_denoise_*): the filter's formula in numpy f64, IEEE operations only (+ - * /, compares,
selects), in the order the header states them -- the tap loop runs dy from -2 to 2 outer, dx from -2 to 2 inner, and every sum is added in
that order, so a device build without contraction gives the same bits.  Shared by the GPU tests and the CPU-only property tests.

    color    [h][w][3]  linear radiance (f32 or f64; widened first)
    features [h][w][8]  albedo rgb, normal xyz, depth, coverage (the layout of gi_render_features_*)
"""
import numpy as np

DEFAULTS = dict(iterations=5, demodulate=1, sigma_color=1.0, sigma_normal=0.5, sigma_depth=0.1, sigma_albedo=0.25)
H5 = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)
ALBEDO_FLOOR = 1e-3
DC_EPS = 1e-12
ULP = 2.0 ** -52


def margin(iterations):
    """How far a pixel's result reaches into the frame: 2 taps of step 2^i on each level."""
    return 2 * ((1 << iterations) - 1)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def inv_sigmas(p, level):
    """The four factors of d, computed once in double: 4^level / sigma_color^2 (the colour sigma halves per level), 1 / sigma^2 for the
    others; a sigma of 0 switches its term off."""
    def inv(s, scale=1.0):
        return scale / (s * s) if s != 0 else 0.0
    return inv(p["sigma_color"], float(4 ** level)), inv(p["sigma_normal"]), inv(p["sigma_depth"]), inv(p["sigma_albedo"])


def sq3(v):
    return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]


def modulation(features, demodulate):
    a = features[..., 0:3]
    return np.where(a > ALBEDO_FLOOR, a, ALBEDO_FLOOR) if demodulate else np.ones_like(a)


def level(c, g, step, inv):
    """One a-trous level on the demodulated colour c [h][w][3] with guides g [h][w][8]."""
    h, w = c.shape[:2]
    inv_c, inv_n, inv_z, inv_a = inv
    fin = np.isfinite(c).all(-1)
    num = np.zeros((h, w, 3))
    den = np.zeros((h, w))
    with np.errstate(all="ignore"):
        c2 = sq3(c)
        for dy in range(-2, 3):
            oy = dy * step
            py = slice(max(0, -oy), min(h, h - oy))
            if py.start >= py.stop:
                continue
            qy = slice(py.start + oy, py.stop + oy)
            for dx in range(-2, 3):
                ox = dx * step
                px = slice(max(0, -ox), min(w, w - ox))
                if px.start >= px.stop:
                    continue
                qx = slice(px.start + ox, px.stop + ox)
                cp, cq = c[py, px], c[qy, qx]
                gp, gq = g[py, px], g[qy, qx]
                dc = np.where(fin[py, px], sq3(cp - cq) / (c2[py, px] + (c2[qy, qx] + DC_EPS)), 0.0)
                dn = sq3(gp[..., 3:6] - gq[..., 3:6])
                dcov = gp[..., 7] - gq[..., 7]
                da = sq3(gp[..., 0:3] - gq[..., 0:3]) + dcov * dcov
                zs = gp[..., 6] + gq[..., 6]
                r = np.where(zs > 0, (gp[..., 6] - gq[..., 6]) / np.where(zs > 0, zs, 1.0), 0.0)
                dz = r * r
                d = ((dc * inv_c + dn * inv_n) + dz * inv_z) + da * inv_a
                t = np.where(d < 1.0, 1.0 - d, 0.0)          # 1 - min(d, 1); a NaN d counts as 1
                wgt = (H5[dy + 2] * H5[dx + 2]) * (t * t)
                ok = fin[qy, qx]                              # a tap with a non-finite channel is skipped
                wgt = np.where(ok, wgt, 0.0)
                num[py, px] += wgt[..., None] * np.where(ok[..., None], cq, 0.0)
                den[py, px] += wgt
        return np.where((den > 0)[..., None], num / np.where(den > 0, den, 1.0)[..., None], 0.0)


def expected(color, features, out_dtype=np.float64, **kw):
    """The whole pass.  Inputs of either float type are widened; the f64 result is rounded once to out_dtype."""
    p = params(**kw)
    color = np.asarray(color)
    if p["iterations"] == 0:
        return color.astype(out_dtype)
    g = np.asarray(features).astype(np.float64)
    m = modulation(g, p["demodulate"])
    with np.errstate(all="ignore"):
        c = color.astype(np.float64) / m
        for i in range(p["iterations"]):
            c = level(c, g, 1 << i, inv_sigmas(p, i))
        return (c * m).astype(out_dtype)


def expected_window(color, features, x0, y0, ww, wh, out_dtype=np.float64, **kw):
    """expected(...)[y0:y0+wh, x0:x0+ww] from a crop with a margin of 2 (2^iterations - 1) pixels, cut at the frame's edges -- for frames too
    large to evaluate whole.  Beyond the margin nothing reaches the window, and where the crop ends at the frame's edge the taps are the
    frame's own missing taps."""
    p = params(**kw)
    h, w = np.asarray(color).shape[:2]
    mg = margin(p["iterations"])
    xa, ya = max(0, x0 - mg), max(0, y0 - mg)
    xb, yb = min(w, x0 + ww + mg), min(h, y0 + wh + mg)
    full = expected(np.asarray(color)[ya:yb, xa:xb], np.asarray(features)[ya:yb, xa:xb], out_dtype, **p)
    return full[y0 - ya:y0 - ya + wh, x0 - xa:x0 - xa + ww]


def synthetic(w, h, seed=1, noise=0.5):
    """A seeded test frame: two surfaces with orthogonal normals meeting at a slanted edge, a checker albedo, a background strip on the right
    (coverage 0, everything 0), fractional coverage on the strip's border, and gamma-distributed noise on the colour.
    Returns (noisy colour, features, clean colour)."""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    feat = np.zeros((h, w, 8))
    left = x + 0.3 * y < 0.55 * w
    check = ((x // 5 + y // 4) % 2).astype(bool)
    feat[..., 0:3] = np.where(check[..., None], [0.8, 0.7, 0.2], [0.15, 0.3, 0.6])
    feat[..., 3:6] = np.where(left[..., None], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0])
    feat[..., 6] = np.where(left, 4.0 + 0.02 * y, 6.0 + 0.01 * x)
    feat[..., 7] = 1.0
    bg = x >= w - max(1, w // 6)
    edge = (x == w - max(1, w // 6) - 1) & (w > 2)
    feat[edge] *= 0.5
    feat[bg] = 0.0
    light = np.where(left, 1.5, 0.4)[..., None] * (1.0 + 0.2 * np.sin(x / 9.0))[..., None]
    clean = feat[..., 0:3] * light
    clean[bg] = [0.05, 0.05, 0.08]
    noisy = clean * rs.gamma(1.0 / max(noise, 1e-6), max(noise, 1e-6), size=(h, w, 1)) if noise > 0 else clean.copy()
    return noisy, feat, clean


def rmse(a, b, mask=None):
    d = (np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2
    if mask is not None:
        d = d[mask]
    return float(np.sqrt(d.mean()))
