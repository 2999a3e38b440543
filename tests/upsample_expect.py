"""Expectation of the guided upsampler (gi_upsample_*): the formula of include/gi_hip.h in numpy f64, IEEE operations only (+ - * /, compares,
selects), in the order the header states them -- the 16 taps run Y from Y0-1 to Y0+2 outer, X from X0-1 to X0+2 inner, and every sum is added in
that order, so a device build without contraction gives the same bits.  Shared by the GPU tests and the CPU-only property tests.

    low_color    [hl][wl][3]  linear radiance of the reduced-size frame (f32 or f64; widened first)
    low_features [hl][wl][8]  its feature buffers: albedo rgb, normal xyz, depth, coverage (the layout of gi_render_features_*)
    features     [h][w][8]    the full-size feature buffers; wl = ceil(w / factor), hl = ceil(h / factor)
"""
import numpy as np

import denoise_expect as de

DEFAULTS = dict(demodulate=1, sigma_normal=0.5, sigma_depth=0.1, sigma_albedo=0.0)
MIN_FACTOR, MAX_FACTOR = 2, 8


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def inv_sigmas(p):
    """1 / sigma^2 per term, computed once in double; a sigma of 0 switches its term off."""
    def inv(s):
        return 1.0 / (s * s) if s != 0 else 0.0
    return inv(p["sigma_normal"]), inv(p["sigma_depth"]), inv(p["sigma_albedo"])


def low_size(w, h, factor):
    return -(-w // factor), -(-h // factor)


def box_reduce(a, factor):
    """The mean of every factor x factor block of a [h][w][k] (ragged blocks at the right and bottom edges take the pixels they have): a
    stand-in for a reduced-size render of the same view."""
    h, w = a.shape[:2]
    wl, hl = low_size(w, h, factor)
    out = np.zeros((hl, wl) + a.shape[2:])
    for Y in range(hl):
        for X in range(wl):
            out[Y, X] = a[Y * factor:(Y + 1) * factor, X * factor:(X + 1) * factor].reshape((-1,) + a.shape[2:]).mean(0)
    return out


def nearest(low, w, h, factor):
    """Nearest-pixel replication of a low frame to w x h."""
    y, x = np.mgrid[0:h, 0:w]
    return np.asarray(low)[np.minimum(y // factor, low.shape[0] - 1), np.minimum(x // factor, low.shape[1] - 1)]


def expected(low_color, low_features, features, factor, out_dtype=np.float64, **kw):
    """The whole pass.  Inputs of either float type are widened; the f64 result is rounded once to out_dtype."""
    p = params(**kw)
    S = int(factor)
    gl = np.asarray(low_features).astype(np.float64)
    gf = np.asarray(features).astype(np.float64)
    h, w = gf.shape[:2]
    hl, wl = gl.shape[:2]
    assert MIN_FACTOR <= S <= MAX_FACTOR and (wl, hl) == low_size(w, h, S) and np.asarray(low_color).shape == (hl, wl, 3)
    inv_n, inv_z, inv_a = inv_sigmas(p)
    ml, mf = de.modulation(gl, p["demodulate"]), de.modulation(gf, p["demodulate"])
    with np.errstate(all="ignore"):
        c = np.asarray(low_color).astype(np.float64) / ml
        fin = np.isfinite(c).all(-1)
        y, x = np.mgrid[0:h, 0:w]
        Nx, Ny = 2 * x + 1 - S, 2 * y + 1 - S
        X0, Y0 = Nx // (2 * S), Ny // (2 * S)             # numpy's // on integers is floor division, also below zero
        num = np.zeros((h, w, 3))
        den = np.zeros((h, w))
        for j in range(-1, 3):
            Y = Y0 + j
            ny = np.abs(2 * S * Y - Ny)
            ty = np.where(ny < 4 * S, (4 * S - ny).astype(np.float64) / float(4 * S), 0.0)
            for i in range(-1, 3):
                X = X0 + i
                nx = np.abs(2 * S * X - Nx)
                tx = np.where(nx < 4 * S, (4 * S - nx).astype(np.float64) / float(4 * S), 0.0)
                inside = (X >= 0) & (X < wl) & (Y >= 0) & (Y < hl)
                Yc, Xc = np.clip(Y, 0, hl - 1), np.clip(X, 0, wl - 1)
                gq, cq = gl[Yc, Xc], c[Yc, Xc]
                ok = inside & fin[Yc, Xc]                 # taps outside the low frame and taps with a non-finite channel are skipped
                dn = de.sq3(gf[..., 3:6] - gq[..., 3:6])
                dcov = gf[..., 7] - gq[..., 7]
                da = de.sq3(gf[..., 0:3] - gq[..., 0:3]) + dcov * dcov
                zs = gf[..., 6] + gq[..., 6]
                r = np.where(zs > 0, (gf[..., 6] - gq[..., 6]) / np.where(zs > 0, zs, 1.0), 0.0)
                dz = r * r
                d = (dn * inv_n + dz * inv_z) + da * inv_a
                e = np.where(d < 1.0, 1.0 - d, 0.0)       # 1 - min(d, 1); a NaN d counts as 1
                wgt = np.where(ok, (ty * tx) * (e * e), 0.0)
                num += wgt[..., None] * np.where(ok[..., None], cq, 0.0)
                den += wgt
        Yn, Xn = np.minimum(y // S, hl - 1), np.minimum(x // S, wl - 1)
        near = np.where(fin[Yn, Xn][..., None], c[Yn, Xn] * mf, 0.0)
        out = np.where((den > 0)[..., None], (num / np.where(den > 0, den, 1.0)[..., None]) * mf, near)
        return out.astype(out_dtype)


def tent(low_color, w, h, factor):
    """A plain tent interpolation of the low frame: the same formula with every sigma 0 and without demodulation (the features play no part)."""
    low_color = np.asarray(low_color)
    wl, hl = low_size(w, h, factor)
    return expected(low_color, np.zeros((hl, wl, 8)), np.zeros((h, w, 8)), factor, demodulate=0, sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0)
