"""Expectation of a reflection probe (gi_cubemap_*; include/gi_hip.h states the definition): the texels' directions, the capture's rays from
gio_halton_sample's (u, v), the box levels and the lobe filter, in numpy, and the capture as the texel fold of Oracle.radiance.  Shared by the GPU
tests and the oracle-only tests.

Everything here is IEEE + - * / and sqrt in the header's order, so it is the device's bit for bit: the capture's rays too (no trigonometry).  np.sum
adds pairwise, so every sum below is a loop of single additions.  The filter loops over the source texels of a face in ascending order, vectorised
over the output texels, and adds the six faces in order."""
import numpy as np

import bake_expect as be

MAX_LEVELS = 12
DEFAULT_SEED = be.DEFAULT_SEED


def default_exponents():
    return [max(0, 16 - 3 * l) for l in range(MAX_LEVELS)]


def texel_fyx(n):
    """(f, y, x) of the texels t = (f n + y) n + x of a cube of face n, in ascending t."""
    t = np.arange(6 * n * n)
    return t // (n * n), (t // n) % n, t % n


def coords(n, ju=0.5, jv=0.5):
    """(f, a, b) per texel in ascending t; ju, jv: scalars or one value per texel."""
    f, y, x = texel_fyx(n)
    a = (2.0 * (x.astype(np.float64) + ju)) / float(n) - 1.0
    b = (2.0 * (y.astype(np.float64) + jv)) / float(n) - 1.0
    return f, a, b


def face_dirs(f, a, b):
    """The unnormalised direction of (a, b) on face f, [len][3]."""
    one = np.ones_like(a)
    table = [(one, -b, -a), (-one, -b, a), (a, one, b), (a, -one, -b), (a, -b, one), (-a, -b, -one)]
    out = np.zeros((len(a), 3))
    for g, cols in enumerate(table):
        m = f == g
        for k in range(3):
            out[m, k] = cols[k][m]
    return out


def unit(u):
    """u * (1.0 / sqrt((ux ux + uy uy) + uz uz))."""
    return u * (1.0 / np.sqrt((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]))[:, None]


def directions(n, ju=0.5, jv=0.5):
    """Unnormalised texel directions [6 n n][3]."""
    return face_dirs(*coords(n, ju, jv))


def measure(a, b):
    r = (1.0 + a * a) + b * b
    return 1.0 / (r * np.sqrt(r))


def weight(R, d, m, e):
    """The lobe weight of one source texel (d [3], m) for the output directions R [n][3]."""
    c = (R[:, 0] * d[0] + R[:, 1] * d[1]) + R[:, 2] * d[2]
    w = np.where(c > 0, c, 0.0)
    for _ in range(e):
        w = w * w
    return w * m


def capture_rays(pos, n, n_samples, stream_base=0):
    """(rays [6 n n n_samples][6], streams): sample k of texel t in row t * n_samples + k; origin pos, direction through the texel at the jitter
    (double) halton(0, stream), (double) halton(1, stream), normalised as Ray does."""
    st = be.streams(6 * n * n, n_samples, stream_base)
    u, v = be.uv(st)
    f, y, x = (np.repeat(q, n_samples) for q in texel_fyx(n))
    a = (2.0 * (x.astype(np.float64) + u.astype(np.float64))) / float(n) - 1.0
    b = (2.0 * (y.astype(np.float64) + v.astype(np.float64))) / float(n) - 1.0
    d = unit(face_dirs(f, a, b))
    P = np.asarray(pos, np.float64).reshape(1, 3)
    return np.concatenate([np.repeat(P, len(st), 0), d], 1), st


def box_level(src):
    """B_l [6][n][n][3] from B_(l-1) [6][2 n][2 n][3]: ((p00 + p01) + (p10 + p11)) * 0.25."""
    return ((src[:, 0::2, 0::2] + src[:, 0::2, 1::2]) + (src[:, 1::2, 0::2] + src[:, 1::2, 1::2])) * 0.25


def filter_level(src, e):
    """F_l [6][n][n][3] from B_(l-1) = src [6][2 n][2 n][3] with the lobe squared e times."""
    ns = src.shape[1]
    n = ns // 2
    L = np.asarray(src, np.float64).reshape(-1, 3)
    R = unit(directions(n))
    f, a, b = coords(ns)
    d, m = unit(face_dirs(f, a, b)), measure(a, b)
    per_face = ns * ns
    W_all, A_all = None, None
    for g in range(6):
        W, A = np.zeros(len(R)), np.zeros((len(R), 3))
        for s in range(g * per_face, (g + 1) * per_face):
            w = weight(R, d[s], m[s], e)
            W = W + w
            A = A + w[:, None] * L[s]
        W_all, A_all = (W, A) if g == 0 else (W_all + W, A_all + A)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (A_all / W_all[:, None]).reshape(6, n, n, 3)


def prefilter(cube, levels, exponents=None):
    """The chain [F_0 .. F_(levels-1)] of the cube [6][N][N][3]."""
    e = default_exponents() if exponents is None else list(exponents)
    B = np.ascontiguousarray(cube, np.float64)
    out = [B.copy()]
    for l in range(1, levels):
        out.append(filter_level(B, e[l]))
        B = box_level(B)
    return out


def expected_capture(oracle, rays, streams, n_samples, seed=DEFAULT_SEED):
    """The capture whose rays are given (row t * n_samples + k), [6 n n][3]: the texel fold of Oracle.radiance on them."""
    return be.fold_texel(oracle.radiance(rays, streams, seed).reshape(-1, n_samples, 3))


def mixed_cube(n, seed):
    """Radiance of mixed magnitudes, 10^-12 .. 10^8, a tenth of it zero."""
    rs = np.random.RandomState(seed)
    L = rs.rand(6, n, n, 3) * 10.0 ** rs.randint(-12, 9, (6, n, n, 1))
    L[rs.rand(6, n, n) < 0.1] = 0.0
    return L


def root_box_middle(tables):
    b = tables["node_bbox"][0]
    return np.ascontiguousarray(b[0:3] + 0.5 * (b[3:6] - b[0:3]))
