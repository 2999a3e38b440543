"""Expectation of a light bake (gi_bake_*; include/gi_hip.h states the definition), built from the oracle as it is: gio_halton_sample for (u, v),
gio_hemi_cos_n / gio_unit_vec for the directions, Oracle.radiance on explicit rays for L_k, and the two folds in numpy.  Shared by the GPU tests
and the oracle-only tests.

What is exact here and what is not: stream indices, (u, v), Nn, O and the fold are the device's bit for bit (IEEE operations only); the directions go
through sin / cos / acos / sqrt of the host's libm where the device calls OCML's, 4 ulp apart at the most (tests/parity_checks.py: check_kats).  The
GPU tests therefore hand the DEVICE's rays (gi_bake_rays) to Oracle.radiance, so that no edge-grazing ray can land on another entity."""
import ctypes as C

import numpy as np

import oracle_lib as ol

SHADOW_BIAS = 0.0001
TEXEL, SH9 = 0, 1
FOUR_PI = 12.566370614359172
DEFAULT_SEED = ol.DEFAULT_SEED


def streams(n_points, n_samples, stream_base=0):
    """stream = stream_base + i * n_samples + k, row i * n_samples + k; AssertionError when the last does not fit 32 bits."""
    assert stream_base + n_points * n_samples <= 2 ** 32
    return (stream_base + np.arange(n_points * n_samples, dtype=np.uint64)).astype(np.uint32)


def uv(stream):
    """Halton dimensions 0 and 1 at the stream indices, as the floats the sampler returns."""
    L = ol.lib()
    u = np.array([L.gio_halton_sample(0, int(s)) for s in stream], np.float32)
    v = np.array([L.gio_halton_sample(1, int(s)) for s in stream], np.float32)
    return u, v


def unit_normals(normals):
    """Nn = N / sqrt((Nx Nx + Ny Ny) + Nz Nz), per component."""
    N = np.asarray(normals, np.float64).reshape(-1, 3)
    return N / np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])[:, None]


def _ray_dirs(d):
    """Ray(O, d) normalises d once more (include/ray.h: glm::normalize = d * (1 / sqrt(dot(d, d))))."""
    return d * (1.0 / np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]))[:, None]


def texel_rays(points, normals, n_samples, stream_base=0):
    """(rays [n * n_samples][6], streams): O = P + SHADOW_BIAS Nn, d = hemisphereSample_cos(Nn, u, v, 2)."""
    L = ol.lib()
    P = np.asarray(points, np.float64).reshape(-1, 3)
    Nn = unit_normals(normals)
    O = P + SHADOW_BIAS * Nn
    st = streams(len(P), n_samples, stream_base)
    u, v = uv(st)
    d = np.zeros((len(st), 3))
    out = np.zeros(3)
    for j in range(len(st)):
        n3 = np.ascontiguousarray(Nn[j // n_samples])
        L.gio_hemi_cos_n(n3.ctypes.data_as(ol.c_dp), C.c_float(u[j]), C.c_float(v[j]), 2.0, out.ctypes.data_as(ol.c_dp))
        d[j] = out
    return np.concatenate([np.repeat(O, n_samples, 0), _ray_dirs(d)], 1), st


def probe_rays(points, n_samples, stream_base=0):
    """(rays [n * n_samples][6], streams): O = P, d = randomUnitVec((double) u, (double) v)."""
    L = ol.lib()
    P = np.asarray(points, np.float64).reshape(-1, 3)
    st = streams(len(P), n_samples, stream_base)
    u, v = uv(st)
    d = np.zeros((len(st), 3))
    out = np.zeros(3)
    for j in range(len(st)):
        L.gio_unit_vec(float(u[j]), float(v[j]), out.ctypes.data_as(ol.c_dp))
        d[j] = out
    return np.concatenate([np.repeat(P, n_samples, 0), _ray_dirs(d)], 1), st


def sh9_basis(d):
    """Y_j of the header at unit directions d [...][3] -> [...][9]."""
    d = np.asarray(d, np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.stack([np.full(x.shape, 0.28209479177387814), 0.4886025119029199 * y, 0.4886025119029199 * z, 0.4886025119029199 * x,
                     1.0925484305920792 * (x * y), 1.0925484305920792 * (y * z), 0.31539156525252005 * (3.0 * (z * z) - 1.0),
                     1.0925484305920792 * (x * z), 0.5462742152960396 * (x * x - y * y)], -1)


def fold_texel(L):
    """L [n][n_samples][3] -> [n][3]: the sum in ascending k from +0.0, one addition at a time (np.sum adds pairwise), divided by (double) n_samples."""
    L = np.asarray(L, np.float64)
    acc = np.zeros((L.shape[0], 3))
    for k in range(L.shape[1]):
        acc = acc + L[:, k]
    return acc / float(L.shape[1])


def fold_sh9(L, d):
    """L, d [n][n_samples][3] -> [n][9][3]: acc[j][c] += L_k[c] Y_j(d_k) in ascending k, then (acc * 4 pi) / (double) n_samples."""
    L = np.asarray(L, np.float64)
    Y = sh9_basis(d)
    acc = np.zeros((L.shape[0], 9, 3))
    for k in range(L.shape[1]):
        acc = acc + L[:, k][:, None, :] * Y[:, k][:, :, None]
    return (acc * FOUR_PI) / float(L.shape[1])


def fold(mode, L, d=None):
    return fold_texel(L) if mode == TEXEL else fold_sh9(L, d)


def expected_bake(oracle, mode, rays, stream, n_samples, seed=DEFAULT_SEED):
    """The bake of the points whose rays are given (row i * n_samples + k): the fold of Oracle.radiance on them."""
    L = oracle.radiance(rays, stream, seed).reshape(-1, n_samples, 3)
    return fold(mode, L, np.asarray(rays)[:, 3:6].reshape(-1, n_samples, 3))


def bake(oracle, mode, points, normals, n_samples, stream_base=0, seed=DEFAULT_SEED):
    """The whole statement from the oracle alone."""
    rays, st = texel_rays(points, normals, n_samples, stream_base) if mode == TEXEL else probe_rays(points, n_samples, stream_base)
    return expected_bake(oracle, mode, rays, st, n_samples, seed)


# ---- test points
def surface_points(oracle, w=6, h=4):
    """The first hits of a w x h oracle frame (sample 0): positions on real surfaces and their normals, turned towards the camera."""
    rays = np.array([oracle.primary_ray(w, h, 0, x, y)[1] for y in range(h) for x in range(w)])
    hit, ent, res, _ = oracle.trace(rays)
    m = hit.astype(bool)
    P, N = res[m, 0:3], res[m, 3:6]
    back = (N * rays[m, 3:6]).sum(1) > 0
    return np.ascontiguousarray(P), np.ascontiguousarray(np.where(back[:, None], -N, N))


def probe_points(tables):
    """Six probes in free space inside the octree's root box and one outside it."""
    b = tables["node_bbox"][0]
    lo, ext = b[0:3], b[3:6] - b[0:3]
    f = np.array([[0.5, 0.5, 0.5], [0.3, 0.6, 0.4], [0.7, 0.55, 0.45], [0.45, 0.8, 0.6], [0.6, 0.35, 0.7], [0.35, 0.45, 0.3], [1.4, 0.5, 0.5]])
    return np.ascontiguousarray(lo + f * ext)


def ambient_floor_scene(gi, ambient):
    """One large floor quad at y = 0 under an ambient term: a ray that starts below it and looks down meets nothing."""
    s = gi.Scene()
    white = s.add_material(1, 1, 1, (0.8, 0.8, 0.8))
    a, b, c, d = (-50, 0, -50), (-50, 0, 50), (50, 0, 50), (50, 0, -50)
    s.add_triangles(np.array([[a, b, c], [a, c, d]], float), mat_idx=[white, white])
    s.add_light((0, 20, 0), (1, 1, 1), 0.1)
    s.set_ambient(ambient)
    s.set_camera((0.3, 6.0, 4.0), (0, 0, 0))
    return s.rebuild()
