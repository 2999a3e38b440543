"""Expectation of the ambient-occlusion / bent-normal pass (gi_render_occlusion_*; include/gi_hip.h states the definition), built from the oracle as
it is: Oracle.primary_ray for the rays and Halton indices, Oracle.trace for the hit point and normal, the oracle's counter RNG (gio_counter_rand) and
cosine hemisphere sampler (gio_hemi_cos_n) for the directions, Oracle.visible on the rows (O, T_j) for the segments.  Shared by the GPU tests and
the oracle-only tests.

Valid for scenes whose alpha test cannot depend on the draw (features_expect.DRAW_FREE_SCENES): Oracle.trace and Oracle.visible draw with seed 0 and
stream = row number, the pass with the frame's seed and the Halton index.

What is exact here and what is not: hit point, normal, O and the RNG draws are the device's bit for bit (the feature pass's tests pin the first
three, gi_kat 8 the fourth); the hemisphere sampler calls sin / cos / sqrt of the host's libm where the device calls OCML's, 4 ulp apart at the most
(tests/parity_checks.py: check_kats), so T_j and the bent vector carry that, and a segment that grazes an edge within it may flip."""
import ctypes as C

import numpy as np

import features_expect as fe
import oracle_lib as ol

SHADOW_BIAS = 0.0001
P_AO_U, P_AO_V = 32, 33
DEFAULT_SEED = ol.DEFAULT_SEED


def default_radius(tables):
    """What radius = 0 stands for: a tenth of the diagonal of the octree's root box, 0.1 sqrt((dx dx + dy dy) + dz dz)."""
    b = tables["node_bbox"][0]
    dx, dy, dz = float(b[3] - b[0]), float(b[4] - b[1]), float(b[5] - b[2])
    return 0.1 * float(np.sqrt((dx * dx + dy * dy) + dz * dz))


def scene_diagonal(tables):
    b = tables["node_bbox"][0]
    return float(np.linalg.norm(b[3:6] - b[0:3]))


def directions(nf, idx, dirs, seed=DEFAULT_SEED):
    """d_j = hemisphereSample_cos(Nf, u, v, 1) with u = (float) draw(seed, stream idx, depth 0, purpose 32, a = j), v likewise with purpose 33:
    [n][dirs][3] for normals nf [n][3] and Halton indices idx [n]."""
    L = ol.lib()
    out = np.zeros((len(nf), dirs, 3))
    d = np.zeros(3)
    for i in range(len(nf)):
        n3 = np.ascontiguousarray(nf[i], np.float64)
        for j in range(dirs):
            u = np.float32(L.gio_counter_rand(C.c_uint64(seed), int(idx[i]), 0, P_AO_U, j, 0))
            v = np.float32(L.gio_counter_rand(C.c_uint64(seed), int(idx[i]), 0, P_AO_V, j, 0))
            L.gio_hemi_cos_n(n3.ctypes.data_as(ol.c_dp), C.c_float(u), C.c_float(v), 1.0, d.ctypes.data_as(ol.c_dp))
            out[i, j] = d
    return out


def sample_geometry(oracle, w, h, s, dirs, seed=DEFAULT_SEED):
    """What does not depend on the radius, for sample s of every pixel (row-major): hit [n] bool, ent [n], O [n][3], Nf [n][3], d [n][dirs][3]
    (rows of misses are 0)."""
    rays, idx = fe.sample_rays(oracle, w, h, s)
    hit, ent, res, _ = oracle.trace(rays)
    hit = hit.astype(bool)
    N = res[:, 3:6]
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
        nh = N * inv[:, None]
    dn = (nh[:, 0] * rays[:, 3] + nh[:, 1] * rays[:, 4]) + nh[:, 2] * rays[:, 5]
    nf = np.where((dn > 0)[:, None], -nh, nh)
    nf = np.where(hit[:, None], nf, 0.0)
    O = np.where(hit[:, None], res[:, 0:3] + SHADOW_BIAS * nf, 0.0)
    d = np.zeros((len(rays), dirs, 3))
    hi = np.flatnonzero(hit)
    d[hi] = directions(nf[hi], idx[hi], dirs, seed)
    return {"hit": hit, "ent": np.where(hit, ent, -1).astype(np.int32), "O": O, "Nf": nf, "d": d}


def segment_rows(g, radius):
    """The rows (O, T_j) of Oracle.visible / gi_visible for the hit pixels of a sample, [n_hit * dirs][6], T_j = O + radius d_j."""
    hi = np.flatnonzero(g["hit"])
    O = np.repeat(g["O"][hi][:, None, :], g["d"].shape[1], axis=1)
    T = O + radius * g["d"][hi]
    return np.concatenate([O, T], 2).reshape(-1, 6)


def sample_open(oracle, g, radius, rows=None):
    """open [n][dirs] bool of a sample: Oracle.visible on its rows (misses: all open, they are not asked)."""
    n, dirs = g["d"].shape[:2]
    op = np.ones((n, dirs), bool)
    hi = np.flatnonzero(g["hit"])
    if len(hi):
        vis, _ = oracle.visible(segment_rows(g, radius) if rows is None else rows)
        op[hi] = vis.reshape(len(hi), dirs).astype(bool)
    return op


def sample_values(g, op):
    """(count [n] int, open_s [n], bent_s [n][3]) of a sample: open_s = count / dirs, bent_s = (sum of d_j over the open j, ascending) / dirs; a miss has
    openness 1 and bent 0."""
    n, dirs = op.shape
    bent = np.zeros((n, 3))
    for j in range(dirs):                       # ascending j, one addition at a time (np.sum adds pairwise)
        bent = bent + np.where(op[:, j][:, None], g["d"][:, j], 0.0)
    cnt = op.sum(1)
    hit = g["hit"]
    open_s = np.where(hit, cnt / float(dirs), 1.0)
    bent_s = np.where(hit[:, None], bent / float(dirs), 0.0)
    return np.where(hit, cnt, dirs).astype(np.int64), open_s, bent_s


def expected_occlusion(oracle, w, h, n, dirs, radius, seed=DEFAULT_SEED, geometry=None):
    """The pass on a whole w x h frame: occ [h][w][4] = openness, bent xyz (the f64 sums over s in ascending order, divided once by n), counts
    [n][h][w] open segments per (sample, pixel) (dirs on a miss), hit [n][h][w], ent [n][h][w].  geometry: sample_geometry of samples 0 .. n-1,
    when the caller has it already (it does not depend on the radius)."""
    acc = np.zeros((h * w, 4))
    counts, hits, ents = [], [], []
    for s in range(n):
        g = geometry[s] if geometry is not None else sample_geometry(oracle, w, h, s, dirs, seed)
        cnt, open_s, bent_s = sample_values(g, sample_open(oracle, g, radius))
        acc = acc + np.concatenate([open_s[:, None], bent_s], 1)
        counts.append(cnt.reshape(h, w)); hits.append(g["hit"].reshape(h, w)); ents.append(g["ent"].reshape(h, w))
    return {"occlusion": (acc / float(n)).reshape(h, w, 4), "counts": np.array(counts), "hit": np.array(hits), "ent": np.array(ents)}


def flips_under_perturbation(oracle, g, radius, ulps=4):
    """How many segments of a sample change their answer when every coordinate of T_j moves by `ulps` ulp, up or down (the allowance between the
    host's and the device's hemisphere sampler): the room the oracle has on these rows.  Returns (flipped, asked)."""
    rows = segment_rows(g, radius)
    if not len(rows):
        return 0, 0
    base, _ = oracle.visible(rows)
    flipped = np.zeros(len(rows), bool)
    for sign in (+1.0, -1.0):
        q = rows.copy()
        q[:, 3:6] = q[:, 3:6] + sign * ulps * np.spacing(np.abs(q[:, 3:6]))
        vis, _ = oracle.visible(q)
        flipped |= vis != base
    return int(flipped.sum()), len(rows)


# ---- analytic scenes (built with the product's host builders, which need no GPU)
def floor_scene(gi):
    """One large floor quad at y = 0, seen from above."""
    s = gi.Scene()
    white = s.add_material(1, 1, 1, (0.8, 0.8, 0.8))
    a, b, c, d = (-50, 0, -50), (-50, 0, 50), (50, 0, 50), (50, 0, -50)
    s.add_triangles(np.array([[a, b, c], [a, c, d]], float), mat_idx=[white, white])
    s.add_light((0, 20, 0), (1, 1, 1), 0.1)
    s.set_camera((0.3, 6.0, 4.0), (0, 0, 0))
    return s.rebuild()


BOX_LO, BOX_HI = (-2.0, -1.5, -2.5), (2.0, 1.5, 2.5)


def closed_box_scene(gi):
    """A closed box of twelve triangles with the camera inside."""
    s = gi.Scene()
    white = s.add_material(1, 1, 1, (0.8, 0.8, 0.8))
    (x0, y0, z0), (x1, y1, z1) = BOX_LO, BOX_HI
    faces = [((x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0)), ((x0, y0, z1), (x0, y1, z1), (x1, y1, z1), (x1, y0, z1)),
             ((x0, y0, z0), (x0, y1, z0), (x0, y1, z1), (x0, y0, z1)), ((x1, y0, z0), (x1, y0, z1), (x1, y1, z1), (x1, y1, z0)),
             ((x0, y1, z0), (x1, y1, z0), (x1, y1, z1), (x0, y1, z1)), ((x0, y0, z0), (x0, y0, z1), (x1, y0, z1), (x1, y0, z0))]
    tris = []
    for (a, b, c, d) in faces:
        tris.extend([[a, b, c], [a, c, d]])
    s.add_triangles(np.array(tris, float), mat_idx=[white] * len(tris))
    s.add_light((0, 1.0, 0), (1, 1, 1), 0.1)
    s.set_camera((0.3, 0.2, 1.9), (-0.4, -0.1, -2.5))
    return s.rebuild()


BOX_DIAGONAL = float(np.linalg.norm(np.array(BOX_HI) - np.array(BOX_LO)))
