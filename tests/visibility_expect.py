"""Expectation of probe visibility (gi_probe_visibility_*, gi_render_baked_visibility_*; include/gi_hip.h states the definition): the numpy statement of
the octahedral map, the capture's rays, its distances and fold, the bilinear value of a map, and step 4 of the baked-light pass with the eight
probes weighted by a back-face term and a Chebyshev test.  Shared by the GPU tests and the CPU tests.

Every operation is written in the header's order, one IEEE operation at a time (np.sum adds pairwise, so every sum is a loop of single additions), so
that given identical first hits the values are the device's bit for bit.  The capture's distances come from Oracle.trace on the statement's rays:
valid for scenes whose alpha test cannot depend on the draw (features_expect.DRAW_FREE_SCENES)."""
import numpy as np

import bake_expect as bake
import baked_expect as be

DEFAULT_SEED = bake.DEFAULT_SEED
TW_FLOOR, WB_BASE = 0.001, 0.2
DEFAULT_FLOOR = 0.05


# ---------------------------------------------------------------------------------------------------------------- the octahedral map
def sgn(q):
    return np.where(q >= 0.0, 1.0, -1.0)


def _fold(px, py):
    return (1.0 - np.abs(py)) * sgn(px), (1.0 - np.abs(px)) * sgn(py)


def decode(a, b):
    """The unnormalised direction [...][3] of (a, b) in [0, 1]^2."""
    a, b = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64))
    px = 2.0 * a - 1.0
    py = 2.0 * b - 1.0
    vz = (1.0 - np.abs(px)) - np.abs(py)
    fx, fy = _fold(px, py)
    low = vz < 0.0
    return np.stack([np.where(low, fx, px), np.where(low, fy, py), vz], -1)


def encode(v):
    """(a, b) of the vectors v [...][3], none 0 0 0."""
    v = np.asarray(v, np.float64)
    s = (np.abs(v[..., 0]) + np.abs(v[..., 1])) + np.abs(v[..., 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        px = v[..., 0] / s
        py = v[..., 1] / s
    fx, fy = _fold(px, py)
    low = v[..., 2] < 0.0
    px, py = np.where(low, fx, px), np.where(low, fy, py)
    return (px + 1.0) * 0.5, (py + 1.0) * 0.5


# ---------------------------------------------------------------------------------------------------------------- the capture
def capture_rays(points, M, n_samples, stream_base=0):
    """(rays [n M M n_samples][6], streams): sample k of texel t = (i M + y) M + x in row t * n_samples + k; origin P_i, direction decode(a, b) at
    the jitter (double) halton(0, stream), (double) halton(1, stream), normalised as Ray does."""
    P = np.asarray(points, np.float64).reshape(-1, 3)
    st = bake.streams(len(P) * M * M, n_samples, stream_base)
    u, v = bake.uv(st)
    t = np.repeat(np.arange(len(P) * M * M), n_samples)
    x, y, i = t % M, (t // M) % M, t // (M * M)
    a = (x.astype(np.float64) + u.astype(np.float64)) / float(M)
    b = (y.astype(np.float64) + v.astype(np.float64)) / float(M)
    d = decode(a, b)
    d = d * (1.0 / np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]))[:, None]
    return np.concatenate([P[i], d], 1), st


def distances(hit, res, rays, max_dist):
    """r per ray from a trace's answer (hit [n], res [n][8] with the hit point first): the hit's distance from the ray's origin, max_dist on a
    miss, never more than max_dist."""
    dx, dy, dz = (res[:, k] - rays[:, k] for k in range(3))
    r = np.where(np.asarray(hit).astype(bool), np.sqrt((dx * dx + dy * dy) + dz * dz), max_dist)
    return np.where(r < max_dist, r, max_dist)


def fold(dist):
    """dist [n_texels][n_samples] -> [n_texels][2]: m = sum(r_k) / n, m2 = sum(r_k r_k) / n, the sums in ascending k from +0.0."""
    dist = np.asarray(dist, np.float64)
    s1, s2 = np.zeros(len(dist)), np.zeros(len(dist))
    for k in range(dist.shape[1]):
        s1 = s1 + dist[:, k]
        s2 = s2 + dist[:, k] * dist[:, k]
    n = float(dist.shape[1])
    return np.stack([s1 / n, s2 / n], 1)


def expected_maps(oracle, points, M, n_samples, max_dist, stream_base=0):
    """(maps [n][M][M][2], rays, (hit, ent, res)) of the whole statement from the oracle alone."""
    rays, _ = capture_rays(points, M, n_samples, stream_base)
    hit, ent, res, _ = oracle.trace(rays)
    d = distances(hit, res, rays, max_dist)
    return fold(d.reshape(-1, n_samples)).reshape(-1, M, M, 2), rays, (hit, ent, res)


def probe_points(tables):
    """The test probes: bake_expect.probe_points (six in free space inside the octree's root box, one outside it) moved off the box's middle and
    its symmetry planes by a small fixed fraction of its size -- from the middle of the Cornell box a texel's ray runs into the diagonal a wall's
    two triangles share, where a 4-ulp move of the direction changes the entity (tests/test_visibility_cpu.py shows that from here none does)."""
    b = tables["node_bbox"][0]
    return np.ascontiguousarray(bake.probe_points(tables) + np.array([0.017, 0.029, -0.023]) * (b[3:6] - b[0:3]))


def hits_flip_under_perturbation(oracle, rays, ulps=4):
    """How many of the rays meet another entity (or none) when every component of the direction moves by `ulps` ulp, up or down: the room the
    statement has at these probe positions.  Returns (flipped, asked)."""
    rays = np.asarray(rays, np.float64)
    base_hit, base_ent = oracle.trace(rays)[:2]
    flipped = np.zeros(len(rays), bool)
    for sx in (1.0, -1.0):
        for sy in (1.0, -1.0):
            for sz in (1.0, -1.0):
                moved = rays.copy()
                moved[:, 3:6] = rays[:, 3:6] + np.array([sx, sy, sz]) * ulps * np.spacing(np.abs(rays[:, 3:6]))
                hit, ent = oracle.trace(moved)[:2]
                flipped |= (hit != base_hit) | ((hit != 0) & (ent != base_ent))
    return int(flipped.sum()), len(rays)


# ---------------------------------------------------------------------------------------------------------------- the look-up
def bilinear(maps, q, a, b):
    """(m, m2) [n] of the maps [n_probe][M][M][2] of the probes q [n] at (a, b) [n]: texel centres at (x + 0.5) / M, clamped at the border, along x
    on both rows, then along y; no wrap."""
    M = maps.shape[1]
    x0, x1, tx = be.grid_cell(a, 0.0, 1.0, M)
    y0, y1, ty = be.grid_cell(b, 0.0, 1.0, M)
    out = []
    for ch in range(2):
        lo = maps[q, y0, x0, ch] + tx * (maps[q, y0, x1, ch] - maps[q, y0, x0, ch])
        hi = maps[q, y1, x0, ch] + tx * (maps[q, y1, x1, ch] - maps[q, y1, x0, ch])
        out.append(lo + ty * (hi - lo))
    return out[0], out[1]


def chebyshev(r, m, m2, vis_floor):
    """1 where r <= m (or unordered), else max(vis_floor, (var / (var + (r - m)^2))^3) with var = |m m - m2|."""
    var = np.abs(m * m - m2)
    dd = r - m
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ch = var / (var + dd * dd)
    ch = (ch * ch) * ch
    return np.where(r > m, np.where(ch > vis_floor, ch, vis_floor), 1.0)


def corner_weights(vis, box, P, Nf, normal_bias=0.0, vis_floor=DEFAULT_FLOOR):
    """Per corner c = cx + 2 cy + 4 cz: (q [8][n], tw, wb, vs [8][n], r [8][n], m [8][n]) -- the probe, its three factors, and the distance and mean
    the Chebyshev test compared (m is NaN where r == 0).  vis [nz][ny][nx][M][M][2]."""
    nz, ny, nx = vis.shape[:3]
    M = vis.shape[3]
    maps = np.asarray(vis, np.float64).reshape(-1, M, M, 2)
    box = np.asarray(box, np.float64).reshape(6)
    P, Nf = np.asarray(P, np.float64), np.asarray(Nf, np.float64)
    cells = [be.grid_cell(P[:, k], box[k], box[3 + k], n) for k, n in enumerate((nx, ny, nz))]
    n3 = (nx, ny, nz)
    out = []
    for c in range(8):
        j, w, Q = [], [], []
        for a in range(3):
            i0, i1, t = cells[a]
            up = (c >> a) & 1
            j.append(i1 if up else i0)
            w.append(t if up else 1.0 - t)
            Q.append(box[a] + ((j[a].astype(np.float64) + 0.5) / float(n3[a])) * (box[3 + a] - box[a]))
        q = (j[2] * ny + j[1]) * nx + j[0]
        tw = (w[0] * w[1]) * w[2]
        tw = np.where(tw > TW_FLOOR, tw, TW_FLOOR)
        ex, ey, ez = Q[0] - P[:, 0], Q[1] - P[:, 1], Q[2] - P[:, 2]
        le = np.sqrt((ex * ex + ey * ey) + ez * ez)
        with np.errstate(divide="ignore", invalid="ignore"):
            cb = np.where(le > 0.0, ((ex * Nf[:, 0] + ey * Nf[:, 1]) + ez * Nf[:, 2]) / le, 1.0)
        h = (cb + 1.0) * 0.5
        wb = h * h + WB_BASE
        v = np.stack([(P[:, k] + Nf[:, k] * normal_bias) - Q[k] for k in range(3)], 1)
        r = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        a_, b_ = encode(v)
        m, m2 = bilinear(maps, q, a_, b_)
        vs = np.where(r == 0.0, 1.0, chebyshev(r, m, m2, vis_floor))
        out.append((q, tw, wb, vs, r, np.where(r == 0.0, np.nan, m)))
    return [np.stack([o[k] for o in out]) for k in range(6)]


def irradiance(sh, vis, box, P, Nf, normal_bias=0.0, vis_floor=DEFAULT_FLOOR):
    """D [n][3] at the points P under the unit normals Nf: num / den over the eight corners in ascending c, each channel < 0 becoming 0."""
    probes = np.asarray(sh, np.float64).reshape(-1, 9, 3)
    F = be.sh9_factor(Nf)
    q, tw, wb, vs, _, _ = corner_weights(vis, box, P, Nf, normal_bias, vis_floor)
    num, den = np.zeros((len(P), 3)), np.zeros(len(P))
    for c in range(8):
        w = (tw[c] * wb[c]) * vs[c]
        num = num + w[:, None] * be.probe_value(probes[q[c]], F)
        den = den + w
    d = num / den[:, None]
    return np.where(d < 0.0, 0.0, d)


def sample_diffuse(g, tables, sh, vis, box, normal_bias=0.0, vis_floor=DEFAULT_FLOOR):
    """The diffuse term [n][3] of one sample from its first hits g (baked_expect.sample_hits): albedo * D on the diffuse lobe, +0.0 elsewhere."""
    rough = tables["mats"][np.where(g["hit"], g["mat"], 0), 0]
    sel = np.flatnonzero(g["hit"] & (be.lobe_of(rough) == 2))
    out = np.zeros((len(g["hit"]), 3))
    if len(sel):
        out[sel] = g["albedo"][sel] * irradiance(sh, vis, box, g["P"][sel], g["Nf"][sel], normal_bias, vis_floor)
    return out


def random_vis(grid, M, seed, scale):
    """Random positive maps [nz][ny][nx][M][M][2] with m in (0.2, 1.2) * scale and m2 = m m (1 + a tenth at the most): m2 >= m m."""
    nx, ny, nz = grid
    rs = np.random.default_rng(seed)
    m = rs.uniform(0.2, 1.2, (nz, ny, nx, M, M)) * scale
    return np.ascontiguousarray(np.stack([m, (m * m) * (1.0 + rs.uniform(0.0, 0.1, m.shape))], -1))


def open_vis(grid, M, max_dist):
    """Maps that say nothing is nearer than max_dist in any direction."""
    nx, ny, nz = grid
    v = np.zeros((nz, ny, nx, M, M, 2))
    v[..., 0], v[..., 1] = max_dist, max_dist * max_dist
    return v


# ---------------------------------------------------------------------------------------------------------------- the end-to-end scene
ROOM_LO, ROOM_HI, WALL_X, WALL_HALF = (-4.0, 0.0, -2.0), (4.0, 3.0, 2.0), 0.0, 0.05
ROOM_GRID = (4, 1, 1)                      # nx, ny, nz: two probes in either room, the wall between probes 1 and 2


def quad(a, b, c, d):
    return [[a, b, c], [a, c, d]]


def two_room_scene(gi):
    """A dark two-room scene: a floor and a ceiling, a thick dividing wall across them at x = 0 that reaches past both on every side, and one light
    in room A (x < 0).  No ambient light, so room B (x > 0) is black.  The camera stands in room B and looks at its floor by the wall."""
    s = gi.Scene()
    white = s.add_material(1, 1, 1, (0.8, 0.8, 0.8))
    (x0, y0, z0), (x1, y1, z1) = ROOM_LO, ROOM_HI
    tris = quad((x0, y0, z0), (x0, y0, z1), (x1, y0, z1), (x1, y0, z0))                                        # the floor: entities 0 and 1
    tris += quad((x0, y1, z0), (x1, y1, z0), (x1, y1, z1), (x0, y1, z1))                                       # the ceiling
    for x in (WALL_X - WALL_HALF, WALL_X + WALL_HALF):                                                          # the wall's two faces
        tris += quad((x, y0, z0 - 1.0), (x, y1 + 1.0, z0 - 1.0), (x, y1 + 1.0, z1 + 1.0), (x, y0, z1 + 1.0))
    s.add_triangles(np.array(tris, float), mat_idx=[white] * len(tris))
    s.add_light((-2.0, 2.0, 0.0), (40.0, 40.0, 40.0), 0.1)
    s.set_ambient((0, 0, 0))
    s.set_camera((3.5, 2.5, 0.3), (0.5, 0.0, 0.0))
    return s.rebuild()


def room_box():
    """The probe grid's box: it straddles the wall, probes at x = -3, -1, 1, 3, one and a half units above the floor."""
    return np.array([ROOM_LO[0], 1.0, -1.0, ROOM_HI[0], 2.0, 1.0])
