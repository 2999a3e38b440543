"""Synthetic photon clusters with chosen candidate counts and key patterns, and the gather queries that meet them: the inputs of
tests/test_gpu_gather_kernels.py (the stream passes' gather kernels on the GPU) and tests/test_gather_forms_cpu.py (the CPU build of gather())."""
import numpy as np

import gi_raytracer_amd as gi

# candidate counts around the boundaries of the kernels' staging: ksel_tau's first group (8, 16, 32 keys), rank 32, chunks of 64, a long list
SMALL = (1, 7, 8, 9, 15, 16)        # at most 16 photons (kMaxPhotonsPerLeaf): the cluster is a leaf of its own
BIG = (17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193, 255, 256, 257, 1200)
REQUIRED = {1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193, 255, 256, 257}
TIES = ("shell", "tie", "dup", "dupgroup")   # patterns whose query at the centre has float keys tied across rank 32 (n > 32)
R = 2.0 ** -20                      # every photon of a cluster lies within 3 R (3e-6) of its centre: inside the +-1e-5 box of a query's leaf
RUN = 64                            # queries per cluster at its centre, one wave in the caller's order


def _unit(rs, n):
    u = rs.randn(n, 3)
    return u / np.linalg.norm(u, axis=1)[:, None]


def _rows(off, c, rs):
    return np.concatenate([c + off, _unit(rs, len(off)), rs.rand(len(off), 3)], 1)


def _near(n, rs):
    return _unit(rs, n) * (R * rs.uniform(0.5, 0.75, n))[:, None]


def _shell(n, rs):
    # radii 1 + k 2^-40 apart: squared distances from the centre differ by ~1e-9 relative, far below float resolution (one float key)
    return _unit(rs, n) * (R * (1 + rs.permutation(n) * 2.0 ** -40))[:, None]


def cluster(pattern, n, c, rs):
    """n photons [n][9] around the centre c; the query at c meets the pattern's keys.  Copies are whole rows: position, direction, colour."""
    if pattern == "random":                         # keys of every size
        return _rows(_unit(rs, n) * (R * rs.uniform(0.05, 3.0, n))[:, None], c, rs)
    if pattern == "shell":                          # every key equal
        return _rows(_shell(n, rs), c, rs)
    if pattern == "tie":                            # 10 nearer ones, the rest on the shell: a float tie group across rank 32
        return _rows(np.concatenate([_near(10, rs), _shell(n - 10, rs)]), c, rs)
    if pattern == "dup":                            # exact copies; from 33 on the tie group across rank 32 is made of pairs of copies
        if n >= 33:
            g = n - 10
            sh = _rows(_shell(g - g // 2, rs), c, rs)
            return np.concatenate([_rows(_near(10, rs), c, rs), sh, sh[:g // 2]])
        r = cluster("random", n - n // 2, c, rs)
        return np.concatenate([r, r[:n // 2]])
    assert pattern == "dupgroup" and n >= 33       # 28 nearer ones, five copies of ONE photon at ranks 29 .. 33, the rest farther away
    one = _rows(_unit(rs, 1) * R, c, rs)
    far = _rows(_unit(rs, n - 33) * (R * rs.uniform(2.0, 3.0, n - 33))[:, None], c, rs)
    return np.concatenate([_rows(_near(28, rs), c, rs), np.repeat(one, 5, 0), far])


def scene():
    s = gi.Scene()
    m = s.add_material(1.0, 1.0, 1.0, (1, 1, 1))
    s.add_triangles(np.array([[[0, 0, 0], [4, 0, 0], [0, 0, 4]], [[4, 0, 0], [4, 0, 4], [0, 0, 4]], [[0, 4, 0], [4, 4, 0], [0, 4, 4]]], float), mat_idx=[m] * 3)
    s.add_light((2, 3, 2), (1, 1, 1), .05)
    return s.rebuild()


def build():
    """Clusters in the cells of a 4 x 4 x 4 grid over the map's box, each cell split in eight subcells.  A cluster sits at 0.4 of a subcell from
    its low corner, so the leaves that hold its photons keep far from the subcell's faces.  A small cluster takes subcell 0 of a cell and is a leaf
    of its own there; every cell with photons holds a cluster of more than 16, so it is split and the small cluster's neighbours are empty leaves
    or subcells whose photons keep away from the shared faces: a query anywhere in that leaf has exactly the cluster's photons as candidates.
    Subcell 0 of the last cell stays empty: a leaf without candidates.
    Returns the scene, the photons [n][9], the queries [m][6], the clusters as (count, pattern, centre) and the cluster of each query's run (-1: no run)."""
    sc = scene()
    root = sc.tables()["node_bbox"][0]
    lo, ext = root[:3], root[3:] - root[:3]
    cell, sub = ext / 4, ext / 8
    specs_small = [(n, p) for n in SMALL for p in ("random", "shell", "dup")]
    specs_big = [(n, p) for n in BIG for p in (("random", "shell", "dup") if n < 33 else ("random", "shell", "tie", "dup", "dupgroup"))]
    n_cells = len(specs_small) + 1

    def corner(k, s):
        ijk = np.array([k % 4, (k // 4) % 4, k // 16], float)
        bits = np.array([s & 1, (s >> 1) & 1, (s >> 2) & 1], float)
        return lo + cell * ijk + sub * bits

    placed = [(n, p, corner(k, 0) + 0.4 * sub) for k, (n, p) in enumerate(specs_small)]
    placed += [(n, p, corner(j % n_cells, 1 + j // n_cells) + 0.4 * sub) for j, (n, p) in enumerate(specs_big)]
    placed.sort(key=lambda t: (t[1] != "tie", -t[0]))          # the 1200-photon tie group first: the queries of the short sets
    rs = np.random.RandomState(23)
    ph, runs, extra = [], [], []
    for j, (n, p, c) in enumerate(placed):
        ph.append(cluster(p, n, c, rs))
        # RUN queries at the centre (the random pattern: within 1e-12 of it, one leaf, a key set per lane), three more in the cluster
        pos = c + (_unit(rs, RUN) * 1e-12 * rs.rand(RUN, 1) if p == "random" else 0.0)
        runs.append(np.concatenate([np.broadcast_to(pos, (RUN, 3)), _unit(rs, RUN)], 1))
        extra.append(np.concatenate([c + _unit(rs, 3) * R * rs.rand(3, 1), _unit(rs, 3)], 1))
    out = lo - ext * (0.1 + rs.rand(3, 3))                                              # outside the map
    empty = corner(n_cells - 1, 0) + sub * (0.2 + 0.6 * rs.rand(3, 3))                  # in a leaf without candidates
    extra.append(np.concatenate([np.concatenate([out, empty]), _unit(rs, 6)], 1))
    extra = np.concatenate(extra)
    q = np.concatenate(runs + [extra[rs.permutation(len(extra))]])
    cl = np.concatenate([np.repeat(np.arange(len(placed)), RUN), np.full(len(extra), -1)])   # cluster of each query's run (-1: no run)
    return sc, np.concatenate(ph), q, placed, cl


def float_keys(ph, c):
    """The sorted float keys the query at a cluster's centre c meets: (float)d2 of the photons within the +-1e-5 box around it."""
    pos = ph[:, :3]
    d = pos[np.abs(pos - c).max(1) < 1e-5] - c
    return np.sort((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).astype(np.float32))
