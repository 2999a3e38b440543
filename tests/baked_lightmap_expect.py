"""Expectation of the baked-light pass with a lightmap (gi_render_baked_lightmap_*; include/gi_hip.h states the definition): the numpy statement of
the row that serves an entity, the chart coordinate of a hit, the two filters and the diffuse term, on first hits taken from the oracle as
baked_expect.sample_hits takes them.  Shared by the GPU tests and the CPU tests.

Every operation is written in the header's order, one IEEE operation at a time (numpy does not contract), so that given identical first hits the
diffuse term is the device's bit for bit.  Entity data comes from the scene's host tables through lightmap_expect.entity_records."""
import numpy as np

import gi_raytracer_amd as gi

import baked_expect as be
import lightmap_expect as le

NEAREST, BILINEAR = gi.LM_NEAREST, gi.LM_BILINEAR
FILTERS = (BILINEAR, NEAREST)


# ---------------------------------------------------------------------------------------------------------------- the look-up, one function a step
def row_of_ent(ent, n_ent, sphere=None):
    """[n_ent]: the lowest chart row j with ent[j] == e, -1 where there is none.  Rows naming no entity, or a sphere, serve nothing."""
    rows = np.full(n_ent, -1, np.int64)
    for j in range(len(ent) - 1, -1, -1):
        e = int(ent[j])
        if 0 <= e < n_ent and not (sphere is not None and sphere[e]):
            rows[e] = j
    return rows


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def coord_of(p0, e1v, e2v, P, tri_uv):
    """(u, v) of the points P [n][3] on the triangles p0, e1v, e2v [n][3] under the chart rows tri_uv [n][3][2]: the header's formula."""
    p0, e1v, e2v, P, t = (np.asarray(a, np.float64) for a in (p0, e1v, e2v, P, tri_uv))
    with np.errstate(all="ignore"):
        d = P - p0
        d00, d01, d11, d20, d21 = _dot(e1v, e1v), _dot(e1v, e2v), _dot(e2v, e2v), _dot(d, e1v), _dot(d, e2v)
        den = d00 * d11 - d01 * d01
        b1 = (d11 * d20 - d01 * d21) / den
        b2 = (d00 * d21 - d01 * d20) / den
        b0 = 1 - b1 - b2
        u = (b0 * t[:, 0, 0] + b1 * t[:, 1, 0]) + b2 * t[:, 2, 0]
        v = (b0 * t[:, 0, 1] + b1 * t[:, 1, 1]) + b2 * t[:, 2, 1]
    return u, v


def coord(tables, ent_hit, P, rows, uv):
    """(u, v) of the hits at P [n][3] on the entities ent_hit [n] served by the chart rows `rows` [n] of uv [n_chart][3][2]."""
    rec = le.entity_records(tables)
    uv = np.asarray(uv, np.float64).reshape(-1, 3, 2)
    return coord_of(rec["p0"][ent_hit], rec["e1v"][ent_hit], rec["e2v"][ent_hit], P, uv[rows])


def bilinear(atlas, u, v):
    """E [n][3]: per axis baked_expect.grid_cell(a, 0.0, 1.0, n) -- texel centres at (x + .5) / n, clamped to the border texels, a NaN to texel 0 --
    then a + t * (b - a) along x on both rows, then along y, then each channel clamped at 0 from below."""
    atlas = np.asarray(atlas, np.float64)
    h, w = atlas.shape[:2]
    with np.errstate(all="ignore"):
        x0, x1, tx = be.grid_cell(u, 0.0, 1.0, w)
        y0, y1, ty = be.grid_cell(v, 0.0, 1.0, h)
        rows = []
        for y in (y0, y1):
            a, b = atlas[y, x0], atlas[y, x1]
            rows.append(a + tx[:, None] * (b - a))
        d = rows[0] + ty[:, None] * (rows[1] - rows[0])
        return np.where(d < 0.0, 0.0, d)


def nearest_texel(a, n):
    """min(n - 1, max(0, floor(a * n))), a NaN going to 0."""
    with np.errstate(all="ignore"):
        v = np.asarray(a, np.float64) * float(n)
        f = np.where(v >= 1.0, np.where(v < float(n), np.floor(v), float(n - 1)), 0.0)      # (a NaN fails v >= 1.0)
    return f.astype(np.int64)


def nearest(atlas, u, v):
    """E [n][3]: the texel the coordinate falls into, as it is."""
    atlas = np.asarray(atlas, np.float64)
    h, w = atlas.shape[:2]
    return atlas[nearest_texel(v, h), nearest_texel(u, w)]


def lookup(atlas, u, v, filter):
    return bilinear(atlas, u, v) if filter == BILINEAR else nearest(atlas, u, v)


def footprint_touches_border(atlas_shape, u, v):
    """Per coordinate: the bilinear footprint is clamped on some axis -- the coordinate lies beyond the outermost texel centres (or is a NaN)."""
    h, w = atlas_shape[:2]
    with np.errstate(all="ignore"):
        gu, gv = np.asarray(u) * float(w) - 0.5, np.asarray(v) * float(h) - 0.5
        return ~((gu > 0.0) & (gu < float(w - 1)) & (gv > 0.0) & (gv < float(h - 1)))


def hit_rows(g, tables, ent):
    """(diffuse [n] bool: a hit on the diffuse lobe, row [n]: the chart row that serves the hit entity or -1) of the first hits g."""
    rough = tables["mats"][np.where(g["hit"], g["mat"], 0), 0]
    diffuse = g["hit"] & (be.lobe_of(rough) == 2)
    kind = np.asarray(tables["ent_kind"]).reshape(-1)
    rows = row_of_ent(ent, len(kind), kind == 1)
    return diffuse, np.where(diffuse, rows[np.where(g["hit"], g["ent"], 0)], -1)


def sample_terms_lm(g, tables, atlas, ent, uv, filter, sh=None, box=None):
    """(diffuse term [n][3], charted [n] bool, uncharted [n] bool) of one sample from its first hits g: a diffuse-lobe hit on an entity with a row
    reads the atlas, one without reads the grid sh in box if it is given and is +0.0 otherwise; every other sample is +0.0."""
    n = len(g["hit"])
    diffuse, row = hit_rows(g, tables, ent)
    charted, uncharted = diffuse & (row >= 0), diffuse & (row < 0)
    out = np.zeros((n, 3))
    sel = np.flatnonzero(charted)
    if len(sel):
        u, v = coord(tables, g["ent"][sel], g["P"][sel], row[sel], uv)
        out[sel] = g["albedo"][sel] * lookup(atlas, u, v, filter)
    sel = np.flatnonzero(uncharted)
    if sh is not None and len(sel):
        out[sel] = g["albedo"][sel] * be.irradiance(sh, box, g["P"][sel], g["Nf"][sel])
    return out, charted, uncharted


# ---------------------------------------------------------------------------------------------------------------- charts and atlases of the tests
ATLAS_SIZES = ((8, 8), (5, 3), (1, 1))          # width, height
ROUGHNESSES = (1.0, 0.5, 0.95, 0.0005, 1.0, 0.05)      # diffuse, glossy, diffuse, mirror, diffuse, glossy: material m gets entry m % 6
CORNERS = np.array([[[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]], [[1.0, 1.0], [0.0, 1.0], [1.0, 0.0]]])


def cell_triangle(k, cells, spread=1.1):
    """The chart triangle of cell k of a cells x cells grid: half of the cell, which half and which vertex first by k; the whole chart is spread
    about its middle so that the outer cells reach beyond [0, 1]."""
    cx, cy = k % cells, (k // cells) % cells
    t = np.roll(CORNERS[k % 2], k % 3, axis=0)
    uv = (np.array([cx, cy], np.float64) + 0.05 + 0.9 * t) / float(cells)
    return (uv - 0.5) * spread + 0.5


def grid_chart(tables, uncharted_every=4, twice=None):
    """(ent [n_chart], uv [n_chart][3][2], twice rows (j, j2) or None): triangle entity number k of the scene in cell k of a square grid of cells;
    every `uncharted_every`-th triangle entity is left out; the entity `twice` -- it must be a charted one -- is listed again in a last row, in
    a cell of its own: the lower row serves it."""
    kind = np.asarray(tables["ent_kind"]).reshape(-1)
    tris = np.flatnonzero(kind != 1)
    cells = int(np.ceil(np.sqrt(len(tris) + 1)))
    ent, uv = [], []
    for k, e in enumerate(tris):
        if k % uncharted_every == uncharted_every - 1:
            continue
        ent.append(int(e))
        uv.append(cell_triangle(k, cells))
    rows = None
    if twice is not None:
        assert int(twice) in ent
        rows = (ent.index(int(twice)), len(ent))
        ent.append(int(twice))
        uv.append(cell_triangle(len(tris), cells))
    return np.array(ent, np.int32), np.ascontiguousarray(uv, np.float64), rows


def most_hit_charted_diffuse_entity(g, tables, ent):
    """The entity with a chart row that most diffuse-lobe first hits of g land on (the lowest index of equals)."""
    diffuse, row = hit_rows(g, tables, ent)
    hits = np.bincount(g["ent"][diffuse & (row >= 0)], minlength=1)
    assert hits.max() > 0
    return int(np.argmax(hits))


def frame_chart(oracle, tables, w=24, h=16):
    """The chart the tests use on a scene: grid_chart with the entity listed twice chosen from sample 0 of the w x h frame."""
    ent, _, _ = grid_chart(tables)
    g = be.sample_hits(oracle, tables, w, h, 0)
    return grid_chart(tables, twice=most_hit_charted_diffuse_entity(g, tables, ent))


def swapped(ent, uv, rows):
    """The chart with the two rows of the twice-listed entity exchanged."""
    j, j2 = rows
    uv = uv.copy()
    uv[[j, j2]] = uv[[j2, j]]
    return ent, uv


def permuted(ent, uv, seed):
    """The chart's rows in another order in which every entity is served by the row that served it before: the serving rows shuffled among the
    serving rows' positions, the later rows of entities listed more than once kept where they are, behind them."""
    first = np.array(sorted({int(e): j for j, e in reversed(list(enumerate(ent)))}.values()))
    perm = np.arange(len(ent))
    perm[first] = np.random.default_rng(seed).permutation(first)
    return np.ascontiguousarray(ent[perm]), np.ascontiguousarray(uv[perm])


def packed_quads_chart(n_quads, cols, margin=0.08):
    """(ent, uv) of a mesh of n_quads quads of two triangles each, [a, b, c] and [a, c, d] as occlusion_expect.closed_box_scene makes them: quad q
    in cell q of a grid of `cols` columns, laid out as lightmap_expect.QUAD inside the cell less a margin for the gutter."""
    rows = -(-n_quads // cols)
    ent, uv = [], []
    for q in range(n_quads):
        cell = np.array([q % cols, q // cols], np.float64)
        for k in range(2):
            ent.append(2 * q + k)
            uv.append((cell + margin + (1.0 - 2.0 * margin) * le.QUAD[k]) / np.array([cols, rows], np.float64))
    return np.array(ent, np.int32), np.ascontiguousarray(uv, np.float64)


def random_atlas(size, seed):
    w, h = size
    return np.random.default_rng(seed).uniform(-0.2, 2.0, (h, w, 3))
