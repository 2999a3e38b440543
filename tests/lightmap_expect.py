"""Expectation of a lightmap atlas (gi_lightmap_*; include/gi_hip.h states the definition), in numpy: coverage and owners, the texels' points, the
rank, scatter and dilation, and the whole thing as lightmap(bake_fn, ...).  Shared by the GPU tests and the statement's own tests.

Everything here is f64 and IEEE + - * / in the header's order (numpy does not contract), so the device's texel table and atlas are expected bit for
bit.  Entity data comes from the scene's HOST tables (Scene.tables(): tri_pos, tri_nrm, ent_kind), laid out as the library lays them out: edges
e1v = p1 - p0 and e2v = p2 - p0, the face normal normalize(cross(e1v, e2v)) with glm's operand order, interpolated normals iff all three vertex
normals are non-zero.  Every texel is tested against every row -- the chart box is part of the coverage test, not a short cut."""
import numpy as np

NONE = 0x7FFFFFFF


def edge(ax, ay, bx, by, px, py):
    """E(a, b, p) = (b.x - a.x) * (p.y - a.y) - (b.y - a.y) * (p.x - a.x)."""
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def centres(width, height):
    """(pu [height][width], pv [height][width]): pu = ((double) x + 0.5) / (double) width, pv = ((double) y + 0.5) / (double) height."""
    pu = (np.arange(width, dtype=np.float64) + 0.5) / float(width)
    pv = (np.arange(height, dtype=np.float64) + 0.5) / float(height)
    return np.broadcast_to(pu[None, :], (height, width)), np.broadcast_to(pv[:, None], (height, width))


def edges(tri, pu, pv):
    """(area, e0, e1, e2) of a chart row tri [..][3][2] at the points (pu, pv); broadcasting."""
    tri = np.asarray(tri, np.float64)
    a, b, c = tri[..., 0, :], tri[..., 1, :], tri[..., 2, :]
    area = edge(a[..., 0], a[..., 1], b[..., 0], b[..., 1], c[..., 0], c[..., 1])
    e0 = edge(b[..., 0], b[..., 1], c[..., 0], c[..., 1], pu, pv)
    e1 = edge(c[..., 0], c[..., 1], a[..., 0], a[..., 1], pu, pv)
    e2 = edge(a[..., 0], a[..., 1], b[..., 0], b[..., 1], pu, pv)
    return area, e0, e1, e2


def in_box(tri, pu, pv):
    """The centre lies in the row's chart box: between the smallest and the largest of its three coordinates, per axis, both ends included."""
    tri = np.asarray(tri, np.float64)
    u, v = tri[..., 0], tri[..., 1]
    return (pu >= u.min(-1)) & (pu <= u.max(-1)) & (pv >= v.min(-1)) & (pv <= v.max(-1))


def covers(tri, pu, pv):
    """In the row's chart box AND the edge test: inclusive edges, either winding; area 0 or not finite covers nothing."""
    area, e0, e1, e2 = edges(tri, pu, pv)
    pos = (e0 >= 0) & (e1 >= 0) & (e2 >= 0)
    neg = (e0 <= 0) & (e1 <= 0) & (e2 <= 0)
    return np.isfinite(area) & (area != 0) & in_box(tri, pu, pv) & np.where(area > 0, pos, neg)


def owners(uv, width, height):
    """[height][width] int32: the lowest chart row that covers the texel's centre, NONE where no row does."""
    uv = np.asarray(uv, np.float64).reshape(-1, 3, 2)
    pu, pv = centres(width, height)
    own = np.full((height, width), NONE, np.int32)
    with np.errstate(all="ignore"):
        for j in range(len(uv) - 1, -1, -1):
            own[covers(uv[j], pu, pv)] = j
    return own


def _len2(v):
    return v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2]


def _cross(x, y):
    return np.stack([x[..., 1] * y[..., 2] - y[..., 1] * x[..., 2], x[..., 2] * y[..., 0] - y[..., 2] * x[..., 0], x[..., 0] * y[..., 1] - y[..., 0] * x[..., 1]], -1)


def entity_records(tables):
    """What the library lays out per entity from the host tables: p0, e1v, e2v, n0, n1, n2, fnorm, smooth, sphere."""
    P = np.asarray(tables["tri_pos"], np.float64).reshape(-1, 3, 3)
    N = np.asarray(tables["tri_nrm"], np.float64).reshape(-1, 3, 3)
    kind = np.asarray(tables.get("ent_kind", np.zeros(len(P), np.int32))).reshape(-1)
    sphere = kind == 1
    e1v, e2v = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    with np.errstate(all="ignore"):
        cr = _cross(e1v, e2v)
        d = cr[:, 0] * cr[:, 0] + cr[:, 1] * cr[:, 1] + cr[:, 2] * cr[:, 2]
        fnorm = cr * (1.0 / np.sqrt(d))[:, None]
    smooth = ~sphere & (_len2(N[:, 0]) > 0) & (_len2(N[:, 1]) > 0) & (_len2(N[:, 2]) > 0)
    return {"p0": P[:, 0], "e1v": e1v, "e2v": e2v, "n0": N[:, 0], "n1": N[:, 1], "n2": N[:, 2], "fnorm": fnorm, "smooth": smooth, "sphere": sphere}


def texel_table(tables, ent, uv, width, height, flip=False):
    """(owner [height][width] int32 with -1 where not covered, points [n_cov][3], normals [n_cov][3], texel [n_cov] int32), covered texels in
    ascending t = y * width + x.  A texel whose normal is 0 0 0 or not finite is not covered, and no other row inherits it."""
    ent = np.asarray(ent, np.int32).reshape(-1)
    uv = np.asarray(uv, np.float64).reshape(-1, 3, 2)
    rec = entity_records(tables)
    own = owners(uv, width, height).reshape(-1)
    t = np.flatnonzero(own != NONE)
    j = own[t]
    e = ent[j]
    assert ((e >= 0) & (e < len(rec["p0"]))).all() and not rec["sphere"][e].any()
    pu, pv = centres(width, height)
    with np.errstate(all="ignore"):
        area, _, e1, e2 = edges(uv[j], pu.reshape(-1)[t], pv.reshape(-1)[t])
        b1, b2 = (e1 / area)[:, None], (e2 / area)[:, None]
        P = (rec["p0"][e] + b1 * rec["e1v"][e]) + b2 * rec["e2v"][e]
        Ns = ((1 - b1 - b2) * rec["n0"][e] + b1 * rec["n1"][e]) + b2 * rec["n2"][e]
        N = np.where(rec["smooth"][e][:, None], Ns, rec["fnorm"][e])
        if flip:
            N = -N
    ok = np.isfinite(N).all(1) & ~(N == 0).all(1)
    owner = np.full(width * height, -1, np.int32)
    owner[t[ok]] = j[ok]
    return owner.reshape(height, width), np.ascontiguousarray(P[ok]), np.ascontiguousarray(N[ok]), t[ok].astype(np.int32)


NEIGHBOURS = ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))     # (dx, dy), the order of the sum


def dilate(values, filled, passes):
    """(values [h][w][3], filled [h][w] bool) after `passes` passes.  Unfilled texels hold 0 0 0 (whatever they held); a pass reads only the state
    before it: an unfilled texel with filled 8-neighbours takes their sum, from +0.0 in the order of NEIGHBOURS, divided by (double) count."""
    f = np.asarray(filled) != 0
    v = np.where(f[..., None], np.asarray(values, np.float64), 0.0)
    h, w = f.shape
    for _ in range(int(passes)):
        fp = np.zeros((h + 2, w + 2), bool)
        vp = np.zeros((h + 2, w + 2, 3))
        fp[1:-1, 1:-1], vp[1:-1, 1:-1] = f, v
        s = np.zeros((h, w, 3))
        n = np.zeros((h, w), np.int64)
        for dx, dy in NEIGHBOURS:
            nf = fp[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
            nv = vp[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
            with np.errstate(all="ignore"):
                s = np.where(nf[..., None], s + nv, s)
            n = n + nf
        take = ~f & (n > 0)
        with np.errstate(all="ignore"):
            mean = s / np.where(n > 0, n, 1).astype(np.float64)[..., None]
        v = np.where(take[..., None], mean, v)
        f = f | take
    return v, f


def scatter(rows, texel, width, height):
    """(values [h][w][3], filled [h][w]): row i of the bake at texel[i], 0 0 0 elsewhere."""
    v = np.zeros((width * height, 3))
    f = np.zeros(width * height, bool)
    v[texel] = np.asarray(rows, np.float64).reshape(-1, 3)
    f[texel] = True
    return v.reshape(height, width, 3), f.reshape(height, width)


def lightmap(bake_fn, tables, ent, uv, width, height, dilate_passes=2, flip=False):
    """The whole statement: (atlas [h][w][3] f64, owner [h][w], n_covered); bake_fn(points, normals) returns the bake's rows [n_cov][3] -- sample k
    of row i on stream_base + i * n_samples + k is the bake's own business."""
    owner, P, N, texel = texel_table(tables, ent, uv, width, height, flip)
    rows = np.asarray(bake_fn(P, N), np.float64).reshape(-1, 3) if len(texel) else np.zeros((0, 3))
    v, f = scatter(rows, texel, width, height)
    return dilate(v, f, dilate_passes)[0], owner, len(texel)


# ---- hand charts
QUAD = np.array([[[0.0, 0.0], [1.0, 0.0], [1.0, 1.0]], [[0.0, 0.0], [1.0, 1.0], [0.0, 1.0]]])      # two rows over the whole chart, sharing the diagonal


def random_chart(n_tri, seed):
    """A chart row for every entity 0 .. n_tri-1 and a second one for every third: pseudo-random triangles of 0.002 to 0.1 chart units, both
    windings, overlaps, some reaching outside [0, 1] and some wholly outside, two degenerate.  Sized so that a few thousand rows leave some texels of
    a 32 x 32 atlas uncovered."""
    rs = np.random.RandomState(seed)
    ent = np.concatenate([np.arange(n_tri), np.arange(0, n_tri, 3)]).astype(np.int32)
    c = rs.uniform(-0.1, 1.1, (len(ent), 1, 2))
    uv = c + rs.uniform(-1, 1, (len(ent), 3, 2)) * 10.0 ** rs.uniform(-2.7, -1.0, (len(ent), 1, 1))
    uv[1] += 3.0                                    # wholly outside
    uv[2, 2] = uv[2, 0] + 2.0 * (uv[2, 1] - uv[2, 0])      # (nearly) degenerate: three points on a line
    uv[3] = uv[3, [0, 0, 1]]                        # degenerate exactly: two vertices coincide
    return ent, np.ascontiguousarray(uv)


REVIEW_SLIVER = np.array([[[0.10869142996232407, 0.10869142996232406], [0.07134501804683216, 0.07134501804683217], [0.27964704219680525, 0.27964704219680525]]])


def sliver_rows(width, height, seed, n=200):
    """Rows whose three vertices are collinear exactly or up to an ulp: on the chart's diagonal and on a row of texel centres.  Their areas round to
    0 or to a tiny value of either sign, and the edge values round to 0 or to the area's sign for every centre on the line EXTENDED: only the chart
    box ends such a row."""
    rs = np.random.RandomState(seed)
    t = rs.uniform(0.02, 0.7, (n, 3))
    diag = np.stack([t, t], -1)
    pv = (rs.randint(0, height, n) + 0.5) / float(height)
    line = np.stack([t, np.broadcast_to(pv[:, None], (n, 3))], -1)
    uv = np.concatenate([diag, line])
    step = rs.randint(-1, 2, uv.shape)
    return np.ascontiguousarray(np.where(step < 0, np.nextafter(uv, -1.0), np.where(step > 0, np.nextafter(uv, 2.0), uv)))
