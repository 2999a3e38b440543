"""The numpy statement of a lightmap atlas (tests/lightmap_expect.py) on hand-made cases whose answers are known in closed form.  No GPU."""
import numpy as np

import lightmap_expect as le


def quad_tables(smooth=None):
    """The quad (0,0,0) (2,0,0) (2,0,4) (0,0,4) as two triangles sharing the diagonal, vertex order as le.QUAD's chart: x = 2 u, z = 4 v."""
    a, b, c, d = (0.0, 0.0, 0.0), (2.0, 0.0, 0.0), (2.0, 0.0, 4.0), (0.0, 0.0, 4.0)
    pos = np.array([[a, b, c], [a, c, d]])
    nrm = np.zeros((2, 3, 3)) if smooth is None else np.asarray(smooth, float)
    return {"tri_pos": pos, "tri_nrm": nrm, "ent_kind": np.zeros(2, np.int32)}


def test_unit_quad_covers_every_texel_and_the_diagonal_goes_to_the_lower_row():
    own = le.owners(le.QUAD, 8, 8)
    assert (own != le.NONE).all()
    x, y = np.meshgrid(np.arange(8), np.arange(8))
    assert (own[x == y] == 0).all()                        # centres exactly on the shared edge
    assert (own[x > y] == 0).all() and (own[x < y] == 1).all()
    swapped = le.owners(le.QUAD[::-1], 8, 8)               # row 0 is now the other triangle
    assert (swapped[x == y] == 0).all() and (swapped[x > y] == 1).all() and (swapped[x < y] == 0).all()


def test_clockwise_winding_gives_the_same_owners_and_points():
    t = quad_tables()
    cw_uv = le.QUAD[:, [0, 2, 1]]                          # the chart wound the other way; the entity's vertices follow
    t_cw = dict(t, tri_pos=t["tri_pos"][:, [0, 2, 1]])
    a = le.texel_table(t, [0, 1], le.QUAD, 8, 8)
    b = le.texel_table(t_cw, [0, 1], cw_uv, 8, 8)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[3], b[3])
    assert np.array_equal(a[1], b[1])                      # dyadic coordinates: both orders are exact
    assert np.array_equal(a[2], -b[2])                     # the face normal turns with the winding


def test_a_7x5_atlas():
    own = le.owners(le.QUAD, 7, 5)
    assert own.shape == (5, 7) and (own != le.NONE).all()
    pu, pv = le.centres(7, 5)
    assert pu[0, 0] == 0.5 / 7.0 and pv[4, 0] == 4.5 / 5.0
    assert np.array_equal(own == 0, pu >= pv)              # row 0 holds u >= v, the edge included
    assert own[2, 3] == 0                                  # (3.5 / 7, 2.5 / 5) = (0.5, 0.5) lies on the diagonal


def test_slivers_degenerate_rows_and_the_outside():
    sliver = np.array([[[0.0, 0.51], [1.0, 0.51], [1.0, 0.52]]])       # between the centre rows 0.4375 and 0.5625 of 8
    assert (le.owners(sliver, 8, 8) == le.NONE).all()
    line = np.array([[[0.1, 0.1], [0.5, 0.5], [0.9, 0.9]], [[0.2, 0.2], [0.2, 0.2], [0.9, 0.1]]])
    assert (le.owners(line, 8, 8) == le.NONE).all()        # area 0: nothing, not even the centres on the line
    assert (le.owners(np.concatenate([line, le.QUAD]), 8, 8) >= 2).all()
    nan = np.array([[[0.0, 0.0], [np.nan, 0.0], [1.0, 1.0]], [[0.0, 0.0], [np.inf, 0.0], [1.0, 1.0]]])
    assert (le.owners(nan, 8, 8) == le.NONE).all()
    big = np.array([[[-1.0, -1.0], [3.0, -1.0], [-1.0, 3.0]]])         # reaches outside [0, 1]: clipped
    assert (le.owners(big, 8, 8) == 0).all()
    shifted = le.QUAD + 1.0                                # a copy one period away: no wrap
    assert (le.owners(shifted, 8, 8) == le.NONE).all()
    half = np.array([[[0.5, -2.0], [1.5, -2.0], [1.5, 2.0]], [[0.5, -2.0], [1.5, 2.0], [0.5, 2.0]]])   # u in [0.5, 1.5]
    own = le.owners(half, 8, 8)
    assert (own[:, :4] == le.NONE).all() and (own[:, 4:] != le.NONE).all()


def test_rows_collinear_up_to_an_ulp_end_at_their_chart_box():
    # three vertices on the diagonal, an ulp off: the area is tiny and not 0, and the edge values alone accept every centre of the diagonal
    tri = le.REVIEW_SLIVER
    pu, pv = le.centres(32, 32)
    area, e0, e1, e2 = le.edges(tri[0], pu, pv)
    assert area != 0 and abs(area) < 1e-17
    edge_only = np.where(area > 0, (e0 >= 0) & (e1 >= 0) & (e2 >= 0), (e0 <= 0) & (e1 <= 0) & (e2 <= 0))
    assert edge_only[11, 11] and edge_only[15, 15]              # far outside the box, which ends at 0.2796 = texel 8.4
    own = le.owners(tri, 32, 32)
    assert [tuple(p) for p in np.argwhere(own == 0)] == [(k, k) for k in range(3, 9)]     # centres 0.109 .. 0.266 of the box [0.0713, 0.2796]
    # a box end exactly on a centre is included
    on = np.array([[[0.171875, 0.171875], [0.421875, 0.421875], [0.3, np.nextafter(0.3, 1.0)]]])  # centres 5 and 13 of 32
    assert [tuple(p) for p in np.argwhere(le.owners(on, 32, 32) == 0)] == [(k, k) for k in range(5, 14)]
    # exactly collinear rows have area 0 and cover nothing, on the diagonal and on a row of centres
    v = 5.5 / 32.0
    flat = np.array([[[0.1, 0.1], [0.3, 0.3], [0.7, 0.7]], [[0.1, v], [0.3, v], [0.7, v]]])
    assert (le.owners(flat, 32, 32) == le.NONE).all()
    # an ulp off a row of centres: what is covered lies on that row between the end vertices, never beyond
    bent = np.array([[[0.1, v], [0.3, np.nextafter(v, 1.0)], [0.7, v]]])
    own = le.owners(bent, 32, 32)
    ys, xs = np.nonzero(own == 0)
    assert len(xs) > 0 and (ys == 5).all() and xs.min() >= 3 and xs.max() <= 21            # centres 3.5 / 32 = 0.109 .. 21.5 / 32 = 0.672
    for w, h in ((32, 32), (7, 5), (8, 8)):
        uv = le.sliver_rows(w, h, 11)
        pu, pv = le.centres(w, h)
        some = 0
        for j in range(len(uv)):
            cov = le.owners(uv[j:j + 1], w, h) == 0
            some += bool(cov.any())
            assert le.in_box(uv[j], pu, pv)[cov].all()
            if j >= len(uv) // 2 and cov.any():                                            # rows along a row of centres stay on it
                assert len(np.unique(np.nonzero(cov)[0])) == 1
        assert some > 50


def test_the_lower_row_wins_everywhere_in_an_overlap():
    small = np.array([[[0.25, 0.25], [0.75, 0.25], [0.25, 0.75]]])
    big = np.array([[[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]]])
    in_small = le.owners(small, 16, 16) == 0
    assert in_small.sum() > 10
    a = le.owners(np.concatenate([small, big]), 16, 16)
    b = le.owners(np.concatenate([big, small]), 16, 16)
    assert (a[in_small] == 0).all() and (a[~in_small & (b == 0)] == 1).all()
    assert (b[in_small] == 0).all() and (b != 1).all()     # the big row is first: the small one owns nothing


def test_points_of_an_axis_aligned_quad_are_the_closed_form():
    owner, P, N, texel = le.texel_table(quad_tables(), [0, 1], le.QUAD, 8, 4)
    assert len(texel) == 32 and np.array_equal(texel, np.arange(32)) and owner.min() == 0
    x, y = texel % 8, texel // 8
    want = np.stack([2.0 * ((x + 0.5) / 8.0), np.zeros(32), 4.0 * ((y + 0.5) / 4.0)], 1)
    assert np.array_equal(P, want)                         # dyadic chart and geometry: every operation is exact
    assert np.array_equal(N, np.tile([0.0, -1.0, 0.0], (32, 1)))       # cross((2,0,0), (2,0,4)) = (0,-8,0)
    flipped = le.texel_table(quad_tables(), [0, 1], le.QUAD, 8, 4, flip=True)
    assert np.array_equal(flipped[2], -N) and np.array_equal(flipped[1], P)
    again = le.texel_table(quad_tables(), [1, 0, 1], np.concatenate([le.QUAD[::-1], le.QUAD[1:]]), 8, 4)   # an entity in several rows
    assert np.array_equal(again[1], P)


def test_interpolated_normals_that_cancel_uncover_the_texel():
    up, down = (0.0, 1.0, 0.0), (0.0, -1.0, 0.0)
    # row 0: n0 = up, n1 = down, n2 = down: N = (1 - 2 (b1 + b2)) up, zero where b1 + b2 = 1/2; row 1: plain
    t = quad_tables(smooth=[[up, down, down], [up, up, up]])
    chart = np.array([[[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]], [[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]]])        # both rows cover the same half
    owner, P, N, texel = le.texel_table(t, [0, 1], chart, 4, 4)
    pu, pv = le.centres(4, 4)
    zero = pu + pv == 0.5                                  # b1 = pu, b2 = pv here
    assert zero.sum() == 2 and (owner[zero] == -1).all()   # not covered, and row 1 does not inherit them
    inside = pu + pv <= 1.0
    assert (owner[inside & ~zero] == 0).all() and (owner[~inside] == -1).all()
    assert len(texel) == int((inside & ~zero).sum()) and (np.diff(texel) > 0).all()
    assert np.array_equal(N[:, 1], (((1 - pu - pv) * 1.0 + pu * -1.0) + pv * -1.0).reshape(-1)[texel]) and (N[:, [0, 2]] == 0).all()


def test_dilation_grows_a_ring_per_pass_and_keeps_the_value():
    v = np.zeros((5, 5, 3))
    f = np.zeros((5, 5), bool)
    v[2, 2], f[2, 2] = (0.3, 1.7, 2.9), True
    for passes, half in ((0, 0), (1, 1), (2, 2), (5, 2)):
        out, fill = le.dilate(v, f, passes)
        want = np.zeros((5, 5), bool)
        want[2 - half:3 + half, 2 - half:3 + half] = True
        assert np.array_equal(fill, want)
        assert (out[want] == v[2, 2]).all() and (out[~want] == 0).all()        # one neighbour: value / 1.0


def test_dilation_sums_in_order_and_divides_by_the_count():
    v = np.zeros((3, 5, 3))
    f = np.zeros((3, 5), bool)
    v[1, 1], f[1, 1] = 1.0, True
    v[1, 3], f[1, 3] = 3.0, True
    out, fill = le.dilate(v, f, 1)
    assert fill.all()
    assert (out[:, 2] == 2.0).all() and (out[:, 0] == 1.0).all() and (out[:, 4] == 3.0).all()
    # three neighbours of dyadic values: sum / 3.0 as numpy computes it
    v = np.zeros((2, 2, 3))
    f = np.array([[True, True], [True, False]])
    v[0, 0], v[0, 1], v[1, 0] = 0.25, 0.5, 2.0
    v[1, 1] = 99.0                                         # an unfilled texel's value plays no part
    out, _ = le.dilate(v, f, 1)
    assert (out[1, 1] == np.float64(2.75) / 3.0).all() and np.array_equal(out[f], v[f])
    # the order of the sum shows where it is not associative
    v = np.zeros((3, 3, 3))
    f = np.ones((3, 3), bool)
    f[1, 1] = False
    vals = [1e16, 1.0, -1e16, 1.0, 1.0, 3.0, 1.0, 1.0]
    for (dx, dy), val in zip(le.NEIGHBOURS, vals):
        v[1 + dy, 1 + dx] = val
    acc = 0.0
    for val in vals:
        acc = acc + val
    assert acc != sum(sorted(vals))
    assert (le.dilate(v, f, 1)[0][1, 1] == acc / 8.0).all()


def test_zero_passes_is_the_identity_and_borders_are_handled():
    rs = np.random.RandomState(3)
    v, f = rs.standard_normal((4, 6, 3)), rs.rand(4, 6) < 0.4
    out, fill = le.dilate(v, f, 0)
    assert np.array_equal(fill, f) and np.array_equal(out[f], v[f]) and (out[~f] == 0).all()
    v = np.zeros((3, 4, 3))
    f = np.zeros((3, 4), bool)
    v[0, 0], f[0, 0] = 5.0, True                           # a corner: three neighbours exist
    out, fill = le.dilate(v, f, 1)
    assert fill.sum() == 4 and fill[:2, :2].all() and (out[:2, :2] == 5.0).all()
    out, fill = le.dilate(v, f, 3)
    assert fill.all() and (out == 5.0).all()
    none = le.dilate(np.ones((2, 2, 3)), np.zeros((2, 2)), 4)
    assert not none[1].any() and (none[0] == 0).all()
    one = le.dilate(np.full((1, 1, 3), 2.0), np.ones((1, 1)), 2)       # a 1 x 1 atlas
    assert (one[0] == 2.0).all()


def test_the_whole_statement_scatters_ranks_and_dilates():
    calls = []

    def bake_fn(P, N):
        calls.append((P.copy(), N.copy()))
        return np.stack([np.arange(len(P)) + 1.0, P[:, 0], P[:, 2]], 1)

    tri = np.array([[[0.0, 0.0], [0.5, 0.0], [0.0, 0.5]]])
    atlas, owner, n = le.lightmap(bake_fn, quad_tables(), [0], tri, 8, 8, dilate_passes=0)
    assert n == int((owner == 0).sum()) and n == len(calls[0][0]) and n > 3
    t = np.flatnonzero(owner.reshape(-1) == 0)
    assert np.array_equal(atlas.reshape(-1, 3)[t, 0], np.arange(n) + 1.0)      # row i went to the i-th covered texel in ascending t
    assert (atlas.reshape(-1, 3)[owner.reshape(-1) < 0] == 0).all()
    wide, owner2, _ = le.lightmap(bake_fn, quad_tables(), [0], tri, 8, 8, dilate_passes=2)
    assert np.array_equal(owner2, owner) and (np.abs(wide).sum(-1) > 0).sum() > n and np.array_equal(wide.reshape(-1, 3)[t], atlas.reshape(-1, 3)[t])
    empty, owner3, n3 = le.lightmap(bake_fn, quad_tables(), np.zeros(0, np.int32), np.zeros((0, 3, 2)), 4, 3)
    assert n3 == 0 and (owner3 == -1).all() and empty.shape == (3, 4, 3) and not empty.any() and len(calls) == 2
