"""The statement of a light bake (tests/bake_expect.py; include/gi_hip.h: gi_bake_*) pinned on the oracle alone -- no GPU."""
import numpy as np
import pytest

import gi_raytracer_amd as gi

import bake_expect as be
import parity_checks as pc

AMBIENT = (0.25, 0.5, 0.75)          # dyadic: N copies add up and divide back without rounding
COUNTS = (16, 5)


@pytest.fixture(scope="module")
def floor():
    scene = be.ambient_floor_scene(gi, AMBIENT)
    return scene, pc.oracle_for(scene).build_photon_map()


def test_texels_below_the_floor_looking_away_return_the_ambient_term_exactly(floor):
    scene, o = floor
    # straight down under the floor; tilted normals only beyond its edge, leaning outwards: whatever rises there moves away from the quad
    P = np.array([[0.0, -1.0, 0.0], [60.0, -0.5, -2.0], [-70.0, -4.0, 1.5]])
    N = np.array([[0.0, -1.0, 0.0], [0.3, -2.0, 0.0], [-0.2, -0.9, 0.0]])
    for ns in COUNTS:
        rays, st = be.texel_rays(P, N, ns, stream_base=11)
        assert not o.trace(rays)[0].any()                                  # every ray misses
        got = be.bake(o, be.TEXEL, P, N, ns, stream_base=11)
        assert got.shape == (3, 3) and (got == np.array(AMBIENT)).all()


def test_probes_that_see_nothing_hold_the_ambient_term_in_band_0(floor):
    scene, o = floor
    P = np.array([[0.0, -1e6, 0.0], [40.0, -2e6, -3.0]])
    A = np.array(AMBIENT)
    for ns in COUNTS:
        rays, st = be.probe_rays(P, ns)
        assert not o.trace(rays)[0].any()
        got = be.bake(o, be.SH9, P, None, ns)
        assert got.shape == (2, 9, 3)
        acc = np.zeros(3)
        for k in range(ns):                                                 # c0 = ((N A Y0) 4 pi) / N, as numpy computes it
            acc = acc + A * 0.28209479177387814
        c0 = (acc * 12.566370614359172) / float(ns)
        assert (got[:, 0] == c0).all()
        np.testing.assert_allclose(c0, A * np.sqrt(4 * np.pi), rtol=1e-15)
        # the other bands: the ambient term times the sample mean of Y_j over these directions
        want = be.fold_sh9(np.broadcast_to(A, (2, ns, 3)), rays[:, 3:6].reshape(2, ns, 3))
        assert got.tobytes() == want.tobytes()


def test_basis_at_the_six_axis_directions_equals_the_closed_forms():
    d = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], float)
    Y = be.sh9_basis(d)
    c0, c1, c2, c6, c8 = 0.28209479177387814, 0.4886025119029199, 1.0925484305920792, 0.31539156525252005, 0.5462742152960396
    assert c0 == 0.5 * np.sqrt(1 / np.pi) and abs(c1 - np.sqrt(3 / (4 * np.pi))) < 1e-16 and abs(c2 - 0.5 * np.sqrt(15 / np.pi)) < 3e-16
    assert abs(c6 - 0.25 * np.sqrt(5 / np.pi)) < 1e-16 and abs(c8 - 0.25 * np.sqrt(15 / np.pi)) < 1e-16
    want = np.zeros((6, 9))
    want[:, 0] = c0
    want[2, 1], want[3, 1] = c1, -c1                    # y
    want[4, 2], want[5, 2] = c1, -c1                    # z
    want[0, 3], want[1, 3] = c1, -c1                    # x
    want[:, 6] = [-c6, -c6, -c6, -c6, 2 * c6, 2 * c6]    # 3 z z - 1
    want[:, 8] = [c8, c8, -c8, -c8, 0, 0]               # x x - y y
    assert (Y == want).all()                            # the cross terms x y, y z, x z vanish on the axes


def test_texel_directions_lie_in_the_normals_hemisphere():
    N = np.array([[0.2, 0.3, -0.9], [0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [3.0, -4.0, 12.0], [-0.6, 0.0, -0.8], [1e-3, 2e-3, -5e-4]])
    P = np.zeros((len(N), 3))
    Nn = be.unit_normals(N)
    for ns in COUNTS:
        rays, st = be.texel_rays(P, N, ns, stream_base=1000)
        assert (rays[:, 0:3] == np.repeat(be.SHADOW_BIAS * Nn, ns, 0)).all()
        d = rays[:, 3:6]
        assert (np.abs((d * d).sum(1) - 1.0) < 1e-15).all()
        assert ((d * np.repeat(Nn, ns, 0)).sum(1) > 0).all()


def test_stream_indices_are_the_formula_and_stay_within_32_bits():
    assert be.streams(3, 5, 7).tolist() == [7 + i * 5 + k for i in range(3) for k in range(5)]
    assert int(be.streams(2, 4, 2 ** 32 - 8)[-1]) == 2 ** 32 - 1
    with pytest.raises(AssertionError):
        be.streams(2, 4, 2 ** 32 - 7)
    g = gi.probe_grid([0, 0, 0, 4, 2, 6], 2, 1, 3)
    assert g.shape == (3, 1, 2, 3) and g[0, 0, 0].tolist() == [1.0, 1.0, 1.0] and g[2, 0, 1].tolist() == [3.0, 1.0, 5.0]
