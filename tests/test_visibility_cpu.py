"""Probe visibility without a GPU: the per-lane functions of gi_visibility.h compiled for the host as a program of its own
(tests/cpp/visibility_lookup.cpp), plainly and under the sanitizers, bit for bit against the numpy statement (tests/visibility_expect.py) on random
inputs and on its edge inputs; what the statement itself promises (no leak through a wall, open maps change nothing); the room the capture's rays
have at the GPU tests' probe positions; the binding's parameter blocks and the command line's refusals.

The leak test's closed form.  On a 2 x 1 x 1 grid the y and z axes have one probe, so t_y = t_z = 0 and the six corners with c_y or c_z set name
probes 0 and 1 again with a trilinear weight of 0, which step 2 of the definition raises to 0.001.  The statement's D is therefore not
B * (tx wb1 f) / ((1 - tx) wb0 + tx wb1 f) but the same with those six terms in the sums, in corner order:
    num = B * (((tx wb1 f + .001 wb1 f) + .001 wb1 f) + .001 wb1 f),   den = the eight weights in ascending c,
and that is what is asserted bit for bit; the two-term form is within 1 % of it, which is asserted too, as is D < 0.1 * (0.4 * B)."""
import os
import subprocess

import numpy as np
import pytest

import gi_raytracer_amd as gi
import gi_raytracer_amd.__main__ as cli

import bake_expect as bake
import baked_expect as be
import features_expect as fe
import host_build
import parity_checks as pc
import visibility_expect as ve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer"]
BUILDS = ["plain", "sanitized"]
SIZES = (1, 3, 8)
ULP = 2.0 ** -52


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("visibility_lookup")
    out = {}
    for name, extra in (("plain", []), ("sanitized", SANITIZE)):
        out[name] = str(d / f"visibility_lookup_{name}")
        subprocess.run([os.environ.get("CXX", "g++")] + host_build.flags() + extra + [os.path.join(ROOT, "tests", "cpp", "visibility_lookup.cpp"), "-o", out[name]], check=True)
    return out


def run_program(exe, *args):
    r = subprocess.run([exe] + [a if isinstance(a, str) else (float(a).hex() if isinstance(a, float) else str(a)) for a in args], capture_output=True, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
    return np.array([[float.fromhex(t) for t in ln.split()] for ln in r.stdout.split("\n") if ln])


def bits(a):
    return np.ascontiguousarray(a, np.float64).tobytes()


def hexes(a):
    return [float(v) for v in np.asarray(a, np.float64).reshape(-1)]


def unit(v):
    return v / np.sqrt((v * v).sum(-1))[..., None]


def lookup(exe, tmp_path, sh, vis, box, P, Nf, bias, floor):
    """pv_irradiance of the program on these tables: everything goes through a file of hexadecimal floats."""
    nz, ny, nx = sh.shape[:3]
    head = [float(nx), float(ny), float(nz)] + hexes(box) + [float(vis.shape[3]), float(bias), float(floor), float(len(P))]
    path = tmp_path / "lookup.txt"
    path.write_text("\n".join(float(v).hex() for v in head + hexes(sh) + hexes(vis) + hexes(np.concatenate([P, Nf], 1))))
    return run_program(exe, "lookup", str(path))


# ---------------------------------------------------------------------------------------------------------------- 1. bit for bit against the statement
@pytest.mark.parametrize("build", BUILDS)
def test_host_build_of_decode_and_encode_equals_the_statement_bit_for_bit(programs, build):
    rs = np.random.default_rng(21)
    ab = np.concatenate([rs.uniform(0.0, 1.0, (60, 2)), [[0, 0], [1, 1], [0, 1], [0.5, 0.5], [0.5, 0], [0, 0.5], [1, 0.5], [0.25, 0.25], [0.75, 0.25], [0.5, 0.25]]])
    got = run_program(programs[build], "decode", *hexes(ab))
    want = ve.decode(ab[:, 0], ab[:, 1])
    assert got.shape == (len(ab), 3) and bits(got) == bits(want)
    assert (want[:, 2] == 0).any() and (want[:, 2] < 0).any() and (want[:, 2] > 0).any()                  # vz == 0 lies on the upper sheet
    assert bits(gi.octa_decode(ab[:, 0], ab[:, 1])) == bits(want)                                         # the package's helper is the statement too
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    signs = np.array([[x, y, z] for x in (1.0, -1.0, 0.0, -0.0) for y in (1.0, -1.0, 0.0, -0.0) for z in (1.0, -1.0, 0.0, -0.0) if x or y or z])
    v = np.concatenate([unit(rs.normal(size=(60, 3))), 7.5 * rs.normal(size=(20, 3)), axes, signs, [[0.3, -0.7, 0.0], [1e-300, 0.0, -1e-300]]])
    got = run_program(programs[build], "encode", *hexes(v))
    a, b = ve.encode(v)
    assert bits(got) == bits(np.stack([a, b], 1))
    assert (a >= 0).all() and (a <= 1).all() and (b >= 0).all() and (b <= 1).all()
    ga, gb = gi.octa_encode(v)
    assert bits(ga) == bits(a) and bits(gb) == bits(b)
    # round trips of the texel centres of every map size the tests use: the same point of the square, to the last few bits
    for M in SIZES + (64,):
        c = (np.arange(M) + 0.5) / M
        ca, cb = (q.reshape(-1) for q in np.meshgrid(c, c))
        ra, rb = ve.encode(ve.decode(ca, cb))
        assert np.abs(ra - ca).max() <= 4 * ULP and np.abs(rb - cb).max() <= 4 * ULP, M
        got = run_program(programs[build], "encode", *hexes(run_program(programs[build], "decode", *hexes(np.stack([ca, cb], 1)))))
        assert bits(got) == bits(np.stack([ra, rb], 1))


@pytest.mark.parametrize("build", BUILDS)
def test_host_build_of_the_fold_equals_the_statement_bit_for_bit(programs, build):
    rs = np.random.default_rng(22)
    for n in (1, 2, 17):
        d = rs.uniform(0.0, 30.0, (9, n)) * 10.0 ** rs.integers(-3, 3, (9, 1))
        assert bits(run_program(programs[build], "fold", n, *hexes(d))) == bits(ve.fold(d)), n


@pytest.mark.parametrize("build", BUILDS)
def test_host_build_of_the_weighted_lookup_equals_the_statement_bit_for_bit(programs, build, tmp_path):
    rs = np.random.default_rng(23)
    box = np.array([-1.0, 0.5, -2.0, 1.5, 2.0, 0.25])
    seen_behind = seen_front = 0
    for k, grid in enumerate(be.GRIDS):
        sh = be.random_sh(grid, 40 + k)
        P = np.concatenate([rs.uniform(-2.5, 2.5, (40, 3)), [box[:3], box[3:]]])          # inside and outside the box: clamping happens
        N = unit(rs.normal(size=(len(P), 3)))
        for M in SIZES:
            vis = ve.random_vis(grid, M, 50 + M, 1.5)
            for bias in (0.0, 0.01):
                got = lookup(programs[build], tmp_path, sh, vis, box, P, N, bias, 0.05)
                want = ve.irradiance(sh, vis, box, P, N, bias, 0.05)
                assert bits(got) == bits(want), (grid, M, bias)
                assert (want >= 0).all()
            _, _, _, vs, r, m = ve.corner_weights(vis, box, P, N)
            seen_behind += int((r > m).sum()); seen_front += int((r <= m).sum())
            assert ((vs >= 0.05) & (vs <= 1.0)).all()
    assert seen_behind > 0 and seen_front > 0


@pytest.mark.parametrize("build", BUILDS)
def test_edge_inputs_of_the_lookup_equal_the_statement_bit_for_bit(programs, build, tmp_path):
    grid, M = (2, 2, 2), 3
    box = np.array([0.0, 0.0, 0.0, 4.0, 4.0, 4.0])
    probes = gi.probe_grid(box, *grid).reshape(-1, 3)
    sh = be.random_sh(grid, 60)
    N0 = np.array([0.0, 1.0, 0.0])
    P = np.array([probes[0], probes[7], [2.0, 2.0, 2.0], [-3.0, 9.0, 4.5], [1.0, 1.0, 1.5]])      # on a probe (le == 0, r == 0), the middle, outside the box
    N = np.tile(N0, (len(P), 1))
    r_mid = float(np.sqrt((1.0 * 1.0 + 1.0 * 1.0) + 1.0 * 1.0))                                   # every probe is this far from the middle
    cases = {"zero": np.zeros((2, 2, 2, M, M, 2)), "r_equals_m": ve.open_vis(grid, M, r_mid), "random": ve.random_vis(grid, M, 61, 2.0)}
    for name, vis in cases.items():
        for bias in (0.0, 0.25):
            got = lookup(programs[build], tmp_path, sh, vis, box, P, N, bias, 0.05)
            want = ve.irradiance(sh, vis, box, P, N, bias, 0.05)
            assert bits(got) == bits(want) and np.isfinite(want).all(), (name, bias)
    q, tw, wb, vs, r, m = ve.corner_weights(cases["zero"], box, P, N)
    assert (r[:, 0] == 0).sum() == 1 and vs[0, 0] == 1.0 and wb[0, 0] == 1.0 * 1.0 + 0.2            # P on probe 0: cb = 1, vis = 1
    assert (vs[r > 0] == 0.05).all()                                                               # m == m2 == 0: no variance, the floor
    q, tw, wb, vs, r, m = ve.corner_weights(cases["r_equals_m"], box, P, N)
    assert (r[:, 2] == r_mid).all() and (vs[:, 2] == 1.0).all()                                    # r == m is in front
    assert (tw[:, 3] == ve.TW_FLOOR).sum() == 7                                                    # outside the box: one corner has all the weight
    r = subprocess.run([programs[build], "edges"], capture_output=True, text=True)
    assert r.returncode == 0 and "edges: 0 bad" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr


# ---------------------------------------------------------------------------------------------------------------- 2. no leak, on the statement alone
def test_a_probe_behind_a_wall_counts_for_the_floor_only():
    B, f = 2.0, ve.DEFAULT_FLOOR
    grid, M = (2, 1, 1), 3
    box = np.array([0.0, 0.0, 0.0, 4.0, 1.0, 1.0])                  # probe 0 at x = 1, probe 1 at x = 3
    sh = np.zeros((1, 1, 2, 9, 3))
    sh[0, 0, 1, 0] = B / (1.0 * 0.28209479177387814)                # DC only: D_c = B at probe 1, 0 at probe 0
    F0 = 1.0 * 0.28209479177387814
    Dc = 0.0 + F0 * sh[0, 0, 1, 0]
    m = 0.6                                                         # probe 1 sees a wall 0.6 away in every direction; probe 0 sees nothing near
    vis = np.zeros((1, 1, 2, M, M, 2))
    vis[0, 0, 0, :, :, 0], vis[0, 0, 0, :, :, 1] = 10.0, 10.0 * 10.0
    vis[0, 0, 1, :, :, 0], vis[0, 0, 1, :, :, 1] = m, m * m
    P, N = np.array([[1.8, 0.2, 0.5]]), np.array([[0.0, 1.0, 0.0]])
    _, _, tx = be.grid_cell(P[:, 0], 0.0, 4.0, 2)
    assert abs(tx[0] - 0.4) < 1e-15
    q, tw, wb, vs, r, mm = ve.corner_weights(vis, box, P, N)
    assert q[:, 0].tolist() == [0, 1] * 4 and r[1, 0] > m and r[0, 0] < 10.0                      # P lies beyond the wall as probe 1 sees it
    assert vs[:, 0].tolist() == [1.0, f] * 4                                                      # var = 0, so ch = 0: the floor
    wb0, wb1 = wb[0, 0], wb[1, 0]
    assert wb0 != wb1 and (wb[0::2, 0] == wb0).all() and (wb[1::2, 0] == wb1).all()
    w = [(t * b) * v for t, b, v in zip([1.0 - tx[0], tx[0]] + [ve.TW_FLOOR] * 6, [wb0, wb1] * 4, [1.0, f] * 4)]
    num, den = 0.0, 0.0
    for c in range(8):
        num = num + w[c] * (Dc if c & 1 else np.zeros(3))
        den = den + w[c]
    got = ve.irradiance(sh, vis, box, P, N)[0]
    assert bits(got) == bits(num / den)                                                           # the closed form with all eight corners, bit for bit
    two_terms = B * (tx[0] * wb1 * f) / ((1.0 - tx[0]) * wb0 + tx[0] * wb1 * f)
    assert np.abs(got / two_terms - 1.0).max() < 0.01                                              # the six floored corners add 3 / 1000 to either weight
    plain = be.irradiance(sh, box, P, N)[0]
    assert np.allclose(plain, 0.4 * B, rtol=1e-14)
    assert (got < 0.1 * (0.4 * B)).all() and (got > 0).all(), (got, plain)                         # less than a tenth of the leak is left
    # without the wall in probe 1's map nothing is held back
    assert np.allclose(ve.irradiance(sh, ve.open_vis(grid, M, 10.0), box, P, N)[0], B * (0.403 * wb1) / (0.603 * wb0 + 0.403 * wb1), rtol=1e-14)


# ---------------------------------------------------------------------------------------------------------------- 3. open maps change nothing
def test_open_maps_and_equal_back_face_weights_give_the_trilinear_value():
    """With every map open vis = 1; at the middle between two probes of a 2 x 1 x 1 grid, under a normal perpendicular to the grid's axis, every
    wb is h * h + 0.2 with cb = 0 and every probe has the same sum of trilinear weights, so D is the trilinear value.  The bound: a weight has two
    roundings, its product with D_c one, a sum of eight positive terms seven; num is within 10 ulp, den within 9, the quotient adds one: 20 ulp."""
    grid, M = (2, 1, 1), 3
    box = np.array([0.0, 0.0, 0.0, 4.0, 1.0, 1.0])
    sh = np.zeros((1, 1, 2, 9, 3))
    sh[..., 0, :] = np.random.default_rng(31).uniform(0.5, 2.0, (1, 1, 2, 3))                      # DC only, positive: no cancellation in the sums
    P, N = np.array([[2.0, 0.5, 0.5]]), np.array([[0.0, 0.0, 1.0]])
    vis = ve.open_vis(grid, M, 100.0)
    q, tw, wb, vs, r, m = ve.corner_weights(vis, box, P, N)
    assert (vs == 1.0).all() and (wb == wb[0, 0]).all() and (r <= m).all()
    got, want = ve.irradiance(sh, vis, box, P, N), be.irradiance(sh, box, P, N)
    assert (np.abs(got - want) <= 20 * ULP * np.abs(want)).all() and (want > 0).all()
    # and wherever the hit is and whatever its normal: probes that all hold the same light give that light (the weights are normalised)
    rs = np.random.default_rng(32)
    grid = (3, 2, 4)
    sh = np.broadcast_to(be.random_sh((1, 1, 1), 33)[0, 0, 0], (4, 2, 3, 9, 3)).copy()
    P, N = rs.uniform(-1.0, 5.0, (50, 3)), unit(rs.normal(size=(50, 3)))
    got = ve.irradiance(sh, ve.random_vis(grid, 3, 34, 2.0), np.array([0.0, 0.0, 0.0, 4.0, 4.0, 4.0]), P, N)
    want = be.irradiance(sh, np.array([0.0, 0.0, 0.0, 4.0, 4.0, 4.0]), P, N)
    assert np.allclose(got, want, rtol=1e-13, atol=1e-15)


# ---------------------------------------------------------------------------------------------------------------- the GPU tests' probe positions
@pytest.mark.parametrize("name", ["cornell", "spheres_opaque", "test_scene"])
def test_no_ray_of_the_gpu_tests_captures_changes_its_hit_under_a_4_ulp_move(name):
    """tests/test_gpu_visibility.py allows the device's hit to differ from the oracle's for 1 ray in 1 000; at its probe positions none should."""
    scene = pc.load_scene(name)
    o, t = pc.oracle_for(scene), scene.tables()
    points = ve.probe_points(t)
    assert len(points) == len(bake.probe_points(t)) == 7
    flipped = asked = 0
    for M in (3, 8):
        rays, _ = ve.capture_rays(points, M, 2)
        assert name in fe.DRAW_FREE_SCENES and fe.oracle_is_draw_free(o, rays)
        f, a = ve.hits_flip_under_perturbation(o, rays)
        flipped += f; asked += a
    print(f"{name}: {flipped} of {asked} capture rays meet another entity under a 4-ulp move of the direction")
    assert flipped == 0 and asked == len(points) * (9 + 64) * 2


def test_statement_rays_cover_the_sphere_and_stay_in_their_texels():
    P = np.array([[0.5, -1.0, 2.0], [3.0, 0.0, 0.0]])
    for M in SIZES:
        rays, st = ve.capture_rays(P, M, 3, stream_base=7)
        assert st[0] == 7 and (np.diff(st.astype(np.int64)) == 1).all() and len(rays) == 2 * M * M * 3
        assert np.abs(np.sqrt((rays[:, 3:6] ** 2).sum(1)) - 1.0).max() < 4 * ULP and (rays[:M * M * 3, 0:3] == P[0]).all()
        a, b = ve.encode(rays[:, 3:6])
        t = np.repeat(np.arange(2 * M * M), 3)
        assert (np.floor(a * M + 1e-12).astype(int).clip(0, M - 1) == t % M).all() and (np.floor(b * M + 1e-12).astype(int).clip(0, M - 1) == (t // M) % M).all()
    assert (rays[:, 5] > 0).any() and (rays[:, 5] < 0).any()


# ---------------------------------------------------------------------------------------------------------------- 4. the binding and the command line
def test_default_params_and_the_binding_s_checks():
    L = gi.lib()
    p = gi.ProbeVisibilityParams()
    L.gi_probe_visibility_default_params(p)
    assert (p.size, p.n_samples, p.stream_base, p.seed, p.max_dist) == (8, 16, 0, gi.DEFAULT_SEED, 1e30)
    v = gi.BakedVisibilityParams()
    L.gi_baked_visibility_default_params(v)
    assert (v.size, v.normal_bias, v.vis_floor) == (8, 0.0, 0.05)
    L.gi_probe_visibility_default_params(None); L.gi_baked_visibility_default_params(None)      # a null block is left alone
    vis = ve.random_vis((3, 2, 4), 5, 1, 1.0)
    vp, a = gi.baked_visibility_params(vis, (4, 2, 3), normal_bias=0.01, vis_floor=0.5)
    assert (vp.size, vp.normal_bias, vp.vis_floor) == (5, 0.01, 0.5) and a.dtype == np.float64 and bits(a) == bits(vis)
    assert gi.baked_visibility_params(vis.astype(np.float32))[1].dtype == np.float32
    assert gi.baked_visibility_params(None) [1] is None and gi.baked_visibility_params(None)[0].size == 8
    for kw in (dict(vis=vis[0]), dict(vis=vis[..., :1]), dict(vis=vis[:, :, :, :4]), dict(vis=np.zeros((1, 1, 1, 65, 65, 2))), dict(vis=np.zeros((1, 1, 0, 3, 3, 2))),
               dict(vis=vis, grid=(3, 2, 4)), dict(vis=vis, normal_bias=-0.1), dict(vis=vis, normal_bias=float("inf")), dict(vis=vis, normal_bias=float("nan")),
               dict(vis=vis, vis_floor=0.0), dict(vis=vis, vis_floor=1.5), dict(vis=vis, vis_floor=float("nan")), dict(vis=None, vis_floor=-1.0)):
        with pytest.raises(ValueError):
            gi.baked_visibility_params(**kw)
    assert gi.PROBE_VISIBILITY_MAX_SIZE == 64


@pytest.mark.parametrize("args", [["--probe-visibility", "8"], ["--probes", "2", "2", "2", "--probe-visibility", "8"], ["--baked", "b", "--probe-visibility", "0"],
                                  ["--baked", "b", "--probe-visibility", "65"], ["--baked", "b", "--probe-visibility", "8", "--baked-lightmap", "8", "8"],
                                  ["--baked", "b", "--baked-probes", "512", "512", "64", "--probe-visibility", "8"], ["--lightmap", "8", "8", "--probe-visibility", "4"]])
def test_command_line_refuses_before_it_touches_the_device(args):
    with pytest.raises(SystemExit) as e:
        cli.main([os.path.join(ROOT, pc.SCN["cornell"])] + args)
    assert e.value.code == 2


def test_command_line_takes_the_flag_with_the_preview_s_grid():
    ap = cli.parser()
    a = ap.parse_args(["s.scn", "--baked", "lit", "--baked-probes", "3", "2", "4", "--probe-visibility", "6"])
    cli.check_args(ap, a)
    assert a.probe_visibility == 6 and a.baked_probes == [3, 2, 4]
    a = ap.parse_args(["s.scn", "--baked", "lit", "--probe-visibility", "64"])      # the default grid
    cli.check_args(ap, a)
    assert a.probe_visibility == 64
