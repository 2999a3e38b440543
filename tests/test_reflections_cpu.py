"""Reflection probe sets without a GPU: the per-lane functions of gi_reflections.h compiled for the host as a program of its own
(tests/cpp/reflections_lookup.cpp), plainly and under the sanitizers, bit for bit against the numpy statement (tests/reflections_expect.py) on
random inputs and on the edge inputs; what the statement itself promises (the parallax: a direction-coded cube read at the box-projected
direction, not at R); the room the look-up has on the GPU tests' frames; the binding's parameter blocks, reflection_probe_cells and the command
line's refusals.

The parallax bound.  A texel of a cube of face n spans at most 2 / n per face coordinate, so any point of it on the cube is within half a
diagonal, sqrt(2) / n, of its centre; the cube's points are at least 1 from the origin, so the angle between the direction read (the centre's)
and the direction asked for is at most sqrt(2) / n radians."""
import os
import subprocess

import numpy as np
import pytest

import gi_raytracer_amd as gi
import gi_raytracer_amd.__main__ as cli

import baked_expect as be
import features_expect as fe
import host_build
import parity_checks as pc
import reflections_expect as re_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer"]
BUILDS = ["plain", "sanitized"]
FACE, LEVELS = be.CHAIN_FACE, be.CHAIN_LEVELS
SIZES = ((13, 9), (24, 16))          # the GPU tests' frames
N = 2                                # and their samples


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("reflections_lookup")
    out = {}
    for name, extra in (("plain", []), ("sanitized", SANITIZE)):
        out[name] = str(d / f"reflections_lookup_{name}")
        subprocess.run([os.environ.get("CXX", "g++")] + host_build.flags() + extra + [os.path.join(ROOT, "tests", "cpp", "reflections_lookup.cpp"), "-o", out[name]], check=True)
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float64).tobytes()


def hexes(a):
    return [float(v) for v in np.asarray(a, np.float64).reshape(-1)]


def unit(v):
    return v / np.sqrt((v * v).sum(-1))[..., None]


def program_lookup(exe, tmp_path, probes, chains, face, levels, P, R, level):
    """rs_specular of the program on these tables: everything goes through a file of hexadecimal floats."""
    level = np.broadcast_to(np.asarray(level, np.float64), (len(P),))
    head = [float(len(probes)), float(face), float(levels), float(len(P))]
    path = tmp_path / "lookup.txt"
    path.write_text("\n".join(float(v).hex() for v in head + hexes(probes) + hexes(chains) + hexes(np.concatenate([P, R, level[:, None]], 1))))
    r = subprocess.run([exe, "lookup", str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
    return np.array([[float.fromhex(t) for t in ln.split()] for ln in r.stdout.split("\n") if ln])


def unit_box_tables(K, seed):
    """random_probes for a scene whose root box is -1 .. 2, 0 .. 1.5, -2 .. 0.5."""
    return re_.random_probes({"node_bbox": np.array([[-1.0, 0.0, -2.0, 2.0, 1.5, 0.5]])}, K, seed)


# ---------------------------------------------------------------------------------------------------------------- 1. bit for bit against the statement
@pytest.mark.parametrize("build", BUILDS)
def test_host_build_of_the_lookup_equals_the_statement_on_random_inputs(programs, build, tmp_path):
    rs = np.random.default_rng(41)
    seen = np.zeros(3, np.int64)
    for K in (1, 2, 5, 64):
        probes = unit_box_tables(K, 70 + K)
        chains = re_.flat_chains(re_.random_chains(K, 80 + K))
        P = rs.uniform([-1.4, -0.3, -2.4], [2.4, 1.8, 0.9], (120, 3))          # inside the scene's box and around it
        R = unit(rs.normal(size=(120, 3))) * rs.uniform(0.5, 2.0, (120, 1))     # any length
        level = rs.integers(0, LEVELS, 120)
        want = re_.lookup_detail(probes, chains, FACE, LEVELS, P, R, level)
        got = program_lookup(programs[build], tmp_path, probes, chains, FACE, LEVELS, P, R, level)
        assert got.shape == (120, 3) and bits(got) == bits(want["S"]), K
        seen += np.bincount(want["route"], minlength=3)
        assert (probes[:, 9] == 0).any()
    assert (seen > 0).all(), seen                                               # fallback, single and blended all happened


@pytest.mark.parametrize("build", BUILDS)
def test_edge_inputs_of_the_lookup_equal_the_statement_bit_for_bit(programs, build, tmp_path):
    nan = float("nan")
    # two probes equally far from the hits on x = 0; probe 0 without a fade band, probe 1 with one of 0.5
    two = np.array([[1.0, 0.5, 0.25, -1.0, -1.0, -1.0, 2.0, 2.0, 2.0, 0.0],
                    [-1.0, 0.5, 0.25, -2.0, -1.5, -1.0, 1.0, 1.5, 3.0, 0.5]])
    chains2 = re_.flat_chains(re_.random_chains(2, 90))
    Rs = np.array([[0.3, -0.7, 0.2], [0.0, 1.0, -2.0], [0.0, 0.0, 1.5], [0.0, 0.0, 0.0], [-0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])      # none, one, two and three zero components
    Ps = np.array([[2.0, 0.0, 0.0],          # on a face of box 0 alone (outside box 1): fade 0 gives w = 1
                   [1.0, 0.0, 0.0],          # on a face of box 1 (edge 0, w = 0) and inside box 0
                   [-1.5, 1.5, 0.0],         # on a face of box 1 alone: W = 0, the fall-back
                   [1.0, 0.5, 0.25],         # P = pos of probe 0
                   [0.5, 0.0, 0.0],          # edge / fade of probe 1 = 0.5 / 0.5 = exactly 1
                   [0.75, 0.0, 0.0],         # inside the band: 0.25 / 0.5
                   [0.0, 9.0, 0.0],          # in no box, equally far from both probes: the tie goes to probe 0
                   [0.0, 0.5, 0.25],         # inside both, equally far
                   [nan, 0.0, 0.0], [0.0, nan, 0.0], [0.5, 0.5, nan],      # a NaN fails every containment and is never nearer
                   [5.0, 5.0, 5.0], [-5.0, 0.0, 0.0]])
    P = np.repeat(Ps, len(Rs), 0)
    R = np.tile(Rs, (len(Ps), 1))
    for level in range(LEVELS):
        want = re_.lookup_detail(two, chains2, FACE, LEVELS, P, R, level)
        got = program_lookup(programs[build], tmp_path, two, chains2, FACE, LEVELS, P, R, level)
        assert bits(got) == bits(want["S"]), level
    d = re_.lookup_detail(two, chains2, FACE, LEVELS, Ps, np.tile(Rs[0], (len(Ps), 1)), 0)
    assert d["inside"][:, 0].tolist() == [True, False] and d["w"][0, 0] == 1.0 and d["route"][0] == 1
    assert d["inside"][:, 1].tolist() == [True, True] and d["w"][1, 1] == 0.0 and d["route"][1] == 1
    assert d["inside"][:, 2].tolist() == [False, True] and d["w"][1, 2] == 0.0 and d["route"][2] == 0 and d["kstar"][2] == 1
    assert d["w"][1, 4] == 1.0 and d["w"][1, 5] == 0.5 and d["route"][4] == 2
    assert d["route"][6] == 0 and d["kstar"][6] == 0 and d["route"][7] == 2
    assert (d["route"][8:11] == 0).all() and (d["kstar"][8:11] == 0).all() and not d["inside"][:, 8:11].any()
    assert d["kstar"][11] == 0 and d["kstar"][12] == 1
    # P = pos with R = 0 0 0: t = 0, D = 0 0 0, so D = R; and R with zero components leaves those axes out of t
    ins, w, D, t = re_.probe_terms(two[0], Ps[3:4].repeat(len(Rs), 0), Rs)
    assert t[3] == 0.0 and (D[3] == 0.0).all() and t[2] == (2.0 - 0.25) / 1.5 and t[5] == 1.0 and t[6] == 1.5
    # K = 1 and K = 64 on points that graze nothing
    rs = np.random.default_rng(43)
    for K in (1, 64):
        probes, chains = unit_box_tables(K, 5), re_.flat_chains(re_.random_chains(K, 7))
        Pk = np.concatenate([rs.uniform(-1.0, 2.0, (30, 3)), probes[:, 0:3][:8], probes[:, 3:6][:4], probes[:, 6:9][:4]])      # the positions and box corners too
        Rk = unit(rs.normal(size=(len(Pk), 3)))
        level = rs.integers(0, LEVELS, len(Pk))
        got = program_lookup(programs[build], tmp_path, probes, chains, FACE, LEVELS, Pk, Rk, level)
        assert bits(got) == bits(re_.lookup_detail(probes, chains, FACE, LEVELS, Pk, Rk, level)["S"]), K
    r = subprocess.run([programs[build], "edges"], capture_output=True, text=True)
    assert r.returncode == 0 and "edges: 0 bad" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr


def test_the_statement_s_texel_rule_is_the_package_s():
    rs = np.random.default_rng(44)
    D = np.concatenate([rs.normal(size=(300, 3)), np.eye(3), -np.eye(3), [[1.0, 1.0, 1.0], [-1.0, 1.0, -1.0], [0.5, -0.5, 0.1]]])
    for n in (1, 2, 8):
        assert np.array_equal(re_.texel_of(D, n), gi.cube_texel_of(D, n))
    bad = np.array([[np.nan, 1.0, 0.0], [0.0, 0.0, 0.0], [np.inf, 1.0, 1.0], [1.0, np.nan, np.nan]])
    t = re_.texel_of(bad, 8)
    assert ((t >= 0) & (t < 6 * 64)).all() and t[0] == 0 and t[1] == 0


# ---------------------------------------------------------------------------------------------------------------- 2. parallax
@pytest.mark.parametrize("build", BUILDS)
def test_a_direction_coded_cube_is_read_at_the_projected_direction(programs, build, tmp_path):
    chain = re_.flat_chains([re_.direction_chain(FACE, LEVELS)])
    probe = np.array([[0.2, -0.1, 0.3, -2.0, -1.0, -1.5, 2.0, 1.0, 1.5, 0.0]])
    rs = np.random.default_rng(45)
    P = rs.uniform([-1.9, -0.95, -1.4], [1.9, 0.95, 1.4], (400, 3))             # strictly inside the box
    R = unit(rs.normal(size=(400, 3)))
    level = rs.integers(0, LEVELS, 400)
    bound = np.sqrt(2.0) / (FACE >> level)
    ins, w, D, t = re_.probe_terms(probe[0], P, R)
    assert ins.all() and (w == 1.0).all() and (t > 0).all()
    Q = P + t[:, None] * R
    assert (np.abs((Q - probe[0, 3:6]) * (Q - probe[0, 6:9])).min(1) < 1e-12).all()      # Q lies on the box
    far = re_.angle_between(Q - probe[0, 0:3], R) > 2.0 * bound                  # the direction without parallax is elsewhere: only such P are asked
    assert far.sum() >= 100
    P, R, level, bound, Q = P[far], R[far], level[far], bound[far], Q[far]
    S, route = re_.lookup(probe, chain, FACE, LEVELS, P, R, level)
    assert (route == "single").all()
    assert (re_.angle_between(S, Q - probe[0, 0:3]) <= bound).all()
    assert (re_.angle_between(S, R) > bound).all()                              # so the look-up without parallax cannot pass
    got = program_lookup(programs[build], tmp_path, probe, chain, FACE, LEVELS, P, R, level)
    assert bits(got) == bits(S)
    assert (re_.angle_between(got, Q - probe[0, 0:3]) <= bound).all() and (re_.angle_between(got, R) > bound).all()


# ---------------------------------------------------------------------------------------------------------------- 3. the room the GPU tests have
@pytest.mark.parametrize("name", ["cornell", "spheres_opaque", "test_scene"])
def test_no_specular_sample_of_the_gpu_tests_changes_under_a_4_ulp_move(name):
    """tests/test_gpu_reflections.py allows 1 specular sample in 1 000 to take another route or texel on the device; on its frames, scenes, probes
    and Ks a move of every component of P and R by 4 ulp either way changes no containment, no route and no texel -- and all three routes occur."""
    base = pc.named_scene(name)
    scene = be.with_roughnesses(base)
    o, t = be.oracle_with_camera(scene, base.settings), scene.tables()
    assert name in fe.DRAW_FREE_SCENES
    flipped = asked = 0
    routes = np.zeros(3, np.int64)
    for (w, h) in SIZES:
        for s in range(N):
            g = be.sample_hits(o, t, w, h, s)
            f, a = be.texel_flips_under_perturbation(g, t, FACE, LEVELS, be.CHAIN_EXPONENTS)
            assert f == 0
            for K in re_.KS:
                probes = re_.random_probes(t, K)
                f, a = re_.flips_under_perturbation(g, t, probes, FACE, LEVELS, be.CHAIN_EXPONENTS)
                flipped += f; asked += a
                _, route = re_.sample_specular(g, t, probes, np.zeros((K, be.chain_offsets(FACE, LEVELS)[-1], 3)), be.CHAIN_EXPONENTS)
                routes += np.bincount(route[route >= 0], minlength=3)
            if name == "cornell":                                                # the end-to-end parallax test's probe
                f, a = re_.flips_under_perturbation(g, t, re_.scene_box_probe(t), FACE, LEVELS, be.CHAIN_EXPONENTS)
                flipped += f; asked += a
    print(f"{name}: {flipped} of {asked} specular samples change a containment, a route or a texel under a 4-ulp move; routes {dict(zip(re_.ROUTES, routes.tolist()))}")
    assert flipped == 0 and asked > 0
    assert (routes > 0).all(), routes


# ---------------------------------------------------------------------------------------------------------------- 4. the binding and the command line
def test_default_params_and_the_binding_s_checks():
    L = gi.lib()
    p = gi.BakedReflectionsParams()
    p.n_probes = 7
    L.gi_baked_reflections_default_params(p)
    assert p.n_probes == 0
    L.gi_baked_reflections_default_params(None)                                 # a null block is left alone
    assert gi.REFLECTIONS_MAX_PROBES == 64
    for name in ("gi_baked_reflections_default_params", "gi_render_baked_reflections_host", "gi_render_baked_reflections_device"):
        assert name in gi.ABI_SYMBOLS and hasattr(L, name)
    probes = unit_box_tables(3, 1)
    chains = re_.random_chains(3, 2)
    rp, t, c, face, levels = gi.baked_reflections_params(probes, chains)
    assert (rp.n_probes, face, levels) == (3, FACE, LEVELS) and bits(t) == bits(probes) and bits(c) == bits(re_.flat_chains(chains)) and c.shape == (3, be.chain_offsets(FACE, LEVELS)[-1], 3)
    rp, t, c, face, levels = gi.baked_reflections_params(probes, re_.flat_chains(chains))          # the flat form: face and levels are the caller's
    assert rp.n_probes == 3 and face is None and levels is None and bits(c) == bits(re_.flat_chains(chains))
    rp, t, c, face, levels = gi.baked_reflections_params(None, None)
    assert rp.n_probes == 0 and t is None and c is None
    assert gi.baked_reflections_params(np.zeros((0, 10)), [])[0].n_probes == 0

    def changed(k, j, v):
        q = probes.copy()
        q[k, j] = v
        return q

    other = [be.random_chain(3, 4, 3)]                                          # a chain of another face
    for kw in (dict(probes=probes[:, :9], chains=chains), dict(probes=probes[0], chains=chains[:1]), dict(probes=probes, chains=chains[:2]), dict(probes=probes, chains=None),
               dict(probes=None, chains=chains), dict(probes=np.zeros((65, 10)) + probes[0], chains=chains * 22), dict(probes=changed(1, 0, float("nan")), chains=chains),
               dict(probes=changed(2, 9, float("inf")), chains=chains), dict(probes=changed(0, 9, -0.1), chains=chains), dict(probes=changed(1, 6, probes[1, 3]), chains=chains),
               dict(probes=changed(1, 8, probes[1, 5] - 1.0), chains=chains), dict(probes=probes, chains=chains[:2] + other), dict(probes=probes, chains=chains[:2] + [chains[2][:2] + chains[2][1:2]]),
               dict(probes=probes, chains=re_.flat_chains(chains)[:, :, :2])):
        with pytest.raises(ValueError):
            gi.baked_reflections_params(**kw)


def test_reflection_probe_cells_overlap_by_twice_the_fade_with_probes_at_the_centres():
    box = np.array([-1.0, 0.5, -2.0, 3.0, 2.0, 0.25])
    for (nx, ny, nz), fade in (((2, 1, 1), 0.125), ((3, 2, 4), 0.0625), ((1, 1, 1), 0.0), ((4, 4, 4), 0.5)):
        t = gi.reflection_probe_cells(box, nx, ny, nz, fade)
        assert t.shape == (nx * ny * nz, 10) and t.dtype == np.float64 and (t[:, 9] == fade).all()
        assert bits(t[:, 0:3]) == bits(gi.probe_grid(box, nx, ny, nz).reshape(-1, 3))                      # the probes sit at the cells' centres
        assert np.allclose(t[:, 0:3], 0.5 * (t[:, 3:6] + t[:, 6:9]), rtol=0, atol=1e-15 * 8)
        g = t.reshape(nz, ny, nx, 10)
        for axis, n in ((2, nx), (1, ny), (0, nz)):
            k = 2 - axis
            lo, hi = np.moveaxis(g[..., 3 + k], axis, 0), np.moveaxis(g[..., 6 + k], axis, 0)
            assert (lo[0] == box[k] - fade).all() and (hi[-1] == box[3 + k] + fade).all()                  # together the cells cover the box grown by fade
            if n > 1:
                assert np.allclose(hi[:-1] - lo[1:], 2.0 * fade, rtol=0, atol=1e-15 * 8)                   # neighbours overlap by 2 * fade
                cell = (box[3 + k] - box[k]) / n
                assert np.allclose(hi - lo, cell + 2.0 * fade, rtol=0, atol=1e-15 * 8)
        rp, tt, c, face, levels = gi.baked_reflections_params(t, np.zeros((len(t), 6, 3)))               # a table the binding takes
        assert rp.n_probes == len(t)
    # the middle of the overlap band between two cells is in both boxes, a cell's middle in its own alone
    t = gi.reflection_probe_cells(box, 2, 1, 1, 0.125)
    mid = np.array([[1.0, 1.0, -1.0], [0.0, 1.0, -1.0]])
    d = re_.lookup_detail(t, np.zeros((2, 6, 3)), 1, 1, mid, np.array([[0.0, 1.0, 0.0]] * 2), 0)
    assert d["inside"][:, 0].all() and d["route"][0] == 2 and (d["w"][:, 0] == 1.0).all() and d["inside"][:, 1].tolist() == [True, False]
    for bad in (dict(nx=0, ny=1, nz=1, fade=0.1), dict(nx=5, ny=5, nz=3, fade=0.1), dict(nx=1, ny=1, nz=1, fade=-0.1), dict(nx=1, ny=1, nz=1, fade=float("nan"))):
        with pytest.raises(ValueError):
            gi.reflection_probe_cells(box, **bad)
    with pytest.raises(ValueError):
        gi.reflection_probe_cells([0, 0, 0, 1, 0, 1], 1, 1, 1, 0.1)


@pytest.mark.parametrize("args", [["--baked-reflections", "2", "1", "1"], ["--baked-reflection-fade", "0.1"], ["--baked", "b", "--baked-reflection-fade", "0.1"],
                                  ["--baked", "b", "--baked-reflections", "2", "1", "1", "--baked-lightmap", "8", "8"],
                                  ["--baked", "b", "--baked-reflections", "2", "1", "1", "--probe-visibility", "4"],
                                  ["--baked", "b", "--baked-reflections", "0", "1", "1"], ["--baked", "b", "--baked-reflections", "5", "5", "3"],
                                  ["--baked", "b", "--baked-reflections", "2", "1", "1", "--baked-reflection-fade", "-1"],
                                  ["--baked", "b", "--baked-reflections", "2", "1", "1", "--baked-reflection-fade", "nan"],
                                  ["--baked", "b", "--baked-reflections", "2", "1", "1", "--baked-reflection", "0", "0", "0"],
                                  ["--probes", "2", "2", "2", "--baked-reflections", "2", "1", "1"]])
def test_command_line_refuses_before_it_touches_the_device(args):
    with pytest.raises(SystemExit) as e:
        cli.main([os.path.join(ROOT, pc.SCN["cornell"])] + args)
    assert e.value.code == 2


def test_command_line_takes_the_flags():
    ap = cli.parser()
    a = ap.parse_args(["s.scn", "--baked", "lit", "--baked-reflections", "4", "4", "4", "--baked-reflection-fade", "0.25"])
    cli.check_args(ap, a)
    assert a.baked_reflections == [4, 4, 4] and a.baked_reflection_fade == 0.25
    a = ap.parse_args(["s.scn", "--baked", "lit", "--baked-reflections", "2", "1", "1"])
    cli.check_args(ap, a)
    assert a.baked_reflection_fade is None
