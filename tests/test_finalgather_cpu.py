"""The final-gather pass without a GPU: the walk-free per-lane functions of gi_finalgather.h compiled for the host as a program of its own
(tests/cpp/finalgather_lookup.cpp), plainly and under the sanitizers, bit for bit against the numpy statement (tests/finalgather_expect.py) on
random inputs and on the edge inputs; the binding's parameter block; the command line's refusals; and the two measurements the GPU tests'
allowance is made of -- the room the oracle has on the gather rays of the GPU tests' frames, and how far a 4-ulp move of d_j and of i_Q moves a
pixel's diffuse term."""
import os
import subprocess

import numpy as np
import pytest

import gi_raytracer_amd as gi
import gi_raytracer_amd.__main__ as cli

import baked_expect as be
import features_expect as fe
import finalgather_expect as fg
import host_build
import parity_checks as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer"]
BUILDS = ["plain", "sanitized"]
FACE, LEVELS = be.CHAIN_FACE, be.CHAIN_LEVELS
N = 2
DIRS = (1, 4, 5)
LEVEL_COLOURS = ((0.5, 2.0, 0.125), (1.5, 0.25, 1.0), (0.75, 0.5, 3.0))


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("finalgather_lookup")
    out = {}
    for name, extra in (("plain", []), ("sanitized", SANITIZE)):
        out[name] = str(d / f"finalgather_lookup_{name}")
        subprocess.run([os.environ.get("CXX", "g++")] + host_build.flags() + extra + [os.path.join(ROOT, "tests", "cpp", "finalgather_lookup.cpp"), "-o", out[name]], check=True)
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float64).tobytes()


def hexes(a):
    return [float(v) for v in np.asarray(a, np.float64).reshape(-1)]


def run(exe, tmp_path, mode, numbers):
    path = tmp_path / f"{mode}.txt"
    path.write_text("\n".join(float(v).hex() for v in numbers))
    r = subprocess.run([exe, mode, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
    return np.array([[float.fromhex(t) for t in ln.split()] for ln in r.stdout.split("\n") if ln])


def program_lookup(exe, tmp_path, sh, box, chain, level_of_mat, Q, nf, color, emissive, rough, mat, d, i):
    nz, ny, nx = sh.shape[:3]
    head = [nx, ny, nz] + hexes(box) + [FACE if chain is not None else 0, len(chain) if chain is not None else 0, len(level_of_mat), len(Q)]
    flat = np.concatenate([c.reshape(-1, 3) for c in chain]) if chain is not None else np.zeros((0, 3))
    rows = np.concatenate([Q, nf, color, emissive, rough[:, None], mat[:, None].astype(np.float64), d, i], 1)
    return run(exe, tmp_path, "lookup", head + hexes(sh) + hexes(flat) + hexes(level_of_mat) + hexes(rows))


def unit(v):
    return v / np.sqrt((v * v).sum(-1))[..., None]


def rows_for(rs, n):
    Q = rs.uniform(-2.0, 2.0, (n, 3))                                   # the grid box is -1 .. 1: most Q are outside it and clamp
    nf = unit(rs.normal(size=(n, 3)))
    color, emissive, i = rs.uniform(0, 1, (n, 3)), rs.uniform(0, 2, (n, 3)) * (rs.uniform(size=(n, 1)) < 0.3), rs.uniform(0, 3, (n, 3))
    rough = rs.choice(np.array(be.ROUGHNESSES + (0.9, 0.001)), n)
    mat = rs.integers(0, 4, n)
    d = unit(rs.normal(size=(n, 3)))
    return Q, nf, color, emissive, rough, mat, d, i


# ---------------------------------------------------------------------------------------------------------------- 1. bit for bit against the statement
@pytest.mark.parametrize("build", BUILDS)
def test_host_build_of_the_secondary_shade_equals_the_statement(programs, build, tmp_path):
    rs = np.random.default_rng(51)
    box = np.array([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0])
    level_of_mat = np.array([0, 1, 2, 1])
    seen = set()
    for grid in be.GRIDS:
        sh = be.random_sh(grid, 60 + grid[0])
        for chain in (be.random_chain(61), None):                         # a specular Q with and without a chain
            args = rows_for(rs, 150)
            want = fg.lookup(sh, box, chain, level_of_mat, *args)
            got = program_lookup(programs[build], tmp_path, sh, box, chain, level_of_mat, *args)
            assert got.shape == (150, 3) and bits(got) == bits(want), (grid, chain is None)
            Q, rough = args[0], args[4]
            outside = ((Q < -1) | (Q > 1)).any(1)
            seen |= {("diffuse", bool(o)) for o in outside[rough >= .9]} | {("specular", chain is not None)}
            if chain is None:                                             # without a chain a specular Q is base_Q alone
                s = rough < .9
                assert bits(want[s]) == bits((args[3] + args[2] * args[7])[s])
    assert seen == {("diffuse", True), ("diffuse", False), ("specular", True), ("specular", False)}
    # edge rows: a NaN normal, a Q far outside the box and at its corners, NaN and infinite Q, a zero direction
    nan, inf = float("nan"), float("inf")
    Q = np.array([[0.1, 0.2, 0.3], [50.0, -50.0, 1e300], [1.0, 1.0, 1.0], [-1.0, -1.0, -1.0], [nan, 0.0, 0.0], [inf, -inf, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    nf = np.array([[nan, 0.0, 1.0], [0.0, 1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 1.0, 0.0], [0.0, 1.0, 0.0], [nan, nan, nan]])
    n = len(Q)
    d = np.array([[0.0, -1.0, 0.0]] * (n - 2) + [[0.0, 0.0, 0.0], [0.3, -0.4, 0.5]])
    sh, chain = be.random_sh((3, 2, 4), 62), be.random_chain(63)
    for rough in (1.0, 0.5, 0.0005):
        args = (Q, nf, np.full((n, 3), 0.5), np.full((n, 3), 0.25), np.full(n, rough), np.arange(n) % 4, d, np.full((n, 3), 1.5))
        with np.errstate(invalid="ignore"):
            want = fg.lookup(sh, box, chain, level_of_mat, *args)
        got = program_lookup(programs[build], tmp_path, sh, box, chain, level_of_mat, *args)
        assert bits(got) == bits(want), rough
        if rough >= .9:                                                   # a NaN normal poisons the grid's factors; a Q anywhere reads finite probes
            assert np.isnan(want[0]).any() and np.isfinite(want[1:7]).all()
        else:                                                             # a NaN or zero R reads texel 0 of its level: finite
            assert np.isfinite(want).all()
    r = subprocess.run([programs[build], "edges"], capture_output=True, text=True)
    assert r.returncode == 0 and "edges: 0 bad" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr


@pytest.mark.parametrize("build", BUILDS)
def test_host_build_of_the_fold_equals_the_statement(programs, build, tmp_path):
    rs = np.random.default_rng(52)
    ambient = np.array([0.25, 0.5, 1.5])
    for dirs in (1, 4, 5, 64):                                           # the ends of n_dirs, and a count that is no power of two
        color, L = rs.uniform(0, 1, 3), rs.uniform(0, 4, (dirs, 3))
        got = run(programs[build], tmp_path, "fold", [dirs] + hexes(color) + hexes(L))
        assert bits(got[0]) == bits(fg.fold_rows(color, L)), dirs
        miss = run(programs[build], tmp_path, "fold", [dirs] + hexes(color) + hexes(np.tile(ambient, (dirs, 1))))      # every ray a miss
        assert bits(miss[0]) == bits(fg.fold_rows(color, np.tile(ambient, (dirs, 1))))
        if dirs in (1, 4, 64):
            assert bits(miss[0]) == bits(color * ambient)                # a power of two of equal addends divides back exactly
    for bad in ([0, 1, 1, 1], [65, 1, 1, 1] + [0.0] * 195):
        path = tmp_path / "bad.txt"
        path.write_text("\n".join(float(v).hex() for v in bad))
        assert subprocess.run([programs[build], "fold", str(path)], capture_output=True).returncode == 2


# ---------------------------------------------------------------------------------------------------------------- 2. the binding and the command line
def test_default_params_and_the_binding_s_checks():
    L = gi.lib()
    p = gi.FinalGatherParams()
    p.n_dirs, p.reserved = 3, 9
    L.gi_final_gather_default_params(p)
    b = gi.BakedParams()
    L.gi_baked_default_params(b)
    assert (p.n_dirs, p.reserved) == (16, 0) and p.baked.terms == be.DIRECT | be.DIFFUSE | be.EMISSIVE and p.baked.n_samples == b.n_samples == 4
    assert (p.baked.nx, p.baked.face, p.baked.levels, list(p.baked.log2_exponent)) == (b.nx, b.face, b.levels, list(b.log2_exponent))
    L.gi_final_gather_default_params(None)                               # a null block is left alone
    assert gi.FINAL_GATHER_MAX_DIRS == 64 and gi.STRUCTS["gi_final_gather_params"] is gi.FinalGatherParams
    for name in ("gi_final_gather_default_params", "gi_render_final_gather_host", "gi_render_final_gather_device", "gi_last_final_gather_ms"):
        assert name in gi.ABI_SYMBOLS and hasattr(L, name)
    for name in ("run_final_gather", "run_final_gather_device", "last_final_gather_ms"):
        assert hasattr(gi.RayTracer, name)
    sh, chain = be.random_sh((3, 2, 4), 1), be.random_chain(2)
    box = [0, 0, 0, 1, 2, 3]
    fp, s, c = gi.final_gather_params(n=2, dirs=5, sh=sh, grid_box=box, chain=chain, exponents=be.CHAIN_EXPONENTS)
    assert (fp.n_dirs, fp.reserved, fp.baked.n_samples, fp.baked.terms) == (5, 0, 2, 15) and (fp.baked.nx, fp.baked.ny, fp.baked.nz) == (3, 2, 4)
    assert (fp.baked.face, fp.baked.levels) == (FACE, LEVELS) and bits(s) == bits(sh) and c.shape == (be.chain_offsets(FACE, LEVELS)[-1], 3)
    fp, s, c = gi.final_gather_params(sh=sh, grid_box=box, chain=chain, exponents=be.CHAIN_EXPONENTS, terms=be.DIFFUSE)      # a chain for the secondary hits alone
    assert fp.n_dirs == 16 and fp.baked.terms == be.DIFFUSE and c is not None and fp.baked.face == FACE
    for kw in (dict(dirs=0), dict(dirs=65), dict(dirs=-1), dict(dirs=1.5), dict(dirs="4"), dict(n=0), dict(terms=be.DIFFUSE), dict(terms=be.SPECULAR), dict(terms=16),
               dict(sh=sh), dict(sh=sh, grid_box=[0, 0, 0, 1, 1, 0]), dict(n=2 ** 31, width=24, height=16)):
        with pytest.raises(ValueError):
            gi.final_gather_params(**kw)


@pytest.mark.parametrize("args", [["--final-gather", "4"], ["--baked", "b", "--final-gather", "0"], ["--baked", "b", "--final-gather", "65"],
                                  ["--baked", "b", "--final-gather", "4", "--baked-lightmap", "8", "8"], ["--baked", "b", "--final-gather", "4", "--probe-visibility", "4"],
                                  ["--baked", "b", "--final-gather", "4", "--baked-reflections", "2", "1", "1"],
                                  ["--baked", "b", "--final-gather", "4", "--baked-samples", "0"], ["--baked", "b", "--final-gather", "4", "--baked-probes", "0", "1", "1"]])
def test_command_line_refuses_before_it_touches_the_device(args):
    with pytest.raises(SystemExit) as e:
        cli.main([os.path.join(ROOT, pc.SCN["cornell"])] + args)
    assert e.value.code == 2


def test_command_line_takes_the_flag():
    ap = cli.parser()
    a = ap.parse_args(["s.scn", "--baked", "lit", "--final-gather", "8"])
    cli.check_args(ap, a)
    assert a.final_gather == 8
    a = ap.parse_args(["s.scn", "--baked", "lit"])
    cli.check_args(ap, a)
    assert a.final_gather is None


# ---------------------------------------------------------------------------------------------------------------- 3. the room the GPU tests have
@pytest.mark.parametrize("name", ["cornell", "test_scene", "spheres_opaque"])
def test_the_oracle_flips_no_gather_ray_and_the_allowance_is_the_measured_one(name):
    """tests/test_gpu_finalgather.py allows 1 gather ray in 1 000 to hit another entity on the device.  On its frames (fg.FRAMES) the oracle alone
    flips none under a 4-ulp move of every component of d_j.  The same move, and a 4-ulp move of i_Q, change a pixel's diffuse term by at most
    fg.DELTA_DIRS and fg.DELTA_POW of the pixel's value floored at 1e-6 of the frame's largest: what the GPU tests' allowance, 16 times their
    sum, is made of."""
    base = pc.named_scene(name)
    scene = be.with_roughnesses(base)
    o, t = be.oracle_with_camera(scene, base.settings), scene.tables()
    assert name in fe.DRAW_FREE_SCENES
    box = be.inner_box(t)
    chain = [np.ascontiguousarray(np.broadcast_to(np.array(c), (6, FACE >> l, FACE >> l, 3))) for l, c in enumerate(LEVEL_COLOURS)]
    flipped = asked = 0
    delta_d = delta_i = 0.0
    kinds = np.zeros(4, np.int64)
    for k, (w, h) in enumerate(fg.FRAMES[name]):
        sh = be.random_sh(be.GRIDS[1 + k], 101 + k)
        hits = [be.sample_hits(o, t, w, h, s) for s in range(N)]
        for dirs in DIRS:
            a = fg.expected_final_gather(o, t, w, h, N, dirs, sh, box, chain, be.CHAIN_EXPONENTS, hits=hits)
            for rows in a["rows"]:
                f, n = fg.flips_under_perturbation(o, rows)
                flipped += f; asked += n
            kinds += np.bincount(a["kind"][a["kind"] >= 0], minlength=4)
            for u in (4, -4):
                b = fg.expected_final_gather(o, t, w, h, N, dirs, sh, box, chain, be.CHAIN_EXPONENTS, hits=hits, d_ulps=u)
                c = fg.expected_final_gather(o, t, w, h, N, dirs, sh, box, chain, be.CHAIN_EXPONENTS, hits=hits, i_ulps=u)
                assert np.array_equal(b["ids"], a["ids"])
                delta_d = max(delta_d, fg.relative_change(b["diffuse"], a["diffuse"]))
                delta_i = max(delta_i, fg.relative_change(c["diffuse"], a["diffuse"]))
    print(f"{name}: {flipped} of {asked} gather rays hit another entity under a 4-ulp move of d_j; the move changes a pixel's diffuse term by {delta_d:.3e} at the most, "
          f"a 4-ulp move of i_Q by {delta_i:.3e}; kinds {kinds.tolist()}")
    assert flipped == 0 and asked > 0
    assert delta_d <= fg.DELTA_DIRS and delta_i <= fg.DELTA_POW
    assert fg.ALLOWANCE == 16.0 * (fg.DELTA_DIRS + fg.DELTA_POW)
    assert kinds[0] > 0 and kinds[2] > 0 and kinds[3] > 0, kinds           # misses, diffuse-lobe Q outside the grid box, specular Q
