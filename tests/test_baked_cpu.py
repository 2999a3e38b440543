"""The baked-light pass without a GPU: the per-lane functions of gi_baked.h compiled for the host as a program of its own (tests/cpp/baked_lookup.cpp),
plainly and under the sanitizers, bit for bit against the numpy statement (tests/baked_expect.py) on random points, normals, grids and directions
and on its edge inputs; the room the statement's texel choice has on the GPU tests' own frames; the binding's parameter block and the command
line's refusals."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer"]
BUILDS = ["plain", "sanitized"]


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("baked_lookup")
    out = {}
    for name, extra in (("plain", []), ("sanitized", SANITIZE)):
        out[name] = str(d / f"baked_lookup_{name}")
        subprocess.run([os.environ.get("CXX", "g++")] + host_build.flags() + extra + [os.path.join(ROOT, "tests", "cpp", "baked_lookup.cpp"), "-o", out[name]], check=True)
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


# ---------------------------------------------------------------------------------------------------------------- the per-lane functions
@pytest.mark.parametrize("build", BUILDS)
def test_host_build_of_the_grid_cell_equals_the_statement_bit_for_bit(programs, build):
    rs = np.random.default_rng(11)
    for n in (1, 2, 3, 7, 64):
        gmin, gmax = -1.25, 2.5
        p = np.concatenate([rs.uniform(-3.0, 4.0, 60), [gmin, gmax, np.nextafter(gmin, 9.0), np.nextafter(gmax, -9.0)], gmin + (gmax - gmin) * (np.arange(n + 1) / n)])
        got = run_program(programs[build], "cell", gmin, gmax, n, *hexes(p))
        i0, i1, t = be.grid_cell(p, gmin, gmax, n)
        assert bits(got) == bits(np.stack([i0, i1, t], 1)), n
        assert (i0 >= 0).all() and (i1 <= n - 1).all() and (t >= 0).all() and (t < 1).all()
        assert (i0 == 0).any() and (i1 == n - 1).any()                                       # both clamps happen


@pytest.mark.parametrize("build", BUILDS)
def test_host_build_of_the_sh_factors_equals_the_statement_bit_for_bit(programs, build):
    n = np.concatenate([unit(np.random.default_rng(12).normal(size=(40, 3))), np.eye(3), -np.eye(3)])
    got = run_program(programs[build], "factor", *hexes(n))
    assert got.shape == (len(n), 9) and bits(got) == bits(be.sh9_factor(n))
    # the factors are the cosine lobe's over pi: a constant environment of radiance 1 (c0 = sqrt(4 pi), the rest 0) gives D = 1 for every normal
    assert np.allclose(be.sh9_factor(n)[:, 0] * np.sqrt(4.0 * np.pi), 1.0, rtol=1e-15)


@pytest.mark.parametrize("build", BUILDS)
def test_host_build_of_the_texel_choice_equals_the_statement(programs, build):
    rs = np.random.default_rng(13)
    d = np.concatenate([unit(rs.normal(size=(80, 3))), 7.5 * rs.normal(size=(20, 3)), [[1, 1, 0.5], [-1, 1, 1], [0.25, -1, 1], [0, 0, -2], [0, 3, 0]]])
    for n in (1, 2, 8, 32):
        got = run_program(programs[build], "texel", n, *hexes(d))[:, 0]
        assert np.array_equal(got, gi.cube_texel_of(d, n)), n
        assert np.array_equal(got, be.chain_texel(d, np.zeros(len(d), np.int64), n, 1))


@pytest.mark.parametrize("build", BUILDS)
def test_host_build_of_the_level_table_equals_the_statement(programs, build):
    rs = np.random.default_rng(14)
    rough = np.concatenate([10.0 ** rs.uniform(-4, 0, 60), [0.0, 0.0005, 0.001, 0.5, 0.9, 1.0]])
    seen = set()
    for exponents in ((0,), (0, 7), (0, 5, 1), (0, 13, 10, 7, 4, 1), (0, 1, 5, 3)):
        levels = len(exponents)
        got = run_program(programs[build], "level", levels, *exponents, *hexes(rough))[:, 0]
        want = be.level_table(rough, levels, exponents)
        assert np.array_equal(got, want), exponents
        assert (want[rough < .001] == 0).all() and (levels == 1 or (want[rough >= .001] >= 1).all())
        seen |= set(want.tolist())
    assert seen == {0, 1, 2, 3, 4, 5}
    assert be.level_table([0.5, 0.05, 0.0005, 1.0], 3, (0, 5, 1)).tolist() == [2, 1, 0, 2]      # log2(3) = 1.58, log2(21) = 4.39, a mirror, log2(2) = 1
    assert be.level_table([1.0 / 7.0], 3, (0, 4, 2)).tolist() == [1]                             # log2(8) = 3: a tie, the lower level


def filled(n, seed):
    """fill() of tests/cpp/baked_lookup.cpp."""
    i = np.arange(n, dtype=np.uint64)
    return ((i * np.uint64(2654435761) + np.uint64(seed)) & np.uint64(0xFFFFFFFF)).astype(np.float64) / 4294967296.0 * 1.25 - 0.25


@pytest.mark.parametrize("build", BUILDS)
def test_host_build_of_the_grid_lookup_equals_the_statement_bit_for_bit(programs, build):
    rs = np.random.default_rng(15)
    for (nx, ny, nz) in be.GRIDS:
        box = np.array([-1.0, 0.5, -2.0, 1.5, 2.0, 0.25])
        sh = filled(nx * ny * nz * 27, 5).reshape(nz, ny, nx, 9, 3)
        P = np.concatenate([rs.uniform(-2.5, 2.5, (60, 3)), [box[:3], box[3:]]])      # inside and outside the box: clamping happens
        N = unit(rs.normal(size=(len(P), 3)))
        got = run_program(programs[build], "grid", nx, ny, nz, *hexes(box), 5, *hexes(np.concatenate([P, N], 1)))
        want = be.irradiance(sh, box, P, N)
        assert bits(got) == bits(want), (nx, ny, nz)
        assert (want >= 0).all() and (want == 0).any() and (want > 0).any()             # the clamp at 0 happens


@pytest.mark.parametrize("build", BUILDS)
def test_edge_inputs_stay_inside_their_tables(programs, build):
    r = subprocess.run([programs[build], "edges"], capture_output=True, text=True)
    assert r.returncode == 0 and "edges: 0 bad" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr


# ---------------------------------------------------------------------------------------------------------------- the GPU tests' own frames
@pytest.mark.parametrize("name", ["cornell", "spheres_opaque", "test_scene"])
def test_no_reflection_of_the_gpu_tests_frames_lies_within_4_ulp_of_a_texel_border(name):
    """tests/test_gpu_baked.py allows the device's texel to differ from the statement's for 1 sample in 1 000; on its frames none should."""
    base = pc.load_scene(name)
    scene = be.with_roughnesses(base)
    o, t = be.oracle_with_camera(scene, base.settings), scene.tables()
    assert name in fe.DRAW_FREE_SCENES and fe.oracle_is_draw_free(o, fe.sample_rays(o, 24, 16, 0)[0])
    flipped = asked = 0
    lobes = set()
    for s in range(2):
        g = be.sample_hits(o, t, 24, 16, s)
        f, a = be.texel_flips_under_perturbation(g, t, be.CHAIN_FACE, be.CHAIN_LEVELS, be.CHAIN_EXPONENTS)
        flipped += f; asked += a
        lobes |= set(be.sample_terms(g, t)[3].tolist())
    print(f"{name}: {flipped} of {asked} reflections change their texel under a 4-ulp move")
    assert flipped == 0 and asked > 0
    assert lobes >= {1, 2}, lobes                                                       # glossy and diffuse hits in every scene's frame


def test_all_three_lobes_are_hit_over_the_scenes():
    lobes = set()
    for name in ("cornell", "spheres_opaque", "test_scene"):
        base = pc.load_scene(name)
        scene = be.with_roughnesses(base)
        g = be.sample_hits(be.oracle_with_camera(scene, base.settings), scene.tables(), 24, 16, 0)
        lobes |= set(be.sample_terms(g, scene.tables())[3].tolist())
    assert lobes >= {0, 1, 2}, lobes


# ---------------------------------------------------------------------------------------------------------------- the binding and the command line
def test_default_params_and_the_binding_s_checks():
    L = gi.lib()
    p = gi.BakedParams()
    L.gi_baked_default_params(p)
    assert (p.n_samples, p.terms, p.nx, p.ny, p.nz, p.face, p.levels) == (4, gi.BAKED_DIRECT | gi.BAKED_EMISSIVE, 1, 1, 1, 32, 1)
    assert list(p.grid_min) == [0, 0, 0] and list(p.grid_max) == [1, 1, 1] and list(p.log2_exponent) == [16, 13, 10, 7, 4, 1, 0, 0, 0, 0, 0, 0]
    sh, chain, box = be.random_sh((3, 2, 4), 1), be.random_chain(2), (0, 0, 0, 1, 2, 3)
    bp, s, c = gi.baked_params(n=2, sh=sh, grid_box=box, chain=chain, exponents=be.CHAIN_EXPONENTS)
    assert (bp.nx, bp.ny, bp.nz, bp.face, bp.levels, bp.terms) == (3, 2, 4, 8, 3, 15) and list(bp.log2_exponent)[:3] == [0, 5, 1]
    assert list(bp.grid_max) == [1, 2, 3] and s.shape == sh.shape and c.shape == (6 * (64 + 16 + 4), 3)
    assert bits(c[:384]) == bits(chain[0].reshape(-1, 3)) and bits(c[384:480]) == bits(chain[1].reshape(-1, 3))
    assert gi.baked_params(n=1)[0].terms == gi.BAKED_DIRECT | gi.BAKED_EMISSIVE
    assert gi.baked_params(n=1, sh=sh, grid_box=box, terms=gi.BAKED_DIFFUSE)[0].terms == gi.BAKED_DIFFUSE
    for kw in (dict(n=0), dict(sh=sh), dict(sh=sh[0], grid_box=box), dict(sh=sh, grid_box=(0, 0, 0, 1, 0, 3)), dict(sh=sh, grid_box=(0, 0, 0, 1, 2, float("nan"))),
               dict(grid_box=box), dict(chain=chain[1:] + chain[:1]), dict(chain=[chain[0][:, :, :7]]), dict(chain=[np.zeros((6, 6, 6, 3))] * 3), dict(exponents=(0, 1)),
               dict(chain=chain, exponents=(0, 17, 1)), dict(terms=0), dict(terms=16), dict(terms=gi.BAKED_DIFFUSE), dict(terms=gi.BAKED_SPECULAR, sh=sh, grid_box=box),
               dict(n=480, width=3840, height=2160)):
        with pytest.raises(ValueError):
            gi.baked_params(**kw)


@pytest.mark.parametrize("args", [["--baked-samples", "2"], ["--baked-probes", "2", "2", "2"], ["--baked-reflection", "0", "1", "0"], ["--baked", "b", "--probes", "2", "2", "2"],
                                  ["--baked", "b", "--lightmap", "8", "8"], ["--baked", "b", "--reflection-probe", "0", "1", "0"], ["--baked", "b", "--baked-samples", "0"],
                                  ["--baked", "b", "--baked-probes", "2", "0", "2"], ["--baked", "b", "--baked-reflection", "0", "inf", "0"],
                                  ["--baked", "b", "-o", "b.ppm"]])
def test_command_line_refuses_before_it_touches_the_device(args):
    with pytest.raises(SystemExit) as e:
        cli.main([os.path.join(ROOT, pc.SCN["cornell"])] + args)
    assert e.value.code == 2


def test_command_line_keeps_the_frame_and_the_preview_apart():
    ap = cli.parser()
    a = ap.parse_args(["s.scn", "--baked", "out", "--samples", "4", "4"])
    cli.check_args(ap, a)
    assert a.output == "out_frame.ppm" and a.baked == "out"
    a = ap.parse_args(["s.scn", "--baked", "lit", "--occlusion", "ao", "--aperture", "0.1"])      # goes with the frame's flags
    cli.check_args(ap, a)
    assert a.output == "out.ppm"
    a = ap.parse_args(["s.scn"])
    cli.check_args(ap, a)
    assert a.output == "out.ppm" and a.baked is None
