"""Reflection probes without a GPU: the per-lane functions of gi_cubemap.h compiled for the host as a program of its own (tests/cpp/cubemap_kat.cpp),
plainly and under the sanitizers, bit for bit against the numpy statement (tests/cubemap_expect.py); properties of that statement; the package's
cube_directions / cube_texel_of; the command line's refusals; and a capture at the centre of the Cornell box through the oracle alone."""
import os
import subprocess

import numpy as np
import pytest

import gi_raytracer_amd as gi
import gi_raytracer_amd.__main__ as cli

import bake_expect as be
import cubemap_expect as ce
import host_build
import parity_checks as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer"]
FACES = (1, 2, 3, 5)
BELOW_ONE = float(np.nextafter(np.float32(1.0), np.float32(0.0)))           # the largest float below 1: the largest jitter the sampler returns
JITTERS = (0.0, 0.5, BELOW_ONE)
EXPONENTS = (0, 1, 16)


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("cubemap_kat")
    out = {}
    for name, extra in (("plain", []), ("sanitized", SANITIZE)):
        out[name] = str(d / f"cubemap_kat_{name}")
        subprocess.run([os.environ.get("CXX", "g++")] + host_build.flags() + extra + [os.path.join(ROOT, "tests", "cpp", "cubemap_kat.cpp"), "-o", out[name]], check=True)
    return out


def run_program(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    return np.array([[float.fromhex(t) for t in ln.split()] for ln in r.stdout.split("\n") if ln])


def bits(a):
    return np.ascontiguousarray(a, np.float64).tobytes()


# ---------------------------------------------------------------------------------------------------------------- the per-lane functions
@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_host_build_of_directions_and_measure_equals_the_statement_bit_for_bit(programs, build):
    for n in FACES:
        for ju in JITTERS:
            for jv in JITTERS:
                got = run_program(programs[build], "dirs", n, float(ju).hex(), float(jv).hex())
                f, a, b = ce.coords(n, ju, jv)
                u = ce.face_dirs(f, a, b)
                want = np.concatenate([u, ce.unit(u), ce.measure(a, b)[:, None]], 1)
                assert got.shape == (6 * n * n, 7) and bits(got) == bits(want), (n, ju, jv)


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_host_build_of_the_lobe_weight_equals_the_statement_bit_for_bit(programs, build):
    for n, ns in ((1, 2), (1, 1), (2, 3), (3, 5), (5, 5)):
        R = ce.unit(ce.directions(n))
        f, a, b = ce.coords(ns)
        d, m = ce.unit(ce.face_dirs(f, a, b)), ce.measure(a, b)
        for e in EXPONENTS:
            got = run_program(programs[build], "weights", n, ns, e).reshape(len(R), len(d))
            want = np.stack([ce.weight(R, d[s], m[s], e) for s in range(len(d))], 1)
            assert bits(got) == bits(want), (n, ns, e)
            assert (want >= 0).all() and ((want > 0).any() or (e == 16 and n != ns))      # cos^65536 underflows unless a source shares the centre


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_host_build_of_the_box_mean_equals_the_statement_bit_for_bit(programs, build):
    cube = ce.mixed_cube(4, 3)
    cube[0, 0, 0, 0], cube[0, 0, 1, 0], cube[0, 1, 0, 0], cube[0, 1, 1, 0] = 1e16, 1.0, -1e16, 1.0        # the order of the sum shows
    blocks = np.stack([cube[:, 0::2, 0::2], cube[:, 0::2, 1::2], cube[:, 1::2, 0::2], cube[:, 1::2, 1::2]], -1).reshape(-1, 4)
    got = run_program(programs[build], "box", *[float(v).hex() for v in blocks.reshape(-1)])
    want = ce.box_level(cube)
    assert bits(got.reshape(-1)) == bits(want.reshape(-1))
    assert want[0, 0, 0, 0] == ((1e16 + 1.0) + (-1e16 + 1.0)) * 0.25 != 0.5


# ---------------------------------------------------------------------------------------------------------------- properties of the statement
def test_directions_of_face_2_cover_all_eight_octants():
    d = ce.unit(ce.directions(2))
    assert (np.abs((d * d).sum(1) - 1.0) < 1e-15).all()
    octants = {tuple(int(c > 0) for c in row) for row in d}
    assert len(octants) == 8 and (d != 0).all()
    for f, axis, sign in ((0, 0, 1), (1, 0, -1), (2, 1, 1), (3, 1, -1), (4, 2, 1), (5, 2, -1)):         # each face looks down its axis
        face = d[f * 4:(f + 1) * 4]
        assert (np.argmax(np.abs(face), 1) == axis).all() and (np.sign(face[:, axis]) == sign).all()
    # row y grows downward: on the four side faces the first row looks up
    for f in (0, 1, 4, 5):
        assert (d[f * 4:f * 4 + 2, 1] > 0).all() and (d[f * 4 + 2:f * 4 + 4, 1] < 0).all()


@pytest.mark.parametrize("n", [1, 4, 7])
def test_texel_of_a_texels_direction_is_the_texel(n):
    d = gi.cube_directions(n)
    assert d.shape == (6, n, n, 3) and bits(d) == bits(ce.unit(ce.directions(n)))
    assert np.array_equal(gi.cube_texel_of(d, n).reshape(-1), np.arange(6 * n * n))
    for ju, jv in ((0.0625, 0.9375), (0.9375, 0.0625)):                                                # anywhere inside the texel, and at any length
        assert np.array_equal(gi.cube_texel_of(3.5 * gi.cube_directions(n, ju, jv), n).reshape(-1), np.arange(6 * n * n))
    with pytest.raises(ValueError):
        gi.cube_directions(0)


def test_a_cube_of_one_colour_filters_to_that_colour():
    """The weights are normalised: A / W of a constant cube is the constant.  Within 4 ulp at every level for a colour whose components are powers
    of two: every product w * c is then exact, every partial sum A_g is c * W_g, and the quotient is c itself.  A general colour rounds each of
    the 6 * 4 n^2 products and additions of a level; the worst case of that many sequential roundings is one ulp per term, which is the bound
    asserted for it, and the largest error met is printed (7 ulp over the 384 source texels of face 8 under the lobe 2^5, 3 ulp under the default lobe, 2 ulp and below at
    the smaller levels): 4 ulp does not hold for every colour and lobe."""
    for colour, per_term in ((np.array([0.25, 2.0, 2.0 ** -9]), 0), (np.array([0.3, 1.7, 2.9e-3]), 1)):
        cube = np.ascontiguousarray(np.broadcast_to(colour, (6, 8, 8, 3)))
        for exponents in (None, (0, 5, 1, 0), (0, 13, 13, 0)):
            chain = ce.prefilter(cube, 4, exponents)
            assert [c.shape for c in chain] == [(6, 8, 8, 3), (6, 4, 4, 3), (6, 2, 2, 3), (6, 1, 1, 3)]
            for l, level in enumerate(chain):
                ulps = float((np.abs(level - colour) / np.spacing(colour)).max())
                terms = 0 if l == 0 else 6 * (2 * level.shape[1]) ** 2
                print(f"colour {colour.tolist()} exponents {exponents} level {l}: {ulps:.1f} ulp over {terms} source texels")
                assert ulps <= 4 + per_term * terms
        assert np.array_equal(ce.box_level(cube), np.broadcast_to(colour, (6, 4, 4, 3)))


def test_a_wide_lobe_sees_the_whole_hemisphere_and_a_narrow_one_its_own_texels():
    cube = np.zeros((6, 4, 4, 3))
    cube[0] = 1.0                                                      # only +X shines
    wide, narrow = ce.filter_level(cube, 0), ce.filter_level(cube, 12)
    assert (wide[0] > wide[2]).all() and (wide[2] > 0).all() and (wide[1] == 0).all()      # -X looks away from every lit texel
    assert (np.abs(narrow[0] - 1.0) < 1e-6).all() and (narrow[1:] < 1e-6).all()
    assert ce.default_exponents() == [16, 13, 10, 7, 4, 1, 0, 0, 0, 0, 0, 0] and len(ce.default_exponents()) == gi.CUBEMAP_MAX_LEVELS == ce.MAX_LEVELS


def test_streams_and_jitter_of_the_captures_rays():
    P = np.array([0.25, -1.5, 3.0])
    rays, st = ce.capture_rays(P, 3, 5, stream_base=1000)
    assert st.tolist() == [1000 + t * 5 + k for t in range(54) for k in range(5)]
    assert (rays[:, 0:3] == P).all() and (np.abs((rays[:, 3:6] ** 2).sum(1) - 1.0) < 1e-15).all()
    assert np.array_equal(gi.cube_texel_of(rays[:, 3:6], 3), np.repeat(np.arange(54), 5))              # every sample stays inside its texel


# ---------------------------------------------------------------------------------------------------------------- the binding and the command line
def test_params_defaults_and_chain_texels():
    L = gi.lib()
    p = gi.CubemapParams()
    L.gi_cubemap_default_params(p)
    assert (p.face, p.n_samples, p.levels, p.stream_base, p.seed) == (32, 64, 1, 0, gi.DEFAULT_SEED) and list(p.log2_exponent) == ce.default_exponents()
    assert L.gi_cubemap_chain_texels(8, 4) == 6 * (64 + 16 + 4 + 1) and L.gi_cubemap_chain_texels(5, 1) == 150 and L.gi_cubemap_chain_texels(1, 1) == 6
    for face, levels in ((0, 1), (-8, 1), (8, 0), (8, 13), (6, 3), (8, 5), (26755, 1)):
        assert L.gi_cubemap_chain_texels(face, levels) == -1, (face, levels)
    assert L.gi_cubemap_chain_texels(26754, 1) == 6 * 26754 ** 2 <= 2 ** 32


@pytest.mark.parametrize("args", [["--reflection-probe", "0", "1", "0", "--probes", "2", "2", "2"], ["--reflection-probe", "0", "1", "0", "--lightmap", "8", "8"],
                                  ["--probe-face", "8"], ["--probe-levels", "2"], ["--reflection-probe", "0", "1", "0", "--probe-face", "6", "--probe-levels", "3"],
                                  ["--reflection-probe", "0", "1", "0", "--probe-levels", "13"], ["--reflection-probe", "0", "nan", "0"],
                                  ["--reflection-probe", "0", "1", "0", "--probe-samples", "0"], ["--reflection-probe", "0", "1", "0", "--samples", "4"],
                                  ["--reflection-probe", "0", "1", "0", "--probe-face", "30000"]])
def test_command_line_refuses_before_it_touches_the_device(args):
    with pytest.raises(SystemExit) as e:
        cli.main([os.path.join(ROOT, pc.SCN["cornell"]), "-o", "unused.npz"] + args)
    assert e.value.code == 2


# ---------------------------------------------------------------------------------------------------------------- a capture through the oracle alone
def test_capture_at_the_centre_of_the_cornell_box_is_the_fold_of_the_oracles_radiance():
    scene = pc.load_scene("cornell")
    o = pc.oracle_for(scene).build_photon_map()
    pos = ce.root_box_middle(scene.tables())
    face, ns = 2, 4
    rays, st = ce.capture_rays(pos, face, ns)
    got = ce.expected_capture(o, rays, st, ns).reshape(6, face, face, 3)
    L = o.radiance(rays, st).reshape(6 * face * face, ns, 3)
    acc = np.zeros((6 * face * face, 3))
    for k in range(ns):
        acc = acc + L[:, k]
    assert bits(got) == bits((acc / float(ns)).reshape(got.shape)) and bits(got) == bits(be.fold_texel(L).reshape(got.shape))
    assert all((got[f] != 0).any() for f in range(6))
