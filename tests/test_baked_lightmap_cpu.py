"""The baked-light pass's lightmap look-up without a GPU: lm_coord, lm_bilinear and lm_nearest of gi_baked.h compiled for the host as a program of its
own (tests/cpp/baked_lightmap_lookup.cpp), plainly and under the sanitizers, bit for bit against the numpy statement
(tests/baked_lightmap_expect.py) on random triangles, points, chart rows and atlases and on their edge inputs; the conditions the GPU tests'
frames have to meet, checked with the oracle alone, so that the GPU tests cannot pass for want of cases; the binding's parameter block and the
command line's refusals."""
import os
import subprocess

import numpy as np
import pytest

import gi_raytracer_amd as gi
import gi_raytracer_amd.__main__ as cli

import baked_expect as be
import baked_lightmap_expect as bl
import features_expect as fe
import host_build
import lightmap_expect as le
import parity_checks as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer"]
BUILDS = ["plain", "sanitized"]
SCENES = ["cornell", "test_scene", "spheres_opaque"]
FRAMES = ((24, 16), (13, 9))


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("baked_lightmap_lookup")
    out = {}
    for name, extra in (("plain", []), ("sanitized", SANITIZE)):
        out[name] = str(d / f"baked_lightmap_lookup_{name}")
        subprocess.run([os.environ.get("CXX", "g++")] + host_build.flags() + extra + [os.path.join(ROOT, "tests", "cpp", "baked_lightmap_lookup.cpp"), "-o", out[name]], check=True)
    return out, d


def run_program(exe, d, what, arrays, *args):
    """The program on the arrays, written as raw doubles; its output as raw doubles."""
    paths = []
    for k, a in enumerate(arrays):
        paths.append(str(d / f"{what}_{k}.f64"))
        np.ascontiguousarray(a, "<f8").tofile(paths[-1])
    out = str(d / f"{what}_out.f64")
    r = subprocess.run([exe, what] + [str(a) for a in args] + paths + [out], capture_output=True, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
    return np.fromfile(out, "<f8")


def bits(a):
    return np.ascontiguousarray(a, np.float64).tobytes()


# ---------------------------------------------------------------------------------------------------------------- the per-lane functions
def coord_inputs():
    """A few thousand (triangle, P, chart row): points inside, on the edges of and outside their triangles, and off their planes; chart rows inside and
    outside [0, 1]; then degenerate triangles (two equal vertices, three on a line, a point), a NaN point and a NaN chart coordinate."""
    rs = np.random.default_rng(31)
    n = 3000
    p0 = rs.uniform(-5.0, 5.0, (n, 3))
    e1, e2 = rs.normal(size=(n, 3)) * 10.0 ** rs.uniform(-2, 1, (n, 1)), rs.normal(size=(n, 3)) * 10.0 ** rs.uniform(-2, 1, (n, 1))
    b = rs.uniform(-0.3, 1.3, (n, 2))
    b[:200] = rs.integers(0, 2, (200, 2))                                  # vertices and the far corner
    P = p0 + b[:, :1] * e1 + b[:, 1:] * e2 + rs.normal(size=(n, 3)) * (rs.uniform(size=(n, 1)) < 0.3) * 1e-3
    uv = rs.uniform(-0.25, 1.25, (n, 3, 2))
    e2[-40:-30] = e1[-40:-30] * 2.0                                        # three vertices on a line: den is 0 or rounding
    e2[-30:-20] = 0.0                                                      # two equal vertices
    e1[-20:-10] = 0.0; e2[-20:-10] = 0.0                                   # a point
    P[-10:-5, 1] = np.nan
    uv[-5:, 1, 0] = np.nan
    return p0, e1, e2, P, uv


@pytest.mark.parametrize("build", BUILDS)
def test_host_build_of_the_chart_coordinate_equals_the_statement_bit_for_bit(programs, build):
    exe, d = programs[0][build], programs[1]
    p0, e1, e2, P, uv = coord_inputs()
    got = run_program(exe, d, "coord", [np.concatenate([p0, e1, e2, P, uv.reshape(-1, 6)], 1)]).reshape(-1, 2)
    u, v = bl.coord_of(p0, e1, e2, P, uv)
    assert bits(got) == bits(np.stack([u, v], 1))
    assert np.isnan(u[-40:]).any() and np.isfinite(u[:-40]).all() and ((u < 0) | (u > 1)).any()
    # it inverts the point a lightmap puts under a texel: P = (p0 + b1 e1v) + b2 e2v at the barycentrics of a chart point gives that chart point back
    rs = np.random.default_rng(32)
    m = 500
    b1 = rs.uniform(0.0, 1.0, m); b2 = rs.uniform(0.0, 1.0, m) * (1.0 - b1)
    Q = (p0[:m] + b1[:, None] * e1[:m]) + b2[:, None] * e2[:m]
    uq, vq = bl.coord_of(p0[:m], e1[:m], e2[:m], Q, uv[:m])
    want = (1 - b1 - b2)[:, None] * uv[:m, 0] + b1[:, None] * uv[:m, 1] + b2[:, None] * uv[:m, 2]
    assert np.allclose(np.stack([uq, vq], 1), want, rtol=0, atol=1e-9)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("size", bl.ATLAS_SIZES)
def test_host_build_of_the_two_filters_equals_the_statement_bit_for_bit(programs, build, size):
    exe, d = programs[0][build], programs[1]
    w, h = size
    rs = np.random.default_rng(33 + w)
    atlas = bl.random_atlas(size, 40 + w)
    if w * h > 1:
        atlas[0, 0, 1] = np.nan                                            # an unfilled texel's bits pass through
    centres = np.stack([a.reshape(-1) for a in le.centres(w, h)], 1)
    edges = np.array([[0.0, 0.0], [1.0, 1.0], [-0.0, 1.0], [np.nextafter(1.0, 0.0), np.nextafter(0.0, -1.0)], [0.5, 0.5], [-7.0, 9.0], [1e300, -1e300],
                      [np.inf, -np.inf], [np.nan, 0.5], [0.5, np.nan], [np.nan, np.nan]])
    uv = np.concatenate([rs.uniform(-0.3, 1.3, (1500, 2)), centres, np.arange(w + 1)[:, None] / w * np.ones((1, 2)), np.arange(h + 1)[:, None] / h * np.ones((1, 2)), edges])
    got = run_program(exe, d, "filter", [atlas, uv], w, h).reshape(-1, 6)
    want = np.concatenate([bl.bilinear(atlas, uv[:, 0], uv[:, 1]), bl.nearest(atlas, uv[:, 0], uv[:, 1])], 1)
    assert bits(got) == bits(want), size
    # at a texel centre both filters give the texel (clamped at 0 under the bilinear one); NaN coordinates read texel 0 of their axis
    at = atlas[np.arange(h).repeat(w), np.tile(np.arange(w), h)]
    c0 = 1500
    assert bits(want[c0:c0 + w * h, 3:]) == bits(at)
    ok = np.isfinite(at).all(1)
    assert np.array_equal(want[c0:c0 + w * h, :3][ok], np.where(at < 0, 0.0, at)[ok])
    assert bits(want[-1, 3:]) == bits(atlas[0, 0])
    assert bl.footprint_touches_border((h, w), uv[:1500, 0], uv[:1500, 1]).any() and (want[np.isfinite(want).all(1), :3] >= 0).all() and (w * h == 1 or ((want[:, 3:] < 0).any() and np.isnan(want).any()))


def test_row_of_ent_takes_the_lowest_row_and_skips_spheres():
    ent = np.array([3, 1, 3, 7, -1, 2, 1, 5], np.int32)
    sphere = np.array([0, 0, 1, 0, 0, 0], bool)
    assert bl.row_of_ent(ent, 6, sphere).tolist() == [-1, 1, -1, 0, -1, 7]
    assert bl.row_of_ent(ent[:0], 3).tolist() == [-1, -1, -1]


# ---------------------------------------------------------------------------------------------------------------- the GPU tests' own frames
def setup(name):
    base = pc.load_scene(name)
    scene = be.with_roughnesses(base, bl.ROUGHNESSES)
    return be.oracle_with_camera(scene, base.settings), scene.tables()


@pytest.mark.parametrize("name", SCENES)
def test_the_gpu_tests_frames_meet_their_conditions(name):
    """tests/test_gpu_baked_lightmap.py compares these frames with the statement: each must have charted and uncharted diffuse hits, bilinear
    footprints the border clamps, and a hit on the entity listed twice."""
    o, t = setup(name)
    assert name in fe.DRAW_FREE_SCENES and fe.oracle_is_draw_free(o, fe.sample_rays(o, 24, 16, 0)[0])
    ent, uv, rows = bl.frame_chart(o, t)
    assert rows is not None and ent[rows[0]] == ent[rows[1]] and rows[0] < rows[1] and not np.array_equal(uv[rows[0]], uv[rows[1]])
    kind = np.asarray(t["ent_kind"]).reshape(-1)
    assert (kind[ent] != 1).all() and np.isfinite(uv).all() and ((uv < 0) | (uv > 1)).any()
    pe, pu = bl.permuted(ent, uv, 5)
    served, served_p = bl.row_of_ent(ent, len(kind), kind == 1), bl.row_of_ent(pe, len(kind), kind == 1)
    assert not np.array_equal(pe, ent) and np.array_equal(served >= 0, served_p >= 0) and bits(uv[served[served >= 0]]) == bits(pu[served_p[served_p >= 0]])
    for (w, h) in FRAMES:
        for n in (1, 2):
            total = w * h * n
            charted = uncharted = twice = 0
            border = {size: 0 for size in bl.ATLAS_SIZES[:2]}                   # (of a 1 x 1 atlas every footprint is clamped)
            for s in range(n):
                g = be.sample_hits(o, t, w, h, s)
                diffuse, row = bl.hit_rows(g, t, ent)
                sel = np.flatnonzero(diffuse & (row >= 0))
                charted += len(sel)
                uncharted += int((diffuse & (row < 0)).sum())
                u, v = bl.coord(t, g["ent"][sel], g["P"][sel], row[sel], uv)
                for size in border:
                    border[size] += int(bl.footprint_touches_border((size[1], size[0]), u, v).sum())
                twice += int((g["ent"][sel] == ent[rows[0]]).sum())
            print(f"{name} {w}x{h} n {n}: {charted} charted, {uncharted} uncharted diffuse hits, clamped footprints {border}, {twice} on the entity listed twice, of {total}")
            assert charted * 10 >= total and uncharted * 100 >= total and min(border.values()) * 100 >= total and twice >= 1, (name, w, h, n)


# ---------------------------------------------------------------------------------------------------------------- the binding and the command line
def test_default_params_and_the_binding_s_checks():
    p = gi.BakedLightmapParams()
    gi.lib().gi_baked_lightmap_default_params(p)
    assert (p.width, p.height, p.filter, p.n_chart) == (256, 256, gi.LM_BILINEAR, 0) and (gi.LM_NEAREST, gi.LM_BILINEAR) == (0, 1)
    atlas = bl.random_atlas((5, 3), 1)
    ent, uv = np.array([2, 0, 2], np.int32), np.random.default_rng(2).uniform(0, 1, (3, 3, 2))
    lp, a, e, c = gi.baked_lightmap_params(atlas, ent, uv)
    assert (lp.width, lp.height, lp.filter, lp.n_chart) == (5, 3, gi.LM_BILINEAR, 3) and bits(a) == bits(atlas) and e.dtype == np.int32 and c.shape == (3, 3, 2)
    assert gi.baked_lightmap_params(atlas.astype(np.float32), ent, uv, "nearest")[1].dtype == np.float32
    assert gi.baked_lightmap_params(atlas, ent, uv, gi.LM_NEAREST)[0].filter == gi.LM_NEAREST
    assert gi.baked_lightmap_params(atlas, ent[:0], uv[:0])[0].n_chart == 0
    bad_uv = uv.copy()
    bad_uv[1, 2, 0] = np.inf
    for args in ((atlas[0], ent, uv), (atlas[:, :, :2], ent, uv), (np.zeros((0, 4, 3)), ent, uv), (atlas, ent[:2], uv), (atlas, ent, bad_uv), (atlas, ent, uv, "cubic"),
                 (atlas, ent, uv, 2), (atlas, ent, uv, 0.5)):
        with pytest.raises(ValueError):
            gi.baked_lightmap_params(*args)
    # the diffuse term of a lightmap needs no probe grid; without a lightmap it still does
    assert gi.baked_params(n=1, lightmap=True)[0].terms == gi.BAKED_DIRECT | gi.BAKED_DIFFUSE | gi.BAKED_EMISSIVE
    assert gi.baked_params(n=1, terms=gi.BAKED_DIFFUSE, lightmap=True)[0].terms == gi.BAKED_DIFFUSE
    with pytest.raises(ValueError):
        gi.baked_params(n=1, terms=gi.BAKED_DIFFUSE)


@pytest.mark.parametrize("args", [["--baked-lightmap", "8", "8"], ["--baked", "b", "--baked-lightmap", "0", "8"], ["--baked", "b", "--baked-lightmap", "8", "9000"],
                                  ["--baked", "b", "--baked-lightmap", "8", "8", "--lightmap-samples", "0"], ["--baked", "b", "--lightmap-samples", "4"],
                                  ["--baked", "b", "--baked-lightmap", "8", "8", "--lightmap-dilate", "1"], ["--baked", "b", "--baked-lightmap", "8192", "8192"]])
def test_command_line_refuses_before_it_touches_the_device(args):
    with pytest.raises(SystemExit) as e:
        cli.main([os.path.join(ROOT, pc.SCN["cornell"])] + args)
    assert e.value.code == 2


def test_command_line_takes_the_lightmap_beside_the_preview():
    ap = cli.parser()
    a = ap.parse_args(["s.scn", "--baked", "lit", "--baked-lightmap", "32", "16", "--lightmap-samples", "8"])
    cli.check_args(ap, a)
    assert a.baked_lightmap == [32, 16] and a.lightmap_samples == 8 and a.lightmap is None
