"""The ambient-occlusion pass without a GPU: the statement itself (tests/occlusion_expect.py, oracle only) on frames whose answer is known, the room
the oracle has on the frames the GPU tests compare, and the host side of the Python mirror and the CLI (argument checks, defaults, ABI names)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import gi_raytracer_amd as gi
from gi_raytracer_amd import __main__ as cli

import features_expect as fe
import occlusion_expect as oe
import parity_checks as pc

W, H = 24, 16
PARITY_SCENES = ("cornell", "spheres_opaque", "test_scene")


@pytest.fixture(scope="module")
def oracles():
    cache = {}

    def get(name):
        if name not in cache:
            scene = {"floor": lambda: oe.floor_scene(gi), "box": lambda: oe.closed_box_scene(gi)}.get(name, lambda: pc.named_scene(name))()
            cache[name] = (scene, pc.oracle_for(scene), scene.tables())
        return cache[name]

    return get


def test_floor_seen_from_above_is_fully_open(oracles):
    scene, o, t = oracles("floor")
    e = oe.expected_occlusion(o, W, H, 2, 8, 3.0)
    assert e["hit"].any() and (e["counts"] == 8).all()
    assert (e["occlusion"][:, :, 0] == 1.0).all()
    hit_all = e["hit"].all(0)
    assert hit_all.any() and (e["occlusion"][:, :, 2][hit_all] > 0).all()           # dot(bent, floor normal (0, 1, 0)) > 0
    miss_all = ~e["hit"].any(0)
    assert (e["occlusion"][:, :, 1:4][miss_all] == 0).all()


def test_inside_a_closed_box_nothing_is_open(oracles):
    scene, o, t = oracles("box")
    for radius in (oe.BOX_DIAGONAL, 2.5 * oe.BOX_DIAGONAL):
        e = oe.expected_occlusion(o, W, H, 2, 8, radius)
        assert e["hit"].all()
        assert (e["counts"] == 0).all() and (e["occlusion"] == 0.0).all()


def test_openness_falls_as_the_radius_grows(oracles):
    scene, o, t = oracles("cornell")
    D = oe.scene_diagonal(t)
    geo = [oe.sample_geometry(o, W, H, s, 8) for s in range(2)]
    prev = None
    for radius in (0.02 * D, 0.1 * D, 0.4 * D, 2.0 * D):
        e = oe.expected_occlusion(o, W, H, 2, 8, radius, geometry=geo)
        if prev is not None:
            assert (prev["counts"] >= e["counts"]).all() and (prev["occlusion"][:, :, 0] >= e["occlusion"][:, :, 0]).all()
        prev = e
    assert 0 < prev["occlusion"][:, :, 0].mean() < 1


@pytest.mark.parametrize("name", PARITY_SCENES)
def test_the_oracle_has_room_on_the_frames_the_gpu_is_compared_on(oracles, name):
    """No segment of the parity frames changes its answer when T_j moves by 4 ulp: the allowance between the two hemisphere samplers flips nothing."""
    scene, o, t = oracles(name)
    assert name in fe.DRAW_FREE_SCENES and fe.oracle_is_draw_free(o, fe.sample_rays(o, W, H, 0)[0])
    D = oe.scene_diagonal(t)
    for s in range(2):
        g = oe.sample_geometry(o, W, H, s, 8)
        for radius in (oe.default_radius(t), 2.0 * D):
            flipped, asked = oe.flips_under_perturbation(o, g, radius)
            print(f"{name} sample {s} radius {radius:.4f}: {flipped} of {asked} segments flip under 4 ulp")
            assert asked > 0 and flipped == 0


def test_statement_conventions(oracles):
    scene, o, t = oracles("cornell")
    g = oe.sample_geometry(o, W, H, 0, 4)
    hit = g["hit"]
    assert hit.any()
    rays, _ = fe.sample_rays(o, W, H, 0)
    assert (np.abs(np.linalg.norm(g["Nf"][hit], axis=1) - 1) < 1e-15).all()
    assert ((g["Nf"][hit] * rays[hit, 3:6]).sum(1) <= 0).all()                      # the normal faces the viewer
    d = g["d"][hit]
    assert (np.abs(np.linalg.norm(d, axis=2) - 1) < 1e-6).all()                      # float cosine / sine inside the sampler
    assert ((d * g["Nf"][hit][:, None, :]).sum(2) > -1e-7).all()                     # in the hemisphere of Nf
    b = t["node_bbox"][0]
    assert oe.default_radius(t) == 0.1 * math.sqrt(((b[3] - b[0]) ** 2 + (b[4] - b[1]) ** 2) + (b[5] - b[2]) ** 2)


def test_bad_arguments_raise_value_error_before_the_library_is_called():
    for kw in (dict(n=0), dict(n=-3), dict(n=2.5), dict(n="x"), dict(dirs=0), dict(dirs=65), dict(dirs=-1), dict(dirs=1.5), dict(radius=-1e-9),
               dict(radius=float("nan")), dict(radius=float("inf")), dict(radius=-float("inf")), dict(n=480, width=3840, height=2160)):
        with pytest.raises(ValueError):
            gi.occlusion_params(**kw)
    assert gi.occlusion_params(n=479, width=3840, height=2160).n_samples == 479
    p = gi.occlusion_params(n=3, dirs=64, radius=0.25)
    assert (p.n_samples, p.n_dirs, p.radius) == (3, 64, 0.25)
    assert gi.occlusion_params(dirs=1).n_dirs == 1 and gi.occlusion_params(radius=0).radius == 0.0


def test_default_params_and_layout():
    p = gi.occlusion_params()
    assert isinstance(p, gi.OcclusionParams) and (p.n_samples, p.n_dirs, p.radius) == (16, 16, 0.0)
    assert C.sizeof(gi.OcclusionParams) == 2 * 4 + 8
    assert [f[0] for f in gi.OcclusionParams._fields_] == ["n_samples", "n_dirs", "radius"]
    q = gi.OcclusionParams(7, 7, 7.0)
    gi.lib().gi_occlusion_default_params(C.byref(q))
    assert (q.n_samples, q.n_dirs, q.radius) == (16, 16, 0.0)
    gi.lib().gi_occlusion_default_params(None)                                        # a null pointer is ignored
    for name in ("run_occlusion", "run_occlusion_device", "occlusion_params", "last_occlusion_ms"):
        assert callable(getattr(gi.RayTracer, name))


def test_abi_names_and_header():
    for name in ("gi_occlusion_default_params", "gi_render_occlusion_device", "gi_render_occlusion_host", "gi_last_occlusion_ms"):
        assert name in gi.ABI_SYMBOLS and hasattr(gi.lib(), name)
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(pc.ROOT, "include", "gi_hip.h")).read(), flags=re.S)
    code = re.sub(r"\s+", " ", code)
    assert "typedef struct gi_occlusion_params { int32_t n_samples; int32_t n_dirs; double radius; } gi_occlusion_params;" in code
    assert "void gi_occlusion_default_params(gi_occlusion_params*);" in code
    for where, d in (("device", "d"), ("host", "h")):
        assert f"int gi_render_occlusion_{where}(gi_ctx*, const gi_render_params*, const gi_occlusion_params*, void* {d}_out, int out_is_f64);" in code
    assert "int gi_last_occlusion_ms(gi_ctx*, float* ms);" in code


def test_cli_accepts_the_occlusion_options(capsys):
    ap = cli.parser()
    a = ap.parse_args(["s.scn", "--occlusion", "out/ao", "--occlusion-samples", "4", "--occlusion-dirs", "32", "--occlusion-radius", "0.5"])
    assert (a.occlusion, a.occlusion_samples, a.occlusion_dirs, a.occlusion_radius) == ("out/ao", 4, 32, 0.5)
    cli.check_args(ap, a)
    assert cli.occlusion_kwargs(a) == {"n": 4, "dirs": 32, "radius": 0.5}
    a = ap.parse_args(["s.scn", "--occlusion", "ao"])
    cli.check_args(ap, a)
    assert cli.occlusion_kwargs(a) == {}
    a = ap.parse_args(["s.scn"])
    assert a.occlusion is None
    cli.check_args(ap, a)
    for bad in (["--occlusion-dirs", "8"], ["--occlusion", "ao", "--occlusion-dirs", "65"], ["--occlusion", "ao", "--occlusion-samples", "0"],
                ["--occlusion", "ao", "--occlusion-radius", "-1"], ["--occlusion", "ao", "--width", "3840", "--height", "2160", "--occlusion-samples", "480"]):
        with pytest.raises(SystemExit) as ex:
            cli.check_args(ap, ap.parse_args(["s.scn"] + bad))
        assert ex.value.code == 2
    capsys.readouterr()
