"""The thin lens without a GPU: the header declares the entries and the Python mirror binds them; gi_lens_vertices; the refusals of lens_params and
of the command line; the checkpoint's lens tag; the properties of the numpy statement (tests/lens_expect.py) the GPU tests compare the device with;
and primary_ray_at itself, compiled for the host as a program of its own (tests/cpp/lens_rays.cpp), plainly and under the sanitizers, bit for bit
against that statement."""
import ctypes as C
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import gi_raytracer_amd as gi
import gi_raytracer_amd.__main__ as cli

import host_build
import lens_expect as le
from test_progressive_cpu import hand_made_blob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("gi_set_lens", "gi_get_lens", "gi_lens_vertices", "gi_group_set_lens", "gi_debug_primary_rays", "gi_focus_distance")
W, H = 7, 5
RADIUS = 0.25
LENSES = ((3, 0.0), (6, 0.4), (16, 1.0))


def camera():
    s = gi.Scene()
    s.set_camera((10.0, 5.0, 0.3), (0.1, 0.2, -0.3))
    st = s.settings
    return le.camera({"cam_pos": list(st.cam_pos), "cam_up": list(st.cam_up), "cam_forward": list(st.cam_forward), "sensor_diag": st.sensor_diag, "focal_dist": st.focal_dist})


# ---------------------------------------------------------------------------------------------------------------- surface
def test_header_declares_and_the_library_exports_the_entries():
    txt = open(os.path.join(ROOT, "include/gi_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\bint\s+(gi_[a-z_]*(?:lens|primary_rays|focus_distance)[a-z_]*)\s*\(", txt))
    assert declared == set(ENTRIES) and re.search(r"\bvoid\s+gi_lens_default\s*\(", txt)
    assert "typedef struct gi_lens { double radius; double rotation; int32_t blades; int32_t reserved; } gi_lens;" in txt
    L = gi.lib()
    for n in ENTRIES + ("gi_lens_default",):
        assert n in gi.ABI_SYMBOLS and hasattr(L, n), n
    assert C.sizeof(gi.Lens) == 24 and C.sizeof(gi.RenderParams) == 136            # the lens is not a field of gi_render_params
    assert len(L.gi_debug_primary_rays.argtypes) == 5 and len(L.gi_focus_distance.argtypes) == 5
    for name in ("set_lens", "lens", "primary_rays", "focus_distance", "focus_at"):
        assert hasattr(gi.RayTracer, name), name
    assert callable(gi.RayTracerGroup.set_lens)
    cpp = open(os.path.join(ROOT, "include/gi/raytracer.h")).read()
    assert "bool setLens(double radius, int blades = 6, double rotation = 0)" in cpp and "bool focusAt(double dist)" in cpp


def test_default_lens_is_a_six_bladed_pinhole():
    l = gi.lens_params()
    assert (l.radius, l.rotation, l.blades, l.reserved) == (0.0, 0.0, 6, 0)
    l = gi.lens_params(radius=0.5, blades=9, rotation=-0.25)
    assert (l.radius, l.rotation, l.blades, l.reserved) == (0.5, -0.25, 9, 0)


@pytest.mark.parametrize("blades", [3, 4, 6, 7, 16])
@pytest.mark.parametrize("rotation", [0.0, 0.4, -2.5])
def test_vertices_are_unit_length_and_the_last_is_the_first(blades, rotation):
    v = gi.lens_vertices(gi.lens_params(1.0, blades, rotation))
    assert v.shape == (blades + 1, 2) and v[blades].tobytes() == v[0].tobytes()
    assert np.abs(np.hypot(v[:, 0], v[:, 1]) - 1.0).max() <= 2 ** -52
    for k in range(blades):                                    # the host's libm at rotation + (2 pi k) / blades
        th = rotation + (2.0 * math.pi * k) / blades
        assert v[k, 0] == math.cos(th) and v[k, 1] == math.sin(th), k
    turn = np.arctan2(v[1:, 1], v[1:, 0]) - np.arctan2(v[:-1, 1], v[:-1, 0])
    assert np.allclose(np.mod(turn, 2 * math.pi), 2 * math.pi / blades)
    assert gi.lens_vertices(gi.lens_params(0.0, blades, rotation)).tobytes() == v.tobytes()      # the radius plays no part


# ---------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("kw", [dict(radius=-1e-9), dict(radius=float("nan")), dict(radius=float("inf")), dict(radius="wide"), dict(blades=2), dict(blades=17), dict(blades=0),
                                dict(blades=-6), dict(blades=6.5), dict(blades="six"), dict(blades=2 ** 40), dict(rotation=float("nan")), dict(rotation=float("inf")),
                                dict(rotation=-float("inf")), dict(rotation="a quarter")], ids=lambda kw: " ".join(f"{k}={v}" for k, v in kw.items()))
def test_lens_params_refuses_what_the_library_would(kw):
    with pytest.raises(ValueError, match="lens: " + next(iter(kw))):
        gi.lens_params(**kw)


def test_the_library_refuses_the_same_lenses_without_a_device():
    xy = np.full((18, 2), -7.0)
    p = xy.ctypes.data_as(C.POINTER(C.c_double))
    L = gi.lib()
    for bad in (gi.Lens(-1.0, 0, 6, 0), gi.Lens(float("nan"), 0, 6, 0), gi.Lens(1, float("inf"), 6, 0), gi.Lens(1, 0, 2, 0), gi.Lens(1, 0, 17, 0), gi.Lens(1, 0, 6, 7)):
        assert L.gi_lens_vertices(C.byref(bad), p) == gi.GI_E_INVALID and (xy == -7.0).all()
        with pytest.raises(ValueError):
            gi.lens_vertices(bad)
    assert L.gi_lens_vertices(None, p) == gi.GI_E_INVALID and L.gi_lens_vertices(C.byref(gi.lens_params(1.0)), None) == gi.GI_E_INVALID
    assert L.gi_set_lens(None, C.byref(gi.lens_params(1.0))) == gi.GI_E_INVALID and L.gi_get_lens(None, None) == gi.GI_E_INVALID
    assert L.gi_group_set_lens(None, C.byref(gi.lens_params(1.0))) == gi.GI_E_INVALID


@pytest.mark.parametrize("flags, message", [(["--blades", "6"], "need --aperture"), (["--blade-rotation", "10"], "need --aperture"), (["--focus", "3"], "need --aperture"),
                                            (["--focus-pixel", "1", "1"], "need --aperture"), (["--aperture", "0.1", "--focus", "3", "--focus-pixel", "1", "1"], "do not go together"),
                                            (["--aperture", "-0.5"], "radius must be finite and >= 0"), (["--aperture", "nan"], "radius must be finite and >= 0"),
                                            (["--aperture", "inf"], "radius must be finite and >= 0"), (["--aperture", "0.1", "--blades", "2"], "blades must be 3 .. 16"),
                                            (["--aperture", "0.1", "--blades", "17"], "blades must be 3 .. 16"), (["--aperture", "0.1", "--blades", "six"], "invalid int value"),
                                            (["--aperture", "0.1", "--focus", "0"], "distance > 0"), (["--aperture", "0.1", "--focus", "nan"], "distance > 0"),
                                            (["--aperture", "0.1", "--blade-rotation", "inf"], "rotation must be finite"),
                                            (["--aperture", "0.1", "--width", "13", "--height", "9", "--focus-pixel", "13", "0"], "a pixel of the 13 x 9 frame"),
                                            (["--aperture", "wide"], "invalid float value")],
                         ids=lambda v: " ".join(v) if isinstance(v, list) else None)
def test_cli_refuses_before_touching_a_device(flags, message, capsys):
    with pytest.raises(SystemExit) as e:
        cli.main(["no_such_scene.scn"] + flags)
    assert e.value.code == 2 and message in capsys.readouterr().err


def test_cli_accepts_the_lens_flags_next_to_the_other_passes():
    ap = cli.parser()
    a = ap.parse_args(["s.scn", "--aperture", "0.2", "--blades", "7", "--blade-rotation", "30", "--focus-pixel", "3", "4", "--width", "16", "--height", "8",
                       "--features", "f", "--occlusion", "ao", "--denoise", "d.ppm", "--upsample", "2"])
    cli.check_args(ap, a)
    l = cli.lens_of(a)
    assert (l.radius, l.blades, l.rotation) == (0.2, 7, math.radians(30.0)) and a.focus_pixel == [3, 4]
    a = ap.parse_args(["s.scn", "--aperture", "0", "--focus", "4.5", "--progressive", "2"])
    cli.check_args(ap, a)
    assert cli.lens_of(a).radius == 0.0 and a.focus == 4.5
    a = ap.parse_args(["s.scn"])
    cli.check_args(ap, a)
    assert cli.lens_of(a) is None


# ---------------------------------------------------------------------------------------------------------------- the checkpoint's tag
def fnv1a_tag(radius, rotation, blades):
    """Worked by hand from include/gi_hip.h: 64-bit FNV-1a over the 24 bytes of gi_lens, the low 32 bits, 0 -> 1."""
    h = 0xcbf29ce484222325
    for b in struct.pack("<ddii", radius, rotation, blades, 0):
        h = ((h ^ b) * 0x100000001b3) % 2 ** 64
    return (h % 2 ** 32) or 1


def test_lens_tag_of_two_hand_computed_lenses_and_the_pinhole():
    assert gi.lens_tag(gi.lens_params(0.25, 3, 0.0)) == fnv1a_tag(0.25, 0.0, 3) == 2054404731
    assert gi.lens_tag(gi.lens_params(0.25, 16, 1.0)) == fnv1a_tag(0.25, 1.0, 16) == 2684099413
    assert gi.lens_tag(gi.lens_params(0.0, 16, 1.0)) == 0 and gi.lens_tag(gi.lens_params()) == 0
    assert gi.lens_tag(gi.lens_params(0.25, 3, 0.0)) != gi.lens_tag(gi.lens_params(0.25, 4, 0.0)) != gi.lens_tag(gi.lens_params(0.25, 4, 0.1))


def test_a_hand_made_checkpoint_parses_with_lens_tag():
    blob, f = hand_made_blob()
    h = gi.parse_checkpoint_header(blob)
    assert h["lens_tag"] == 0 and h["reserved1"] == 0                  # a pinhole checkpoint keeps its bytes
    tagged = blob[:188] + struct.pack("<I", 2684099413) + blob[192:]
    h = gi.parse_checkpoint_header(tagged)
    assert h["lens_tag"] == 2684099413 and h["reserved1"] == h["lens_tag"] and h["n_photon"] == f["n_photon"]
    assert struct.calcsize(gi.CHECKPOINT_HEADER) == 192


# ---------------------------------------------------------------------------------------------------------------- the numpy statement
@pytest.mark.parametrize("blades, rotation", LENSES)
def test_properties_of_the_stated_rays(blades, rotation):
    cam = camera()
    lens = gi.lens_params(RADIUS, blades, rotation)
    verts = gi.lens_vertices(lens)
    F = le.frame(cam, W, H)
    idx = np.concatenate([le.frame_indices(W, H, s) for s in range(4)])
    rays = le.rays(cam, W, H, idx, RADIUS, verts)
    eye, l, k = le.eyes(cam, W, H, verts, RADIUS, idx)
    assert le.same(rays[:, 0:3], eye) and np.abs(np.sqrt(le.dot(rays[:, 3:6], rays[:, 3:6])) - 1.0).max() < 1e-15
    # every eye point lies in the lens plane, inside the polygon of radius `radius`: on the inner side of every edge
    off = eye - cam["cam_pos"]
    assert np.abs(le.dot(off, cam["cam_forward"])).max() < 1e-12
    e2 = np.stack([le.dot(off, F["right"]), le.dot(off, cam["cam_up"])], 1) / RADIUS
    assert np.abs(e2 - l).max() < 1e-12
    for j in range(blades):
        a, b = verts[j], verts[j + 1]
        side = (b[0] - a[0]) * (e2[:, 1] - a[1]) - (b[1] - a[1]) * (e2[:, 0] - a[0])
        assert (side >= -1e-12).all(), j
    # every ray passes through its pixel's point of the sensor plane
    scale = float(np.linalg.norm(cam["cam_pos"])) + cam["focal_dist"]
    pp = le.pixel_pos(cam, W, H, *le.pixel_offsets(W, H, idx))
    to = pp - eye
    dist = np.linalg.norm(to - le.dot(to, rays[:, 3:6])[:, None] * rays[:, 3:6], axis=1)
    assert dist.max() <= 1e-12 * scale, dist.max()
    # ... which is the point the pinhole ray of the same sample goes through
    pin = le.rays(cam, W, H, idx)
    assert (pin[:, 0:3] == cam["cam_pos"]).all()
    t = cam["focal_dist"] / le.dot(pin[:, 3:6], cam["cam_forward"])
    assert np.abs(pin[:, 0:3] + t[:, None] * pin[:, 3:6] - pp).max() <= 1e-12 * scale


@pytest.mark.parametrize("blades, rotation", LENSES)
def test_lens_points_are_uniform_over_the_polygon(blades, rotation):
    """4096 samples of one pixel: the mean of the eye points within 3 standard errors (their own) of cam_pos, and every blade's triangle with
    between half and twice its fair share.  A condition on the seed, checked here."""
    cam = camera()
    verts = gi.lens_vertices(gi.lens_params(RADIUS, blades, rotation))
    inc = le.halton_index(W, H, 1, 3, 2) - le.halton_index(W, H, 0, 3, 2)
    idx = le.halton_index(W, H, 0, 3, 2) + inc * np.arange(4096, dtype=np.uint32)
    eye, l, k = le.eyes(cam, W, H, verts, RADIUS, idx)
    off = eye - cam["cam_pos"]
    se = off.std(0, ddof=1) / math.sqrt(len(idx))
    assert (np.abs(off.mean(0)) <= 3 * se + 1e-15).all(), (off.mean(0), se)
    share = np.bincount(k, minlength=blades) / len(idx)
    assert share.shape == (blades,) and (share >= 0.5 / blades).all() and (share <= 2.0 / blades).all(), share
    r2 = l[:, 0] ** 2 + l[:, 1] ** 2
    assert r2.max() <= 1.0 + 1e-15 and abs(r2.mean() - (1 + 2 * math.cos(math.pi / blades) ** 2) / 6) < 0.02      # E|l|^2 of a regular polygon of circumradius 1


# ---------------------------------------------------------------------------------------------------------------- the device function on the host
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("lens_rays")
    out = {}
    for name, extra in (("plain", []), ("sanitized", SANITIZE)):
        out[name] = str(d / f"lens_rays_{name}")
        subprocess.run([os.environ.get("CXX", "g++")] + host_build.flags() + extra + [os.path.join(ROOT, "tests", "cpp", "lens_rays.cpp"), "-o", out[name]], check=True)
    return out


def run_program(exe, cam, seed, radius, rotation, blades, idx):
    args = [str(W), str(H), str(seed), float(radius).hex(), float(rotation).hex(), str(blades)]
    args += [float(x).hex() for key in ("cam_pos", "cam_up", "cam_forward") for x in cam[key]] + [cam["sensor_diag"].hex(), cam["focal_dist"].hex()]
    r = subprocess.run([exe] + args + [str(int(i)) for i in idx], capture_output=True, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    lines = r.stdout.split("\n")
    return int(lines[0].split()[1]), np.array([[float.fromhex(t) for t in ln.split()] for ln in lines[1:] if ln])


@pytest.mark.parametrize("build", ["plain", "sanitized"])
@pytest.mark.parametrize("blades, rotation", LENSES)
def test_host_build_of_primary_ray_at_equals_the_statement_bit_for_bit(programs, build, blades, rotation):
    cam = camera()
    idx = np.concatenate([le.frame_indices(W, H, s) for s in range(4)] + [np.array([2039157, 721123, 0xffffffff], np.uint32)])
    for seed in (le.DEFAULT_SEED, 12345):
        lens = gi.lens_params(RADIUS, blades, rotation)
        tag, got = run_program(programs[build], cam, seed, RADIUS, rotation, blades, idx)
        assert tag == gi.lens_tag(lens)
        assert le.same(got, le.rays(cam, W, H, idx, RADIUS, gi.lens_vertices(lens), seed))
    tag, got = run_program(programs[build], cam, 12345, 0.0, rotation, blades, idx)                 # radius 0: the pinhole's branch
    assert tag == 0 and le.same(got, le.rays(cam, W, H, idx)) and (got[:, 0:3] == cam["cam_pos"]).all()
