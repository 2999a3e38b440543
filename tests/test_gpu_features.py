"""First-hit feature buffers (gi_render_features_*, k_aov) on the GPU, through the C ABI via the Python mirror.

The expectation comes from the oracle as it is (tests/features_expect.py): Oracle.primary_ray, Oracle.trace, Oracle.tex_eval.
What is exact and what has an allowance:
 * every buffer is bit-equal on the seven draw-free scenes: ids, coverage, normal, albedo of constant-colour materials -- and also depth (one sqrt
   per sample) and textured albedo (the look-up's floor / pow table), for which the project's OCML-versus-glibc allowance of 4 ulp per sample
   (tests/parity_checks.py: check_kats) was on offer: measured on the MI355X they came out bit-equal on every pixel of all fourteen cases, so
   that is what is asserted;
 * single-sample spot checks elsewhere (large frames, gi_trace comparison) keep the 4 ulp allowance for the depth.
Fractional-alpha hits (scenes `spheres`, `textures`, `large_alpha`) are covered by construction -- aov_sample calls the beauty pass's trace with the beauty pass's
keys -- plus determinism, dependence on the seed and agreement with gi_trace where the draw cannot matter; the oracle offers no way to replay the draw
of a frame's sample without changing it."""
import ctypes as C
import os

import numpy as np
import pytest

import gi_raytracer_amd as gi
from gi_raytracer_amd import __main__ as cli

import features_expect as fe
import host_build
import parity_checks as pc

pytestmark = pytest.mark.gpu

W, H = 96, 72


@pytest.fixture(scope="module")
def setups():
    cache = {}

    def get(name):
        if name not in cache:
            scene = pc.named_scene(name)
            cache[name] = (scene, gi.RayTracer(0).setScene(scene), pc.oracle_for(scene), scene.tables())
        return cache[name]

    return get


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("name", fe.DRAW_FREE_SCENES)
def test_features_match_the_oracle_on_every_pixel(setups, name, n):
    scene, rt, o, t = setups(name)
    if n == 1:
        assert fe.oracle_is_draw_free(o, fe.sample_rays(o, W, H, 0)[0])
    want, want_ids, textured, vmax = fe.expected_features(o, t, W, H, n)
    got = rt.run_features(W, H, n)
    f = got["features"]
    assert f.shape == (H, W, 8) and f.dtype == np.float64 and got["ids"].shape == (H, W, 2) and got["ids"].dtype == np.int32
    assert np.array_equal(got["ids"], want_ids)
    assert got["coverage"].tobytes() == np.ascontiguousarray(want[:, :, 7]).tobytes()
    assert np.ascontiguousarray(got["normal"]).tobytes() == np.ascontiguousarray(want[:, :, 3:6]).tobytes()
    plain = ~textured
    assert np.ascontiguousarray(got["albedo"][plain]).tobytes() == np.ascontiguousarray(want[:, :, 0:3][plain]).tobytes()
    # depth and textured albedo: bit-equal as well (see the module docstring); the figures are printed before the assertion
    d_err = np.abs(got["depth"] - want[:, :, 6])
    a_err = np.abs(got["albedo"] - want[:, :, 0:3])
    print(f"{name} n={n}: depth differs on {int((d_err != 0).sum())} pixels (max {d_err.max():.3e}), albedo of the {int(textured.sum())} textured pixels on "
          f"{int((a_err[textured] != 0).sum())} values (max {a_err.max():.3e}), largest depth {vmax[:, :, 6].max():.3f}")
    assert got["depth"].tobytes() == np.ascontiguousarray(want[:, :, 6]).tobytes()
    assert np.ascontiguousarray(got["albedo"]).tobytes() == np.ascontiguousarray(want[:, :, 0:3]).tobytes()
    assert (f[got["coverage"] == 0] == 0).all()


# whether the hit FLAG of some primary ray depends on the alpha draw (worked out with the oracle alone, fe.hit_depends_on_draw): in large_alpha the
# half-transparent triangles stand against the empty background above the floor's far edge
FLAG_DEPENDS_ON_DRAW = {"spheres": False, "textures": True, "large_alpha": True}


@pytest.mark.parametrize("name", ["spheres", "textures", "large_alpha"])
def test_fractional_alpha_uses_the_frame_keys(setups, name):
    scene, rt, o, t = setups(name)
    n = 6
    a = rt.run_features(W, H, n)
    b = rt.run_features(W, H, n)
    assert a["features"].tobytes() == b["features"].tobytes() and a["ids"].tobytes() == b["ids"].tobytes()
    c = rt.run_features(W, H, n, seed=12345)
    assert (a["ids"] != c["ids"]).any() and (a["features"] != c["features"]).any()      # another seed, other alpha draws, other first hits
    # ... and another coverage where the oracle says the hit FLAG of some primary ray depends on the draw.  It does in `textures`; in `spheres`
    # the translucent sphere has other geometry behind it for every ray of this camera, so the draw decides which entity is hit and never whether
    # one is (measured with the oracle: 0 of 6912 rays per sample change their flag, ~95 their entity) -- there the coverage must NOT move.
    vary = any(fe.hit_depends_on_draw(o, fe.sample_rays(o, W, H, s)[0]) for s in range(n))
    assert vary == FLAG_DEPENDS_ON_DRAW[name]
    assert bool((a["coverage"] != c["coverage"]).any()) == vary
    # where the draw cannot matter -- sample 0 lands on an opacity-1, IOR-1 entity and gi_trace (seed 0, stream = ray number) lands on the same --
    # the features of that sample are that entity's
    one = rt.run_features(W, H, 1)
    rays, _ = fe.sample_rays(o, W, H, 0)
    hit, ent, res = rt.trace(rays)
    ent = ent.reshape(H, W)
    res = res.reshape(H, W, 8)
    ids = one["ids"]
    mat = np.where(ids[:, :, 1] >= 0, ids[:, :, 1], 0)
    opaque = (ids[:, :, 0] >= 0) & (t["mats"][mat, 1] == 1.0) & (t["mats"][mat, 2] == 1.0) & (ent == ids[:, :, 0]) & (hit.reshape(H, W) == 1)
    if len(t["tex_kind"]):                      # an image texture's alpha channel multiplies the opacity: leave those materials out
        dtex = t["mat_tex"][mat, 0]
        image = (dtex >= 0) & (t["tex_kind"][np.where(dtex >= 0, dtex, 0)] == 2)
        opaque &= ~image
    assert opaque.mean() > 0.2, float(opaque.mean())
    assert (one["coverage"][opaque] == 1).all()
    assert np.ascontiguousarray(one["normal"][opaque]).tobytes() == np.ascontiguousarray(res[:, :, 3:6][opaque]).tobytes()
    d = res[:, :, 0:3] - rays.reshape(H, W, 6)[:, :, 0:3]
    depth = np.sqrt(d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1] + d[:, :, 2] * d[:, :, 2])
    assert (np.abs(one["depth"] - depth)[opaque] <= 4 * fe.ULP * depth[opaque]).all()
    const = opaque.copy()
    if len(t["tex_kind"]):
        dtex = t["mat_tex"][mat, 0]
        const &= (dtex < 0) | (t["tex_kind"][np.where(dtex >= 0, dtex, 0)] == 0)
        col = np.where((dtex >= 0)[:, :, None], t["tex_param"][np.where(dtex >= 0, dtex, 0), 0:3], t["mats"][mat, 3:6])
    else:
        col = t["mats"][mat, 3:6]
    assert np.ascontiguousarray(one["albedo"][const]).tobytes() == np.ascontiguousarray(col[const]).tobytes()
    n_checked = int(const.sum())
    if len(t["tex_kind"]):
        # checkerboard materials (`textures` has no opaque constant-colour one in view): the look-up at the oracle's uv, where the oracle's own
        # draws land on the same entity too
        ohit, oent, ores, _ = o.trace(rays)
        for tex in np.flatnonzero(t["tex_kind"] == 1):
            sel = opaque & (dtex == tex) & (oent.reshape(H, W) == ids[:, :, 0])
            want = o.tex_eval(int(tex), ores.reshape(H, W, 8)[sel][:, 6:8])[:, :3]
            assert (np.abs(one["albedo"][sel] - want) <= 4 * fe.ULP * np.abs(want)).all()
            n_checked += int(sel.sum())
    assert n_checked > 100, n_checked


def test_layout_f32_ids_and_stripes(setups):
    scene, rt, o, t = setups("caustics")
    n = 3
    full = rt.run_features(W, H, n)
    f32 = rt.run_features(W, H, n, f64=False)
    assert f32["features"].dtype == np.float32 and f32["features"].tobytes() == full["features"].astype(np.float32).tobytes()
    assert np.array_equal(f32["ids"], full["ids"])
    no_ids = rt.run_features(W, H, n, want_ids=False)
    assert no_ids["ids"] is None and no_ids["features"].tobytes() == full["features"].tobytes()
    feat = np.zeros_like(full["features"])
    ids = np.zeros_like(full["ids"])
    for rank in range(3):
        part = rt.run_features(W, H, n, stripe_h=16, rank=rank, world=3)
        rows = fe.frame_rows(H, 16, rank, 3)
        assert part["features"].shape == (len(rows), W, 8)
        feat[rows] = part["features"]
        ids[rows] = part["ids"]
    assert feat.tobytes() == full["features"].tobytes() and ids.tobytes() == full["ids"].tobytes()


@pytest.mark.parametrize("w,h", [(1920, 1080), (3840, 2160)])
def test_large_frames_run_and_are_deterministic(setups, w, h):
    scene, rt, o, t = setups("caustics")
    a = rt.run_features(w, h, 1)
    b = rt.run_features(w, h, 1)
    assert a["features"].tobytes() == b["features"].tobytes() and a["ids"].tobytes() == b["ids"].tobytes()
    cov = a["coverage"]
    assert 0.3 < cov.mean() < 1.0 and set(np.unique(cov)) <= {0.0, 1.0}
    assert ((a["ids"][:, :, 0] >= 0) == (cov == 1)).all() and rt.last_features_ms() > 0
    # a few pixels spread over the frame against the oracle (sample 0)
    for (x, y) in ((0, 0), (w - 1, h - 1), (w // 2, h // 2), (w // 3, (2 * h) // 3), (w - 9, 7)):
        _, ray = o.primary_ray(w, h, 0, x, y)
        hit, ent, mat, albedo, normal, depth, tex = fe.sample_features(o, t, ray[None, :])
        assert a["ids"][y, x, 0] == ent[0] and a["ids"][y, x, 1] == mat[0] and cov[y, x] == float(hit[0])
        assert np.ascontiguousarray(a["normal"][y, x]).tobytes() == normal[0].tobytes() and np.ascontiguousarray(a["albedo"][y, x]).tobytes() == albedo[0].tobytes()
        assert abs(a["depth"][y, x] - depth[0]) <= 4 * fe.ULP * depth[0]


def test_bad_arguments_and_missing_scene(setups):
    scene, rt, o, t = setups("caustics")
    L = rt.L
    p = rt.params(3840, 2160)
    rows = rt.local_rows(p)
    out = np.zeros((rows, 3840, 8), np.float32)
    ptr = out.ctypes.data_as(C.c_void_p)
    assert gi.halton_sample_cap(3840, 2160) == 479
    assert L.gi_render_features_host(rt.h, C.byref(p), 480, ptr, 0, None) == gi.GI_E_INVALID
    assert b"480" in L.gi_last_error(rt.h) and b"479" in L.gi_last_error(rt.h)
    assert L.gi_render_features_host(rt.h, C.byref(p), 0, ptr, 0, None) == gi.GI_E_INVALID
    assert L.gi_render_features_host(rt.h, C.byref(p), -3, ptr, 0, None) == gi.GI_E_INVALID
    assert L.gi_render_features_host(rt.h, C.byref(p), 1, None, 0, None) == gi.GI_E_INVALID
    bad = rt.params(0, 10)
    assert L.gi_render_features_host(rt.h, C.byref(bad), 1, ptr, 0, None) == gi.GI_E_INVALID
    with pytest.raises(gi.GiError):
        rt.run_features(3840, 2160, 480)
    assert not out.any()
    empty = gi.RayTracer(0)
    small = empty.params(16, 16)
    o16 = np.zeros((16, 16, 8))
    assert L.gi_render_features_host(empty.h, C.byref(small), 1, o16.ctypes.data_as(C.c_void_p), 1, None) == gi.GI_E_STATE
    assert L.gi_render_features_device(empty.h, C.byref(small), 1, C.c_void_p(16), 1, None) == gi.GI_E_STATE      # refused before the pointer is used


def test_the_frame_is_left_alone(setups):
    scene = pc.load_scene("caustics")
    rt = gi.RayTracer(0).setScene(scene)
    rt.tracePhotonsOnDevice(3000)
    kw = dict(min_samples=7, max_samples=7)
    before = rt.run(64, 48, **kw)
    k_before, ms_before = rt.last_kernel_ms(), rt.last_render_ms()
    assert k_before["trace"] > 0
    assert rt.last_features_ms() == 0.0
    feat = rt.run_features(64, 48, 7)
    assert rt.last_features_ms() > 0
    assert rt.last_kernel_ms() == k_before and rt.last_render_ms() == ms_before      # the frame's times are still the frame's
    after = rt.run(64, 48, **kw)
    assert before.tobytes() == after.tobytes()
    assert rt.run_features(64, 48, 7)["features"].tobytes() == feat["features"].tobytes()
    # the other schedules of the frame, with a feature pass in between
    for mode in ("rounds", "megakernel", "wavefront"):
        rt.set_render_mode(mode)
        a = rt.run(64, 48, **kw)
        rt.run_features(64, 48, 2)
        assert rt.run(64, 48, **kw).tobytes() == a.tobytes()


def test_per_node_walk_gives_the_same_buffers(setups):
    # (large_alpha: k_aov's first hits come from the beauty pass's trace, which in a scene with large alpha-tested entities must not cut its walk short)
    for name in ("caustics", "spheres_opaque", "textures_opaque", "large_alpha", "large_alpha_tex"):
        scene, rt, o, t = setups(name)
        wide = rt.run_features(W, H, 2)
        try:
            assert rt.set_wide_nodes(False) is False
            per_node = rt.run_features(W, H, 2)
        finally:
            rt.set_wide_nodes(True)
        assert wide["features"].tobytes() == per_node["features"].tobytes() and wide["ids"].tobytes() == per_node["ids"].tobytes()


def test_cli_writes_the_feature_files(setups, tmp_path, capsys):
    scn = os.path.join(pc.ROOT, pc.SCN["caustics"])
    plain = tmp_path / "plain"
    plain.mkdir()
    assert cli.main([scn, "-o", str(plain / "out.ppm"), "--width", "80", "--height", "56", "--samples", "2", "--photons", "2000"]) == 0
    assert sorted(os.listdir(plain)) == ["out.ppm"]
    line_plain = capsys.readouterr().out
    assert "features" not in line_plain
    with_f = tmp_path / "with"
    with_f.mkdir()
    assert cli.main([scn, "-o", str(with_f / "out.ppm"), "--width", "80", "--height", "56", "--samples", "2", "--photons", "2000",
                     "--features", str(with_f / "f"), "--feature-samples", "3"]) == 0
    assert sorted(os.listdir(with_f)) == ["f_albedo.pfm", "f_coverage.pfm", "f_depth.pfm", "f_normal.pfm", "out.ppm"]
    assert "features 3 spp" in capsys.readouterr().out
    assert open(plain / "out.ppm", "rb").read() == open(with_f / "out.ppm", "rb").read()
    scene, rt, o, t = setups("caustics")
    want = rt.run_features(80, 56, 3, f64=False)
    for name, shape in (("albedo", (56, 80, 3)), ("normal", (56, 80, 3)), ("depth", (56, 80)), ("coverage", (56, 80))):
        img = fe.read_pfm(with_f / f"f_{name}.pfm")
        assert img.shape == shape and img.tobytes() == np.ascontiguousarray(want[name]).tobytes(), name


def test_cpp_render_features_matches_the_python_mirror(setups):
    """RayTracer::renderFeatures of the drop-in C++ class (include/gi/raytracer.h) fills its struct with what run_features returns."""
    import re
    import subprocess
    exe = os.path.join(pc.ROOT, "tests", "cpp", "test_features")
    host_build.client("tests/cpp/test_features.cpp", exe, "-O1")
    out = subprocess.run([exe, os.path.join(pc.ROOT, pc.SCN["caustics"]), "80", "56", "3"], check=True, capture_output=True, text=True).stdout
    npix = 80 * 56
    assert f"features 80x56 n 3 sizes {npix * 3} {npix * 3} {npix} {npix} {npix} {npix}" in out, out
    m = re.search(r"sums (\S+) (\S+) (\S+) (\S+) (-?\d+) (-?\d+)", out)
    assert m and "n=0 ok 0" in out, out
    scene, rt, o, t = setups("caustics")
    f = rt.run_features(80, 56, 3)

    def seq_sum(a):                # the C++ program adds in memory order
        s = 0.0
        for v in np.ascontiguousarray(a).reshape(-1):
            s += float(v)
        return s
    assert [float(m.group(k)) for k in (1, 2, 3, 4)] == [seq_sum(f["albedo"]), seq_sum(f["normal"]), seq_sum(f["depth"]), seq_sum(f["coverage"])]
    assert int(m.group(5)) == int((f["ids"][:, :, 0] < 0).sum()) == int(m.group(6)) == int((f["ids"][:, :, 1] < 0).sum()) > 0      # misses
