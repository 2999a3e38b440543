"""The a-trous denoiser (gi_denoise_*, k_dn_pack / k_dn_level) on the GPU, through the C ABI via the Python mirror.

The expectation is tests/denoise_expect.py: the header's formula in numpy f64 with the same operations in the same order.  The library is built
without contraction and the filter uses IEEE operations only, so every comparison here is equality of bytes unless a test says otherwise."""
import ctypes as C
import os

import numpy as np
import pytest

import gi_raytracer_amd as gi
from gi_raytracer_amd import __main__ as cli

import denoise_expect as de
import host_build
import parity_checks as pc

pytestmark = pytest.mark.gpu

W, H = 96, 72


@pytest.fixture(scope="module")
def rt0():
    return gi.RayTracer(0)          # no scene: the denoiser needs none


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def report(tag, got, want):
    bad = int((np.ascontiguousarray(got).view(np.uint8) != np.ascontiguousarray(want).view(np.uint8)).reshape(got.shape + (-1,)).any(-1).sum())
    with np.errstate(all="ignore"):
        rel = np.abs(got.astype(np.float64) - want) / np.maximum(np.abs(want), 1e-300)
    print(f"{tag}: {bad} of {got.size} values differ" + (f", largest relative error {np.nanmax(rel):.3e}" if bad else ""))


@pytest.mark.parametrize("w,h", [(1, 1), (3, 2), (37, 29), (96, 72), (200, 131), (32, 16), (33, 17), (65, 33)])
def test_synthetic_frames_match_the_expectation(rt0, w, h):
    noisy, feat, _ = de.synthetic(w, h, seed=w + h)
    for it in range(1, 7):
        for demodulate in (1, 0):
            kw = dict(iterations=it, demodulate=demodulate)
            got, want = rt0.denoise(noisy, feat, **kw), de.expected(noisy, feat, **kw)
            report(f"{w}x{h} {kw}", got, want)
            assert same(got, want), kw
    for off in ("sigma_color", "sigma_normal", "sigma_depth", "sigma_albedo"):
        for demodulate in (1, 0):
            kw = {off: 0.0, "iterations": 3, "demodulate": demodulate}
            assert same(rt0.denoise(noisy, feat, **kw), de.expected(noisy, feat, **kw)), kw
    assert same(rt0.denoise(noisy, feat, iterations=0), noisy)
    assert same(rt0.denoise(noisy, feat), de.expected(noisy, feat))          # the defaults


@pytest.mark.parametrize("name", ["caustics", "cornell", "textures_opaque", "spheres"])
def test_rendered_frames_match_the_expectation(name):
    scene = pc.load_scene(name)
    rt = gi.RayTracer(0).setScene(scene)
    if name == "caustics":
        rt.tracePhotonsOnDevice(3000)
    color = rt.run(W, H, min_samples=4, max_samples=4)
    fb = rt.run_features(W, H, 4)
    got, want = rt.denoise(color, fb), de.expected(color, fb["features"])
    report(name, got, want)
    assert same(got, want)
    assert (got != color).any() and np.isfinite(got).all()
    assert same(rt.denoise(color, fb["features"], iterations=2, demodulate=0), de.expected(color, fb["features"], iterations=2, demodulate=0))


@pytest.mark.parametrize("c64", [False, True])
@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("o64", [False, True])
def test_float_and_double_buffers(rt0, c64, f64, o64):
    noisy, feat, _ = de.synthetic(61, 47, seed=9)
    color = noisy.astype(np.float64 if c64 else np.float32)
    feats = feat.astype(np.float64 if f64 else np.float32)
    odt = np.float64 if o64 else np.float32
    for it in (0, 1, 4):
        got = rt0.denoise(color, feats, f64=o64, iterations=it)
        # the expectation widens its inputs and rounds its f64 result once
        assert same(got, de.expected(color, feats, odt, iterations=it)), it


def test_out_may_alias_color_and_calls_repeat(rt0):
    noisy, feat, _ = de.synthetic(130, 77, seed=11)
    want = de.expected(noisy, feat)
    assert same(rt0.denoise(noisy, feat), want) and same(rt0.denoise(noisy, feat), want)
    # device buffers from the HIP runtime the library itself uses (no second runtime in this process)
    hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")

    def upload(a):
        d = C.c_void_p()
        assert hip.hipMalloc(C.byref(d), C.c_size_t(a.nbytes)) == 0
        assert hip.hipMemcpy(d, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0      # hipMemcpyHostToDevice
        return d

    def download(d, like):
        got = np.zeros_like(like)
        assert hip.hipDeviceSynchronize() == 0
        assert hip.hipMemcpy(got.ctypes.data_as(C.c_void_p), d, C.c_size_t(got.nbytes), 2) == 0   # hipMemcpyDeviceToHost
        return got

    for dt, is64 in ((np.float64, True), (np.float32, False)):
        color, feats = noisy.astype(dt), feat.astype(dt)
        e = de.expected(color, feats, dt)
        d_col, d_ft, d_out = upload(color), upload(feats), upload(np.zeros_like(color))
        try:
            p = rt0.denoise_params(130, 77)
            rt0.denoise_device(p, d_col.value, d_ft.value, d_out.value, is64, is64, is64)
            assert same(download(d_out, color), e) and same(download(d_col, color), color)
            rt0.denoise_device(p, d_col.value, d_ft.value, d_col.value, is64, is64, is64)       # in place
            assert same(download(d_col, color), e) and rt0.last_denoise_ms() > 0
        finally:
            for d in (d_col, d_ft, d_out):
                hip.hipFree(d)


def test_non_finite_pixels(rt0):
    w, h, it = 70, 60, 2
    noisy, feat, _ = de.synthetic(w, h, seed=3)
    clean_out = rt0.denoise(noisy, feat, iterations=it)
    bad = noisy.copy()
    spots = [(10, 12, np.nan), (40, 30, np.inf), (41, 30, -np.inf), (0, 0, np.nan), (h - 1, w - 1, np.inf)]
    for (y, x, v) in spots:
        bad[y, x, 1] = v
    out = rt0.denoise(bad, feat, iterations=it)
    assert np.isfinite(out).all() and same(out, de.expected(bad, feat, iterations=it))
    reach = de.margin(it)
    far = np.ones((h, w), bool)
    for (y, x, _) in spots:
        far[max(0, y - reach):y + reach + 1, max(0, x - reach):x + reach + 1] = False
    assert far.any() and out[far].tobytes() == clean_out[far].tobytes()
    assert same(rt0.denoise(bad, feat), de.expected(bad, feat))
    nan_frame = np.full((9, 7, 3), np.nan)
    assert not rt0.denoise(nan_frame, feat[:9, :7], iterations=3).any()


@pytest.mark.parametrize("w,h", [(1920, 1080), (3840, 2160)])
def test_large_frames_run_and_match_in_windows(rt0, w, h):
    noisy, feat, _ = de.synthetic(w, h, seed=2)
    noisy, feat = noisy.astype(np.float32), feat.astype(np.float32)
    a = rt0.denoise(noisy, feat)
    ms = rt0.last_denoise_ms()
    b = rt0.denoise(noisy, feat)
    assert a.dtype == np.float32 and a.tobytes() == b.tobytes() and ms > 0 and np.isfinite(a).all()
    print(f"{w}x{h}: five levels, f32 in and out: {ms:.3f} ms, then {rt0.last_denoise_ms():.3f} ms")
    for (x0, y0) in ((0, 0), (w - 64, 0), (0, h - 64), (w - 64, h - 64), (w // 2 - 32, h // 2 - 32)):
        want = de.expected_window(noisy, feat, x0, y0, 64, 64, np.float32)
        assert same(a[y0:y0 + 64, x0:x0 + 64], want), (x0, y0)
    # and a window of a deeper pass, whose steps of 32 and 64 take sub-lattices of a few cells
    c = rt0.denoise(noisy, feat, iterations=7)
    assert same(c[h - 64:, w // 2:w // 2 + 64], de.expected_window(noisy, feat, w // 2, h - 64, 64, 64, np.float32, iterations=7))


def test_the_frame_is_left_alone():
    scene = pc.load_scene("caustics")
    rt = gi.RayTracer(0).setScene(scene)
    rt.tracePhotonsOnDevice(3000)
    kw = dict(min_samples=7, max_samples=7)
    before = rt.run(64, 48, **kw)
    fb = rt.run_features(64, 48, 7)
    k_before, ms_before, f_before = rt.last_kernel_ms(), rt.last_render_ms(), rt.last_features_ms()
    assert k_before["trace"] > 0 and f_before > 0 and rt.last_denoise_ms() == 0.0
    den = rt.denoise(before, fb)
    assert rt.last_denoise_ms() > 0
    assert rt.last_kernel_ms() == k_before and rt.last_render_ms() == ms_before and rt.last_features_ms() == f_before
    after = rt.run(64, 48, **kw)
    assert before.tobytes() == after.tobytes()
    assert rt.run_features(64, 48, 7)["features"].tobytes() == fb["features"].tobytes()
    assert same(rt.denoise(after, fb), den)
    for mode in ("rounds", "megakernel", "wavefront"):
        rt.set_render_mode(mode)
        a = rt.run(64, 48, **kw)
        rt.denoise(a, fb, iterations=3)
        assert rt.run(64, 48, **kw).tobytes() == a.tobytes()


def test_bad_arguments_are_refused_and_leave_the_output_alone(rt0):
    L = rt0.L
    noisy, feat, _ = de.synthetic(20, 10)
    out = np.full((10, 20, 3), 7.0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(p, color=noisy, features=feat, o=out):
        return L.gi_denoise_host(rt0.h, C.byref(p) if p is not None else None, vp(color) if color is not None else None, 1,
                                 vp(features) if features is not None else None, 1, vp(o) if o is not None else None, 1)

    for kw in (dict(iterations=-1), dict(iterations=9), dict(sigma_color=-1.0), dict(sigma_normal=float("nan")), dict(sigma_depth=-0.5), dict(sigma_albedo=float("nan"))):
        assert call(rt0.denoise_params(20, 10, **kw)) == gi.GI_E_INVALID, kw
        msg = L.gi_last_error(rt0.h)
        assert msg.startswith(b"denoise:") and next(iter(kw)).encode() in msg, msg
    for (w, h) in ((0, 10), (20, 0), (-3, 10)):
        assert call(rt0.denoise_params(w, h)) == gi.GI_E_INVALID and b"width" in L.gi_last_error(rt0.h)
    good = rt0.denoise_params(20, 10)
    assert call(None) == gi.GI_E_INVALID
    assert call(good, color=None) == gi.GI_E_INVALID and call(good, features=None) == gi.GI_E_INVALID and call(good, o=None) == gi.GI_E_INVALID
    assert L.gi_denoise_device(rt0.h, C.byref(rt0.denoise_params(20, 10, iterations=9)), C.c_void_p(16), 1, C.c_void_p(16), 1, C.c_void_p(16), 1) == gi.GI_E_INVALID
    assert (out == 7.0).all()
    with pytest.raises(gi.GiError):
        rt0.denoise(noisy, feat, iterations=12)
    with pytest.raises(TypeError):
        rt0.denoise(noisy, feat, sigma=1.0)
    with pytest.raises(ValueError):
        rt0.denoise(noisy, feat[:, :5])
    assert call(good) == gi.GI_OK and same(out, de.expected(noisy, feat))


def test_quality_on_the_gpu():
    """cornell 256 x 256 at 4 spp against 1024 spp, both from the GPU: the denoised frame must be closer to the target than the noisy one."""
    scene = pc.load_scene("cornell")
    rt = gi.RayTracer(0).setScene(scene)
    rt.tracePhotonsOnDevice(20000)
    noisy = rt.run(256, 256, min_samples=4, max_samples=4)
    target = rt.run(256, 256, min_samples=1024, max_samples=1024)
    fb = rt.run_features(256, 256, 4)
    out = rt.denoise(noisy, fb)
    a, b = de.rmse(noisy, target), de.rmse(out, target)
    print(f"cornell 256x256: rmse against 1024 spp: noisy {a:.5f}, denoised {b:.5f}, ratio {b / a:.3f}, {rt.last_denoise_ms():.3f} ms")
    assert b < a


def read_ppm(path):
    raw = open(path, "rb").read()
    magic, dims, maxv, data = raw.split(b"\n", 3)
    w, h = (int(v) for v in dims.split())
    assert magic == b"P6" and maxv == b"255" and len(data) == w * h * 3
    return np.frombuffer(data, np.uint8).reshape(h, w, 3)


def test_cli_writes_the_denoised_frame(tmp_path, capsys):
    import features_expect as fe
    scn = os.path.join(pc.ROOT, pc.SCN["caustics"])
    common = ["--width", "80", "--height", "56", "--samples", "2", "--photons", "2000"]
    plain = tmp_path / "plain"
    plain.mkdir()
    assert cli.main([scn, "-o", str(plain / "out.ppm")] + common) == 0
    assert sorted(os.listdir(plain)) == ["out.ppm"] and "; denoised (" not in capsys.readouterr().out
    with_d = tmp_path / "with"
    with_d.mkdir()
    assert cli.main([scn, "-o", str(with_d / "out.ppm")] + common + ["--denoise", str(with_d / "den.ppm"), "--denoise-pfm", str(with_d / "den.pfm"),
                                                                      "--denoise-iterations", "4", "--denoise-sigmas", "1.5", "0.5", "0.1", "0.2"]) == 0
    assert sorted(os.listdir(with_d)) == ["den.pfm", "den.ppm", "out.ppm"] and "denoised (2 spp features)" in capsys.readouterr().out
    assert open(plain / "out.ppm", "rb").read() == open(with_d / "out.ppm", "rb").read()
    rt = gi.RayTracer(0).setScene(pc.load_scene("caustics"))
    rt.min_samples = rt.max_samples = 2
    rt.tracePhotons(2000)
    lin = rt.run(80, 56, f64=False)
    fb = rt.run_features(80, 56, 2, f64=False, want_ids=False)
    den = rt.denoise(lin, fb, iterations=4, sigma_color=1.5, sigma_normal=0.5, sigma_depth=0.1, sigma_albedo=0.2)
    assert den.dtype == np.float32 and same(den, de.expected(lin, fb["features"], np.float32, iterations=4, sigma_color=1.5, sigma_normal=0.5, sigma_depth=0.1, sigma_albedo=0.2))
    assert same(read_ppm(with_d / "den.ppm"), gi.to_rgb8(den))
    assert same(fe.read_pfm(with_d / "den.pfm"), den)
    assert same(read_ppm(with_d / "out.ppm"), gi.to_rgb8(lin))


def test_cpp_denoise_matches_the_python_mirror(tmp_path):
    """RayTracer::denoise of the drop-in C++ class (include/gi/raytracer.h) returns what RayTracer.denoise returns."""
    import re
    import subprocess
    exe = os.path.join(pc.ROOT, "tests", "cpp", "test_denoise")
    host_build.client("tests/cpp/test_denoise.cpp", exe, "-O1")
    out = subprocess.run([exe, os.path.join(pc.ROOT, pc.SCN["caustics"]), "80", "56", "3", "4", str(tmp_path / "dump.bin")], check=True, capture_output=True, text=True).stdout
    assert f"denoise 80x56 iterations 4 size {80 * 56 * 3}" in out, out
    assert "defaults ok 1" in out and "iterations=9 ok 0 kept 1" in out and "short colour ok 0" in out, out
    m = re.search(r"sums (\S+) (\S+)", out)
    md = re.search(r"default sum (\S+)", out)
    assert m and md, out
    # the program's own buffers (its feature pass runs on the C++ loader's scene, whose vertex normals differ from the Python loader's in the last
    # bits on a few hundred pixels -- so the mirror is given the program's features, not its own)
    raw = np.fromfile(tmp_path / "dump.bin", np.float64)
    npix = 80 * 56
    albedo, normal, depth, coverage, c_color, c_out = np.split(raw, np.cumsum([npix * 3, npix * 3, npix, npix, npix * 3]))
    assert len(c_out) == npix * 3
    feat = np.concatenate([albedo.reshape(56, 80, 3), normal.reshape(56, 80, 3), depth.reshape(56, 80, 1), coverage.reshape(56, 80, 1)], axis=2)
    mine = gi.RayTracer(0).setScene(pc.load_scene("caustics")).run_features(80, 56, 3)
    assert same(np.ascontiguousarray(mine["coverage"]), feat[:, :, 7].copy()) and np.allclose(mine["features"], feat, rtol=1e-12, atol=1e-12)
    i = np.arange(npix * 3, dtype=np.uint64)
    hsh = (i * np.uint64(2654435761)) & np.uint64(0xffffffff)
    noise = ((hsh >> np.uint64(8)) & np.uint64(0xffff)).astype(np.float64) / 65536.0
    color = (albedo * noise + 0.0625 * np.repeat(coverage, 3)).reshape(56, 80, 3)
    assert color.tobytes() == c_color.tobytes()
    rt = gi.RayTracer(0)
    want = rt.denoise(color, feat, iterations=4)
    assert c_out.tobytes() == want.tobytes() and same(want, de.expected(color, feat, iterations=4))

    def seq_sum(a):                # the C++ program adds in memory order
        s = 0.0
        for v in np.ascontiguousarray(a).reshape(-1):
            s += float(v)
        return s
    assert float(m.group(1)) == seq_sum(color)
    assert float(m.group(2)) == seq_sum(want)
    assert float(md.group(1)) == seq_sum(rt.denoise(color, feat))
