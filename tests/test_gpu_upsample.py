"""The guided upsampler (gi_upsample_*, k_dn_pack on the low frame + k_up_sample) on the GPU, through the C ABI via the Python mirror.

The expectation is tests/upsample_expect.py: the header's formula in numpy f64 with the same operations in the same order.  The library is built
without contraction and the upsampler uses IEEE operations only, so every comparison here is equality of bytes."""
import ctypes as C
import os

import numpy as np
import pytest

import gi_raytracer_amd as gi
from gi_raytracer_amd import __main__ as cli

import denoise_expect as de
import host_build
import parity_checks as pc
import upsample_expect as ue

pytestmark = pytest.mark.gpu

W, H, S = 96, 72, 2                 # the rendered frames: 96 x 72 from a 48 x 36 render
SPP = 4


@pytest.fixture(scope="module")
def rt0():
    return gi.RayTracer(0)          # no scene: the upsampler needs none


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def report(tag, got, want):
    bad = int((np.ascontiguousarray(got).view(np.uint8) != np.ascontiguousarray(want).view(np.uint8)).reshape(got.shape + (-1,)).any(-1).sum())
    with np.errstate(all="ignore"):
        rel = np.abs(got.astype(np.float64) - want) / np.maximum(np.abs(want), 1e-300)
    print(f"{tag}: {bad} of {got.size} values differ" + (f", largest relative error {np.nanmax(rel):.3e}" if bad else ""))


def reduced(w, h, factor, seed=1, noise=0.5):
    """(low colour, low features, full features) of de.synthetic's frame, the low ones box-reduced."""
    noisy, feat, _ = de.synthetic(w, h, seed=seed, noise=noise)
    return ue.box_reduce(noisy, factor), ue.box_reduce(feat, factor), feat


@pytest.mark.parametrize("w,h,factor", [(1, 1, 2), (3, 2, 2), (37, 29, 2), (37, 29, 3), (37, 29, 4), (70, 37, 2), (200, 131, 3), (64, 32, 8), (33, 17, 5), (65, 33, 7), (9, 9, 8), (32, 16, 2)])
def test_synthetic_frames_match_the_expectation(rt0, w, h, factor):
    low, low_feat, feat = reduced(w, h, factor, seed=w + h)
    assert low.shape[:2] == ue.low_size(w, h, factor)[::-1]
    cases = [dict()] + [dict(demodulate=d) for d in (1, 0)]
    cases += [{off: 0.0, "demodulate": d} for off in ("sigma_normal", "sigma_depth", "sigma_albedo") for d in (1, 0)]
    cases += [dict(sigma_albedo=0.25, demodulate=d) for d in (1, 0)]          # the term that is off by default, on
    for kw in cases:
        got, want = rt0.upsample(low, low_feat, feat, factor, **kw), ue.expected(low, low_feat, feat, factor, **kw)
        report(f"{w}x{h} factor {factor} {kw}", got, want)
        assert same(got, want), kw


@pytest.mark.parametrize("c64", [False, True])
@pytest.mark.parametrize("l64", [False, True])
@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("o64", [False, True])
def test_float_and_double_buffers(rt0, c64, l64, f64, o64):
    """61 x 47, factor 2: the two feature buffers take their types independently, so sixteen combinations, not eight."""
    low, low_feat, feat = reduced(61, 47, 2, seed=9)
    ty = lambda is64: np.float64 if is64 else np.float32
    low, low_feat, feat = low.astype(ty(c64)), low_feat.astype(ty(l64)), feat.astype(ty(f64))
    got = rt0.upsample(low, low_feat, feat, 2, f64=o64)
    assert same(got, ue.expected(low, low_feat, feat, 2, ty(o64)))          # the expectation widens its inputs and rounds its f64 result once
    if c64 == l64 == f64 == o64:
        assert same(rt0.upsample(low, low_feat, feat, 2), got)              # the output's type defaults to the colour's


def test_non_finite_low_pixels_and_a_pixel_without_taps(rt0):
    w, h, factor = 70, 60, 2
    low, low_feat, feat = reduced(w, h, factor, seed=3)
    good = rt0.upsample(low, low_feat, feat, factor)
    bad = low.copy()
    spots = [(5, 6, np.nan), (20, 15, np.inf), (20, 16, -np.inf), (0, 0, np.nan), (low.shape[0] - 1, low.shape[1] - 1, np.inf)]
    for (Y, X, v) in spots:
        bad[Y, X, 1] = v
    feat = feat.copy()
    for (y, x) in ((1, 1), (30, 20), (41, 33)):          # normals orthogonal to both surfaces: every tap rejected; (1, 1)'s nearest low pixel is NaN
        feat[y, x, 3:6] = [0.0, 0.0, 1.0]
    out = rt0.upsample(bad, low_feat, feat, factor)
    want = ue.expected(bad, low_feat, feat, factor)
    report("non-finite", out, want)
    assert np.isfinite(out).all() and same(out, want)
    assert not out[1, 1].any() and same(out[30, 20], (low / de.modulation(low_feat, 1))[15, 10] * de.modulation(feat, 1)[30, 20])
    far = np.ones((h, w), bool)
    for (Y, X, _) in spots:
        far[max(0, (Y - 2) * factor):(Y + 3) * factor, max(0, (X - 2) * factor):(X + 3) * factor] = False
    far[1, 1] = far[30, 20] = far[41, 33] = False
    assert far.any() and out[far].tobytes() == good[far].tobytes()
    assert not rt0.upsample(np.full_like(low, np.nan), low_feat, feat, factor).any()


def test_device_pointers_and_a_repeat(rt0):
    w, h, factor = 130, 77, 3
    low, low_feat, feat = reduced(w, h, factor, seed=11)
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
        lc, lf, ff = low.astype(dt), low_feat.astype(dt), feat.astype(dt)
        e = ue.expected(lc, lf, ff, factor, dt)
        d_lc, d_lf, d_ff, d_out = upload(lc), upload(lf), upload(ff), upload(np.full((h, w, 3), 7, dt))
        try:
            p = rt0.upsample_params(w, h, factor)
            assert (p.low_width, p.low_height) == ue.low_size(w, h, factor)
            rt0.upsample_device(p, d_lc.value, d_lf.value, d_ff.value, d_out.value, is64, is64, is64, is64)
            assert same(download(d_out, e), e) and rt0.last_upsample_ms() > 0
            assert same(download(d_lc, lc), lc) and same(download(d_lf, lf), lf) and same(download(d_ff, ff), ff)
            rt0.upsample_device(p, d_lc.value, d_lf.value, d_ff.value, d_out.value, is64, is64, is64, is64)
            assert same(download(d_out, e), e)
        finally:
            for d in (d_lc, d_lf, d_ff, d_out):
                hip.hipFree(d)


def test_the_scratch_is_shared_with_the_denoiser():
    """Both passes pack into the same buffers of the context: in either order and at growing sizes, each still gives its own expectation."""
    rt = gi.RayTracer(0)
    noisy, dfeat, _ = de.synthetic(50, 40, seed=5)
    low, low_feat, feat = reduced(90, 66, 2, seed=6)
    assert same(rt.upsample(low, low_feat, feat, 2), ue.expected(low, low_feat, feat, 2))        # sizes the scratch for 45 x 33
    assert same(rt.denoise(noisy, dfeat), de.expected(noisy, dfeat))                                # 50 x 40: grows it, all three buffers
    assert same(rt.upsample(low, low_feat, feat, 2), ue.expected(low, low_feat, feat, 2))
    assert same(rt.denoise(noisy[:30, :30], dfeat[:30, :30], iterations=2), de.expected(noisy[:30, :30], dfeat[:30, :30], iterations=2))


def test_bad_arguments_are_refused_and_leave_the_output_alone(rt0):
    L = rt0.L
    w, h, factor = 21, 10, 2
    low, low_feat, feat = reduced(w, h, factor)
    out = np.full((h, w, 3), 7.0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None

    def call(p, lc=low, lf=low_feat, ff=feat, o=out):
        return L.gi_upsample_host(rt0.h, C.byref(p) if p is not None else None, vp(lc), 1, vp(lf), 1, vp(ff), 1, vp(o), 1)

    def params(**fields):
        p = rt0.upsample_params(w, h, factor)
        for k, v in fields.items():
            setattr(p, k, v)
        return p

    for kw in (dict(sigma_normal=-1.0), dict(sigma_depth=float("nan")), dict(sigma_albedo=-0.5), dict(sigma_normal=float("nan"))):
        assert call(rt0.upsample_params(w, h, factor, **kw)) == gi.GI_E_INVALID, kw
        msg = L.gi_last_error(rt0.h)
        assert msg.startswith(b"upsample:") and next(iter(kw)).encode() in msg, msg
    for f in (1, 0, -2, 9):
        assert call(params(factor=f)) == gi.GI_E_INVALID and b"factor" in L.gi_last_error(rt0.h), f
    for fields in (dict(width=0), dict(height=0), dict(width=-3)):
        assert call(params(**fields)) == gi.GI_E_INVALID and b"width" in L.gi_last_error(rt0.h), fields
    # low dimensions that are not the ceilings: floor(21 / 2) = 10, one too many, the two swapped, and those of another factor
    for fields in (dict(low_width=10), dict(low_width=12), dict(low_height=4), dict(low_height=6), dict(low_width=5, low_height=11), dict(low_width=7, low_height=4)):
        assert call(params(**fields)) == gi.GI_E_INVALID and b"ceilings" in L.gi_last_error(rt0.h), fields
    good = rt0.upsample_params(w, h, factor)
    assert call(None) == gi.GI_E_INVALID
    assert call(good, lc=None) == gi.GI_E_INVALID and call(good, lf=None) == gi.GI_E_INVALID and call(good, ff=None) == gi.GI_E_INVALID and call(good, o=None) == gi.GI_E_INVALID
    dev = lambda p, ptrs=(16, 16, 16, 16): L.gi_upsample_device(rt0.h, C.byref(p), C.c_void_p(ptrs[0]), 1, C.c_void_p(ptrs[1]), 1, C.c_void_p(ptrs[2]), 1, C.c_void_p(ptrs[3]), 1)
    assert dev(params(factor=9)) == gi.GI_E_INVALID and dev(params(low_width=10)) == gi.GI_E_INVALID
    assert dev(good, (16, 16, 16, None)) == gi.GI_E_INVALID and dev(good, (None, 16, 16, 16)) == gi.GI_E_INVALID
    assert (out == 7.0).all()
    with pytest.raises(gi.GiError):
        rt0.upsample(low, low_feat, feat, factor, sigma_depth=-1.0)
    with pytest.raises(TypeError):
        rt0.upsample(low, low_feat, feat, factor, sigma_color=1.0)        # the upsampler has no colour term
    with pytest.raises(ValueError):
        rt0.upsample(low[:, :10], low_feat[:, :10], feat, factor)
    with pytest.raises(ValueError):
        rt0.upsample(low, low_feat, feat, 3)
    assert call(good) == gi.GI_OK and same(out, ue.expected(low, low_feat, feat, factor))


@pytest.fixture(scope="module")
def cornell():
    rt = gi.RayTracer(0).setScene(pc.load_scene("cornell"))
    rt.tracePhotonsOnDevice(3000)
    return rt


def rendered(rt):
    kw = dict(min_samples=SPP, max_samples=SPP)
    return rt.run(W // S, H // S, **kw), rt.run_features(W // S, H // S, SPP, want_ids=False), rt.run_features(W, H, SPP, want_ids=False)


@pytest.mark.parametrize("name", ["cornell", "textures_opaque"])
def test_rendered_frames_match_the_expectation(name, cornell):
    rt = cornell if name == "cornell" else gi.RayTracer(0).setScene(pc.load_scene(name))
    low, fl, ff = rendered(rt)
    got, want = rt.upsample(low, fl, ff, S), ue.expected(low, fl["features"], ff["features"], S)
    report(name, got, want)
    assert same(got, want)
    assert np.isfinite(got).all() and (got != ue.nearest(low, W, H, S)).any()
    assert same(rt.upsample(low, fl["features"], ff["features"], S, demodulate=0, sigma_albedo=0.25),
                ue.expected(low, fl["features"], ff["features"], S, demodulate=0, sigma_albedo=0.25))


@pytest.mark.parametrize("denoise", [False, True])
def test_run_upsampled_equals_the_steps_done_by_hand(cornell, denoise):
    rt = cornell
    low, fl, ff = rendered(rt)
    if denoise:
        low = rt.denoise(low, fl)
    by_hand = rt.upsample(low, fl, ff, S)
    got = rt.run_upsampled(W, H, S, SPP, denoise=denoise, min_samples=SPP, max_samples=SPP)
    assert got.shape == (H, W, 3) and same(got, by_hand)
    assert same(by_hand, ue.expected(low, fl["features"], ff["features"], S))
    with pytest.raises(ValueError):
        rt.run_upsampled(W + 1, H, S, SPP)
    with pytest.raises(ValueError):
        rt.run_upsampled(W, H, 5, SPP)           # 5 divides neither


def test_an_open_session_survives_an_upsample_between_two_steps(cornell):
    rt = cornell
    wl, hl = W // S, H // S
    oneshot = rt.run(wl, hl, min_samples=7, max_samples=7)
    fl, ff = rt.run_features(wl, hl, SPP, want_ids=False), rt.run_features(W, H, SPP, want_ids=False)
    with rt.progressive(wl, hl, min_samples=7, max_samples=7) as s:
        first = s.step(3)
        up = rt.upsample(first, fl, ff, S)                         # a reduced-size session, upsampled after a step
        assert same(up, ue.expected(first, fl["features"], ff["features"], S))
        assert s.sample_end == 3
        last = s.step(4)
        assert np.array_equal(last.view(np.uint64), oneshot.view(np.uint64))
        assert same(rt.upsample(last, fl, ff, S), rt.upsample(oneshot, fl, ff, S))


def test_the_other_times_are_left_alone(cornell):
    rt = cornell
    low, fl, ff = rendered(rt)
    rt.denoise(low, fl)
    before = (rt.last_kernel_ms(), rt.last_render_ms(), rt.last_features_ms(), rt.last_denoise_ms())
    assert before[1][0] > 0 and before[2] > 0 and before[3] > 0
    fresh = gi.RayTracer(0)
    assert fresh.last_upsample_ms() == 0.0
    rt.upsample(low, fl, ff, S)
    assert rt.last_upsample_ms() > 0
    assert (rt.last_kernel_ms(), rt.last_render_ms(), rt.last_features_ms(), rt.last_denoise_ms()) == before
    after = rendered(rt)
    assert same(after[0], low) and same(after[2]["features"], ff["features"])


def read_ppm(path):
    raw = open(path, "rb").read()
    magic, dims, maxv, data = raw.split(b"\n", 3)
    w, h = (int(v) for v in dims.split())
    assert magic == b"P6" and maxv == b"255" and len(data) == w * h * 3
    return np.frombuffer(data, np.uint8).reshape(h, w, 3)


def test_cli_writes_the_upsampled_frame(tmp_path, capsys):
    import features_expect as fe
    scn = os.path.join(pc.ROOT, pc.SCN["caustics"])
    args = [scn, "-o", str(tmp_path / "o.ppm"), "--pfm", str(tmp_path / "o.pfm"), "--width", "80", "--height", "56", "--samples", "2", "2", "--photons", "2000",
            "--upsample", "2", "--upsample-pfm", str(tmp_path / "low.pfm"), "--denoise", str(tmp_path / "den.ppm"), "--denoise-iterations", "3"]
    assert cli.main(args) == 0
    line = capsys.readouterr().out
    assert "80x56" in line and "upsampled x2 from 40x28 (2 spp features)" in line and "denoised (2 spp features)" in line
    assert sorted(os.listdir(tmp_path)) == ["den.ppm", "low.pfm", "o.pfm", "o.ppm"]
    rt = gi.RayTracer(0).setScene(pc.load_scene("caustics"))
    rt.min_samples = rt.max_samples = 2
    rt.tracePhotons(2000)
    low = rt.run(40, 28, f64=False)
    fl, ff = rt.run_features(40, 28, 2, f64=False, want_ids=False), rt.run_features(80, 56, 2, f64=False, want_ids=False)
    up = rt.upsample(low, fl, ff, 2)
    assert up.dtype == np.float32 and same(up, ue.expected(low, fl["features"], ff["features"], 2, np.float32))
    assert same(fe.read_pfm(tmp_path / "low.pfm"), low) and same(fe.read_pfm(tmp_path / "o.pfm"), up)
    assert same(read_ppm(tmp_path / "o.ppm"), gi.to_rgb8(up))
    assert same(read_ppm(tmp_path / "den.ppm"), gi.to_rgb8(rt.upsample(rt.denoise(low, fl, iterations=3), fl, ff, 2)))


def test_cpp_upsample_matches_the_python_mirror(tmp_path, rt0):
    """RayTracer::upsample of the drop-in C++ class (include/gi/raytracer.h) returns what RayTracer.upsample returns on the program's own buffers."""
    import subprocess
    exe = os.path.join(pc.ROOT, "tests", "cpp", "test_upsample")
    host_build.client("tests/cpp/test_upsample.cpp", exe, "-O1")
    w, h, factor = 75, 41, 3
    wl, hl = ue.low_size(w, h, factor)
    out = subprocess.run([exe, str(w), str(h), str(factor), str(tmp_path / "dump.bin")], check=True, capture_output=True, text=True).stdout
    assert f"upsample {w}x{h} from {wl}x{hl} size {w * h * 3}" in out, out
    assert "sigma_depth=-1 ok 0 kept 1" in out and "factor+1 ok 0 kept 1" in out and "short colour ok 0" in out, out
    raw = np.fromfile(tmp_path / "dump.bin", np.float64)
    low, low_feat, feat, c_out = np.split(raw, np.cumsum([wl * hl * 3, wl * hl * 8, w * h * 8]))
    assert len(c_out) == w * h * 3
    low, low_feat, feat = low.reshape(hl, wl, 3), low_feat.reshape(hl, wl, 8), feat.reshape(h, w, 8)
    assert (feat[..., 7] == 1).all() and set(np.unique(feat[..., 3:5])) == {0.0, 1.0} and low.max() > 1
    want = rt0.upsample(low, low_feat, feat, factor)
    assert c_out.tobytes() == want.tobytes() and same(want, ue.expected(low, low_feat, feat, factor))
