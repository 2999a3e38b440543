"""The guided upsampler: what can be checked without a GPU -- the properties of the expectation the GPU tests compare with
(tests/upsample_expect.py), its quality against the two unguided ways of scaling a frame up, the new command-line flags, the C declarations and
the shape checks of the Python wrapper."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gi_raytracer_amd as gi
from gi_raytracer_amd import __main__ as cli

import denoise_expect as de
import upsample_expect as ue

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def flat_features(w, h, normal=(0.0, 1.0, 0.0), albedo=(0.5, 0.25, 1.0), depth=5.0):
    f = np.zeros((h, w, 8))
    f[..., 0:3], f[..., 3:6], f[..., 6], f[..., 7] = albedo, normal, depth, 1.0
    return f


@pytest.mark.parametrize("factor", [2, 3, 5])
def test_a_constant_colour_stays_within_the_rounding_bound(factor):
    """Per pixel: at most 16 rounded products w c, two sums of at most 16 non-negative terms (15 rounded additions each) and one division; the
    modulation is 1 without demodulate and that product is exact.  32 roundings of at most half an ulp each: out = c (1 + e), |e| <= 16 ulp to
    first order (the second-order term is below 1e-12 ulp).  The weights themselves cancel in num / den."""
    w, h = 50, 39
    _, feat, _ = de.synthetic(w, h)
    low_feat = ue.box_reduce(feat, factor)
    wl, hl = ue.low_size(w, h, factor)
    low = np.empty((hl, wl, 3))
    low[...] = [0.7, 0.123456789, 3.3]
    out = ue.expected(low, low_feat, feat, factor, demodulate=0)
    err = float((np.abs(out - low[0, 0]) / low[0, 0]).max() / de.ULP)
    print(f"constant colour, factor {factor}: at most {err:.2f} ulp")
    assert err <= 16.0 + 1e-6
    assert (out != low[0, 0]).any()          # not a test of nothing: some pixel did go through the weighted mean


@pytest.mark.parametrize("demodulate", [0, 1])
@pytest.mark.parametrize("factor", [2, 4])
def test_a_colour_step_across_orthogonal_normals_survives_bit_for_bit(factor, demodulate):
    h, w = 24, 48                            # the edge at x = 24: a low-pixel boundary for both factors
    # one albedo and one depth, so the edge is in the normals alone; powers of two, so that colour / albedo * albedo is exact and w * c scales num
    # by a power of two (num / den is then exactly c on either side)
    feat = flat_features(w, h)
    feat[:, w // 2:, 3:6] = [1.0, 0.0, 0.0]  # |n_p - n_q|^2 = 2, inv_n = 4: d = 8, weight 0 across the edge
    low_feat = ue.box_reduce(feat, factor)
    step = np.zeros((h, w, 3))
    step[:, : w // 2] = [1.0, 0.5, 0.25]
    low = ue.box_reduce(step, factor)
    assert set(np.unique(low_feat[..., 3])) == {0.0, 1.0}       # no low pixel straddles the edge
    out = ue.expected(low, low_feat, feat, factor, demodulate=demodulate)
    assert out.tobytes() == step.tobytes()


def test_a_pixel_whose_taps_are_all_rejected_takes_the_nearest_low_pixel():
    w, h, S = 21, 14, 3
    rs = np.random.RandomState(5)
    feat = flat_features(w, h, albedo=(0.3, 0.6, 0.9))
    low_feat = ue.box_reduce(feat, S)
    low = rs.uniform(0.1, 2.0, size=low_feat.shape[:2] + (3,))
    lonely = [(0, 0), (7, 10), (h - 1, w - 1)]
    for (y, x) in lonely:
        feat[y, x, 3:6] = [0.0, 0.0, 1.0]   # orthogonal to every low normal: d = 8 for all 16 taps
    for demodulate in (0, 1):
        out = ue.expected(low, low_feat, feat, S, demodulate=demodulate)
        c = low / de.modulation(low_feat, demodulate)
        for (y, x) in lonely:
            want = c[y // S, x // S] * de.modulation(feat, demodulate)[y, x]
            assert out[y, x].tobytes() == want.tobytes(), (demodulate, y, x)
        # and their neighbours are interpolated, not replicated
        assert (out[7, 11] != c[7 // S, 11 // S] * de.modulation(feat, demodulate)[7, 11]).any()


def test_a_non_finite_low_pixel_never_reaches_the_output():
    w, h, S = 40, 30, 2
    _, feat, clean = de.synthetic(w, h, seed=3, noise=0)
    low, low_feat = ue.box_reduce(clean, S), ue.box_reduce(feat, S)
    good = ue.expected(low, low_feat, feat, S)
    bad = low.copy()
    spots = [(3, 4, np.nan), (8, 9, np.inf), (8, 10, -np.inf), (0, 0, np.nan), (low.shape[0] - 1, low.shape[1] - 1, np.inf)]
    for (Y, X, v) in spots:
        bad[Y, X, 1] = v
    out = ue.expected(bad, low_feat, feat, S)
    assert np.isfinite(out).all()
    far = np.ones((h, w), bool)              # a full pixel's taps reach two low pixels to either side of its own
    for (Y, X, _) in spots:
        far[max(0, (Y - 2) * S):(Y + 3) * S, max(0, (X - 2) * S):(X + 3) * S] = False
    assert far.any() and (~far).any() and out[far].tobytes() == good[far].tobytes()
    # all taps rejected and the nearest low pixel not finite: 0 0 0
    feat[1, 1, 3:6] = [0.0, 0.0, 1.0]
    assert not ue.expected(bad, low_feat, feat, S)[1, 1].any()
    # a low frame of nothing but NaN
    assert not ue.expected(np.full_like(low, np.nan), low_feat, feat, S).any()


@pytest.mark.parametrize("w,h,factor", [(96, 72, 2), (96, 72, 3), (96, 72, 4), (128, 64, 8)])
def test_guided_upsampling_beats_replication_and_plain_interpolation(w, h, factor):
    """The clean synthetic frame, box-reduced: with the default parameters the upsampled frame must be closer to the full-size frame than
    nearest-pixel replication and than a plain tent interpolation of the same low frame.  A comparison, not a threshold."""
    _, feat, clean = de.synthetic(w, h, noise=0)
    low, low_feat = ue.box_reduce(clean, factor), ue.box_reduce(feat, factor)
    guided = de.rmse(ue.expected(low, low_feat, feat, factor), clean)
    replicated = de.rmse(ue.nearest(low, w, h, factor), clean)
    plain = de.rmse(ue.tent(low, w, h, factor), clean)
    print(f"{w}x{h} factor {factor}: rmse guided {guided:.5f}, nearest {replicated:.5f}, tent {plain:.5f}")
    assert guided < replicated and guided < plain


def test_the_tap_geometry():
    """Every full pixel's four tap columns hold the two low pixels it lies between, the tent weights of a row of taps add up to 2 away from the
    frame's edges (radius two low pixels), and the floor division holds below zero."""
    for S in range(2, 9):
        x = np.arange(0, 5 * S)
        Nx = 2 * x + 1 - S
        X0 = Nx // (2 * S)
        assert X0[0] == -1 and ((X0 == x // S) | (X0 == x // S - 1)).all()
        tx = [np.where(np.abs(2 * S * (X0 + i) - Nx) < 4 * S, (4 * S - np.abs(2 * S * (X0 + i) - Nx)) / (4.0 * S), 0.0) for i in range(-1, 3)]
        assert np.allclose(sum(tx), 2.0) and (tx[1] > 0.5).all() and (tx[2] > 0.5 - 1e-15).all()


def test_cli_upsample_flags(capsys):
    a = cli.parser().parse_args(["s.scn"])
    assert a.upsample is None and a.upsample_pfm is None
    a = cli.parser().parse_args(["s.scn", "--upsample", "4", "--upsample-pfm", "low.pfm", "--width", "640", "--height", "480"])
    assert a.upsample == 4 and a.upsample_pfm == "low.pfm"
    cli.check_args(cli.parser(), a)
    # refused before anything is loaded (the scene file does not exist)
    for bad in (["--upsample", "3", "--width", "640", "--height", "480"],            # 3 does not divide 640
                ["--upsample", "2", "--width", "640", "--height", "481"],
                ["--upsample", "1"], ["--upsample", "9", "--width", "720", "--height", "720"], ["--upsample", "0"],
                ["--upsample-pfm", "low.pfm"],
                ["--upsample", "2", "--progressive", "4"]):
        with pytest.raises(SystemExit) as e:
            cli.main(["s.scn"] + bad)
        assert e.value.code == 2, bad
        assert "upsample" in capsys.readouterr().err.split("error:")[-1], bad


def test_header_declares_the_upsample_entries_with_plain_c_types():
    txt = open(os.path.join(ROOT, "include/gi_hip.h")).read()
    code = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
    assert "void gi_upsample_default_params(gi_upsample_params*);" in code
    for where in ("device", "host"):
        d = where[0]
        assert (f"int gi_upsample_{where}(gi_ctx*, const gi_upsample_params*, const void* {d}_low_color, int low_color_is_f64, const void* {d}_low_features, "
                f"int low_features_is_f64, const void* {d}_features, int features_is_f64, void* {d}_out, int out_is_f64);") in code
    assert "int gi_last_upsample_ms(gi_ctx*, float* ms);" in code
    assert ("typedef struct gi_upsample_params { int32_t width, height; int32_t low_width, low_height; int32_t factor; int32_t demodulate; "
            "double sigma_normal, sigma_depth, sigma_albedo; } gi_upsample_params;") in code
    for name in ("gi_upsample_default_params", "gi_upsample_device", "gi_upsample_host", "gi_last_upsample_ms"):
        assert name in gi.ABI_SYMBOLS and hasattr(gi.lib(), name)
    assert C.sizeof(gi.UpsampleParams) == 6 * 4 + 3 * 8
    assert [f[0] for f in gi.UpsampleParams._fields_] == ["width", "height", "low_width", "low_height", "factor", "demodulate", "sigma_normal", "sigma_depth", "sigma_albedo"]
    # the defaults need no device: the library's and the expectation's agree
    p = gi.UpsampleParams()
    p.width = p.height = p.low_width = p.low_height = p.factor = 77
    gi.lib().gi_upsample_default_params(C.byref(p))
    assert {k: getattr(p, k) for k in ue.DEFAULTS} == ue.DEFAULTS and (p.width, p.height, p.low_width, p.low_height, p.factor) == (0, 0, 0, 0, 0)
    assert (ue.MIN_FACTOR, ue.MAX_FACTOR) == (gi.UPSAMPLE_FACTORS[0], gi.UPSAMPLE_FACTORS[-1])


def test_the_wrapper_checks_shapes_before_it_calls_the_library():
    lc, lf, ff = np.zeros((15, 19, 3)), np.zeros((15, 19, 8), np.float32), np.zeros((29, 37, 8))
    a, b, c = gi.upsample_arrays(lc, {"features": lf}, {"features": ff}, 2)
    assert a.shape == (15, 19, 3) and b.dtype == np.float32 and c.dtype == np.float64
    assert gi.upsample_arrays(lc.astype(np.float16), lf, ff, 2)[0].dtype == np.float64
    for args in ((lc[:, :18], lf[:, :18], ff, 2),            # floor(37 / 2), not the ceiling
                 (lc, lf, ff, 3), (lc, lf[:14], ff, 2), (lc[..., :2], lf, ff, 2), (lc, lf, ff[..., :7], 2), (lc, lf, ff[0], 2),
                 (lc, lf, ff, 1), (lc, lf, ff, 9), (lc, lf, np.zeros((0, 37, 8)), 2)):
        with pytest.raises(ValueError):
            gi.upsample_arrays(*args)
    assert gi.low_frame_size(640, 480, 2) == (320, 240) and gi.low_frame_size(64, 32, 8) == (8, 4)
    for args in ((640, 480, 3), (641, 480, 2), (640, 480, 1), (640, 480, 9), (0, 480, 2)):
        with pytest.raises(ValueError):
            gi.low_frame_size(*args)
