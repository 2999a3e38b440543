"""The a-trous denoiser: what can be checked without a GPU -- the properties of the expectation the GPU tests compare with
(tests/denoise_expect.py), the filter's quality on oracle-rendered frames, the new command-line flags and the C declarations."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gi_raytracer_amd as gi
from gi_raytracer_amd import __main__ as cli

import denoise_expect as de
import features_expect as fe
import parity_checks as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_zero_iterations_is_the_identity():
    noisy, feat, _ = de.synthetic(23, 17)
    assert de.expected(noisy, feat, iterations=0).tobytes() == noisy.tobytes()
    f32 = noisy.astype(np.float32)
    assert de.expected(f32, feat, np.float32, iterations=0).tobytes() == f32.tobytes()
    assert de.expected(f32, feat, np.float64, iterations=0).tobytes() == f32.astype(np.float64).tobytes()


@pytest.mark.parametrize("demodulate", [0, 1])
def test_a_colour_step_across_orthogonal_normals_survives_bit_for_bit(demodulate):
    h, w = 40, 48
    feat = np.zeros((h, w, 8))
    # one albedo, so the edge is in the normals alone; powers of two, so that colour / albedo * albedo is exact and w * c scales num by a power of two
    # (num / den is then exactly c on either side)
    feat[..., 0:3] = [0.5, 0.25, 1.0]
    feat[:, : w // 2, 3:6] = [0.0, 1.0, 0.0]
    feat[:, w // 2:, 3:6] = [1.0, 0.0, 0.0]     # |n_p - n_q|^2 = 2, inv_n = 4: d = 8, weight 0 across the edge
    feat[..., 6] = 5.0
    feat[..., 7] = 1.0
    color = np.zeros((h, w, 3))
    color[:, : w // 2] = 1.0
    out = de.expected(color, feat, sigma_color=0.0, demodulate=demodulate)
    assert out.tobytes() == color.tobytes()


def test_a_constant_frame_stays_within_the_rounding_bound():
    """Per level and pixel: 25 rounded products w c, two sums of at most 25 non-negative terms and one division: c' = c (1 + e), |e| <= 26 ulp
    (the weights cancel exactly in num / den but for these roundings)."""
    h, w = 45, 52
    _, feat, _ = de.synthetic(w, h)
    feat[..., 0:3] = [0.3, 0.6, 0.9]
    color = np.empty((h, w, 3))
    color[...] = [0.7, 0.123456789, 3.3]
    for demodulate in (0, 1):
        worst = 0.0
        for it in range(1, 6):
            out = de.expected(color, feat, iterations=it, demodulate=demodulate)
            err = float((np.abs(out - color) / color).max() / de.ULP)
            worst = max(worst, err / it)
            assert err <= 26 * it, (demodulate, it, err)
        print(f"constant frame, demodulate {demodulate}: at most {worst:.2f} ulp per level")


def test_non_finite_pixels_stay_local_and_the_output_is_finite():
    w, h, it = 70, 60, 2
    noisy, feat, _ = de.synthetic(w, h, seed=3)
    clean_out = de.expected(noisy, feat, iterations=it)
    bad = noisy.copy()
    spots = [(10, 12, np.nan), (40, 30, np.inf), (41, 30, -np.inf), (0, 0, np.nan), (h - 1, w - 1, np.inf)]
    for (y, x, v) in spots:
        bad[y, x, 1] = v
    out = de.expected(bad, feat, iterations=it)
    assert np.isfinite(out).all()
    reach = de.margin(it)
    far = np.ones((h, w), bool)
    for (y, x, _) in spots:
        far[max(0, y - reach):y + reach + 1, max(0, x - reach):x + reach + 1] = False
    assert far.any() and out[far].tobytes() == clean_out[far].tobytes()
    # a frame of nothing but NaN: every tap of every pixel is skipped
    assert not de.expected(np.full((9, 7, 3), np.nan), feat[:9, :7], iterations=3).any()


def test_the_crop_helper_equals_the_full_evaluation():
    w, h = 150, 140
    noisy, feat, _ = de.synthetic(w, h, seed=4)
    assert de.margin(5) == 62 and de.margin(1) == 2
    for it in (1, 3, 4):
        full = de.expected(noisy, feat, iterations=it)
        for (x0, y0, ww, wh) in ((0, 0, 20, 16), (w - 20, h - 16, 20, 16), (60, 55, 24, 24), (0, h - 10, 30, 10)):
            win = de.expected_window(noisy, feat, x0, y0, ww, wh, iterations=it)
            assert win.tobytes() == np.ascontiguousarray(full[y0:y0 + wh, x0:x0 + ww]).tobytes(), (it, x0, y0)


def test_the_filter_denoises_the_synthetic_frame():
    for noise in (1.0, 0.25):
        noisy, feat, clean = de.synthetic(96, 72, seed=7, noise=noise)
        out = de.expected(noisy, feat)
        a, b = de.rmse(noisy, clean), de.rmse(out, clean)
        print(f"synthetic, noise {noise}: rmse {a:.4f} -> {b:.4f}")
        assert b < a


@pytest.mark.parametrize("name", ["cornell", "textures_opaque"])
def test_quality_on_oracle_frames(name):
    """Oracle frame at 4 spp, oracle-built features (4 samples), target the oracle frame at 256 spp: the denoised frame must be closer to the
    target than the noisy one -- on textures_opaque also on the textured pixels alone."""
    w, h, spp = 96, 72, 4
    scene = pc.load_scene(name)
    o, t = pc.oracle_for(scene), scene.tables()
    o.build_photon_map()
    noisy = o.render(w, h, spp)["lin"]
    target = o.render(w, h, 256)["lin"]
    feat, _, textured, _ = fe.expected_features(o, t, w, h, spp)
    out = de.expected(noisy, feat)
    a, b = de.rmse(noisy, target), de.rmse(out, target)
    print(f"{name}: rmse against 256 spp: noisy {a:.5f}, denoised {b:.5f}, ratio {b / a:.3f}")
    assert np.isfinite(out).all() and b < a
    if name == "textures_opaque":
        assert textured.any()
        at, bt = de.rmse(noisy, target, textured), de.rmse(out, target, textured)
        print(f"{name}: on the {int(textured.sum())} textured pixels: noisy {at:.5f}, denoised {bt:.5f}, ratio {bt / at:.3f}")
        assert bt < at


def test_cli_denoise_flags():
    a = cli.parser().parse_args(["s.scn"])
    assert a.denoise is None and a.denoise_pfm is None and a.denoise_iterations is None and a.denoise_sigmas is None
    assert cli.denoise_kwargs(a) == {}
    a = cli.parser().parse_args(["s.scn", "--denoise", "d.ppm", "--denoise-pfm", "d.pfm", "--denoise-iterations", "3", "--denoise-sigmas", "1", "0.5", "0", "0.25"])
    assert a.denoise == "d.ppm" and a.denoise_pfm == "d.pfm"
    assert cli.denoise_kwargs(a) == dict(iterations=3, sigma_color=1.0, sigma_normal=0.5, sigma_depth=0.0, sigma_albedo=0.25)
    with pytest.raises(SystemExit):
        cli.parser().parse_args(["s.scn", "--denoise-sigmas", "1", "2"])
    with pytest.raises(SystemExit):
        cli.main(["s.scn", "--denoise-iterations", "3"])       # refused before anything is loaded: needs --denoise


def test_header_declares_the_denoise_entries_with_plain_c_types():
    txt = open(os.path.join(ROOT, "include/gi_hip.h")).read()
    code = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
    assert "void gi_denoise_default_params(gi_denoise_params*);" in code
    assert ("int gi_denoise_device(gi_ctx*, const gi_denoise_params*, const void* d_color, int color_is_f64, const void* d_features, int features_is_f64, "
            "void* d_out, int out_is_f64);") in code
    assert ("int gi_denoise_host(gi_ctx*, const gi_denoise_params*, const void* h_color, int color_is_f64, const void* h_features, int features_is_f64, "
            "void* h_out, int out_is_f64);") in code
    assert "int gi_last_denoise_ms(gi_ctx*, float* ms);" in code
    assert ("typedef struct gi_denoise_params { int32_t width, height; int32_t iterations; int32_t demodulate; "
            "double sigma_color, sigma_normal, sigma_depth, sigma_albedo; } gi_denoise_params;") in code
    for name in ("gi_denoise_default_params", "gi_denoise_device", "gi_denoise_host", "gi_last_denoise_ms"):
        assert name in gi.ABI_SYMBOLS and hasattr(gi.lib(), name)
    assert C.sizeof(gi.DenoiseParams) == 4 * 4 + 4 * 8
    # the defaults need no device: the library's and the expectation's agree
    p = gi.DenoiseParams()
    gi.lib().gi_denoise_default_params(C.byref(p))
    assert {k: getattr(p, k) for k in de.DEFAULTS} == de.DEFAULTS and (p.width, p.height) == (0, 0)
