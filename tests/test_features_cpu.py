"""First-hit feature buffers: what can be checked without a GPU -- the single-channel PFM writer, the new command-line flags, the C declarations,
and the expectation builder of the GPU tests (tests/features_expect.py) against the oracle alone."""
import os
import re

import numpy as np
import pytest

import gi_raytracer_amd as gi
from gi_raytracer_amd import __main__ as cli

import features_expect as fe
import parity_checks as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_save_pfm_single_channel_round_trip(tmp_path):
    rs = np.random.RandomState(5)
    one = rs.rand(7, 5).astype(np.float32)
    three = rs.rand(7, 5, 3).astype(np.float32)
    gi.save_pfm(tmp_path / "one.pfm", one)
    gi.save_pfm(tmp_path / "one1.pfm", one[:, :, None])
    gi.save_pfm(tmp_path / "three.pfm", three)
    raw = open(tmp_path / "one.pfm", "rb").read()
    assert raw.startswith(b"Pf\n5 7\n-1.0\n") and len(raw) == len(b"Pf\n5 7\n-1.0\n") + 7 * 5 * 4
    assert raw[len(b"Pf\n5 7\n-1.0\n"):] == one[::-1].astype("<f4").tobytes()       # rows bottom to top
    assert open(tmp_path / "three.pfm", "rb").read().startswith(b"PF\n5 7\n-1.0\n")   # three channels as before
    assert fe.read_pfm(tmp_path / "one.pfm").tobytes() == one.tobytes()
    assert fe.read_pfm(tmp_path / "one1.pfm").tobytes() == one.tobytes()
    assert fe.read_pfm(tmp_path / "three.pfm").tobytes() == three.tobytes()
    with pytest.raises(ValueError):
        gi.save_pfm(tmp_path / "bad.pfm", np.zeros((4, 4, 2)))


def test_cli_feature_flags():
    a = cli.parser().parse_args(["s.scn"])
    assert a.features is None and a.feature_samples is None
    a = cli.parser().parse_args(["s.scn", "--features", "out/f", "--feature-samples", "12", "--width", "64", "--height", "48"])
    assert a.features == "out/f" and a.feature_samples == 12
    assert cli.feature_samples(a, 256) == 12
    # default: the frame's max_samples, cut to what the Halton index allows (4K: inc = 4096 * 2187, 2^32 / inc = 479.46)
    a = cli.parser().parse_args(["s.scn", "--features", "f", "--width", "3840", "--height", "2160"])
    assert gi.halton_sample_cap(3840, 2160) == 479 and gi.halton_sample_cap(1920, 1080) == 2 ** 32 // (2048 * 2187) == 958
    assert cli.feature_samples(a, 256) == 256 and cli.feature_samples(a, 1000) == 479
    assert cli.FEATURE_FILES == ("albedo", "normal", "depth", "coverage")


def test_header_declares_the_feature_entries_with_plain_c_types():
    txt = open(os.path.join(ROOT, "include/gi_hip.h")).read()
    code = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
    assert "int gi_render_features_device(gi_ctx*, const gi_render_params*, int32_t n_samples, void* d_out, int out_is_f64, int32_t* d_ids);" in code
    assert "int gi_render_features_host(gi_ctx*, const gi_render_params*, int32_t n_samples, void* h_out, int out_is_f64, int32_t* h_ids);" in code
    assert "int gi_last_features_ms(gi_ctx*, float* ms);" in code
    for name in ("gi_render_features_device", "gi_render_features_host", "gi_last_features_ms"):
        assert name in gi.ABI_SYMBOLS and hasattr(gi.lib(), name)


def test_frame_rows_of_a_rank():
    assert fe.frame_rows(40, 16, 0, 3) == list(range(0, 16))
    assert fe.frame_rows(40, 16, 2, 3) == list(range(32, 40))
    assert sorted(sum((fe.frame_rows(72, 16, r, 3) for r in range(3)), [])) == list(range(72))


def test_expectation_builder_on_the_oracle_alone():
    """The builder of the GPU tests on textures_opaque (checkerboard and image textures, flat and smooth triangles, binary cut-outs), small frame."""
    w, h, n = 24, 18, 3
    scene = pc.load_scene("textures_opaque")
    o, t = pc.oracle_for(scene), scene.tables()
    rays0, idx0 = fe.sample_rays(o, w, h, 0)
    assert fe.oracle_is_draw_free(o, rays0) and not fe.hit_depends_on_draw(o, rays0, trials=3)
    feat, ids, textured, vmax = fe.expected_features(o, t, w, h, n)
    one, ids1, _, _ = fe.expected_features(o, t, w, h, 1)
    assert np.array_equal(ids, ids1)
    # sample 0 alone: the oracle's own table, value for value
    hit, ent, res, _ = o.trace(rays0)
    hit = hit.astype(bool).reshape(h, w)
    assert hit.any()
    assert np.array_equal(one[:, :, 7], hit.astype(np.float64))
    assert np.array_equal(ids[:, :, 0], np.where(hit, ent.reshape(h, w), -1))
    assert np.array_equal(ids[:, :, 1][hit], t["tri_mat"][ent.reshape(h, w)[hit]])
    assert (ids[~hit] == -1).all() and (one[~hit] == 0).all()
    assert one[:, :, 3:6][hit].tobytes() == res.reshape(h, w, 8)[:, :, 3:6][hit].tobytes()
    d = res[:, :3] - rays0[:, :3]
    assert np.allclose(one[:, :, 6].reshape(-1), np.where(hit.reshape(-1), np.linalg.norm(d, axis=1), 0), rtol=1e-15, atol=0)
    # scalar recomputation of the sums for a few pixels, in sample order
    for (x, y) in ((0, 0), (w // 2, h // 2), (w - 1, h - 1), (5, 11)):
        acc = [0.0] * 8
        for s in range(n):
            _, ray = o.primary_ray(w, h, s, x, y)
            v = fe.sample_features(o, t, ray[None, :])
            if v[0][0]:
                for k in range(3):
                    acc[k] += float(v[3][0][k]); acc[3 + k] += float(v[4][0][k])
                acc[6] += float(v[5][0]); acc[7] += 1.0
        assert np.array([a / n for a in acc]).tobytes() == feat[y, x].tobytes()
    assert textured.any()                      # checkerboard / image look-ups are in view
    assert (feat[:, :, 7] >= 0).all() and (feat[:, :, 7] <= 1).all() and (vmax[:, :, 6] >= feat[:, :, 6]).all()
