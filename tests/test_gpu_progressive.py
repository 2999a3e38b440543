"""Progressive render sessions (gi_progressive_*, RayTracer.progressive / resume, --progressive): a frame built in steps has the bits of the
frame the one-shot RayTracer.run builds.  Every comparison is np.array_equal on the uint64 view of f64 frames and exact equality of the
samples-per-pixel buffers; the yardstick is always rt.run.  Shapes: caustics, 3000 photon indices (the gather runs), 21 x 19 pixels (partial
8x8 tiles at the right and bottom edges), 7 samples -- a few seconds per test."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import gi_raytracer_amd as gi

import host_build
import parity_checks as pc

pytestmark = pytest.mark.gpu

W, H, SPP = 21, 19, 7
THRESH = 0.0015            # the noise threshold of the adaptive parity tests (parity_checks.check_render)
ADAPTIVE = dict(min_samples=4, max_samples=24, noise_thresh=THRESH)
MODES = {"wavefront": 0, "rounds": 2}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def new_rt(scene="caustics", photons=3000):
    rt = gi.RayTracer(0).setScene(pc.load_scene(scene))
    if photons:
        rt.tracePhotons(photons)
    return rt


@pytest.fixture(scope="module")
def oneshot():
    """rt.run on a context of its own that never holds a session: oneshot(mode, **kw) -> (frame f64, spp), computed once per key."""
    rt = new_rt()
    cache = {}

    def get(mode="wavefront", w=W, h=H, **kw):
        key = (mode, w, h, tuple(sorted(kw.items())))
        if key not in cache:
            rt.set_render_mode(mode)
            cache[key] = rt.run(w, h, want_spp=True, **kw)
            rt.set_render_mode("wavefront")
        return cache[key]

    return get


@pytest.fixture(scope="module")
def rt():
    """The context the sessions of most tests run on (tests that change the scene or the environment make their own)."""
    return new_rt()


@pytest.mark.parametrize("steps", [[7], [1, 2, 4], [3, 4], [1] * 7, [5, 100]], ids=lambda s: "-".join(map(str, s)))
def test_every_partition_of_the_samples_gives_the_one_shot_frames(rt, oneshot, steps):
    with rt.progressive(W, H, min_samples=SPP, max_samples=SPP) as s:
        img, spp = s.frame(want_spp=True)
        assert (img == 0.5).all() and (spp == 0).all() and s.sample_end == 0 and not s.done and s.pixels_wanting == W * H
        k = 0
        for n in steps:
            k = min(k + n, SPP)
            img, spp = s.step(n, want_spp=True)
            ref, ref_spp = oneshot(min_samples=k, max_samples=k)
            assert same(img, ref) and np.array_equal(spp, ref_spp) and (spp == k).all() and s.sample_end == k, (steps, k)
        assert k == SPP and s.done and s.pixels_wanting == 0
        assert same(s.frame(), oneshot(min_samples=SPP, max_samples=SPP)[0])      # looking at the frame changes nothing
        assert same(s.step(3), oneshot(min_samples=SPP, max_samples=SPP)[0])       # nor does stepping past the end


def test_chunks_inside_a_step(monkeypatch, oneshot):
    """The per-sample radiance buffer holds two samples of the frame: a step of 5 runs in chunks of 2, 2, 1."""
    monkeypatch.setenv("GI_LBUF_MAX_BYTES", str(W * H * 24 * 2))
    rt2 = new_rt()                                   # the budget is read when the context is created
    with rt2.progressive(W, H, min_samples=SPP, max_samples=SPP) as s:
        assert same(s.step(5), oneshot(min_samples=5, max_samples=5)[0])
        img, spp = s.step(2, want_spp=True)
    ref, ref_spp = oneshot(min_samples=SPP, max_samples=SPP)
    assert same(img, ref) and np.array_equal(spp, ref_spp)


def test_stripes(rt, oneshot):
    kw = dict(stripe_h=5, rank=1, world=2, min_samples=SPP, max_samples=SPP)
    ref, ref_spp = oneshot(**kw)
    assert ref.shape == (9, W, 3)                     # rows 5 .. 9 and 15 .. 18
    with rt.progressive(W, H, **kw) as s:
        assert s.pixels_wanting == 9 * W
        s.step(3)
        img, spp = s.step(4, want_spp=True)
        assert same(img, ref) and np.array_equal(spp, ref_spp) and s.done


@pytest.mark.parametrize("mode", list(MODES))
def test_adaptive_sessions(oneshot, mode):
    """Rounds with the step's cap in place of max_samples: after cap k the frame and spp are those of rt.run(min_samples=4, max_samples=k)."""
    ref, ref_spp = oneshot(mode, **ADAPTIVE)
    assert len(np.unique(ref_spp)) >= 2, "the variance rule must stop some pixels early, or the test shows nothing"
    rt = new_rt()
    rt.set_render_mode(mode)
    with rt.progressive(W, H, **ADAPTIVE) as s:
        k = 0
        for n in (4, 4, 16):
            k += n
            img, spp = s.step(n, want_spp=True)
            want, want_spp = oneshot(mode, **dict(ADAPTIVE, max_samples=k))
            assert same(img, want) and np.array_equal(spp, want_spp) and s.sample_end == k, (mode, k)
            assert s.pixels_wanting == int((ref_spp > k).sum())          # exactly the pixels the one-shot frame gives more samples
        assert same(img, ref) and np.array_equal(spp, ref_spp) and s.done


def test_fixed_session_in_rounds_mode(oneshot):
    rt = new_rt()
    rt.set_render_mode("rounds")
    with rt.progressive(W, H, min_samples=SPP, max_samples=SPP) as s:
        img, spp = s.frame(want_spp=True)
        assert (img == 0.5).all() and (spp == 0).all() and s.pixels_wanting == W * H      # the padding records of the tiles are no pixels
        assert same(s.step(3), oneshot("rounds", min_samples=3, max_samples=3)[0])
        img, spp = s.step(4, want_spp=True)
    ref, ref_spp = oneshot("rounds", min_samples=SPP, max_samples=SPP)
    assert same(img, ref) and np.array_equal(spp, ref_spp)
    assert same(ref, oneshot(min_samples=SPP, max_samples=SPP)[0])


def test_f32_output_is_the_rounding_of_the_f64_output(rt):
    with rt.progressive(W, H, min_samples=SPP, max_samples=SPP) as s:
        a = s.step(3, f64=False)
        b = s.frame()
        assert a.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.astype(np.float32).view(np.uint32))
        a = s.step(4, f64=False)
        assert np.array_equal(a.view(np.uint32), s.frame().astype(np.float32).view(np.uint32))
    with rt.progressive(W, H, **ADAPTIVE) as s:      # the rounds write through another kernel
        a = s.step(8, f64=False)
        assert np.array_equal(a.view(np.uint32), s.frame().astype(np.float32).view(np.uint32))


def test_other_entries_between_steps_leave_the_session_alone(rt, oneshot):
    small = rt.run(16, 16, min_samples=2, max_samples=2)
    feat = rt.run_features(W, H, 2)
    den = rt.denoise(oneshot(min_samples=SPP, max_samples=SPP)[0], feat)
    for kw in (dict(min_samples=SPP, max_samples=SPP), ADAPTIVE):
        with rt.progressive(W, H, **kw) as s:
            s.step(3)
            assert same(rt.run(16, 16, min_samples=2, max_samples=2), small)
            assert same(rt.run(40, 30, min_samples=9, max_samples=9), oneshot(w=40, h=30, min_samples=9, max_samples=9)[0])   # a larger frame: every scratch buffer grows
            assert same(rt.run_features(W, H, 2)["features"], feat["features"])
            s.step(1)
            assert same(rt.denoise(oneshot(min_samples=SPP, max_samples=SPP)[0], feat), den)
            rt.set_pool_slots(4096)
            assert same(rt.run(W, H, **ADAPTIVE), oneshot(**ADAPTIVE)[0])
            img, spp = s.step(100, want_spp=True)
            rt.set_pool_slots(1 << 30)
            ref, ref_spp = oneshot(**kw)
            assert same(img, ref) and np.array_equal(spp, ref_spp) and s.done


@pytest.mark.parametrize("kw", [dict(min_samples=SPP, max_samples=SPP), ADAPTIVE], ids=["fixed", "adaptive"])
def test_a_cancelled_step_leaves_the_session_valid(rt, oneshot, kw):
    flag = C.c_int(1)
    with rt.progressive(W, H, **kw) as s:
        with pytest.raises(gi.GiError, match=r"\(-5\)"):
            s.step(2, cancel=flag)
        assert s.sample_end == 0
        s.step(3)
        with pytest.raises(gi.GiError, match=r"\(-5\)"):
            s.step(2, cancel=flag)
        assert s.sample_end == 3
        flag.value = 0
        s.step(2, cancel=flag)
        img, spp = s.step(100, want_spp=True)
        ref, ref_spp = oneshot(**kw)
        assert same(img, ref) and np.array_equal(spp, ref_spp) and s.done


def test_errors():
    L = gi.lib()
    out = np.zeros((H, W, 3))
    ptr = out.ctypes.data_as(C.c_void_p)
    empty = gi.RayTracer(0)
    p = empty.params(W, H, min_samples=SPP, max_samples=SPP)
    assert L.gi_progressive_begin(empty.h, C.byref(p)) == gi.GI_E_STATE                       # no scene
    rt = new_rt()
    assert L.gi_progressive_step_host(rt.h, 1, ptr, 1, None, None) == gi.GI_E_STATE          # no session
    assert L.gi_progressive_status(rt.h, None, None) == gi.GI_E_STATE
    rt.set_render_mode("megakernel")
    assert L.gi_progressive_begin(rt.h, C.byref(p)) == gi.GI_E_STATE                          # sessions run on the streaming passes
    rt.set_render_mode("wavefront")
    bad = rt.params(W, H, min_samples=SPP, max_samples=SPP, stripe_h=0)
    assert L.gi_progressive_begin(rt.h, C.byref(bad)) == gi.GI_E_INVALID
    s = rt.progressive(W, H, min_samples=SPP, max_samples=SPP)
    assert L.gi_progressive_step_host(rt.h, -1, ptr, 1, None, None) == gi.GI_E_INVALID
    assert L.gi_progressive_step_host(rt.h, 1, None, 1, None, None) == gi.GI_E_INVALID
    assert L.gi_progressive_step_device(rt.h, 1, None, 1, None, None) == gi.GI_E_INVALID
    assert s.sample_end == 0
    s.step(1)
    rt.tracePhotons(3000)                                                                      # a photon upload ends the session
    assert L.gi_progressive_step_host(rt.h, 1, ptr, 1, None, None) == gi.GI_E_STATE
    with pytest.raises(gi.GiError, match=r"\(-4\)"):
        s.step(1)
    s = rt.progressive(W, H, min_samples=SPP, max_samples=SPP)
    s.step(1)
    rt.tracePhotonsOnDevice(3000)
    assert L.gi_progressive_step_host(rt.h, 1, ptr, 1, None, None) == gi.GI_E_STATE
    s = rt.progressive(W, H, min_samples=SPP, max_samples=SPP)
    rt.setScene(pc.load_scene("caustics"))                                                     # so does a scene upload
    assert L.gi_progressive_step_host(rt.h, 1, ptr, 1, None, None) == gi.GI_E_STATE
    s = rt.progressive(W, H, min_samples=SPP, max_samples=SPP)
    s.close()
    with pytest.raises(gi.GiError, match=r"\(-4\)"):
        s.frame()


@pytest.mark.parametrize("kw", [dict(min_samples=SPP, max_samples=SPP), ADAPTIVE], ids=["fixed", "adaptive"])
def test_checkpoint_resumes_on_a_new_context(oneshot, kw):
    L = gi.lib()
    a = new_rt()
    s = a.progressive(W, H, **kw)
    s.step(3)
    blob = s.save()
    n = C.c_int64()
    assert L.gi_progressive_state_bytes(a.h, C.byref(n)) == 0 and n.value == len(blob)
    h = gi.parse_checkpoint_header(blob)
    assert h["sample_end"] == 3 and (h["width"], h["height"], h["max_samples"]) == (W, H, kw["max_samples"])
    assert h["schedule"] == (0 if kw["min_samples"] == kw["max_samples"] else 1) and h["n_records"] == (W * H if h["schedule"] == 0 else 3 * 3 * 64)
    del s, a                                                                                   # the context is destroyed
    b = new_rt()
    cut, magic, version = blob[:-1], b"X" + blob[1:], blob[:8] + struct.pack("<I", 2) + blob[12:]
    for wrong in (cut, magic, version, blob[:100], blob + b"\0"):
        assert L.gi_progressive_restore(b.h, wrong, len(wrong)) == gi.GI_E_INVALID
    others = (gi.RayTracer(0), new_rt("cornell", 0), new_rt(photons=0))                        # no scene; another scene; the scene without its photons
    for other in others:
        assert L.gi_progressive_restore(other.h, blob, len(blob)) == gi.GI_E_STATE
    b.set_render_mode("rounds")                                                                # the blob's schedule holds, not the context's mode
    with b.resume(blob) as s:
        assert s.sample_end == 3 and s.save() == blob
        assert same(s.frame(), oneshot(**dict(kw, **({"min_samples": 3} if h["schedule"] == 0 else {}), max_samples=3))[0])
        img, spp = s.step(4 if h["schedule"] == 0 else 21, want_spp=True)
        ref, ref_spp = oneshot(**kw)
        assert same(img, ref) and np.array_equal(spp, ref_spp) and s.done


def test_cli_progressive_writes_the_same_files(tmp_path, capsys):
    import gi_raytracer_amd.__main__ as cli
    scn = os.path.join(pc.ROOT, pc.SCN["caustics"])
    common = ["--width", str(W), "--height", str(H), "--samples", "6", "6", "--photons", "3000"]

    def run(name, *flags):
        d = tmp_path / name
        d.mkdir(exist_ok=True)
        assert cli.main([scn, "-o", str(d / "o.ppm"), "--pfm", str(d / "o.pfm")] + common + list(flags)) == 0
        return open(d / "o.ppm", "rb").read(), open(d / "o.pfm", "rb").read(), capsys.readouterr().out

    ppm, pfm, _ = run("plain")
    ppm2, pfm2, out = run("prog", "--progressive", "2")
    assert ppm2 == ppm and pfm2 == pfm and "3 step(s) of 2" in out and "finished" in out
    assert sorted(os.listdir(tmp_path / "prog")) == ["o.pfm", "o.ppm"]                       # no temporary file stays behind
    ck = str(tmp_path / "ck.bin")
    ppm3, pfm3, out = run("ck", "--progressive", "2", "--checkpoint", ck, "--time-limit", "0")
    assert "1 step(s) of 2" in out and "time limit reached" in out and gi.parse_checkpoint_header(open(ck, "rb").read())["sample_end"] == 2
    assert ppm3 != ppm                                                                        # 2 of the 6 samples
    ppm4, pfm4, out = run("ck", "--progressive", "2", "--checkpoint", ck)
    assert ppm4 == ppm and pfm4 == pfm and "2 step(s) of 2" in out and "resumed from" in out
    assert gi.parse_checkpoint_header(open(ck, "rb").read())["sample_end"] == 6


def test_cpp_caller_drives_a_session_through_the_c_abi(tmp_path):
    """tests/cpp/test_progressive.cpp: begin / step / status / save / restore / end from C++, compared there with gi_render_host and here with
    RayTracer.run on the same scene, photons and seed."""
    import subprocess
    exe = os.path.join(pc.ROOT, "tests", "cpp", "test_progressive")
    host_build.client("tests/cpp/test_progressive.cpp", exe, "-O1")
    dump = tmp_path / "frame.bin"
    r = subprocess.run([exe, os.path.join(pc.ROOT, pc.SCN["caustics"]), str(W), str(H), str(SPP), "3000", str(dump)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    for line in ("initial frame ok 1", "steps equal one-shot 1", "status end 7 wanting 0", "restored equal one-shot 1", "step without session -4", "negative step -2"):
        assert line in r.stdout, r.stdout
    rt = gi.RayTracer(0).setScene(pc.load_scene("caustics"))
    rt.tracePhotonsOnDevice(3000)
    assert same(np.fromfile(dump, np.float64).reshape(H, W, 3), rt.run(W, H, min_samples=SPP, max_samples=SPP))
