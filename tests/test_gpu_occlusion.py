"""The ambient-occlusion / bent-normal pass (gi_render_occlusion_*, k_ao) on the GPU, through the C ABI via the Python mirror.

The expectation comes from the oracle as it is (tests/occlusion_expect.py).  What is exact and what has an allowance:
 * first hits (ids, coverage) are identical, as the feature pass's are;
 * the open COUNT of every (pixel, sample) is compared: the device's hemisphere sampler and the oracle's are 4 ulp apart at the most, so a segment
   that grazes an edge may flip -- at most 1 segment in 1 000 may differ (tests/test_occlusion_cpu.py shows on the CPU that on these frames a 4-ulp
   move of T_j flips none, so none is expected; the count is printed);
 * in pixels whose counts all agree, openness is equal to 1e-15 and the bent vector within 1e-12 absolute (sums of at most 8 unit vectors 4 ulp apart);
 * the analytic frames and every identity (stripes, f32, walk variants, repetition) are exact, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import gi_raytracer_amd as gi

import features_expect as fe
import occlusion_expect as oe
import parity_checks as pc

pytestmark = pytest.mark.gpu

W, H = 24, 16
SIZES = ((13, 9), (24, 16))         # 13 x 9: no multiple of the 8 x 8 tile and less than one workgroup
N, DIRS = 2, 8


@pytest.fixture(scope="module")
def setups():
    cache = {}

    def get(name):
        if name not in cache:
            scene = {"floor": lambda: oe.floor_scene(gi), "box": lambda: oe.closed_box_scene(gi)}.get(name, lambda: pc.named_scene(name))()
            cache[name] = (scene, gi.RayTracer(0).setScene(scene), pc.oracle_for(scene), scene.tables())
        return cache[name]

    return get


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# ---------------------------------------------------------------------------------------------------------------- 1. oracle parity
@pytest.mark.parametrize("name", ["cornell", "spheres_opaque", "test_scene"])
def test_counts_and_values_match_the_oracle(setups, name):
    scene, rt, o, t = setups(name)
    assert name in fe.DRAW_FREE_SCENES and fe.oracle_is_draw_free(o, fe.sample_rays(o, W, H, 0)[0])
    geo = [oe.sample_geometry(o, W, H, s, DIRS) for s in range(N)]
    # first hits: entity of sample 0 and the number of hits over both samples, as the feature pass reports them
    f1, f2 = rt.run_features(W, H, 1), rt.run_features(W, H, N)
    assert np.array_equal(f1["ids"][:, :, 0], geo[0]["ent"].reshape(H, W))
    assert np.array_equal(f2["coverage"] * N, sum(g["hit"].reshape(H, W).astype(np.float64) for g in geo))
    differ = asked = 0
    for radius in (oe.default_radius(t), 2.0 * oe.scene_diagonal(t)):
        want = oe.expected_occlusion(o, W, H, N, DIRS, radius, geometry=geo)
        got1 = rt.run_occlusion(W, H, n=1, dirs=DIRS, radius=radius)
        got = rt.run_occlusion(W, H, n=N, dirs=DIRS, radius=radius)
        assert got["occlusion"].shape == (H, W, 4) and got["occlusion"].dtype == np.float64
        assert same(got["open"], got["occlusion"][:, :, 0]) and same(got["bent"], got["occlusion"][:, :, 1:4])
        # counts per (pixel, sample): open_s = count / 8 and the mean of two such numbers are exact in binary
        c0 = got1["open"] * DIRS
        c01 = got["open"] * (DIRS * N)
        assert (c0 == np.round(c0)).all() and (c01 == np.round(c01)).all()
        counts = np.array([c0, c01 - c0]).astype(np.int64)
        d = int(np.abs(counts - want["counts"]).sum())
        n_seg = int(want["hit"].sum()) * DIRS
        print(f"{name} radius {radius:.4f}: {d} of {n_seg} segments differ from the oracle's")
        differ += d; asked += n_seg
        agree = (counts == want["counts"]).all(0)
        e_open = np.abs(got["open"] - want["occlusion"][:, :, 0])[agree]
        e_bent = np.abs(got["bent"] - want["occlusion"][:, :, 1:4])[agree]
        print(f"   pixels in agreement {int(agree.sum())} of {H * W}: openness differs by at most {e_open.max():.3e}, bent by at most {e_bent.max():.3e}")
        assert (e_open <= 1e-15).all() and (e_bent <= 1e-12).all()
        miss = ~want["hit"].any(0)
        assert (got["open"][miss] == 1.0).all() and (got["bent"][miss] == 0.0).all()
    assert asked > 1000 and differ * 1000 <= asked, (differ, asked)
    if name == "cornell":       # radius 0 stands for a tenth of the root box's diagonal
        assert same(rt.run_occlusion(W, H, n=N, dirs=DIRS, radius=0.0)["occlusion"], rt.run_occlusion(W, H, n=N, dirs=DIRS, radius=oe.default_radius(t))["occlusion"])


# ---------------------------------------------------------------------------------------------------------------- 2. analytic frames
def test_floor_seen_from_above_is_fully_open(setups):
    scene, rt, o, t = setups("floor")
    got = rt.run_occlusion(W, H, n=N, dirs=DIRS, radius=3.0)
    cov = rt.run_features(W, H, N, want_ids=False)["coverage"]
    assert (got["open"] == 1.0).all()
    assert (cov == 1).any() and (got["bent"][:, :, 1][cov == 1] > 0).all()             # dot(bent, (0, 1, 0)) > 0 wherever every sample hits
    assert (got["bent"][cov == 0] == 0).all()


def test_inside_a_closed_box_nothing_is_open(setups):
    scene, rt, o, t = setups("box")
    assert (rt.run_features(W, H, N, want_ids=False)["coverage"] == 1).all()
    for radius in (oe.BOX_DIAGONAL, 2.5 * oe.BOX_DIAGONAL):
        assert not rt.run_occlusion(W, H, n=N, dirs=DIRS, radius=radius)["occlusion"].any()


def test_openness_falls_as_the_radius_grows(setups):
    scene, rt, o, t = setups("cornell")
    D = oe.scene_diagonal(t)
    prev = None
    for radius in (0.02 * D, 0.1 * D, 0.4 * D, 2.0 * D):
        cur = rt.run_occlusion(W, H, n=N, dirs=DIRS, radius=radius)["open"]
        assert prev is None or (prev >= cur).all()
        prev = cur
    assert 0 < prev.mean() < 1


# ---------------------------------------------------------------------------------------------------------------- 3. identities, bit for bit
@pytest.mark.parametrize("name", ["cornell", "spheres", "textures"])       # draw-free; stochastic alpha on spheres; alpha from textures
def test_identities_bit_for_bit(setups, name):
    scene, rt, o, t = setups(name)
    radius = oe.default_radius(t)
    for (w, h) in SIZES:
        kw = dict(n=N, dirs=DIRS, radius=radius)
        full = rt.run_occlusion(w, h, **kw)["occlusion"]
        assert np.isfinite(full).all() and (full[:, :, 0] >= 0).all() and (full[:, :, 0] <= 1).all()
        assert same(rt.run_occlusion(w, h, **kw)["occlusion"], full)                                      # a repeated call
        f32 = rt.run_occlusion(w, h, f64=False, **kw)["occlusion"]
        assert f32.dtype == np.float32 and same(f32, full.astype(np.float32))
        for world in (2, 3):
            frame = np.full_like(full, -7.0)
            for rank in range(world):
                part = rt.run_occlusion(w, h, stripe_h=4, rank=rank, world=world, **kw)["occlusion"]
                rows = fe.frame_rows(h, 4, rank, world)
                assert part.shape == (len(rows), w, 4)
                frame[rows] = part
            assert same(frame, full), (name, w, h, world)
        for switch in (rt.set_wide_nodes, rt.set_entity_boxes, rt.set_content_culling):
            try:
                switch(False)
                off = rt.run_occlusion(w, h, **kw)["occlusion"]
            finally:
                switch(True)
            assert same(off, full), (name, w, h, switch.__name__)
    w, h = SIZES[0]
    for dirs in (1, 64):
        a = rt.run_occlusion(w, h, n=1, dirs=dirs, radius=radius)["occlusion"]
        assert same(rt.run_occlusion(w, h, n=1, dirs=dirs, radius=radius)["occlusion"], a)
        c = a[:, :, 0] * dirs
        assert (c == np.round(c)).all() and (c >= 0).all() and (c <= dirs).all()
        try:
            rt.set_wide_nodes(False)
            assert same(rt.run_occlusion(w, h, n=1, dirs=dirs, radius=radius)["occlusion"], a)
        finally:
            rt.set_wide_nodes(True)


def test_seed_moves_the_alpha_tested_result_and_no_opaque_first_hit(setups):
    scene, rt, o, t = setups("spheres")
    r = oe.default_radius(t)
    a = rt.run_occlusion(W, H, n=N, dirs=DIRS, radius=r)["occlusion"]
    assert not same(rt.run_occlusion(W, H, n=N, dirs=DIRS, radius=r, seed=12345)["occlusion"], a)
    scene, rt, o, t = setups("cornell")
    r = 2.0 * oe.scene_diagonal(t)
    a = rt.run_occlusion(W, H, n=N, dirs=DIRS, radius=r)
    b = rt.run_occlusion(W, H, n=N, dirs=DIRS, radius=r, seed=12345)
    assert not same(a["occlusion"], b["occlusion"])                                      # other directions ...
    cov = rt.run_features(W, H, N, want_ids=False)["coverage"]
    assert same(cov, rt.run_features(W, H, N, want_ids=False, seed=12345)["coverage"])   # ... from the same first hits:
    for g in (a, b):                                                                     # a pixel is open with no bent vector exactly where no sample hits
        assert np.array_equal((g["open"] == 1.0) & (g["bent"] == 0.0).all(2), cov == 0)


# ---------------------------------------------------------------------------------------------------------------- 4. leaves things alone
def test_the_frame_the_timers_and_a_session_are_left_alone(setups):
    scene = pc.load_scene("caustics")
    rt = gi.RayTracer(0).setScene(scene)
    rt.tracePhotonsOnDevice(3000)
    kw = dict(min_samples=6, max_samples=6)
    before = rt.run(48, 32, **kw)
    feat = rt.run_features(48, 32, 2)
    k_before, ms_before, f_before = rt.last_kernel_ms(), rt.last_render_ms(), rt.last_features_ms()
    assert k_before["trace"] > 0 and f_before > 0 and rt.last_occlusion_ms() == 0.0
    ao = rt.run_occlusion(48, 32, n=N, dirs=DIRS)["occlusion"]
    assert rt.last_occlusion_ms() > 0
    assert rt.last_kernel_ms() == k_before and rt.last_render_ms() == ms_before and rt.last_features_ms() == f_before
    assert same(rt.run(48, 32, **kw), before)
    assert same(rt.run_features(48, 32, 2)["features"], feat["features"])
    assert same(rt.run_occlusion(48, 32, n=N, dirs=DIRS)["occlusion"], ao)
    # a progressive session steps on to the same frame with the pass in between
    with rt.progressive(48, 32, **kw) as sess:
        sess.step(2)
        end = sess.sample_end
        assert same(rt.run_occlusion(48, 32, n=N, dirs=DIRS)["occlusion"], ao)
        assert sess.sample_end == end
        assert same(sess.step(4), before)
    # a refused call has no time
    with pytest.raises(gi.GiError):
        p = rt.params(48, 32)
        rt._check(rt.L.gi_render_occlusion_host(rt.h, C.byref(p), C.byref(gi.OcclusionParams(1, 0, 0.0)), np.zeros((32, 48, 4)).ctypes.data_as(C.c_void_p), 1), "render_occlusion_host")
    assert rt.last_occlusion_ms() == 0.0


def test_device_entry_writes_what_the_host_entry_returns(setups):
    scene, rt, o, t = setups("cornell")
    p = rt.params(W, H)
    op = rt.occlusion_params(n=N, dirs=DIRS, radius=oe.default_radius(t))
    hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")      # device buffers from the HIP runtime the library itself uses (no second runtime in this process)
    for f64 in (False, True):
        fill = np.full((H, W, 4), -7.0, np.float64 if f64 else np.float32)
        d = C.c_void_p()
        assert hip.hipMalloc(C.byref(d), C.c_size_t(fill.nbytes)) == 0
        try:
            assert hip.hipMemcpy(d, fill.ctypes.data_as(C.c_void_p), C.c_size_t(fill.nbytes), 1) == 0      # hipMemcpyHostToDevice
            rt.run_occlusion_device(p, op, d.value, f64=f64)
            assert rt.last_occlusion_ms() > 0                                          # waits for the pass
            got = np.zeros_like(fill)
            assert hip.hipDeviceSynchronize() == 0
            assert hip.hipMemcpy(got.ctypes.data_as(C.c_void_p), d, C.c_size_t(got.nbytes), 2) == 0        # hipMemcpyDeviceToHost
        finally:
            assert hip.hipFree(d) == 0
        assert same(got, rt.run_occlusion(W, H, n=N, dirs=DIRS, radius=op.radius, f64=f64)["occlusion"])


# ---------------------------------------------------------------------------------------------------------------- 5. errors
def test_bad_arguments_and_missing_scene_leave_the_output_alone(setups):
    scene, rt, o, t = setups("cornell")
    L = rt.L
    p = rt.params(W, H)
    out = np.full((H, W, 4), -7.0)
    ptr = out.ctypes.data_as(C.c_void_p)
    P = gi.OcclusionParams
    for bad in (P(0, 8, 1.0), P(-3, 8, 1.0), P(1, 0, 1.0), P(1, 65, 1.0), P(1, -1, 1.0), P(1, 8, -1e-9), P(1, 8, float("nan")), P(1, 8, float("inf"))):
        assert L.gi_render_occlusion_host(rt.h, C.byref(p), C.byref(bad), ptr, 1) == gi.GI_E_INVALID, (bad.n_samples, bad.n_dirs, bad.radius)
        assert b"render_occlusion" in L.gi_last_error(rt.h)
        assert L.gi_render_occlusion_device(rt.h, C.byref(p), C.byref(bad), C.c_void_p(16), 1) == gi.GI_E_INVALID      # refused before the pointer is used
    ok = P(1, 8, 1.0)
    assert L.gi_render_occlusion_host(rt.h, C.byref(p), C.byref(ok), None, 1) == gi.GI_E_INVALID
    assert L.gi_render_occlusion_host(rt.h, C.byref(p), None, ptr, 1) == gi.GI_E_INVALID
    assert L.gi_render_occlusion_host(rt.h, None, C.byref(ok), ptr, 1) == gi.GI_E_INVALID
    assert L.gi_render_occlusion_host(None, C.byref(p), C.byref(ok), ptr, 1) == gi.GI_E_INVALID
    assert L.gi_render_occlusion_device(rt.h, C.byref(p), C.byref(ok), None, 1) == gi.GI_E_INVALID
    assert L.gi_last_occlusion_ms(rt.h, None) == gi.GI_E_INVALID
    bad_frame = rt.params(0, 10)
    assert L.gi_render_occlusion_host(rt.h, C.byref(bad_frame), C.byref(ok), ptr, 1) == gi.GI_E_INVALID
    # the Halton index: a 3840 x 2160 frame takes 479 samples
    big = rt.params(3840, 2160, stripe_h=8, rank=0, world=270)      # one stripe of 8 rows
    assert rt.local_rows(big) == 8 and gi.halton_sample_cap(3840, 2160) == 479
    out_big = np.full((8, 3840, 4), -7.0, np.float32)
    assert L.gi_render_occlusion_host(rt.h, C.byref(big), C.byref(P(480, 1, 1.0)), out_big.ctypes.data_as(C.c_void_p), 0) == gi.GI_E_INVALID
    assert b"480" in L.gi_last_error(rt.h) and b"479" in L.gi_last_error(rt.h)
    with pytest.raises(ValueError):
        rt.run_occlusion(3840, 2160, n=480)
    for kw in (dict(n=0), dict(dirs=65), dict(radius=-1.0)):
        with pytest.raises(ValueError):
            rt.run_occlusion(W, H, **kw)
    empty = gi.RayTracer(0)
    small = empty.params(W, H)
    assert L.gi_render_occlusion_host(empty.h, C.byref(small), C.byref(ok), ptr, 1) == gi.GI_E_STATE
    assert L.gi_render_occlusion_device(empty.h, C.byref(small), C.byref(ok), C.c_void_p(16), 1) == gi.GI_E_STATE
    assert (out == -7.0).all() and (out_big == -7.0).all()
    assert L.gi_render_occlusion_host(rt.h, C.byref(p), C.byref(ok), ptr, 1) == gi.GI_OK and (out != -7.0).all()      # and the buffer is the one a good call fills


def test_cli_writes_the_two_files(setups, tmp_path, capsys):
    import os
    from gi_raytracer_amd import __main__ as cli
    scn = os.path.join(pc.ROOT, pc.SCN["cornell"])
    assert cli.main([scn, "-o", str(tmp_path / "out.ppm"), "--width", "24", "--height", "16", "--samples", "1", "--photons", "0",
                     "--occlusion", str(tmp_path / "ao"), "--occlusion-samples", "2", "--occlusion-dirs", "8", "--occlusion-radius", "1.5"]) == 0
    assert sorted(os.listdir(tmp_path)) == ["ao.bent.pfm", "ao.open.pfm", "out.ppm"]
    assert "occlusion" in capsys.readouterr().out
    scene, rt, o, t = setups("cornell")
    want = rt.run_occlusion(24, 16, n=2, dirs=8, radius=1.5, f64=False)
    op, bent = fe.read_pfm(tmp_path / "ao.open.pfm"), fe.read_pfm(tmp_path / "ao.bent.pfm")
    assert op.shape == (16, 24) and same(np.ascontiguousarray(op), np.ascontiguousarray(want["open"]))
    assert bent.shape == (16, 24, 3) and same(np.ascontiguousarray(bent), np.ascontiguousarray(want["bent"]))
    assert open(tmp_path / "ao.open.pfm", "rb").read(2) == b"Pf" and open(tmp_path / "ao.bent.pfm", "rb").read(2) == b"PF"
