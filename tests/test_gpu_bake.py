"""Light baking (gi_bake_*, k_bake_gen / k_bake_fold around the stream passes) on the GPU, through the C ABI via the Python mirror.

The expectation is tests/bake_expect.py.  What is exact and what has an allowance:
 * stream indices and ray origins are the statement's bit for bit; directions within the 4 ulp parity_checks.check_kats grants the samplers
   (device OCML against host libm);
 * the fold kernel on caller data is bit-equal to the numpy fold;
 * a whole bake is compared with the numpy fold of Oracle.radiance on the DEVICE's rays (so that no edge-grazing ray lands on another entity): RMSE
   below parity_checks.RMSE_TOL, printed;
 * every identity (chunks, ranges, splitting, f32, frames and sessions left alone) is exact, bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

import gi_raytracer_amd as gi

import bake_expect as be
import parity_checks as pc

pytestmark = pytest.mark.gpu

COUNTS = (16, 5)                    # 5: no power of 2 or 3
SEEDS = (be.DEFAULT_SEED, 12345)
BASE = 1000
ULP4 = 4 * 2.0 ** -52               # of unit vectors


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.fixture(scope="module")
def setups(golden):
    cache = {}

    def get(name):
        if name not in cache:
            scene = pc.load_scene(name)
            rt = gi.RayTracer(0).setScene(scene)
            o = pc.oracle_for(scene)
            if name == "caustics":
                ph = golden("scene_caustics")["photons"]
                scene.build_photon_map(ph)
                rt.upload_photon_map()
                o.set_photons(ph)
            o.build_photon_map()
            P, N = be.surface_points(o)
            assert len(P) >= 12
            cache[name] = {"scene": scene, "rt": rt, "o": o, "P": P, "N": N, "probes": be.probe_points(scene.tables())}
        return cache[name]

    return get


def bake(rt, s, mode, ns, **kw):
    return rt.bake_texels(s["P"], s["N"], ns, **kw) if mode == be.TEXEL else rt.bake_probes(s["probes"], ns, **kw)


def device_rays(rt, s, mode, ns, **kw):
    return rt.bake_rays(s["P"], s["N"], ns, **kw) if mode == be.TEXEL else rt.bake_rays(s["probes"], None, ns, **kw)


# ---------------------------------------------------------------------------------------------------------------- 1. rays
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("mode", [be.TEXEL, be.SH9])
def test_rays_are_the_statement(setups, mode, seed):
    s = setups("cornell")
    rt = s["rt"]
    for ns in COUNTS:
        for base in (0, BASE):
            rays, st = device_rays(rt, s, mode, ns, stream_base=base, seed=seed)
            want, wst = be.texel_rays(s["P"], s["N"], ns, base) if mode == be.TEXEL else be.probe_rays(s["probes"], ns, base)
            assert st.dtype == np.uint32 and np.array_equal(st, wst)
            assert same(rays[:, 0:3], want[:, 0:3])
            err = np.abs(rays[:, 3:6] - want[:, 3:6]).max()
            print(f"mode {mode} n {ns} base {base}: directions differ by at most {err:.3e} ({int((rays[:, 3:6] == want[:, 3:6]).all(1).sum())} of {len(rays)} bit-equal)")
            assert err <= ULP4


# ---------------------------------------------------------------------------------------------------------------- 2. fold
@pytest.mark.parametrize("ns", [1, 5, 64])
@pytest.mark.parametrize("mode", [be.TEXEL, be.SH9])
def test_fold_kernel_is_the_numpy_fold_bit_for_bit(setups, mode, ns):
    rt = setups("cornell")["rt"]
    rs = np.random.RandomState(100 * mode + ns)
    n = 70                                                                  # more than a wave, no multiple of one
    d = rs.standard_normal((n, ns, 3))
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    L = rs.standard_normal((n, ns, 3)) * 10.0 ** rs.randint(-12, 9, (n, ns, 1))     # mixed sign and magnitude
    L[rs.rand(n, ns) < 0.1] = 0.0
    got = rt.bake_fold(mode, L, d)
    assert same(got, be.fold(mode, L, d))
    if mode == be.TEXEL:
        assert same(rt.bake_fold(mode, L), got)                                      # directions play no part


# ---------------------------------------------------------------------------------------------------------------- 3. the whole bake
@pytest.mark.parametrize("mode", [be.TEXEL, be.SH9])
@pytest.mark.parametrize("name", ["cornell", "caustics"])
def test_bake_is_the_fold_of_the_oracles_radiance(setups, name, mode):
    s = setups(name)
    rt = s["rt"]
    for ns, base, seed in ((16, 0, SEEDS[0]), (5, BASE, SEEDS[1])):
        rays, st = device_rays(rt, s, mode, ns, stream_base=base, seed=seed)
        want = be.expected_bake(s["o"], mode, rays, st, ns, seed)
        got = bake(rt, s, mode, ns, stream_base=base, seed=seed)
        assert got.shape == want.shape and got.dtype == np.float64
        rmse = float(np.sqrt(((got - want) ** 2).mean()))
        print(f"{name} mode {mode} n {ns}: rmse {rmse:.3e}, mean |want| {np.abs(want).mean():.4f}, {int((got == want).all(-1).sum())} of {want[..., 0].size} rows bit-equal")
        assert np.abs(want).max() > 0 and rmse < pc.RMSE_TOL
        # the device's own function-level path tracer on the same rays states it too
        L = rt.radiance(rays, st, seed).reshape(-1, ns, 3)
        again = be.fold(mode, L, rays[:, 3:6].reshape(-1, ns, 3))
        assert float(np.sqrt(((got - again) ** 2).mean())) < pc.RMSE_TOL


# ---------------------------------------------------------------------------------------------------------------- 4. chunks and ranges cannot show
@pytest.mark.parametrize("mode", [be.TEXEL, be.SH9])
def test_chunks_of_points_and_ranges_of_samples_leave_no_trace(setups, mode):
    s = setups("caustics")
    rt = s["rt"]
    key = "P" if mode == be.TEXEL else "probes"
    reps = -(-150 // len(s[key]))                                # the test points over again: other stream indices, so other samples
    many = {"P": np.tile(s["P"], (reps, 1)), "N": np.tile(s["N"], (reps, 1)), "probes": np.tile(s["probes"], (reps, 1))}
    few = {"P": s["P"][:3], "N": s["N"][:3], "probes": s["probes"][:3]}
    assert len(many[key]) > 128 and len(many[key]) % 64
    whole_many, whole_few = bake(rt, many, mode, 5), bake(rt, few, mode, 100)
    try:
        rt.set_pool_slots(64)                                    # the smallest value: three chunks of points, the last a part of one; one sample a range
        assert same(bake(rt, many, mode, 5), whole_many)
        assert same(bake(rt, few, mode, 100), whole_few)         # 64 < 100: ranges of 21 samples, the last of 16
    finally:
        rt.set_pool_slots(1 << 30)
    assert same(bake(rt, few, mode, 100), whole_few)


# ---------------------------------------------------------------------------------------------------------------- 5. splitting the point list
@pytest.mark.parametrize("mode", [be.TEXEL, be.SH9])
def test_a_part_of_the_points_with_its_stream_base_is_those_rows_of_the_whole(setups, mode):
    s = setups("caustics")
    rt = s["rt"]
    ns = 5
    whole = bake(rt, s, mode, ns, stream_base=BASE)
    n = len(whole)
    for a, b in ((0, 2), (2, n - 1), (n - 1, n)):
        part = {"P": s["P"][a:b], "N": s["N"][a:b], "probes": s["probes"][a:b]}
        assert same(bake(rt, part, mode, ns, stream_base=BASE + a * ns), whole[a:b])


# ---------------------------------------------------------------------------------------------------------------- 6. frames and sessions are left alone
def test_frames_timers_and_a_session_are_untouched(setups):
    s = setups("caustics")
    rt = s["rt"]
    kw = dict(min_samples=6, max_samples=6)
    before = rt.run(48, 32, **kw)
    k_before, ms_before = rt.last_kernel_ms(), rt.last_render_ms()
    assert k_before["trace"] > 0
    probes = bake(rt, s, be.SH9, 16)
    assert rt.last_bake_ms() > 0
    assert rt.last_kernel_ms() == k_before and rt.last_render_ms() == ms_before
    texels = bake(rt, s, be.TEXEL, 16)
    assert same(rt.run(48, 32, **kw), before)
    assert same(bake(rt, s, be.SH9, 16), probes) and same(bake(rt, s, be.TEXEL, 16), texels)
    for mode in ("rounds", "megakernel"):                        # the render mode plays no part
        try:
            rt.set_render_mode(mode)
            assert same(bake(rt, s, be.SH9, 16), probes)
        finally:
            rt.set_render_mode("wavefront")
    try:                                                         # nor does the lens
        rt.set_lens(0.35, 5, 0.3)
        assert same(bake(rt, s, be.TEXEL, 16), texels)
    finally:
        rt.set_lens(0.0)
    with rt.progressive(48, 32, **kw) as sess:                   # step, bake, step has the bits of step, step
        sess.step(2)
        end = sess.sample_end
        assert same(bake(rt, s, be.SH9, 16), probes)
        assert sess.sample_end == end
        assert same(sess.step(4), before)


# ---------------------------------------------------------------------------------------------------------------- 7. f32
@pytest.mark.parametrize("mode", [be.TEXEL, be.SH9])
def test_f32_output_is_the_f64_output_rounded_once(setups, mode):
    s = setups("caustics")
    full = bake(s["rt"], s, mode, 5)
    f32 = bake(s["rt"], s, mode, 5, f64=False)
    assert f32.dtype == np.float32 and same(f32, full.astype(np.float32))


def test_device_entry_writes_what_the_host_entry_returns(setups):
    s = setups("cornell")
    rt = s["rt"]
    hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")      # device buffers from the HIP runtime the library itself uses (no second runtime in this process)
    rows = np.ascontiguousarray(np.concatenate([s["P"], s["N"]], 1))
    fill = np.full((len(rows), 3), -7.0)
    d_p, d_o = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d_p), C.c_size_t(rows.nbytes)) == 0 and hip.hipMalloc(C.byref(d_o), C.c_size_t(fill.nbytes)) == 0
    try:
        assert hip.hipMemcpy(d_p, rows.ctypes.data_as(C.c_void_p), C.c_size_t(rows.nbytes), 1) == 0
        assert hip.hipMemcpy(d_o, fill.ctypes.data_as(C.c_void_p), C.c_size_t(fill.nbytes), 1) == 0
        rt.bake_device(rt.bake_params("texel", 5), d_p.value, len(rows), d_o.value, f64=True)
        assert rt.last_bake_ms() > 0
        got = np.zeros_like(fill)
        assert hip.hipDeviceSynchronize() == 0
        assert hip.hipMemcpy(got.ctypes.data_as(C.c_void_p), d_o, C.c_size_t(got.nbytes), 2) == 0
    finally:
        assert hip.hipFree(d_p) == 0 and hip.hipFree(d_o) == 0
    assert same(got, rt.bake_texels(s["P"], s["N"], 5))


# ---------------------------------------------------------------------------------------------------------------- 8. refusals
def test_bad_calls_are_refused_and_leave_output_and_timers_alone(setups):
    s = setups("cornell")
    rt, L = s["rt"], s["rt"].L
    frame = rt.run(24, 16, min_samples=2, max_samples=2)
    good = rt.bake_texels(s["P"], s["N"], 5)
    k_before, ms_before = rt.last_kernel_ms(), rt.last_render_ms()
    assert rt.last_bake_ms() > 0
    rows = np.ascontiguousarray(np.concatenate([s["P"], s["N"]], 1))
    n = len(rows)
    out = np.full((n, 9, 3), -7.0)
    po, pp = out.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(gi._dp)
    NOWHERE = C.c_void_p(16)
    B = gi.BakeParams
    nan, inf = float("nan"), float("inf")

    def host(points, n_points, bp, o=po):
        return L.gi_bake_host(rt.h, points, n_points, C.byref(bp) if bp is not None else None, o, 1)

    ok = B(be.TEXEL, 5, 0, 1)
    for bad in (B(2, 5, 0, 1), B(-1, 5, 0, 1), B(be.TEXEL, 0, 0, 1), B(be.SH9, -3, 0, 1), B(be.TEXEL, 5, 2 ** 32 - 5 * n + 1, 1)):
        assert host(pp, n, bad) == gi.GI_E_INVALID, (bad.mode, bad.n_samples, bad.stream_base)
        assert b"bake" in L.gi_last_error(rt.h)
        assert rt.last_bake_ms() == 0.0
        assert L.gi_bake_device(rt.h, NOWHERE, n, C.byref(bad), NOWHERE, 1) == gi.GI_E_INVALID      # refused before a pointer is used
        assert L.gi_bake_rays(rt.h, pp, n, C.byref(bad), None, None) == gi.GI_E_INVALID
    assert host(pp, n, B(be.TEXEL, 5, 2 ** 32 - 5 * n, 1)) == gi.GI_OK and rt.last_bake_ms() > 0     # the last index is 2^32 - 1: it fits
    out[:] = -7.0
    assert host(pp, -1, ok) == gi.GI_E_INVALID and host(None, n, ok) == gi.GI_E_INVALID and host(pp, n, ok, None) == gi.GI_E_INVALID
    assert host(pp, n, None) == gi.GI_E_INVALID and L.gi_bake_host(None, pp, n, C.byref(ok), po, 1) == gi.GI_E_INVALID
    assert L.gi_bake_device(rt.h, None, n, C.byref(ok), NOWHERE, 1) == gi.GI_E_INVALID and L.gi_bake_device(rt.h, NOWHERE, n, C.byref(ok), None, 1) == gi.GI_E_INVALID
    assert L.gi_last_bake_ms(rt.h, None) == gi.GI_E_INVALID
    for col, value in ((0, nan), (2, inf), (1, -inf), (4, nan), (5, inf)):
        r = rows.copy()
        r[n // 2, col] = value
        assert host(r.ctypes.data_as(gi._dp), n, ok) == gi.GI_E_INVALID and str(n // 2).encode() in L.gi_last_error(rt.h)
    r = rows.copy()
    r[n - 1, 3:6] = 0.0                                                                    # a zero normal counts as non-finite
    assert host(r.ctypes.data_as(gi._dp), n, ok) == gi.GI_E_INVALID
    assert host(r.ctypes.data_as(gi._dp), n, B(be.SH9, 5, 0, 1)) == gi.GI_OK                 # ... for a texel: read as probes ([2 n][3]) the rows are fine
    assert (out[:n] != -7.0).all()
    out[:] = -7.0
    r3 = np.ascontiguousarray(s["probes"].copy())
    r3[0, 1] = nan
    assert host(r3.ctypes.data_as(gi._dp), len(r3), B(be.SH9, 5, 0, 1)) == gi.GI_E_INVALID
    with pytest.raises(gi.GiError):
        rt.bake_probes(r3, 5)
    with pytest.raises(gi.GiError):
        rt.bake_fold(2, np.zeros((2, 3, 3)))
    empty = gi.RayTracer(0)
    assert L.gi_bake_host(empty.h, pp, n, C.byref(ok), po, 1) == gi.GI_E_STATE and b"no scene" in L.gi_last_error(empty.h)
    assert L.gi_bake_device(empty.h, NOWHERE, n, C.byref(ok), NOWHERE, 1) == gi.GI_E_STATE
    assert host(pp, 0, ok) == gi.GI_OK and host(None, 0, ok, None) == gi.GI_OK                  # no points: nothing to do, nothing written
    assert rt.bake_probes(np.zeros((0, 3)), 5).shape == (0, 9, 3) and rt.bake_rays(np.zeros((0, 3)), None, 5)[0].shape == (0, 6)
    assert (out == -7.0).all() and rt.last_bake_ms() == 0.0
    assert rt.last_kernel_ms() == k_before and rt.last_render_ms() == ms_before
    assert same(rt.bake_texels(s["P"], s["N"], 5), good) and same(rt.run(24, 16, min_samples=2, max_samples=2), frame)


# ---------------------------------------------------------------------------------------------------------------- 9. the command line
def test_cli_writes_the_probe_grid(setups, tmp_path, capsys):
    from gi_raytracer_amd import __main__ as cli
    s = setups("cornell")
    scn = os.path.join(pc.ROOT, pc.SCN["cornell"])
    path = tmp_path / "probes.npy"
    assert cli.main([scn, "--probes", "3", "2", "2", "--probe-samples", "5", "--photons", "0", "-o", str(path)]) == 0
    assert os.listdir(tmp_path) == ["probes.npy"] and "probes" in capsys.readouterr().out
    got = np.load(path)
    assert got.shape == (2, 2, 3, 9, 3) and got.dtype == np.float32
    b = s["scene"].tables()["node_bbox"][0]
    grid = gi.probe_grid(b, 3, 2, 2)
    assert grid.shape == (2, 2, 3, 3)
    assert np.allclose(grid[0, 0, 0], b[0:3] + (b[3:6] - b[0:3]) / np.array([6.0, 4.0, 4.0])) and np.allclose(grid[1, 1, 2], b[3:6] - (b[3:6] - b[0:3]) / np.array([6.0, 4.0, 4.0]))
    assert same(got, s["rt"].bake_probes(grid.reshape(-1, 3), 5, f64=False).reshape(2, 2, 3, 9, 3))
    with pytest.raises(SystemExit):
        cli.main([scn, "--probes", "3", "2", "2", "--samples", "1", "-o", str(path)])
