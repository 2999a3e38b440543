"""Reflection probes (gi_cubemap_*: the capture through k_bake_gen and the stream passes, k_cm_box, k_cm_filter, k_cm_resolve) on the GPU, through the
C ABI via the Python mirror.

The expectation is tests/cubemap_expect.py.  What is exact and what has an allowance:
 * stream indices, ray origins and ray directions are the statement's bit for bit (no device trigonometry);
 * the prefilter on caller data is bit-equal to the numpy statement;
 * a whole capture is compared with the texel fold of Oracle.radiance on the device's rays: RMSE below parity_checks.RMSE_TOL, printed;
 * every identity (whole chain, chunks, ranges, f32, frames, bakes and sessions left alone) is exact, bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gi_raytracer_amd as gi

import bake_expect as be
import cubemap_expect as ce
import host_build
import parity_checks as pc

pytestmark = pytest.mark.gpu

SEEDS = (ce.DEFAULT_SEED, 12345)
BASE = 1000


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def same_chain(a, b):
    return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))


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
            cache[name] = {"scene": scene, "rt": rt, "o": o, "pos": ce.root_box_middle(scene.tables())}
        return cache[name]

    return get


# ---------------------------------------------------------------------------------------------------------------- 1. rays
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("face, ns", [(3, 5), (4, 2)])
def test_rays_are_the_statement_bit_for_bit(setups, face, ns, seed):
    s = setups("cornell")
    for base in (0, BASE):
        rays, st = s["rt"].cubemap_rays(s["pos"], face, ns, stream_base=base, seed=seed)
        want, wst = ce.capture_rays(s["pos"], face, ns, base)
        assert st.dtype == np.uint32 and np.array_equal(st, wst)
        assert same(rays[:, 0:3], want[:, 0:3])
        assert same(rays[:, 3:6], want[:, 3:6])


# ---------------------------------------------------------------------------------------------------------------- 2. the prefilter on caller data
# the workgroup and the tile are 256: level 1 of face 20 has 600 output texels over 2 400 source texels, 400 a face -- a multiple of neither
@pytest.mark.parametrize("face, levels, exponents", [(8, 4, (0, 5, 1, 0)), (20, 3, (0, 16, 5))])
def test_prefilter_on_caller_data_is_the_statement_bit_for_bit(setups, face, levels, exponents):
    rt = setups("cornell")["rt"]
    cube = ce.mixed_cube(face, 7 * face)
    got = rt.cubemap_prefilter(cube, levels, exponents)
    want = ce.prefilter(cube, levels, exponents)
    assert [g.shape for g in got] == [(6, face >> l, face >> l, 3) for l in range(levels)]
    assert same(got[0], cube)
    for l in range(levels):
        assert np.isfinite(want[l]).all() and (l == 0 or want[l].max() > 0)
        assert same(got[l], want[l]), f"level {l}: {int((got[l] != want[l]).sum())} of {want[l].size} values differ"


# ---------------------------------------------------------------------------------------------------------------- 3. a whole capture
@pytest.mark.parametrize("name", ["cornell", "caustics"])
def test_capture_is_the_fold_of_the_oracles_radiance(setups, name):
    s = setups(name)
    rt = s["rt"]
    for face, ns, base, seed in ((4, 5, 0, SEEDS[0]), (3, 2, BASE, SEEDS[1])):
        rays, st = rt.cubemap_rays(s["pos"], face, ns, stream_base=base, seed=seed)
        want = ce.expected_capture(s["o"], rays, st, ns, seed).reshape(6, face, face, 3)
        got = rt.bake_reflection_probe(s["pos"], face, ns, stream_base=base, seed=seed)
        assert len(got) == 1 and got[0].shape == want.shape and got[0].dtype == np.float64
        rmse = float(np.sqrt(((got[0] - want) ** 2).mean()))
        print(f"{name} face {face} n {ns}: rmse {rmse:.3e}, mean |want| {np.abs(want).mean():.4f}, {int((got[0] == want).all(-1).sum())} of {6 * face * face} texels bit-equal")
        assert np.abs(want).max() > 0 and rmse < pc.RMSE_TOL
        # the device's own function-level path tracer on the same rays states it too
        again = be.fold_texel(rt.radiance(rays, st, seed).reshape(-1, ns, 3)).reshape(want.shape)
        assert float(np.sqrt(((got[0] - again) ** 2).mean())) < pc.RMSE_TOL


# ---------------------------------------------------------------------------------------------------------------- 4. the whole chain
def test_chain_is_the_prefilter_of_its_own_level_0(setups):
    s = setups("caustics")
    rt = s["rt"]
    chain = rt.bake_reflection_probe(s["pos"], 8, 3, levels=3)
    assert [c.shape for c in chain] == [(6, 8, 8, 3), (6, 4, 4, 3), (6, 2, 2, 3)] and np.abs(chain[0]).max() > 0
    assert same_chain(rt.cubemap_prefilter(chain[0], 3), chain)
    assert same_chain(ce.prefilter(chain[0], 3), chain)
    assert same(rt.bake_reflection_probe(s["pos"], 8, 3)[0], chain[0])            # the levels asked for do not touch the capture


# ---------------------------------------------------------------------------------------------------------------- 5. chunks and ranges cannot show
def test_chunks_of_texels_and_ranges_of_samples_leave_no_trace(setups):
    s = setups("caustics")
    rt = s["rt"]
    whole_many, whole_few = rt.bake_reflection_probe(s["pos"], 5, 5), rt.bake_reflection_probe(s["pos"], 1, 100)
    try:
        rt.set_pool_slots(64)                                    # 150 texels: three chunks, the last a part of one; one sample a range
        assert same_chain(rt.bake_reflection_probe(s["pos"], 5, 5), whole_many)
        assert same_chain(rt.bake_reflection_probe(s["pos"], 1, 100), whole_few)      # 6 texels, 64 < 600: ranges of 10 samples
    finally:
        rt.set_pool_slots(1 << 30)
    assert same_chain(rt.bake_reflection_probe(s["pos"], 5, 5), whole_many)
    assert same_chain(rt.bake_reflection_probe(s["pos"], 1, 100), whole_few)


# ---------------------------------------------------------------------------------------------------------------- 6. f32
def test_f32_chain_is_the_f64_chain_rounded_once(setups):
    s = setups("caustics")
    full = s["rt"].bake_reflection_probe(s["pos"], 4, 5, levels=3)
    f32 = s["rt"].bake_reflection_probe(s["pos"], 4, 5, levels=3, f64=False)
    assert all(a.dtype == np.float32 for a in f32) and same_chain(f32, [a.astype(np.float32) for a in full])


# ---------------------------------------------------------------------------------------------------------------- 7. the others are left alone
def test_frames_bakes_timers_and_a_session_are_untouched(setups):
    s = setups("caustics")
    rt = s["rt"]
    kw = dict(min_samples=6, max_samples=6)
    before = rt.run(48, 32, **kw)
    k_before, ms_before = rt.last_kernel_ms(), rt.last_render_ms()
    assert k_before["trace"] > 0
    probes = rt.bake_probes(s["pos"][None], 16)
    bake_ms = rt.last_bake_ms()
    assert bake_ms > 0
    chain = rt.bake_reflection_probe(s["pos"], 4, 5, levels=2)
    ms, stages = rt.last_cubemap_ms()
    assert ms > 0 and stages["capture"] > 0 and stages["prefilter"] > 0
    assert rt.last_kernel_ms() == k_before and rt.last_render_ms() == ms_before and rt.last_bake_ms() == bake_ms
    assert same(rt.run(48, 32, **kw), before) and same(rt.bake_probes(s["pos"][None], 16), probes)
    assert same_chain(rt.bake_reflection_probe(s["pos"], 4, 5, levels=2), chain)
    for mode in ("rounds", "megakernel"):                        # the render mode plays no part
        try:
            rt.set_render_mode(mode)
            assert same_chain(rt.bake_reflection_probe(s["pos"], 4, 5, levels=2), chain)
        finally:
            rt.set_render_mode("wavefront")
    try:                                                         # nor does the lens
        rt.set_lens(0.35, 5, 0.3)
        assert same_chain(rt.bake_reflection_probe(s["pos"], 4, 5, levels=2), chain)
    finally:
        rt.set_lens(0.0)
    with rt.progressive(48, 32, **kw) as sess:                   # step, capture, step has the bits of step, step
        sess.step(2)
        end = sess.sample_end
        assert same_chain(rt.bake_reflection_probe(s["pos"], 4, 5, levels=2), chain)
        assert sess.sample_end == end
        assert same(sess.step(4), before)


def test_device_entry_writes_what_the_host_entry_returns(setups):
    s = setups("cornell")
    rt = s["rt"]
    hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")      # device buffers from the HIP runtime the library itself uses (no second runtime in this process)
    p = rt.cubemap_params(4, 5, levels=3)
    n = rt.L.gi_cubemap_chain_texels(4, 3)
    assert n == 6 * (16 + 4 + 1)
    fill = np.full((n, 3), -7.0)
    d_o = C.c_void_p()
    assert hip.hipMalloc(C.byref(d_o), C.c_size_t(fill.nbytes)) == 0
    try:
        assert hip.hipMemcpy(d_o, fill.ctypes.data_as(C.c_void_p), C.c_size_t(fill.nbytes), 1) == 0
        rt.cubemap_device(p, s["pos"], d_o.value, f64=True)
        assert rt.last_cubemap_ms()[0] > 0
        got = np.zeros_like(fill)
        assert hip.hipDeviceSynchronize() == 0
        assert hip.hipMemcpy(got.ctypes.data_as(C.c_void_p), d_o, C.c_size_t(got.nbytes), 2) == 0
    finally:
        assert hip.hipFree(d_o) == 0
    want = rt.bake_reflection_probe(s["pos"], 4, 5, levels=3)
    assert same(got, np.concatenate([w.reshape(-1, 3) for w in want]))


# ---------------------------------------------------------------------------------------------------------------- 8. refusals
def test_bad_calls_are_refused_and_leave_output_and_timers_alone(setups):
    s = setups("cornell")
    rt, L = s["rt"], s["rt"].L
    frame = rt.run(24, 16, min_samples=2, max_samples=2)
    good = rt.bake_reflection_probe(s["pos"], 4, 5, levels=2)
    k_before, ms_before, cm_before = rt.last_kernel_ms(), rt.last_render_ms(), rt.last_cubemap_ms()
    assert cm_before[0] > 0
    out = np.full((L.gi_cubemap_chain_texels(4, 2), 3), -7.0)
    po, pp = out.ctypes.data_as(C.c_void_p), np.ascontiguousarray(s["pos"]).ctypes.data_as(gi._dp)
    NOWHERE, NOWHERE_D = C.c_void_p(16), C.cast(C.c_void_p(16), gi._dp)
    nan, inf = float("nan"), float("inf")

    def params(face=4, ns=5, levels=2, base=0, exponents=None):
        return rt.cubemap_params(face, ns, levels, exponents, base)

    def host(pos, p, o=po):
        return L.gi_cubemap_host(rt.h, pos, C.byref(p) if p is not None else None, o, 1)

    bad = [params(face=0), params(face=-4), params(ns=0), params(ns=-3), params(levels=0), params(levels=13), params(face=6, levels=3),
           params(face=4, levels=4), params(exponents=(0, 17)), params(exponents=(0, -1)), params(levels=3, exponents=(0, 5, 17)),
           params(base=2 ** 32 - 6 * 16 * 5 + 1), params(face=30000, ns=1, levels=1)]
    for p in bad:
        what = (p.face, p.n_samples, p.levels, p.stream_base, list(p.log2_exponent))
        assert host(pp, p) == gi.GI_E_INVALID, what
        assert b"cubemap" in L.gi_last_error(rt.h)
        assert L.gi_cubemap_device(rt.h, NOWHERE_D, C.byref(p), NOWHERE, 1) == gi.GI_E_INVALID, what     # refused before a pointer is used
        assert L.gi_cubemap_rays(rt.h, NOWHERE_D, C.byref(p), NOWHERE_D, None) == gi.GI_E_INVALID, what
        assert L.gi_cubemap_prefilter(rt.h, C.byref(p), NOWHERE_D, NOWHERE_D) == gi.GI_E_INVALID, what
    ok = params()
    assert host(pp, params(exponents=(99, 5))) == gi.GI_OK                       # entry 0 is ignored
    assert host(pp, params(base=2 ** 32 - 6 * 16 * 5)) == gi.GI_OK and rt.last_cubemap_ms()[0] > 0     # the last index is 2^32 - 1: it fits
    assert host(pp, ok) == gi.GI_OK and same(out, np.concatenate([g.reshape(-1, 3) for g in good]))
    cm_before = rt.last_cubemap_ms()
    out[:] = -7.0
    assert host(None, ok) == gi.GI_E_INVALID and host(pp, ok, None) == gi.GI_E_INVALID and host(pp, None) == gi.GI_E_INVALID
    assert L.gi_cubemap_host(None, pp, C.byref(ok), po, 1) == gi.GI_E_INVALID
    assert L.gi_cubemap_device(rt.h, None, C.byref(ok), NOWHERE, 1) == gi.GI_E_INVALID and L.gi_cubemap_device(rt.h, pp, C.byref(ok), None, 1) == gi.GI_E_INVALID
    assert L.gi_cubemap_rays(rt.h, pp, C.byref(ok), None, None) == gi.GI_E_INVALID and L.gi_cubemap_prefilter(rt.h, C.byref(ok), None, None) == gi.GI_E_INVALID
    assert L.gi_last_cubemap_ms(rt.h, None, None) == gi.GI_E_INVALID
    for k, value in ((0, nan), (2, inf), (1, -inf)):
        q = np.ascontiguousarray(s["pos"]).copy()
        q[k] = value
        assert host(q.ctypes.data_as(gi._dp), ok) == gi.GI_E_INVALID and b"non-finite" in L.gi_last_error(rt.h)
        with pytest.raises(gi.GiError):
            rt.cubemap_rays(q, 4, 5)
    with pytest.raises(gi.GiError):
        rt.bake_reflection_probe(s["pos"], 6, 5, levels=3)
    with pytest.raises(gi.GiError):
        rt.cubemap_prefilter(np.zeros((6, 6, 6, 3)), 3)
    empty = gi.RayTracer(0)
    assert L.gi_cubemap_host(empty.h, pp, C.byref(ok), po, 1) == gi.GI_E_STATE and b"no scene" in L.gi_last_error(empty.h)
    assert L.gi_cubemap_device(empty.h, NOWHERE_D, C.byref(ok), NOWHERE, 1) == gi.GI_E_STATE
    assert same_chain(empty.cubemap_prefilter(good[0], 2), good)                 # the prefilter needs no scene
    assert (out == -7.0).all() and rt.last_cubemap_ms() == cm_before
    assert rt.last_kernel_ms() == k_before and rt.last_render_ms() == ms_before
    assert same_chain(rt.bake_reflection_probe(s["pos"], 4, 5, levels=2), good) and same(rt.run(24, 16, min_samples=2, max_samples=2), frame)


# ---------------------------------------------------------------------------------------------------------------- 9. the command line and C++
def test_cli_writes_the_chain(setups, tmp_path, capsys):
    from gi_raytracer_amd import __main__ as cli
    s = setups("cornell")
    scn = os.path.join(pc.ROOT, pc.SCN["cornell"])
    path = tmp_path / "probe.npz"
    pos = [repr(float(v)) for v in s["pos"]]
    assert cli.main([scn, "--reflection-probe", *pos, "--probe-face", "4", "--probe-samples", "5", "--probe-levels", "3", "--photons", "0", "-o", str(path)]) == 0
    assert os.listdir(tmp_path) == ["probe.npz"] and "reflection probe" in capsys.readouterr().out
    got = np.load(path)
    assert sorted(got.files) == ["level0", "level1", "level2"]
    want = s["rt"].bake_reflection_probe(s["pos"], 4, 5, levels=3, f64=False)
    for l in range(3):
        assert got[f"level{l}"].shape == (6, 4 >> l, 4 >> l, 3) and same(got[f"level{l}"], want[l])
    for extra in (["--probes", "2", "2", "2"], ["--lightmap", "8", "8"], ["--samples", "1"], ["--probe-levels", "4"]):
        with pytest.raises(SystemExit):
            cli.main([scn, "--reflection-probe", *pos, "--probe-face", "4", "-o", str(path)] + extra)


def test_cpp_reflection_probe_matches_the_python_mirror(tmp_path):
    """RayTracer::bakeReflectionProbe of the drop-in C++ class (include/gi/raytracer.h) returns what RayTracer.bake_reflection_probe returns."""
    exe = str(tmp_path / "test_cubemap")
    host_build.client("tests/cpp/test_cubemap.cpp", exe, "-O1")
    scn = os.path.join(pc.ROOT, pc.SCN["cornell"])
    pos = [float(v) for v in ce.root_box_middle(gi.Scene.load(scn).rebuild().tables())]
    out = subprocess.run([exe, scn, *(repr(v) for v in pos), "4", "3", "3"], check=True, capture_output=True, text=True).stdout
    assert "levels 3" in out and "bad arguments refused 1 kept 1" in out, out
    rt = gi.RayTracer(0).setScene(gi.Scene.load(scn).rebuild())      # no photon map, as in the C++ class before its first frame
    want = rt.bake_reflection_probe(pos, 4, 3, levels=3)
    assert np.abs(want[0]).max() > 0
    for l, level in enumerate(want):
        acc = 0.0
        for v in level.reshape(-1):
            acc = acc + float(v)
        assert f"level {l} size {level.size} sum {acc:.17g}\n" in out, (l, acc, out)
