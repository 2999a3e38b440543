"""The baked-light pass (gi_render_baked_*, k_lit) on the GPU, through the C ABI via the Python mirror.

What is exact and what has an allowance:
 * the direct term is the frame's depth-0 shade: on a scene whose paths all leave after the first hit, with no ambient light and no photons, a
   one-sample frame equals it bit for bit, with one light and with several;
 * given the oracle's first hits (ids and coverage are compared first), the diffuse term equals the numpy statement (tests/baked_expect.py) bit for bit;
 * the specular term is bit-equal wherever the device reads the statement's texel; a reflection within a few ulp of a texel border may read the
   neighbour -- at most 1 sample in 1 000 may (tests/test_baked_cpu.py shows on the CPU that on these frames a 4-ulp move of R flips none, so none is
   expected; the count is printed);
 * every identity (stripes, f32, walk variants, repetition, the pinhole, the beauty sum) is exact, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import gi_raytracer_amd as gi

import baked_expect as be
import features_expect as fe
import occlusion_expect as oe
import parity_checks as pc

pytestmark = pytest.mark.gpu

W, H = 24, 16
SIZES = ((13, 9), (24, 16))         # 13 x 9: no multiple of the 8 x 8 tile and less than one workgroup
N = 2
DIRECT, DIFFUSE, SPECULAR, EMISSIVE = be.DIRECT, be.DIFFUSE, be.SPECULAR, be.EMISSIVE


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def dark(scene):
    """The scene with no ambient light."""
    scene.set_ambient((0, 0, 0))
    return scene.rebuild()


@pytest.fixture(scope="module")
def setups():
    cache = {}

    def get(name):
        if name not in cache:
            if name in ("floor", "box"):
                scene = dark(oe.floor_scene(gi)) if name == "floor" else oe.closed_box_scene(gi)
                rt, o = gi.RayTracer(0).setScene(scene), pc.oracle_for(scene)
            else:                                                  # a scene file, its materials cycled through the three lobes
                base = pc.named_scene(name)
                scene = be.with_roughnesses(base)
                rt = gi.RayTracer(0).setScene(scene)
                rt._adopt(base.settings)
                o = be.oracle_with_camera(scene, base.settings)
            cache[name] = (scene, rt, o, scene.tables())
        return cache[name]

    return get


@pytest.fixture(scope="module")
def inputs():
    """One grid per size and one chain, shared and left unchanged."""
    return {"sh": {g: be.random_sh(g, 100 + k) for k, g in enumerate(be.GRIDS)}, "chain": be.random_chain(7)}


# ---------------------------------------------------------------------------------------------------------------- 1. the direct term is the frame's
@pytest.mark.parametrize("extra_lights", [0, 3])
def test_direct_term_equals_the_one_sample_frame_bit_for_bit(extra_lights):
    scene = oe.floor_scene(gi)
    for k in range(extra_lights):           # the last VISIBLE light wins: the last one is below the floor, hidden from every hit
        scene.add_light(((8.0, 3.0, -6.0), (-7.0, 9.0, 5.0), (-4.0, -2.0, 1.0))[k], ((1.0, 0.5, 0.25), (0.5, 2.0, 1.0), (0.25, 0.5, 3.0))[k], (0.2, 0.1, 0.4)[k])
    scene = dark(scene)
    rt = gi.RayTracer(0).setScene(scene)
    for (w, h) in SIZES:
        frame = rt.run(w, h, min_samples=1, max_samples=1)
        lit = rt.run_baked(w, h, 1, terms=DIRECT)
        assert frame.shape == lit["direct"].shape == (h, w, 3) and (frame > 0).any()
        assert same(np.ascontiguousarray(lit["direct"]), frame), (w, h, float(np.abs(lit["direct"] - frame).max()))
        assert same(np.ascontiguousarray(lit["beauty"]), frame)                  # nothing else is asked for
        try:
            rt.set_wide_nodes(False)
            assert same(np.ascontiguousarray(rt.run_baked(w, h, 1, terms=DIRECT)["direct"]), frame)
        finally:
            rt.set_wide_nodes(True)
    if extra_lights:
        one = gi.RayTracer(0).setScene(dark(oe.floor_scene(gi)))
        assert not same(one.run_baked(W, H, 1, terms=DIRECT)["direct"], rt.run_baked(W, H, 1, terms=DIRECT)["direct"])


# ---------------------------------------------------------------------------------------------------------------- 2. diffuse and specular are the statement's
@pytest.mark.parametrize("name", ["cornell", "spheres_opaque", "test_scene"])
def test_diffuse_and_specular_match_the_statement(setups, inputs, name):
    scene, rt, o, t = setups(name)
    assert name in fe.DRAW_FREE_SCENES and fe.oracle_is_draw_free(o, fe.sample_rays(o, W, H, 0)[0])
    geo = [be.sample_hits(o, t, W, H, s) for s in range(N)]
    f1, f2 = rt.run_features(W, H, 1), rt.run_features(W, H, N)
    assert np.array_equal(f1["ids"][:, :, 0], geo[0]["ent"].reshape(H, W))                      # identical first hits
    assert np.array_equal(f2["coverage"] * N, sum(g["hit"].reshape(H, W).astype(np.float64) for g in geo))
    box, chain = be.inner_box(t), inputs["chain"]
    flat = np.concatenate([c.reshape(-1, 3) for c in chain])
    off = be.chain_offsets(be.CHAIN_FACE, be.CHAIN_LEVELS)
    differ = asked = 0
    for grid in be.GRIDS:
        sh = inputs["sh"][grid]
        terms = [be.sample_terms(g, t, sh, box, chain, be.CHAIN_EXPONENTS) for g in geo]
        kw = dict(sh=sh, grid_box=box, chain=chain, exponents=be.CHAIN_EXPONENTS, terms=DIFFUSE | SPECULAR)
        got1, got = rt.run_baked(W, H, 1, **kw), rt.run_baked(W, H, N, **kw)
        assert got["baked"].shape == (H, W, 12) and got["baked"].dtype == np.float64
        assert all(same(got[k], got["baked"][:, :, 3 * i:3 * i + 3]) for i, k in enumerate(("beauty", "direct", "diffuse", "specular")))
        assert not got["direct"].any()
        # diffuse: bit for bit, one sample and two
        assert same(np.ascontiguousarray(got1["diffuse"]), be.fold([terms[0][0]]).reshape(H, W, 3)), (name, grid)
        assert same(np.ascontiguousarray(got["diffuse"]), be.fold([d for d, _, _, _ in terms]).reshape(H, W, 3)), (name, grid)
        clamped = sum(int(((g["P"][g["hit"]] < box[:3]) | (g["P"][g["hit"]] > box[3:])).any(1).sum()) for g in geo)
        assert clamped > 0 and (got["diffuse"] > 0).any()                                        # hits outside the grid's box: the clamp happens
        # specular, one sample: the statement's value, or -- counted -- the value of another texel of the same level
        spec1 = np.ascontiguousarray(got1["specular"]).reshape(-1, 3)
        want1, texel = terms[0][1], terms[0][2]
        wrong = np.flatnonzero((spec1 != want1).any(1))
        for i in wrong:
            assert texel[i] >= 0, (name, grid, i)                                                # a sample with no specular term must be +0.0
            l = int(np.searchsorted(off, texel[i], side="right")) - 1
            cand = geo[0]["albedo"][i] * flat[off[l]:off[l + 1]]
            assert (cand == spec1[i]).all(1).any(), (name, grid, i, spec1[i], want1[i])          # some texel's value, or the term itself is wrong
        n_spec = [int((tm[2] >= 0).sum()) for tm in terms]
        differ += len(wrong); asked += n_spec[0]
        # two samples: bit for bit in every pixel (a pixel that differs counts as one more sample reading another texel)
        want = be.fold([s for _, s, _, _ in terms])
        bad = int((np.ascontiguousarray(got["specular"]).reshape(-1, 3) != want).any(1).sum())
        differ += bad; asked += sum(n_spec)
        print(f"{name} grid {grid}: {len(wrong)} of {n_spec[0]} one-sample and {bad} of {H * W} two-sample specular values read another texel than the statement's")
        # beauty: per sample one of the two terms is +0.0 and a miss is the ambient colour; halving a sum of two is exact
        misses = (N - sum(g["hit"].reshape(H, W).astype(np.float64) for g in geo)) / N
        assert same(np.ascontiguousarray(got["beauty"]), np.ascontiguousarray(((got["direct"] + got["diffuse"]) + got["specular"]) + misses[:, :, None] * t["ambient"]))
    assert asked > 0 and differ * 1000 <= asked, (differ, asked)      # (with fewer than 1 000 specular samples in the frames, none may differ)
    lobes = set(np.concatenate([tm[3] for tm in terms]).tolist())
    assert lobes >= {1, 2}, lobes


# ---------------------------------------------------------------------------------------------------------------- 3. analytic checks
def test_band_0_alone_gives_albedo_times_a_constant_whatever_the_normal(setups):
    scene, rt, o, t = setups("cornell")
    sh = np.zeros((1, 1, 1, 9, 3))
    sh[0, 0, 0, 0] = (2.0, 0.5, 1.25)
    got = rt.run_baked(W, H, N, sh=sh, grid_box=be.inner_box(t), terms=DIFFUSE)["diffuse"]
    geo = [be.sample_hits(o, t, W, H, s) for s in range(N)]
    D = np.where(np.array([2.0, 0.5, 1.25]) * (1.0 * 0.28209479177387814) < 0, 0.0, (0.0 + (1.0 * 0.28209479177387814) * np.array([2.0, 0.5, 1.25])))
    per = [np.where((be.lobe_of(t["mats"][np.where(g["hit"], g["mat"], 0), 0]) == 2)[:, None] & g["hit"][:, None], g["albedo"] * D, 0.0) for g in geo]
    assert same(np.ascontiguousarray(got), be.fold(per).reshape(H, W, 3)) and (got > 0).any()


def test_a_chain_of_one_colour_shows_on_specular_hits_only(setups):
    scene, rt, o, t = setups("test_scene")
    colour = np.array([0.5, 2.0, 0.125])
    chain = [np.ascontiguousarray(np.broadcast_to(colour, (6, 8 >> l, 8 >> l, 3))) for l in range(3)]
    got = rt.run_baked(W, H, 1, chain=chain, exponents=be.CHAIN_EXPONENTS, terms=SPECULAR)
    g = be.sample_hits(o, t, W, H, 0)
    lobe = np.where(g["hit"], be.lobe_of(t["mats"][np.where(g["hit"], g["mat"], 0), 0]), -1)
    want = np.where(((lobe == 0) | (lobe == 1))[:, None], g["albedo"] * colour, 0.0)
    assert same(np.ascontiguousarray(got["specular"]), want.reshape(H, W, 3)) and (lobe == 2).any() and (want > 0).any()
    assert not got["diffuse"].any() and not got["direct"].any()


def test_misses_show_the_ambient_colour_and_no_term(setups):
    scene, rt, o, t = setups("spheres_opaque")                        # its frame sees past the spheres, and its ambient colour is not 0
    ambient = t["ambient"]
    assert ambient.all() and not t["mats"][:, 6:9].any()
    cov = rt.run_features(W, H, N, want_ids=False)["coverage"]
    got = rt.run_baked(W, H, N, sh=be.random_sh((2, 2, 2), 3), grid_box=be.inner_box(t), chain=be.random_chain(4), exponents=be.CHAIN_EXPONENTS)
    miss = cov == 0
    assert miss.any() and (cov == 1).any()
    assert (got["beauty"][miss] == ambient).all()                     # (a + a) / 2
    assert not got["direct"][miss].any() and not got["diffuse"][miss].any() and not got["specular"][miss].any()
    assert (got["direct"][cov == 1] > 0).any()


# ---------------------------------------------------------------------------------------------------------------- 4. identities, bit for bit
@pytest.mark.parametrize("name", ["cornell", "spheres_opaque"])
def test_identities_bit_for_bit(setups, inputs, name):
    scene, rt, o, t = setups(name)
    kw = dict(sh=inputs["sh"][(3, 2, 4)], grid_box=be.inner_box(t), chain=inputs["chain"], exponents=be.CHAIN_EXPONENTS)
    for (w, h) in SIZES:
        full = rt.run_baked(w, h, N, **kw)["baked"]
        assert np.isfinite(full).all() and (full[:, :, 3:6] > 0).any()
        assert same(rt.run_baked(w, h, N, **kw)["baked"], full)                                   # a repeated call
        f32 = rt.run_baked(w, h, N, f64=False, **kw)["baked"]
        assert f32.dtype == np.float32 and same(f32, full.astype(np.float32))
        for world in (2, 3):
            frame = np.full_like(full, -7.0)
            for rank in range(world):
                part = rt.run_baked(w, h, N, stripe_h=4, rank=rank, world=world, **kw)["baked"]
                rows = fe.frame_rows(h, 4, rank, world)
                assert part.shape == (len(rows), w, 12)
                frame[rows] = part
            assert same(frame, full), (name, w, h, world)
        for switch in (rt.set_wide_nodes, rt.set_content_culling):
            try:
                switch(False)
                off = rt.run_baked(w, h, N, **kw)["baked"]
            finally:
                switch(True)
            assert same(off, full), (name, w, h, switch.__name__)
    w, h = SIZES[0]
    # beauty = ((direct + diffuse) + specular) + emissive, from single-sample calls of one term each
    one = rt.run_baked(w, h, 1, terms=15, **kw)
    parts = [rt.run_baked(w, h, 1, terms=bit, **kw) for bit in (DIRECT, DIFFUSE, SPECULAR)]
    em = rt.run_baked(w, h, 1, terms=EMISSIVE)["beauty"]
    miss = (rt.run_features(w, h, 1, want_ids=False)["coverage"] == 0)[:, :, None]
    for k, part in zip(("direct", "diffuse", "specular"), parts):             # a term alone: beauty is the term, or the ambient colour on a miss
        assert same(np.ascontiguousarray(part[k]), np.ascontiguousarray(one[k])) and same(np.ascontiguousarray(part["beauty"]), np.where(miss, t["ambient"], part[k]))
    assert same(np.ascontiguousarray(one["beauty"]), np.ascontiguousarray(((one["direct"] + one["diffuse"]) + one["specular"]) + em))
    # a lens of radius 0 is the pinhole; under a lens the coverage is the feature pass's
    full = rt.run_baked(W, H, N, **kw)
    try:
        rt.set_lens(radius=0.0, blades=5)
        assert same(rt.run_baked(W, H, N, **kw)["baked"], full["baked"])
        rt.set_lens(radius=0.3, blades=5)
        lens = rt.run_baked(W, H, N, terms=EMISSIVE | DIRECT)
        cov = rt.run_features(W, H, N, want_ids=False)["coverage"]
        assert not same(rt.run_baked(W, H, N, **kw)["baked"], full["baked"])
    finally:
        rt.set_lens(radius=0.0)
    assert cov.shape == (H, W) and np.isfinite(lens["baked"]).all()


def test_under_a_lens_the_misses_are_the_feature_pass_s(setups):
    scene, rt, o, t = setups("spheres_opaque")                        # nothing in it emits: with the emissive term alone, beauty is the misses' ambient colour
    assert t["ambient"].all() and not t["mats"][:, 6:9].any()
    try:
        rt.set_lens(radius=0.5, blades=6)
        cov = rt.run_features(W, H, N, want_ids=False)["coverage"]
        got = rt.run_baked(W, H, N, terms=EMISSIVE)["beauty"]
    finally:
        rt.set_lens(radius=0.0)
    assert 0 < cov.mean() < 1 and (cov == 0.5).any()
    for m, share in ((0, 1.0), (1, 0.5), (2, 0.0)):                   # m misses of two samples: 0, a / 2, (a + a) / 2
        want = np.zeros(3)
        for _ in range(m):
            want = want + t["ambient"]
        assert (got[cov == share] == want / 2.0).all(), m
    assert not same(cov, rt.run_features(W, H, N, want_ids=False)["coverage"])             # the pinhole sees other edges


# ---------------------------------------------------------------------------------------------------------------- 5. refusals and timers
def test_refusals_leave_the_output_and_the_timers_alone(setups, inputs):
    scene, rt, o, t = setups("cornell")
    L = rt.L
    p = rt.params(W, H)
    rt.run(W, H, min_samples=1, max_samples=1)
    rt.run_occlusion(W, H, n=1, dirs=2)
    sh, box = inputs["sh"][(2, 2, 2)], be.inner_box(t)
    good = rt.run_baked(W, H, 1, sh=sh, grid_box=box, chain=inputs["chain"], exponents=be.CHAIN_EXPONENTS)
    out = np.full((H, W, 12), -7.0)
    ptr = out.ctypes.data_as(C.c_void_p)
    bp, s, c = rt.baked_params(n=1, sh=sh, grid_box=box, chain=inputs["chain"], exponents=be.CHAIN_EXPONENTS)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))

    def variant(**kw):
        q = gi.BakedParams.from_buffer_copy(bp)
        for k, v in kw.items():
            if k in ("grid_min", "grid_max"):
                getattr(q, k)[:] = v
            elif k == "exp1":
                q.log2_exponent[1] = v
            else:
                setattr(q, k, v)
        return q

    # the grid's and the chain's rules are asked only where their term is
    assert L.gi_render_baked_host(rt.h, C.byref(p), C.byref(variant(terms=DIRECT, face=0, grid_max=list(box[:3]))), None, None, ptr, 1) == gi.GI_OK
    out[:] = -7.0
    ms0, frame_ms, ao_ms = rt.last_baked_ms(), rt.last_render_ms(), rt.last_occlusion_ms()
    assert ms0 > 0 and frame_ms[0] > 0 and ao_ms > 0
    bad = [variant(n_samples=0), variant(n_samples=-2), variant(terms=0), variant(terms=16), variant(terms=31), variant(nx=0), variant(nz=-1),
           variant(nx=2 ** 16, ny=2 ** 16, nz=2), variant(grid_max=[box[0], box[4], box[5]]), variant(grid_min=[box[3] + 1, box[1], box[2]]),
           variant(grid_min=[float("nan"), box[1], box[2]]), variant(grid_max=[float("inf"), box[4], box[5]]), variant(face=0), variant(face=6),
           variant(levels=0), variant(levels=13), variant(exp1=17), variant(exp1=-1), variant(face=30000, levels=1)]
    for q in bad:
        assert L.gi_render_baked_host(rt.h, C.byref(p), C.byref(q), dp(s), dp(c), ptr, 1) == gi.GI_E_INVALID, bytes(q)[:16]
        assert b"render_baked" in L.gi_last_error(rt.h)
        assert L.gi_render_baked_device(rt.h, C.byref(p), C.byref(q), C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), 1) == gi.GI_E_INVALID      # before a pointer is used
    assert L.gi_render_baked_host(rt.h, C.byref(p), C.byref(bp), None, dp(c), ptr, 1) == gi.GI_E_INVALID      # a set bit with a null pointer
    assert L.gi_render_baked_host(rt.h, C.byref(p), C.byref(bp), dp(s), None, ptr, 1) == gi.GI_E_INVALID
    assert L.gi_render_baked_host(rt.h, C.byref(p), C.byref(bp), dp(s), dp(c), None, 1) == gi.GI_E_INVALID
    assert L.gi_render_baked_host(rt.h, C.byref(p), None, dp(s), dp(c), ptr, 1) == gi.GI_E_INVALID
    assert L.gi_render_baked_host(rt.h, None, C.byref(bp), dp(s), dp(c), ptr, 1) == gi.GI_E_INVALID
    assert L.gi_render_baked_host(None, C.byref(p), C.byref(bp), dp(s), dp(c), ptr, 1) == gi.GI_E_INVALID
    assert L.gi_render_baked_device(rt.h, C.byref(p), C.byref(bp), C.c_void_p(16), C.c_void_p(16), None, 1) == gi.GI_E_INVALID
    assert L.gi_last_baked_ms(rt.h, None) == gi.GI_E_INVALID
    assert L.gi_render_baked_host(rt.h, C.byref(rt.params(0, 10)), C.byref(bp), dp(s), dp(c), ptr, 1) == gi.GI_E_INVALID
    big = rt.params(3840, 2160, stripe_h=8, rank=0, world=270)      # the Halton index: a 3840 x 2160 frame takes 479 samples
    out_big = np.full((8, 3840, 12), -7.0, np.float32)
    assert L.gi_render_baked_host(rt.h, C.byref(big), C.byref(variant(n_samples=480, terms=EMISSIVE)), None, None, out_big.ctypes.data_as(C.c_void_p), 0) == gi.GI_E_INVALID
    assert b"480" in L.gi_last_error(rt.h) and b"479" in L.gi_last_error(rt.h)
    with pytest.raises(ValueError):
        rt.run_baked(3840, 2160, 480)
    with pytest.raises(ValueError):
        rt.run_baked(W, H, 1, sh=sh)
    empty = gi.RayTracer(0)
    small = empty.params(W, H)
    assert L.gi_render_baked_host(empty.h, C.byref(small), C.byref(bp), dp(s), dp(c), ptr, 1) == gi.GI_E_STATE
    assert L.gi_render_baked_device(empty.h, C.byref(small), C.byref(bp), C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), 1) == gi.GI_E_STATE
    assert empty.last_baked_ms() == 0.0
    assert (out == -7.0).all() and (out_big == -7.0).all()
    # no refusal touched a timer: the pass's own keeps the good call's time, the frame's and the occlusion's keep theirs
    assert rt.last_baked_ms() == ms0 and rt.last_render_ms() == frame_ms and rt.last_occlusion_ms() == ao_ms
    assert L.gi_render_baked_host(rt.h, C.byref(p), C.byref(bp), dp(s), dp(c), ptr, 1) == gi.GI_OK and same(out, good["baked"])
    assert rt.last_baked_ms() > 0 and rt.last_render_ms() == frame_ms and rt.last_occlusion_ms() == ao_ms
    # an open progressive session is left alone
    kw = dict(min_samples=4, max_samples=4)
    before = rt.run(W, H, **kw)
    with rt.progressive(W, H, **kw) as sess:
        sess.step(2)
        end = sess.sample_end
        assert same(rt.run_baked(W, H, 1, sh=sh, grid_box=box, chain=inputs["chain"], exponents=be.CHAIN_EXPONENTS)["baked"], good["baked"])
        assert sess.sample_end == end and same(sess.step(2), before)


def test_device_entry_writes_what_the_host_entry_returns(setups, inputs):
    scene, rt, o, t = setups("cornell")
    p = rt.params(W, H)
    bp, s, c = rt.baked_params(n=N, sh=inputs["sh"][(2, 2, 2)], grid_box=be.inner_box(t), chain=inputs["chain"], exponents=be.CHAIN_EXPONENTS)
    want = rt.run_baked(W, H, N, sh=inputs["sh"][(2, 2, 2)], grid_box=be.inner_box(t), chain=inputs["chain"], exponents=be.CHAIN_EXPONENTS, f64=False)["baked"]
    hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")      # device buffers from the HIP runtime the library itself uses (no second runtime in this process)
    bufs = []
    try:
        for a in (s, c, np.full((H, W, 12), -7.0, np.float32)):
            d = C.c_void_p()
            assert hip.hipMalloc(C.byref(d), C.c_size_t(a.nbytes)) == 0
            bufs.append(d)
            assert hip.hipMemcpy(d, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0      # hipMemcpyHostToDevice
        rt.run_baked_device(p, bp, bufs[0].value, bufs[1].value, bufs[2].value, f64=False)
        assert rt.last_baked_ms() > 0                                                  # waits for the pass
        got = np.zeros((H, W, 12), np.float32)
        assert hip.hipDeviceSynchronize() == 0
        assert hip.hipMemcpy(got.ctypes.data_as(C.c_void_p), bufs[2], C.c_size_t(got.nbytes), 2) == 0      # hipMemcpyDeviceToHost
    finally:
        for d in bufs:
            assert hip.hipFree(d) == 0
    assert same(got, want)


# ---------------------------------------------------------------------------------------------------------------- 6. end to end
def test_bakes_feed_the_pass_end_to_end(setups):
    scene, rt, o, t = setups("box")
    box = t["node_bbox"][0]
    sh = rt.bake_probes(gi.probe_grid(box, 2, 2, 2).reshape(-1, 3), 64).reshape(2, 2, 2, 9, 3)
    chain = rt.bake_reflection_probe([0.0, 0.0, 0.0], 8, 16, 3, exponents=be.CHAIN_EXPONENTS)
    got = rt.run_baked(W, H, N, sh=sh, grid_box=box, chain=chain, exponents=be.CHAIN_EXPONENTS)
    cov = rt.run_features(W, H, N, want_ids=False)["coverage"]
    assert np.isfinite(got["baked"]).all() and (cov == 1).all()
    assert (got["diffuse"][cov == 1] > 0).all()                       # a white diffuse box, lit from inside
    assert not got["specular"].any()                                  # nothing in it is glossy
    ref = rt.run(W, H, min_samples=16, max_samples=16)
    print(f"closed box: mean beauty {got['beauty'].mean():.6f} (direct {got['direct'].mean():.6f}, diffuse {got['diffuse'].mean():.6f}), "
          f"mean of the 16-spp path-traced frame {ref.mean():.6f}, ratio {got['beauty'].mean() / ref.mean():.4f}")


def test_cli_writes_the_preview_and_its_terms(tmp_path, capsys):
    import os
    from gi_raytracer_amd import __main__ as cli
    scn = os.path.join(pc.ROOT, pc.SCN["cornell"])
    assert cli.main([scn, "-o", str(tmp_path / "out.ppm"), "--width", "24", "--height", "16", "--samples", "1", "--photons", "0", "--baked", str(tmp_path / "lit"),
                     "--baked-samples", "2", "--baked-probes", "2", "1", "2"]) == 0
    assert sorted(os.listdir(tmp_path)) == ["lit.ppm", "lit_diffuse.pfm", "lit_direct.pfm", "lit_specular.pfm", "out.ppm"]
    assert "baked light" in capsys.readouterr().out
    assert open(tmp_path / "lit.ppm", "rb").read(2) == b"P6"
    d = fe.read_pfm(tmp_path / "lit_diffuse.pfm")
    assert d.shape == (16, 24, 3) and np.isfinite(d).all() and (d > 0).any()
