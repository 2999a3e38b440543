"""Probe visibility (gi_probe_visibility_*, k_pv_capture; gi_render_baked_visibility_*, the PV instances of k_lit) on the GPU, through the C ABI via
the Python mirror.

What is exact and what has an allowance:
 * the capture's rays and its fold equal the numpy statement (tests/visibility_expect.py) bit for bit;
 * on scenes whose alpha test cannot depend on the draw, a map texel equals the statement fed by Oracle.trace bit for bit wherever the device's hit
   entity is the oracle's (gi_trace on the same rays tells); a ray that grazes an edge may pick the neighbour -- at most 1 ray in 1 000 may
   (tests/test_visibility_cpu.py shows on the CPU that at these probe positions a 4-ulp move of the direction flips none; the count is printed);
 * given the oracle's first hits, the look-up's diffuse term equals the statement bit for bit; the other terms are run_baked's bits;
 * every identity (split point lists, walk variants, pool size, repetition, f32, stripes, a null map) is exact, bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

import gi_raytracer_amd as gi

import baked_expect as be
import features_expect as fe
import parity_checks as pc
import visibility_expect as ve

pytestmark = pytest.mark.gpu

W, H = 24, 16
SIZES = ((13, 9), (24, 16))
N = 2
DIRECT, DIFFUSE, SPECULAR, EMISSIVE = be.DIRECT, be.DIFFUSE, be.SPECULAR, be.EMISSIVE


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def diagonal(t):
    b = t["node_bbox"][0]
    return float(np.sqrt(((b[3] - b[0]) ** 2 + (b[4] - b[1]) ** 2) + (b[5] - b[2]) ** 2))


@pytest.fixture(scope="module")
def plain():
    """The scene files as they are: (scene, tracer, oracle, tables) by name."""
    cache = {}

    def get(name):
        if name not in cache:
            scene = pc.named_scene(name)
            cache[name] = (scene, gi.RayTracer(0).setScene(scene), pc.oracle_for(scene) if name in fe.DRAW_FREE_SCENES else None, scene.tables())
        return cache[name]

    return get


@pytest.fixture(scope="module")
def setups():
    """The scene files with their materials cycled through the three lobes, as tests/test_gpu_baked.py sets them up."""
    cache = {}

    def get(name):
        if name not in cache:
            base = pc.named_scene(name)
            scene = be.with_roughnesses(base)
            rt = gi.RayTracer(0).setScene(scene)
            rt._adopt(base.settings)
            cache[name] = (scene, rt, be.oracle_with_camera(scene, base.settings), scene.tables())
        return cache[name]

    return get


@pytest.fixture(scope="module")
def inputs():
    return {"sh": {g: be.random_sh(g, 100 + k) for k, g in enumerate(be.GRIDS)}, "chain": be.random_chain(7)}


# ---------------------------------------------------------------------------------------------------------------- 1. rays, 2. fold
@pytest.mark.parametrize("M", [1, 3, 8])
def test_rays_equal_the_statement_bit_for_bit(M):
    rt = gi.RayTracer(0)                                   # no scene is needed
    rs = np.random.default_rng(5)
    for n_points in (1, 5) + ((24,) if M == 8 else ()):    # 5 x 9 = 45 texels: less than a wave; 24 x 64 = 1536: several workgroups
        P = rs.uniform(-3.0, 3.0, (n_points, 3))
        for ns, base in ((1, 0), (3, 1000)):
            rays, st = rt.probe_visibility_rays(P, M, ns, stream_base=base)
            want, want_st = ve.capture_rays(P, M, ns, base)
            assert same(st, want_st) and same(rays, want), (M, n_points, ns)


def test_fold_equals_the_statement_bit_for_bit():
    rt = gi.RayTracer(0)
    rs = np.random.default_rng(6)
    for ns in (1, 2, 17):
        d = rs.uniform(0.0, 30.0, (300, ns)) * 10.0 ** rs.integers(-3, 3, (300, 1))
        assert same(rt.probe_visibility_fold(d), ve.fold(d)), ns


# ---------------------------------------------------------------------------------------------------------------- 3. the capture on draw-free scenes
@pytest.mark.parametrize("name", ["cornell", "test_scene", "spheres_opaque"])
def test_capture_matches_the_statement_on_the_oracle_s_hits(plain, name):
    scene, rt, o, t = plain(name)
    points = ve.probe_points(t)
    far = diagonal(t)
    differ = asked = 0
    for M in (3, 8):
        want, rays, (hit, ent, res) = ve.expected_maps(o, points, M, 2, far)
        assert fe.oracle_is_draw_free(o, rays)
        got = rt.bake_probe_visibility(points, M, 2, max_dist=far)
        assert got.shape == (len(points), M, M, 2) and got.dtype == np.float64
        assert same(rt.bake_probe_visibility(points, M, 2), got)                       # max_dist None: the scene's diagonal
        dhit, dent, _ = rt.trace(rays)
        agree = ((dhit == hit) & ((hit == 0) | (dent == ent))).reshape(-1, 2).all(1).reshape(len(points), M, M)
        differ += int((~((dhit == hit) & ((hit == 0) | (dent == ent)))).sum()); asked += len(rays)
        assert (got[agree].view(np.uint64) == want[agree].view(np.uint64)).all(), (name, M)
        # misses equal max_dist exactly: a texel whose two rays both miss holds (far, far * far)
        missed = (hit == 0).reshape(-1, 2).all(1).reshape(len(points), M, M) & agree
        assert missed.any() and (got[missed][:, 0] == far).all() and (got[missed][:, 1] == (far * far + far * far) / 2.0).all()
        assert (got[..., 0] <= far).all() and (got[..., 0] > 0).all() and (got[..., 1] >= got[..., 0] ** 2 * (1 - 1e-15)).all()
        # a small max_dist clamps hits
        near = 0.25 * far
        want_near = ve.fold(ve.distances(hit, res, rays, near).reshape(-1, 2)).reshape(-1, M, M, 2)
        got_near = rt.bake_probe_visibility(points, M, 2, max_dist=near)
        assert (got_near[agree].view(np.uint64) == want_near[agree].view(np.uint64)).all() and (got_near[..., 0] == near).any() and (got_near[..., 0] < near).any()
    print(f"{name}: {differ} of {asked} capture rays meet another entity on the device than in the oracle")
    assert differ * 1000 <= asked


# ---------------------------------------------------------------------------------------------------------------- 4. the capture's identities
def test_capture_identities_bit_for_bit(plain):
    scene, rt, o, t = plain("cornell")
    points = ve.probe_points(t)
    M, ns, base = 8, 3, 77
    rt.run(W, H, min_samples=1, max_samples=1)
    rt.bake_probes(points[:2], 4)
    rt.run_baked(W, H, 1)
    times = (rt.last_render_ms(), rt.last_bake_ms(), rt.last_baked_ms())
    assert times[0][0] > 0 and times[1] > 0 and times[2] > 0
    full = rt.bake_probe_visibility(points, M, ns, stream_base=base)
    assert rt.last_probe_visibility_ms() > 0
    assert same(rt.bake_probe_visibility(points, M, ns, stream_base=base), full)                                # repetition
    for cut in (1, 4):                                                                                          # the list split in two calls
        a = rt.bake_probe_visibility(points[:cut], M, ns, stream_base=base)
        b = rt.bake_probe_visibility(points[cut:], M, ns, stream_base=base + cut * M * M * ns)
        assert same(np.concatenate([a, b]), full), cut
    f32 = rt.bake_probe_visibility(points, M, ns, stream_base=base, f64=False)
    assert f32.dtype == np.float32 and same(f32, full.astype(np.float32))
    try:
        rt.set_wide_nodes(False)
        assert same(rt.bake_probe_visibility(points, M, ns, stream_base=base), full)
    finally:
        rt.set_wide_nodes(True)
    try:
        rt.set_pool_slots(64)
        assert same(rt.bake_probe_visibility(points, M, ns, stream_base=base), full)
    finally:
        rt.set_pool_slots(1 << 30)
    assert not same(rt.bake_probe_visibility(points, M, ns, stream_base=base + 1), full)
    assert (rt.last_render_ms(), rt.last_bake_ms(), rt.last_baked_ms()) == times                                 # frame, bake and baked timers untouched


def test_capture_on_an_alpha_scene_is_the_same_across_repeats_and_walks():
    scene = pc.large_alpha_scene()
    rt = gi.RayTracer(0).setScene(scene)
    points = ve.probe_points(scene.tables())
    full = rt.bake_probe_visibility(points, 8, 3, seed=1234)
    assert np.isfinite(full).all() and same(rt.bake_probe_visibility(points, 8, 3, seed=1234), full)
    try:
        rt.set_wide_nodes(False)
        assert same(rt.bake_probe_visibility(points, 8, 3, seed=1234), full)
    finally:
        rt.set_wide_nodes(True)
    assert not same(rt.bake_probe_visibility(points, 8, 3, seed=99), full)                                      # the alpha draws are keyed by the seed


# ---------------------------------------------------------------------------------------------------------------- 5. the look-up
@pytest.mark.parametrize("name", ["cornell", "spheres_opaque", "test_scene"])
def test_lookup_matches_the_statement(setups, inputs, name):
    scene, rt, o, t = setups(name)
    assert name in fe.DRAW_FREE_SCENES and fe.oracle_is_draw_free(o, fe.sample_rays(o, W, H, 0)[0])
    geo = [be.sample_hits(o, t, W, H, s) for s in range(N)]
    f1 = rt.run_features(W, H, 1)
    assert np.array_equal(f1["ids"][:, :, 0], geo[0]["ent"].reshape(H, W))                                      # identical first hits
    box, chain = be.inner_box(t), inputs["chain"]
    scale = 0.5 * diagonal(t)
    behind = front = 0
    for k, grid in enumerate(be.GRIDS):
        sh = inputs["sh"][grid]
        kw = dict(sh=sh, grid_box=box, chain=chain, exponents=be.CHAIN_EXPONENTS, terms=15)
        ref1, ref = rt.run_baked(W, H, 1, **kw), rt.run_baked(W, H, N, **kw)
        for M in (3, 8):
            vis = ve.random_vis(grid, M, 200 + 10 * k + M, scale)
            assert (vis[..., 1] >= vis[..., 0] ** 2).all()
            for bias in (0.0, 0.01):
                per = [ve.sample_diffuse(g, t, sh, vis, box, bias) for g in geo]
                got1 = rt.run_baked_visibility(W, H, 1, vis, normal_bias=bias, **kw)
                got = rt.run_baked_visibility(W, H, N, vis, normal_bias=bias, **kw)
                assert same(np.ascontiguousarray(got1["diffuse"]), be.fold(per[:1]).reshape(H, W, 3)), (name, grid, M, bias)
                assert same(np.ascontiguousarray(got["diffuse"]), be.fold(per).reshape(H, W, 3)), (name, grid, M, bias)
                assert (got["diffuse"] > 0).any() and not same(np.ascontiguousarray(got["diffuse"]), np.ascontiguousarray(ref["diffuse"]))
                for a, b in ((got1, ref1), (got, ref)):                                                          # the other terms are run_baked's
                    assert all(same(np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])) for key in ("direct", "specular"))
                # beauty is the documented sum; with one sample: ((direct + diffuse) + specular) + emissive, the ambient colour on a miss
                em = rt.run_baked(W, H, 1, terms=EMISSIVE)["beauty"]
                miss = ~geo[0]["hit"].reshape(H, W, 1)
                assert same(np.ascontiguousarray(got1["beauty"]), np.where(miss, t["ambient"], ((got1["direct"] + got1["diffuse"]) + got1["specular"]) + np.where(miss, 0.0, em)))
            sel = geo[0]["hit"] & (be.lobe_of(t["mats"][np.where(geo[0]["hit"], geo[0]["mat"], 0), 0]) == 2)
            _, _, _, _, r, m = ve.corner_weights(vis, box, geo[0]["P"][sel], geo[0]["Nf"][sel])
            behind += int((r > m).sum()); front += int((r <= m).sum())
    assert behind > 0 and front > 0, (behind, front)


# ---------------------------------------------------------------------------------------------------------------- 6. the look-up's identities
def test_lookup_identities_bit_for_bit(setups, inputs):
    scene, rt, o, t = setups("cornell")
    grid = (3, 2, 4)
    sh, box, chain = inputs["sh"][grid], be.inner_box(t), inputs["chain"]
    kw = dict(sh=sh, grid_box=box, chain=chain, exponents=be.CHAIN_EXPONENTS)
    vis = ve.random_vis(grid, 8, 300, 0.5 * diagonal(t))
    ent, uv = gi.chart_of_material(scene)
    atlas = np.random.default_rng(8).uniform(0.0, 1.0, (8, 8, 3))
    for (w, h) in SIZES:
        before = rt.run_baked(w, h, N, **kw)["baked"]
        before_lm = rt.run_baked_lightmap(w, h, N, atlas, ent, uv, **kw)["baked"]
        assert same(rt.run_baked_visibility(w, h, N, None, **kw)["baked"], before)                              # a null map: run_baked's bytes
        assert same(rt.run_baked_visibility(w, h, N, vis, terms=DIRECT | SPECULAR | EMISSIVE, **kw)["baked"], rt.run_baked(w, h, N, terms=DIRECT | SPECULAR | EMISSIVE, **kw)["baked"])
        full = rt.run_baked_visibility(w, h, N, vis, **kw)["baked"]
        assert np.isfinite(full).all() and not same(full, before)
        assert same(rt.run_baked_visibility(w, h, N, vis, **kw)["baked"], full)                                 # repetition
        assert same(rt.run_baked_visibility(w, h, N, vis.astype(np.float32).astype(np.float64), **kw)["baked"], rt.run_baked_visibility(w, h, N, vis.astype(np.float32), **kw)["baked"])
        assert same(rt.run_baked(w, h, N, **kw)["baked"], before) and same(rt.run_baked_lightmap(w, h, N, atlas, ent, uv, **kw)["baked"], before_lm)      # as before
        f32 = rt.run_baked_visibility(w, h, N, vis, f64=False, **kw)["baked"]
        assert f32.dtype == np.float32 and same(f32, full.astype(np.float32))
        frame = np.full_like(full, -7.0)
        for rank in range(2):
            part = rt.run_baked_visibility(w, h, N, vis, stripe_h=4, rank=rank, world=2, **kw)["baked"]
            frame[fe.frame_rows(h, 4, rank, 2)] = part
        assert same(frame, full)
        try:
            rt.set_wide_nodes(False)
            assert same(rt.run_baked_visibility(w, h, N, vis, **kw)["baked"], full)
        finally:
            rt.set_wide_nodes(True)


# ---------------------------------------------------------------------------------------------------------------- 7. end to end
def test_maps_keep_the_light_in_its_room_end_to_end():
    scene = ve.two_room_scene(gi)
    rt, o, t = gi.RayTracer(0).setScene(scene), pc.oracle_for(scene), scene.tables()
    nx, ny, nz = ve.ROOM_GRID
    box = ve.room_box()
    points = gi.probe_grid(box, nx, ny, nz).reshape(-1, 3)
    assert points[1, 0] < ve.WALL_X < points[2, 0]                                                              # the grid straddles the wall
    sh = rt.bake_probes(points, 256).reshape(nz, ny, nx, 9, 3)
    vis = rt.bake_probe_visibility(points, 8, 16).reshape(nz, ny, nx, 8, 8, 2)
    assert sh[0, 0, 1, 0].min() > 10 * max(sh[0, 0, 2, 0].max(), 0.0)                                           # room A is lit, room B is dark
    w, h = 24, 16
    got = rt.run_baked_visibility(w, h, 1, vis, sh=sh, grid_box=box, terms=DIFFUSE)["diffuse"]
    plain = rt.run_baked(w, h, 1, sh=sh, grid_box=box, terms=DIFFUSE)["diffuse"]
    g = be.sample_hits(o, t, w, h, 0)
    assert np.array_equal(rt.run_features(w, h, 1)["ids"][:, :, 0], g["ent"].reshape(h, w))
    want = ve.sample_diffuse(g, t, sh, vis, box)
    assert same(np.ascontiguousarray(got), want.reshape(h, w, 3))                                                # the statement on the device's own bakes
    cell = (box[3] - box[0]) / nx
    near = (g["hit"] & (g["ent"] < 2) & (g["P"][:, 0] > ve.WALL_X + ve.WALL_HALF) & (g["P"][:, 0] < ve.WALL_X + cell)).reshape(h, w)      # room B's floor by the wall
    assert near.sum() >= 8
    print(f"two rooms: diffuse over {int(near.sum())} room-B floor pixels within one cell of the wall: {plain[near].sum():.6f} without maps, {got[near].sum():.6f} with")
    assert got[near].sum() < plain[near].sum() and plain[near].sum() > 0


def test_cli_bakes_and_uses_the_maps(tmp_path, capsys):
    from gi_raytracer_amd import __main__ as cli
    scn = os.path.join(pc.ROOT, pc.SCN["cornell"])
    assert cli.main([scn, "-o", str(tmp_path / "out.ppm"), "--width", "24", "--height", "16", "--samples", "1", "--photons", "0", "--baked", str(tmp_path / "lit"),
                     "--baked-samples", "2", "--baked-probes", "2", "2", "2", "--probe-visibility", "4"]) == 0
    assert "visibility maps 4x4" in capsys.readouterr().out
    d = fe.read_pfm(tmp_path / "lit_diffuse.pfm")
    assert d.shape == (16, 24, 3) and np.isfinite(d).all() and (d > 0).any()


# ---------------------------------------------------------------------------------------------------------------- 8. refusals
def test_capture_refusals_leave_the_output_and_the_timers_alone(plain):
    scene, rt, o, t = plain("cornell")
    L = rt.L
    points = ve.probe_points(t)
    rt.run(W, H, min_samples=1, max_samples=1)
    good = rt.bake_probe_visibility(points, 3, 2)
    ms0, frame_ms = rt.last_probe_visibility_ms(), rt.last_render_ms()
    assert ms0 > 0
    out = np.full((len(points), 3, 3, 2), -7.0)
    ptr = out.ctypes.data_as(C.c_void_p)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rays, st = np.full((len(points) * 9 * 2, 6), -7.0), np.full(len(points) * 9 * 2, 7, np.uint32)
    good_p = rt.probe_visibility_params(3, 2)

    def variant(**kw):
        q = gi.ProbeVisibilityParams.from_buffer_copy(good_p)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    n = len(points)
    bad = [(variant(size=0), n), (variant(size=65), n), (variant(size=-1), n), (variant(n_samples=0), n), (good_p, -1), (variant(max_dist=0.0), n), (variant(max_dist=-1.0), n),
           (variant(max_dist=float("inf")), n), (variant(max_dist=float("nan")), n), (variant(stream_base=2 ** 32 - 100), n), (variant(size=64, n_samples=2 ** 20), n),
           (variant(size=64, n_samples=2 ** 31 - 1), 2 ** 31 - 1)]      # (the last: the product is beyond 64 bits)
    for q, k in bad:
        assert L.gi_probe_visibility_host(rt.h, dp(points), k, C.byref(q), ptr, 1) == gi.GI_E_INVALID, bytes(q)
        assert b"probe_visibility" in L.gi_last_error(rt.h)
        assert L.gi_probe_visibility_device(rt.h, C.c_void_p(16), k, C.byref(q), C.c_void_p(16), 1) == gi.GI_E_INVALID      # before a pointer is used
        assert L.gi_probe_visibility_rays(rt.h, dp(points), k, C.byref(q), dp(rays), st.ctypes.data_as(C.POINTER(C.c_uint32))) == gi.GI_E_INVALID
    assert L.gi_probe_visibility_host(rt.h, dp(points), n, None, ptr, 1) == gi.GI_E_INVALID
    assert L.gi_probe_visibility_host(rt.h, None, n, C.byref(good_p), ptr, 1) == gi.GI_E_INVALID
    assert L.gi_probe_visibility_host(rt.h, dp(points), n, C.byref(good_p), None, 1) == gi.GI_E_INVALID
    assert L.gi_probe_visibility_host(None, dp(points), n, C.byref(good_p), ptr, 1) == gi.GI_E_INVALID
    assert L.gi_probe_visibility_device(rt.h, None, n, C.byref(good_p), C.c_void_p(16), 1) == gi.GI_E_INVALID
    assert L.gi_last_probe_visibility_ms(rt.h, None) == gi.GI_E_INVALID
    for k in range(3):                                                                       # the host entries look at the positions
        nan = points.copy()
        nan[2, k] = (float("nan"), float("inf"), -float("inf"))[k]
        assert L.gi_probe_visibility_host(rt.h, dp(nan), n, C.byref(good_p), ptr, 1) == gi.GI_E_INVALID and b"probe_visibility" in L.gi_last_error(rt.h)
        assert L.gi_probe_visibility_rays(rt.h, dp(nan), n, C.byref(good_p), dp(rays), st.ctypes.data_as(C.POINTER(C.c_uint32))) == gi.GI_E_INVALID
    assert L.gi_probe_visibility_fold(rt.h, 4, 0, dp(rays), dp(out)) == gi.GI_E_INVALID and L.gi_probe_visibility_fold(rt.h, -1, 2, dp(rays), dp(out)) == gi.GI_E_INVALID
    assert L.gi_probe_visibility_fold(rt.h, 4, 2, None, dp(out)) == gi.GI_E_INVALID and b"probe_visibility_fold" in L.gi_last_error(rt.h)
    empty = gi.RayTracer(0)
    assert L.gi_probe_visibility_host(empty.h, dp(points), n, C.byref(good_p), ptr, 1) == gi.GI_E_STATE and b"probe_visibility" in L.gi_last_error(empty.h)
    assert L.gi_probe_visibility_device(empty.h, C.c_void_p(16), n, C.byref(good_p), C.c_void_p(16), 1) == gi.GI_E_STATE
    assert empty.last_probe_visibility_ms() == 0.0
    assert (out == -7.0).all() and (rays == -7.0).all() and (st == 7).all()
    assert rt.last_probe_visibility_ms() == ms0 and rt.last_render_ms() == frame_ms                # no refusal touched a timer
    assert L.gi_probe_visibility_host(rt.h, dp(points), 0, C.byref(good_p), ptr, 1) == gi.GI_OK and (out == -7.0).all()      # no points: nothing written
    assert L.gi_probe_visibility_host(rt.h, dp(points), n, C.byref(good_p), ptr, 1) == gi.GI_OK and same(out, good)
    # an open progressive session is left alone
    kw = dict(min_samples=4, max_samples=4)
    before = rt.run(W, H, **kw)
    with rt.progressive(W, H, **kw) as sess:
        sess.step(2)
        end = sess.sample_end
        assert same(rt.bake_probe_visibility(points, 3, 2), good)
        assert sess.sample_end == end and same(sess.step(2), before)


def test_lookup_refusals_leave_the_output_and_the_timers_alone(setups, inputs):
    scene, rt, o, t = setups("cornell")
    L = rt.L
    p = rt.params(W, H)
    grid = (2, 2, 2)
    sh, box = inputs["sh"][grid], be.inner_box(t)
    vis = ve.random_vis(grid, 3, 9, 1.0)
    rt.run(W, H, min_samples=1, max_samples=1)
    good = rt.run_baked_visibility(W, H, 1, vis, sh=sh, grid_box=box, chain=inputs["chain"], exponents=be.CHAIN_EXPONENTS)
    ms0, frame_ms = rt.last_baked_ms(), rt.last_render_ms()
    assert ms0 > 0
    bp, s, c = rt.baked_params(n=1, sh=sh, grid_box=box, chain=inputs["chain"], exponents=be.CHAIN_EXPONENTS)
    vp, v = gi.baked_visibility_params(vis, sh.shape[:3])
    out = np.full((H, W, 12), -7.0)
    ptr = out.ctypes.data_as(C.c_void_p)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    vptr = v.ctypes.data_as(C.c_void_p)

    def variant(block, **kw):
        q = type(block).from_buffer_copy(block)
        for k, val in kw.items():
            setattr(q, k, val)
        return q

    def host(bp_=bp, vp_=vp, s_=s, c_=c, v_=vptr, o_=ptr, p_=p, h_=None):
        return L.gi_render_baked_visibility_host(h_ or rt.h, C.byref(p_) if p_ is not None else None, C.byref(bp_) if bp_ is not None else None,
                                                 C.byref(vp_) if vp_ is not None else None, dp(s_) if s_ is not None else None, dp(c_) if c_ is not None else None, v_, 1, o_, 1)

    for q in (variant(vp, size=0), variant(vp, size=65), variant(vp, normal_bias=-1.0), variant(vp, normal_bias=float("inf")), variant(vp, normal_bias=float("nan")),
              variant(vp, vis_floor=0.0), variant(vp, vis_floor=-0.5), variant(vp, vis_floor=1.5), variant(vp, vis_floor=float("nan"))):
        assert host(vp_=q) == gi.GI_E_INVALID and b"render_baked_visibility" in L.gi_last_error(rt.h), bytes(q)
        assert L.gi_render_baked_visibility_device(rt.h, C.byref(p), C.byref(bp), C.byref(q), C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), 1) == gi.GI_E_INVALID
    for q in (variant(bp, n_samples=0), variant(bp, terms=0), variant(bp, terms=16), variant(bp, nx=0), variant(bp, face=0), variant(bp, levels=13)):      # what gi_render_baked_* refuses
        assert host(bp_=q) == gi.GI_E_INVALID and b"render_baked_visibility" in L.gi_last_error(rt.h), bytes(q)[:16]
    assert host(vp_=None) == gi.GI_E_INVALID and b"render_baked_visibility" in L.gi_last_error(rt.h)
    assert host(bp_=None) == gi.GI_E_INVALID and host(p_=None) == gi.GI_E_INVALID and host(o_=None) == gi.GI_E_INVALID
    assert host(s_=None) == gi.GI_E_INVALID and b"render_baked_visibility" in L.gi_last_error(rt.h)      # a map and the diffuse term, no grid
    assert host(s_=None, v_=None) == gi.GI_E_INVALID and host(c_=None) == gi.GI_E_INVALID
    assert L.gi_render_baked_visibility_host(None, C.byref(p), C.byref(bp), C.byref(vp), dp(s), dp(c), vptr, 1, ptr, 1) == gi.GI_E_INVALID
    empty = gi.RayTracer(0)
    assert host(h_=empty.h, p_=empty.params(W, H)) == gi.GI_E_STATE and b"render_baked_visibility" in L.gi_last_error(empty.h)
    assert empty.last_baked_ms() == 0.0
    with pytest.raises(ValueError):
        rt.run_baked_visibility(W, H, 1, vis)                                                # maps without their grid
    with pytest.raises(ValueError):
        rt.run_baked_visibility(W, H, 1, vis, sh=inputs["sh"][(3, 2, 4)], grid_box=box)      # maps of another grid
    assert (out == -7.0).all()
    assert rt.last_baked_ms() == ms0 and rt.last_render_ms() == frame_ms
    assert host() == gi.GI_OK and same(out, good["baked"]) and rt.last_baked_ms() > 0 and rt.last_render_ms() == frame_ms
