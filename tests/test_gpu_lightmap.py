"""Lightmap atlases (gi_lightmap_*: k_lm_raster, k_lm_point, the rank, k_lm_scatter, k_lm_dilate around the bake) on the GPU, through the C ABI via
the Python mirror.  The expectation is tests/lightmap_expect.py; every comparison is equality of bytes:
 * the texel table (owner, n_covered, points, texel) is the numpy statement's;
 * the dilation entry is the numpy dilation;
 * the atlas is scatter + dilation (statement) of RayTracer.bake_texels on the texel table -- the existing entry is the yardstick -- and, on the
   floor scene, where every ray meets nothing whatever its last bits, of the oracle's bake;
 * chunked bakes, f32, the device entry, frames, timers and sessions left alone: exact."""
import ctypes as C
import os

import numpy as np
import pytest

import gi_raytracer_amd as gi

import bake_expect as be
import lightmap_expect as le
import parity_checks as pc

pytestmark = pytest.mark.gpu

SEEDS = (be.DEFAULT_SEED, 12345)
BASE = 1000
AMBIENT = (0.25, 0.5, 0.125)
UP, DOWN = (0.0, 1.0, 0.0), (0.0, -1.0, 0.0)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def hand_scene():
    """Entities 0, 1: the quad of test_lightmap_cpu with normals that cancel on row 0; 2, 3: the same quad lifted, flat; 4: a sphere."""
    s = gi.Scene()
    m = s.add_material(1, 1, 1, (0.8, 0.8, 0.8))
    a, b, c, d = (0.0, 0.0, 0.0), (2.0, 0.0, 0.0), (2.0, 0.0, 4.0), (0.0, 0.0, 4.0)
    s.add_triangles(np.array([[a, b, c], [a, c, d]]), nrm=np.array([[UP, DOWN, DOWN], [UP, UP, UP]]), mat_idx=[m, m])
    lift = np.array([0.0, 1.0, 0.0])
    s.add_triangles(np.array([[a, b, c], [a, c, d]]) + lift, mat_idx=[m, m])
    s.add_sphere((1.0, 3.0, 1.0), 0.5, m)
    s.add_light((0, 20, 0), (1, 1, 1), 0.1)
    s.set_ambient(AMBIENT)
    s.set_camera((0.3, 6.0, 4.0), (0, 0, 0))
    return s.rebuild()


@pytest.fixture(scope="module")
def setups(golden):
    cache = {}

    def get(name):
        if name not in cache:
            scene = hand_scene() if name == "hand" else (be.ambient_floor_scene(gi, AMBIENT) if name == "floor" else pc.load_scene(name))
            rt = gi.RayTracer(0).setScene(scene)
            if name == "caustics":
                scene.build_photon_map(golden("scene_caustics")["photons"])
                rt.upload_photon_map()
            t = scene.tables()
            ent, uv = le.random_chart(len(t["tri_pos"]), 7) if name in ("cornell", "caustics") else (np.array([0, 1], np.int32), le.QUAD)
            cache[name] = {"scene": scene, "rt": rt, "t": t, "ent": ent, "uv": uv}
        return cache[name]

    return get


def timers(rt):
    return rt.last_kernel_ms(), (rt.last_render_ms(), rt.last_bake_ms(), rt.last_lightmap_ms())


def same_timers(a, b):
    """Every time bit for bit: the frame's per-stage times, the frame's, the bake's, the lightmap's."""
    return a == b


def hip_runtime():
    """The HIP runtime the library itself is linked against and has loaded (no second runtime in this process): by its soname, which the loader
    resolves to the copy already in memory; else under ROCM_PATH."""
    gi.lib()
    try:
        return C.CDLL("libamdhip64.so")
    except OSError:
        return C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))


def check_table(s, ent, uv, w, h, flip=False):
    got = s["rt"].lightmap_texels(ent, uv, w, h, flip=flip)
    want = le.texel_table(s["t"], ent, uv, w, h, flip)
    assert same(got[0], want[0]), "owner"
    assert len(got[3]) == len(want[3]) and same(got[3], want[3]), "texel"
    assert same(got[1], want[1]) and same(got[2], want[2]), "points"
    return got


def expected_atlas(s, ent, uv, w, h, ns, dilate=2, flip=False, stream_base=0, seed=None):
    rt = s["rt"]
    return le.lightmap(lambda P, N: rt.bake_texels(P, N, ns, stream_base=stream_base, seed=seed), s["t"], ent, uv, w, h, dilate, flip)


# ---------------------------------------------------------------------------------------------------------------- 1. the texel table
def test_texel_table_of_the_hand_charts_is_the_statement(setups):
    s = setups("hand")
    half = np.array([[[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]], [[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]]])
    sliver = np.array([[[0.0, 0.51], [1.0, 0.51], [1.0, 0.52]]])
    line = np.array([[[0.1, 0.1], [0.5, 0.5], [0.9, 0.9]], [[0.2, 0.2], [0.2, 0.2], [0.9, 0.1]]])
    big = np.array([[[-1.0, -1.0], [3.0, -1.0], [-1.0, 3.0]]])
    small = np.array([[[0.25, 0.25], [0.75, 0.25], [0.25, 0.75]]])
    far = le.QUAD * 2.0 ** 22 - 2.0 ** 21                              # coordinates beyond the rasteriser's box arithmetic: the whole atlas is tested
    for w, h in ((8, 8), (7, 5), (16, 16), (1, 1)):
        o = check_table(s, [2, 3], le.QUAD, w, h)[0]
        assert (o >= 0).all()
        if w == h:
            assert (np.diag(o) == 0).all()                             # centres exactly on the shared edge
        assert (np.diag(check_table(s, [3, 2], le.QUAD[::-1], w, h)[0]) == 0).all()
        check_table(s, [2, 3], le.QUAD[:, [0, 2, 1]], w, h)
        check_table(s, [2, 3], le.QUAD, w, h, flip=True)
        assert (check_table(s, [2], sliver, w, h)[0] == -1).all() or h != 8     # no centre row of 8 lies between 0.51 and 0.52
        assert (check_table(s, [2, 3], line, w, h)[0] == -1).all()
        assert (check_table(s, [2], big, w, h)[0] == 0).all()
        assert (check_table(s, [2, 3], le.QUAD + 1.0, w, h)[0] == -1).all()
        check_table(s, [2, 3], np.concatenate([small, big[:1] * 0.25 + 0.1]), w, h)
        check_table(s, [3, 2], np.concatenate([big[:1] * 0.25 + 0.1, small]), w, h)
        check_table(s, [2, 3, 2], np.concatenate([le.QUAD[::-1], le.QUAD[1:]]), w, h)
        assert (check_table(s, [2, 3], far, w, h)[0] >= 0).all()
        check_table(s, [0, 1], half, w, h)                             # interpolated normals
    o = check_table(s, [0, 1], half, 4, 4)[0]                          # where they cancel the texel is not covered, and row 1 does not inherit it
    assert o[0, 1] == -1 and o[1, 0] == -1 and o[0, 0] == 0 and (o[3, 1:] == -1).all()


@pytest.mark.parametrize("size", [(32, 32), (7, 5), (8, 8)])
def test_rows_collinear_up_to_an_ulp_end_at_their_chart_box(setups, size):
    s = setups("hand")
    w, h = size
    o = check_table(s, [2], le.REVIEW_SLIVER, 32, 32)[0]
    assert [tuple(p) for p in np.argwhere(o == 0)] == [(k, k) for k in range(3, 9)]       # not (11, 11) .. (15, 15), which the edge values alone accept
    uv = le.sliver_rows(w, h, 11)
    ent = np.tile(np.array([2, 3], np.int32), len(uv) // 2)
    got = check_table(s, ent, uv, w, h)                                                    # 400 rows at once: the lowest wins
    assert len(got[3]) > 0
    for j in (0, 1, 2, 200, 201, 202):                                                     # and one at a time, on the diagonal and on a row of centres
        check_table(s, ent[j:j + 1], uv[j:j + 1], w, h)
    check_table(s, ent[::-1].copy(), uv[::-1].copy(), w, h, flip=True)


@pytest.mark.parametrize("size", [(32, 32), (7, 5)])
def test_texel_table_of_a_random_chart_of_every_triangle(setups, size):
    s = setups("cornell")
    w, h = size
    got = check_table(s, s["ent"], s["uv"], w, h)
    assert 0 < len(got[3]) < w * h and len(np.unique(got[0])) > (10 if w == 32 else 2)     # some texels covered, some not, several owners
    again = s["rt"].lightmap_texels(s["ent"], s["uv"], w, h)
    assert all(same(a, b) for a, b in zip(got, again))
    check_table(s, s["ent"], s["uv"], w, h, flip=True)
    check_table(s, s["ent"][::-1].copy(), s["uv"][::-1].copy(), w, h)


# ---------------------------------------------------------------------------------------------------------------- 2. dilation
@pytest.mark.parametrize("passes", [0, 1, 3, 64])
def test_dilation_is_the_numpy_dilation(setups, passes):
    rt = setups("hand")["rt"]
    rs = np.random.RandomState(passes)
    for density in (0.02, 0.3):
        v = rs.standard_normal((9, 17, 3)) * 10.0 ** rs.randint(-6, 7, (9, 17, 1))
        f = rs.rand(9, 17) < density
        f[4, 8] = True
        assert same(rt.lightmap_dilate(v, f, passes), le.dilate(v, f, passes)[0])
    assert not rt.lightmap_dilate(v, np.zeros((9, 17)), passes).any()


# ---------------------------------------------------------------------------------------------------------------- 3. the atlas
@pytest.mark.parametrize("name", ["cornell", "caustics"])
def test_atlas_is_scatter_and_dilation_of_bake_texels_on_the_table(setups, name):
    s = setups(name)
    rt = s["rt"]
    for (w, h), ns, flip, base, seed in (((32, 32), 5, False, 0, SEEDS[0]), ((7, 5), 16, True, BASE, SEEDS[1]), ((16, 12), 5, False, BASE, SEEDS[1])):
        want, owner, n = expected_atlas(s, s["ent"], s["uv"], w, h, ns, 2, flip, base, seed)
        got, gown, gn = rt.bake_lightmap(s["ent"], s["uv"], w, h, ns, dilate=2, flip=flip, stream_base=base, seed=seed, want_owner=True)
        assert gn == n and n > 0 and same(gown, owner)
        assert got.dtype == np.float64 and np.abs(want).max() > 0
        assert same(got, want), f"{name} {w}x{h}: {int((got != want).any(-1).sum())} texels differ"
        assert same(rt.bake_lightmap(s["ent"], s["uv"], w, h, ns, dilate=2, flip=flip, stream_base=base, seed=seed), got)


def test_atlas_on_the_floor_is_the_oracles_bake(setups):
    s = setups("floor")
    o = pc.oracle_for(s["scene"]).build_photon_map()
    chart = np.array([[[0.1, 0.1], [0.9, 0.2], [0.8, 0.9]], [[0.1, 0.1], [0.8, 0.9], [0.05, 0.7]]])
    for flip in (False, True):
        want, owner, n = le.lightmap(lambda P, N: be.bake(o, be.TEXEL, P, N, 5, BASE, SEEDS[1]), s["t"], [0, 1], chart, 12, 9, 3, flip)
        got, gown, gn = s["rt"].bake_lightmap([0, 1], chart, 12, 9, 5, dilate=3, flip=flip, stream_base=BASE, seed=SEEDS[1], want_owner=True)
        assert gn == n and n > 20 and same(gown, owner) and same(got, want)
        assert np.array_equal(got[owner >= 0], np.tile(be.fold_texel(np.tile(AMBIENT, (1, 5, 1))), (n, 1)))      # every ray meets nothing: the ambient term


def test_chunked_bake_f32_and_no_chart(setups):
    s = setups("caustics")
    rt = s["rt"]
    whole = rt.bake_lightmap(s["ent"], s["uv"], 32, 32, 5)
    try:
        rt.set_pool_slots(64)                                    # chunks of 64 texels, one sample a range
        assert same(rt.bake_lightmap(s["ent"], s["uv"], 32, 32, 5), whole)
    finally:
        rt.set_pool_slots(1 << 30)
    f32 = rt.bake_lightmap(s["ent"], s["uv"], 32, 32, 5, f64=False)
    assert f32.dtype == np.float32 and same(f32, whole.astype(np.float32))
    assert same(rt.bake_lightmap(s["ent"], s["uv"], 32, 32, 5, dilate=0), le.dilate(whole, rt.lightmap_texels(s["ent"], s["uv"], 32, 32)[0] >= 0, 0)[0])
    atlas, owner, n = rt.bake_lightmap(np.zeros(0, np.int32), np.zeros((0, 3, 2)), 9, 4, 5, want_owner=True)
    assert n == 0 and atlas.shape == (4, 9, 3) and not atlas.any() and (owner == -1).all()
    assert rt.L.gi_lightmap_host(rt.h, C.byref(rt.lightmap_params(9, 4, 5)), 0, None, None, atlas.ctypes.data_as(C.c_void_p), 1, None, None) == gi.GI_OK


def test_device_entry_writes_what_the_host_entry_returns(setups):
    s = setups("cornell")
    rt = s["rt"]
    hip = hip_runtime()
    ent, uv = np.ascontiguousarray(s["ent"]), np.ascontiguousarray(s["uv"])
    w, h = 16, 12
    atlas, owner = np.full((h, w, 3), -7.0), np.full((h, w), -7, np.int32)
    bufs = [C.c_void_p() for _ in range(4)]
    hosts = [ent, uv, atlas, owner]
    for b, a in zip(bufs, hosts):
        assert hip.hipMalloc(C.byref(b), C.c_size_t(a.nbytes)) == 0
    try:
        for b, a in zip(bufs, hosts):
            assert hip.hipMemcpy(b, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0
        n = rt.lightmap_device(rt.lightmap_params(w, h, 5), len(ent), bufs[0].value, bufs[1].value, bufs[2].value, f64=True, owner_ptr=bufs[3].value)
        ms, stages = rt.last_lightmap_ms()
        assert ms > 0 and all(v > 0 for v in stages.values()) and sum(stages.values()) <= ms + 0.05
        assert hip.hipDeviceSynchronize() == 0
        for b, a in zip(bufs[2:], hosts[2:]):
            assert hip.hipMemcpy(a.ctypes.data_as(C.c_void_p), b, C.c_size_t(a.nbytes), 2) == 0
    finally:
        for b in bufs:
            assert hip.hipFree(b) == 0
    want = rt.bake_lightmap(ent, uv, w, h, 5, want_owner=True)
    assert n == want[2] and same(atlas, want[0]) and same(owner, want[1])


# ---------------------------------------------------------------------------------------------------------------- 4. everything else is left alone
def test_frames_timers_and_a_session_are_untouched(setups):
    s = setups("caustics")
    rt = s["rt"]
    kw = dict(min_samples=6, max_samples=6)
    before = rt.run(48, 32, **kw)
    P, N = rt.lightmap_texels(s["ent"], s["uv"], 7, 5)[1:3]
    rows = rt.bake_texels(P, N, 16)
    t_before = timers(rt)
    assert t_before[1][1] > 0 and t_before[0]["trace"] > 0
    atlas = rt.bake_lightmap(s["ent"], s["uv"], 16, 12, 5)
    t_after = timers(rt)
    assert t_after[1][2][0] > 0 and t_after[1][2] != t_before[1][2]
    assert same_timers((t_after[0], t_after[1][:2]), (t_before[0], t_before[1][:2]))
    assert same(rt.run(48, 32, **kw), before) and same(rt.bake_texels(P, N, 16), rows)
    with rt.progressive(48, 32, **kw) as sess:                   # step, lightmap, step has the bits of step, step
        sess.step(2)
        end = sess.sample_end
        assert same(rt.bake_lightmap(s["ent"], s["uv"], 16, 12, 5), atlas)
        assert sess.sample_end == end
        assert same(sess.step(4), before)


# ---------------------------------------------------------------------------------------------------------------- 5. refusals
def test_bad_calls_are_refused_and_leave_output_and_timers_alone(setups):
    s = setups("hand")
    rt, L = s["rt"], s["rt"].L
    frame = rt.run(24, 16, min_samples=2, max_samples=2)
    rt.bake_texels([[1.0, 0.5, 1.0]], [UP], 5)
    ent, uv = np.array([2, 3], np.int32), np.ascontiguousarray(le.QUAD)
    assert list(s["t"]["ent_kind"]) == [0, 0, 0, 0, 1]
    w, h = 8, 6
    good = rt.bake_lightmap(ent, uv, w, h, 5)
    t_before = timers(rt)
    assert t_before[1][1] > 0 and t_before[1][2][0] > 0
    atlas, owner, ncov = np.full((h, w, 3), -7.0), np.full((h, w), -7, np.int32), C.c_int32(-7)
    pts, tex = np.full((w * h, 6), -7.0), np.full(w * h, -7, np.int32)
    pa, po = atlas.ctypes.data_as(C.c_void_p), owner.ctypes.data_as(gi._ip)
    NOWHERE = C.c_void_p(16)
    nan, inf = float("nan"), float("inf")
    P = gi.LightmapParams

    def host(p, n=2, e=ent, c=uv, a=pa):
        return L.gi_lightmap_host(rt.h, C.byref(p) if p is not None else None, n, gi._p(e, gi._ip), gi._p(c), a, 1, po, C.byref(ncov))

    def texels(p, n=2, e=ent, c=uv, cap=w * h, o=po):
        return L.gi_lightmap_texels(rt.h, C.byref(p) if p is not None else None, n, gi._p(e, gi._ip), gi._p(c), o, C.byref(ncov), gi._p(pts), gi._p(tex, gi._ip), cap)

    def untouched():
        return (atlas == -7.0).all() and (owner == -7).all() and ncov.value == -7 and (pts == -7.0).all() and (tex == -7).all()

    ok = P(w, h, 5, 2, 0, 0, 1)
    bad_params = (P(0, h, 5, 2, 0, 0, 1), P(w, 8193, 5, 2, 0, 0, 1), P(-1, h, 5, 2, 0, 0, 1), P(w, h, 0, 2, 0, 0, 1), P(w, h, 5, -1, 0, 0, 1), P(w, h, 5, 65, 0, 0, 1),
                  P(w, h, 5, 2, 2, 0, 1), P(w, h, 5, 2, -1, 0, 1), P(w, h, 5, 2, 0, 2 ** 32 - 5 * w * h + 1, 1), P(8192, 8192, 64, 2, 0, 1, 1))
    for bad in bad_params:
        what = (bad.width, bad.height, bad.n_samples, bad.dilate, bad.flip, bad.stream_base)
        assert host(bad) == gi.GI_E_INVALID, what
        assert b"lightmap" in L.gi_last_error(rt.h)
        assert texels(bad) == gi.GI_E_INVALID, what
        assert L.gi_lightmap_device(rt.h, C.byref(bad), 2, NOWHERE, NOWHERE, NOWHERE, 1, NOWHERE, C.byref(ncov)) == gi.GI_E_INVALID, what     # refused before a pointer is used
    assert host(None) == gi.GI_E_INVALID and host(ok, n=-1) == gi.GI_E_INVALID and host(ok, a=None) == gi.GI_E_INVALID
    assert host(ok, e=None) == gi.GI_E_INVALID and host(ok, c=None) == gi.GI_E_INVALID
    assert L.gi_lightmap_host(None, C.byref(ok), 2, gi._p(ent, gi._ip), gi._p(uv), pa, 1, po, None) == gi.GI_E_INVALID
    assert L.gi_lightmap_device(rt.h, C.byref(ok), 2, None, NOWHERE, NOWHERE, 1, None, None) == gi.GI_E_INVALID
    assert L.gi_lightmap_device(rt.h, C.byref(ok), 2, NOWHERE, NOWHERE, None, 1, None, None) == gi.GI_E_INVALID
    assert texels(ok, o=None) == gi.GI_E_INVALID and texels(ok, cap=-1) == gi.GI_E_INVALID and texels(ok, e=None) == gi.GI_E_INVALID
    for e_bad in ([2, -1], [5, 3], [2, 4]):                                                          # out of range twice, then the sphere
        e_bad = np.array(e_bad, np.int32)
        assert host(ok, e=e_bad) == gi.GI_E_INVALID and b"row" in L.gi_last_error(rt.h)
        assert texels(ok, e=e_bad) == gi.GI_E_INVALID
    assert b"sphere" in L.gi_last_error(rt.h)
    for value in (nan, inf, -inf):
        c_bad = uv.copy()
        c_bad[1, 2, 0] = value
        assert host(ok, c=c_bad) == gi.GI_E_INVALID and b"row 1" in L.gi_last_error(rt.h)
        assert texels(ok, c=c_bad) == gi.GI_E_INVALID
    empty = gi.RayTracer(0)
    assert L.gi_lightmap_host(empty.h, C.byref(ok), 2, gi._p(ent, gi._ip), gi._p(uv), pa, 1, po, C.byref(ncov)) == gi.GI_E_STATE and b"no scene" in L.gi_last_error(empty.h)
    assert L.gi_lightmap_device(empty.h, C.byref(ok), 2, NOWHERE, NOWHERE, NOWHERE, 1, None, None) == gi.GI_E_STATE
    assert L.gi_lightmap_texels(empty.h, C.byref(ok), 2, gi._p(ent, gi._ip), gi._p(uv), po, C.byref(ncov), gi._p(pts), gi._p(tex, gi._ip), w * h) == gi.GI_E_STATE
    ms = C.c_float(-7)
    assert L.gi_last_lightmap_ms(rt.h, None, None) == gi.GI_E_INVALID and L.gi_last_lightmap_ms(None, C.byref(ms), None) == gi.GI_E_INVALID and ms.value == -7
    vals, fill, out = np.ones((h, w, 3)), np.ones((h, w), np.int32), np.full((h, w, 3), -7.0)
    for dw, dh, dp, v, f, o in ((0, h, 1, vals, fill, out), (w, 8193, 1, vals, fill, out), (w, h, -1, vals, fill, out), (w, h, 65, vals, fill, out),
                                (w, h, 1, None, fill, out), (w, h, 1, vals, None, out), (w, h, 1, vals, fill, None)):
        assert L.gi_lightmap_dilate(rt.h, dw, dh, dp, gi._p(v), gi._p(f, gi._ip), gi._p(o)) == gi.GI_E_INVALID
    assert L.gi_lightmap_dilate(None, w, h, 1, gi._p(vals), gi._p(fill, gi._ip), gi._p(out)) == gi.GI_E_INVALID and (out == -7.0).all()
    with pytest.raises(gi.GiError):
        rt.bake_lightmap([4], le.QUAD[:1], w, h, 5)
    with pytest.raises(ValueError):
        rt.bake_lightmap([2, 3], le.QUAD[:1], w, h, 5)
    assert untouched()
    assert same_timers(timers(rt), t_before)
    # a table that does not fit: refused, but n_covered and the owners are written
    assert texels(ok, cap=w * h - 1) == gi.GI_E_INVALID and b"capacity" in L.gi_last_error(rt.h)
    assert ncov.value == w * h and (owner >= 0).all() and (pts == -7.0).all() and (tex == -7).all()
    assert texels(ok) == gi.GI_OK and (tex == np.arange(w * h)).all()
    assert same_timers(timers(rt), t_before)                                                          # the check entries have no timer
    assert same(rt.bake_lightmap(ent, uv, w, h, 5), good) and same(rt.run(24, 16, min_samples=2, max_samples=2), frame)


# ---------------------------------------------------------------------------------------------------------------- 6. the command line
def test_cli_writes_the_atlas(setups, tmp_path, capsys):
    from gi_raytracer_amd import __main__ as cli
    s = setups("cornell")
    scn = os.path.join(pc.ROOT, pc.SCN["cornell"])
    ppm, pfm = tmp_path / "lm.ppm", tmp_path / "lm.pfm"
    args = [scn, "--lightmap", "24", "16", "--lightmap-material", "3", "--lightmap-samples", "5", "--lightmap-dilate", "1", "--photons", "0"]
    assert cli.main(args + ["-o", str(ppm), "--pfm", str(pfm)]) == 0
    assert sorted(os.listdir(tmp_path)) == ["lm.pfm", "lm.ppm"] and "texels covered" in capsys.readouterr().out
    ent, uv = gi.chart_of_material(s["scene"], 3)
    assert len(ent) == 192 and (s["t"]["tri_mat"][ent] == 3).all() and same(uv, s["t"]["tri_uv"][ent])
    want = s["rt"].bake_lightmap(ent, uv, 24, 16, 5, dilate=1, f64=False)
    assert np.abs(want).max() > 0
    blob = open(pfm, "rb").read()
    head = b"PF\n24 16\n-1.0\n"
    assert blob.startswith(head) and len(blob) == len(head) + 24 * 16 * 12
    assert same(np.frombuffer(blob[len(head):], "<f4").reshape(16, 24, 3)[::-1], want)
    img = open(ppm, "rb").read()
    assert img.startswith(b"P6\n24 16\n255\n") and img[len(b"P6\n24 16\n255\n"):] == gi.to_rgb8(want).tobytes()
    every = gi.chart_of_material(s["scene"])
    assert len(every[0]) == len(s["t"]["tri_pos"]) and every[1].shape == (len(every[0]), 3, 2)
    with pytest.raises(SystemExit):
        cli.main([scn, "--lightmap", "24", "16", "--samples", "1", "-o", str(ppm)])
    with pytest.raises(SystemExit):
        cli.main([scn, "--lightmap-samples", "5", "-o", str(ppm)])
