"""The baked-light pass with a lightmap (gi_render_baked_lightmap_*, the LM instances of k_lit, k_lm_rows) on the GPU, through the C ABI via the
Python mirror.

Everything here is exact.  Given the oracle's first hits (ids and coverage are compared first, as tests/test_gpu_baked.py does), the diffuse term
equals the numpy statement (tests/baked_lightmap_expect.py) bit for bit under both filters, with a probe grid and without; direct, specular and
emissive are gi_render_baked_*'s bits; every identity (no chart, repetition, f32 out, f32 atlas, stripes, walk variants, the pinhole, permuted
rows) is bit for bit.  tests/test_baked_lightmap_cpu.py shows with the oracle alone that these frames have the cases the comparison needs."""
import ctypes as C
import os

import numpy as np
import pytest

import gi_raytracer_amd as gi

import baked_expect as be
import baked_lightmap_expect as bl
import features_expect as fe
import lightmap_expect as le
import occlusion_expect as oe
import parity_checks as pc

pytestmark = pytest.mark.gpu

W, H = 24, 16
SIZES = ((24, 16), (13, 9))
N = 2
DIRECT, DIFFUSE, SPECULAR, EMISSIVE = be.DIRECT, be.DIFFUSE, be.SPECULAR, be.EMISSIVE
GRID = (2, 2, 2)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.fixture(scope="module")
def setups():
    cache = {}

    def get(name):
        if name not in cache:
            if name in ("floor", "box"):
                scene = oe.floor_scene(gi) if name == "floor" else oe.closed_box_scene(gi)
                rt, o = gi.RayTracer(0).setScene(scene), pc.oracle_for(scene)
                chart = None
            else:
                base = pc.named_scene(name)
                scene = be.with_roughnesses(base, bl.ROUGHNESSES)
                rt = gi.RayTracer(0).setScene(scene)
                rt._adopt(base.settings)
                o = be.oracle_with_camera(scene, base.settings)
                chart = bl.frame_chart(o, scene.tables())
            cache[name] = (scene, rt, o, scene.tables(), chart)
        return cache[name]

    return get


@pytest.fixture(scope="module")
def inputs():
    """One grid, one chain and one atlas per size, shared and left unchanged."""
    return {"sh": be.random_sh(GRID, 101), "chain": be.random_chain(7), "atlas": {size: bl.random_atlas(size, 50 + k) for k, size in enumerate(bl.ATLAS_SIZES)}}


# ---------------------------------------------------------------------------------------------------------------- 1. the diffuse term is the statement's
@pytest.mark.parametrize("name", ["cornell", "test_scene", "spheres_opaque"])
def test_diffuse_term_equals_the_statement_bit_for_bit(setups, inputs, name):
    scene, rt, o, t, (ent, uv, rows) = setups(name)
    box, chain = be.inner_box(t), inputs["chain"]
    seen = {"charted": 0, "uncharted": 0}
    for (w, h) in SIZES:
        geo = [be.sample_hits(o, t, w, h, s) for s in range(N)]
        f1, f2 = rt.run_features(w, h, 1), rt.run_features(w, h, N)
        assert np.array_equal(f1["ids"][:, :, 0], geo[0]["ent"].reshape(h, w))                      # identical first hits
        assert np.array_equal(f2["coverage"] * N, sum(g["hit"].reshape(h, w).astype(np.float64) for g in geo))
        for n in (1, N):
            for sh in (inputs["sh"], None):
                skw = dict(sh=sh, grid_box=box) if sh is not None else {}
                plain = rt.run_baked(w, h, n, chain=chain, exponents=be.CHAIN_EXPONENTS, terms=15 if sh is not None else 13, **skw)
                em = rt.run_baked(w, h, n, terms=EMISSIVE)["beauty"]
                for size in bl.ATLAS_SIZES:
                    atlas = inputs["atlas"][size]
                    for filt in bl.FILTERS:
                        got = rt.run_baked_lightmap(w, h, n, atlas, ent, uv, filter=filt, chain=chain, exponents=be.CHAIN_EXPONENTS, terms=15, **skw)
                        assert got["baked"].shape == (h, w, 12) and got["baked"].dtype == np.float64
                        terms = [bl.sample_terms_lm(g, t, atlas, ent, uv, filt, sh, box) for g in geo[:n]]
                        want = be.fold([d for d, _, _ in terms]).reshape(h, w, 3)
                        assert same(np.ascontiguousarray(got["diffuse"]), want), (name, w, h, n, sh is not None, size, filt, float(np.abs(got["diffuse"] - want).max()))
                        assert same(np.ascontiguousarray(got["direct"]), np.ascontiguousarray(plain["direct"]))
                        assert same(np.ascontiguousarray(got["specular"]), np.ascontiguousarray(plain["specular"]))
                        if n == 1:                                                                  # (a sum of one sample: the emissive image is the term itself)
                            assert same(np.ascontiguousarray(got["beauty"]), np.ascontiguousarray(((got["direct"] + got["diffuse"]) + got["specular"]) + em))
                        seen["charted"] += sum(int(c.sum()) for _, c, _ in terms)
                        seen["uncharted"] += sum(int(u.sum()) for _, _, u in terms)
                        assert (got["diffuse"] > 0).any()
    assert seen["charted"] > 0 and seen["uncharted"] > 0, seen


# ---------------------------------------------------------------------------------------------------------------- 2. analytic cases
def test_an_atlas_of_one_colour_gives_albedo_times_the_colour_on_charted_hits(setups, inputs):
    scene, rt, o, t, (ent, uv, rows) = setups("cornell")
    colour = np.array([0.5, 2.0, 0.125])
    box = be.inner_box(t)
    geo = [be.sample_hits(o, t, W, H, s) for s in range(N)]
    for size in ((8, 8), (5, 3)):
        atlas = np.ascontiguousarray(np.broadcast_to(colour, (size[1], size[0], 3)))
        for filt in bl.FILTERS:
            for sh in (inputs["sh"], None):
                skw = dict(sh=sh, grid_box=box) if sh is not None else {}
                got = rt.run_baked_lightmap(W, H, N, atlas, ent, uv, filter=filt, terms=DIFFUSE, **skw)["diffuse"]
                per = []
                for g in geo:
                    diffuse, row = bl.hit_rows(g, t, ent)
                    other = g["albedo"] * be.irradiance(sh, box, g["P"], g["Nf"]) if sh is not None else np.zeros((len(row), 3))
                    per.append(np.where((diffuse & (row >= 0))[:, None], g["albedo"] * colour, np.where(diffuse[:, None], other, 0.0)))
                    assert (diffuse & (row >= 0)).any() and (diffuse & (row < 0)).any()
                assert same(np.ascontiguousarray(got), be.fold(per).reshape(H, W, 3)), (size, filt, sh is not None)


def test_a_two_texel_atlas_on_the_floor_is_linear_between_the_texel_centres(setups):
    scene, rt, o, t, _ = setups("floor")
    ent, uv = np.array([0, 1], np.int32), le.QUAD
    a, b = np.array([0.25, 1.0, 2.0]), np.array([1.5, 0.5, 0.0])
    atlas = np.stack([a, b])[None]                                    # 2 x 1
    g = be.sample_hits(o, t, W, H, 0)
    got = rt.run_baked_lightmap(W, H, 1, atlas, ent, uv, terms=DIFFUSE)["diffuse"]
    want, charted, _ = bl.sample_terms_lm(g, t, atlas, ent, uv, bl.BILINEAR)
    assert charted.sum() > W * H // 2 and np.array_equal(charted, g["hit"]) and same(np.ascontiguousarray(got), want.reshape(H, W, 3))
    # the statement, spelled out: with x the hit's u, t = clamp(2 x - 0.5, 0, 1) and E = a + t (b - a) between the centres, a and b beyond them;
    # the floor's u runs along one of its sides
    i = np.flatnonzero(charted)
    u, v = bl.coord(t, g["ent"][i], g["P"][i], bl.row_of_ent(ent, 2)[g["ent"][i]], uv)
    tt = np.clip(u * 2.0 - 0.5, 0.0, 1.0)
    E = np.where((tt >= 1.0)[:, None], b, a + tt[:, None] * (b - a))
    assert same(want[i], g["albedo"][i] * E) and ((tt > 0) & (tt < 1)).any() and len(np.unique(tt)) > 4
    near = rt.run_baked_lightmap(W, H, 1, atlas, ent, uv, filter="nearest", terms=DIFFUSE)["diffuse"].reshape(-1, 3)
    assert same(near[i], g["albedo"][i] * np.where((u < 0.5)[:, None], a, b)) and not near[~charted].any()


# ---------------------------------------------------------------------------------------------------------------- 3. identities, bit for bit
@pytest.mark.parametrize("name", ["cornell", "spheres_opaque"])
def test_identities_bit_for_bit(setups, inputs, name):
    scene, rt, o, t, (ent, uv, rows) = setups(name)
    atlas = inputs["atlas"][(8, 8)]
    kw = dict(sh=inputs["sh"], grid_box=be.inner_box(t), chain=inputs["chain"], exponents=be.CHAIN_EXPONENTS)
    none = (ent[:0], uv[:0])
    for (w, h) in SIZES:
        full = rt.run_baked_lightmap(w, h, N, atlas, ent, uv, **kw)["baked"]
        assert np.isfinite(full).all() and (full[:, :, 6:9] > 0).any()
        plain = rt.run_baked(w, h, N, **kw)["baked"]
        assert same(rt.run_baked_lightmap(w, h, N, atlas, *none, **kw)["baked"], plain) and not same(full, plain)      # no rows: the pass without a lightmap
        assert same(rt.run_baked_lightmap(w, h, N, atlas, ent, uv, terms=DIRECT | SPECULAR | EMISSIVE, **kw)["baked"], rt.run_baked(w, h, N, terms=DIRECT | SPECULAR | EMISSIVE, **kw)["baked"])
        assert same(rt.run_baked_lightmap(w, h, N, atlas, *none, chain=inputs["chain"], exponents=be.CHAIN_EXPONENTS)["baked"],
                    rt.run_baked(w, h, N, chain=inputs["chain"], exponents=be.CHAIN_EXPONENTS)["baked"])                # no rows and no grid: no diffuse term
        assert same(rt.run_baked_lightmap(w, h, N, atlas, ent, uv, **kw)["baked"], full)                               # a repeated call
        f32 = rt.run_baked_lightmap(w, h, N, atlas, ent, uv, f64=False, **kw)["baked"]
        assert f32.dtype == np.float32 and same(f32, full.astype(np.float32))
        a32 = atlas.astype(np.float32)
        assert same(rt.run_baked_lightmap(w, h, N, a32, ent, uv, **kw)["baked"], rt.run_baked_lightmap(w, h, N, a32.astype(np.float64), ent, uv, **kw)["baked"])
        for world in (2, 3):
            frame = np.full_like(full, -7.0)
            for rank in range(world):
                part = rt.run_baked_lightmap(w, h, N, atlas, ent, uv, stripe_h=4, rank=rank, world=world, **kw)["baked"]
                rws = fe.frame_rows(h, 4, rank, world)
                assert part.shape == (len(rws), w, 12)
                frame[rws] = part
            assert same(frame, full), (name, w, h, world)
        for switch in (rt.set_wide_nodes, rt.set_content_culling):
            try:
                switch(False)
                off = rt.run_baked_lightmap(w, h, N, atlas, ent, uv, **kw)["baked"]
            finally:
                switch(True)
            assert same(off, full), (name, w, h, switch.__name__)
        try:
            rt.set_lens(radius=0.0, blades=5)
            assert same(rt.run_baked_lightmap(w, h, N, atlas, ent, uv, **kw)["baked"], full)
        finally:
            rt.set_lens(radius=0.0)
        assert same(rt.run_baked_lightmap(w, h, N, atlas, *bl.permuted(ent, uv, 5), **kw)["baked"], full)              # every entity keeps its serving row
        if (w, h) == (W, H):
            assert not same(rt.run_baked_lightmap(w, h, N, atlas, *bl.swapped(ent, uv, rows), **kw)["baked"], full)   # the other row of the entity listed twice serves it


# ---------------------------------------------------------------------------------------------------------------- 4. the device entry
def test_device_entry_writes_what_the_host_entry_returns(setups, inputs):
    scene, rt, o, t, (ent, uv, rows) = setups("cornell")
    atlas = inputs["atlas"][(5, 3)]
    kw = dict(sh=inputs["sh"], grid_box=be.inner_box(t), chain=inputs["chain"], exponents=be.CHAIN_EXPONENTS)
    p = rt.params(W, H)
    bp, s, c = rt.baked_params(n=N, lightmap=True, **kw)
    lp, a, e, u = gi.baked_lightmap_params(atlas, ent, uv, "bilinear")
    want = rt.run_baked_lightmap(W, H, N, atlas, ent, uv, f64=False, **kw)["baked"]
    hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")      # device buffers from the HIP runtime the library itself uses (no second runtime in this process)
    bufs = []
    try:
        for arr in (s, c, a, e, u, np.full((H, W, 12), -7.0, np.float32)):
            d = C.c_void_p()
            assert hip.hipMalloc(C.byref(d), C.c_size_t(arr.nbytes)) == 0
            bufs.append(d)
            assert hip.hipMemcpy(d, arr.ctypes.data_as(C.c_void_p), C.c_size_t(arr.nbytes), 1) == 0      # hipMemcpyHostToDevice
        rt.run_baked_lightmap_device(p, bp, lp, *(b.value for b in bufs), f64=False)
        assert rt.last_baked_ms() > 0                                                  # waits for the pass
        got = np.zeros((H, W, 12), np.float32)
        assert hip.hipDeviceSynchronize() == 0
        assert hip.hipMemcpy(got.ctypes.data_as(C.c_void_p), bufs[5], C.c_size_t(got.nbytes), 2) == 0      # hipMemcpyDeviceToHost
    finally:
        for d in bufs:
            assert hip.hipFree(d) == 0
    assert same(got, want)


# ---------------------------------------------------------------------------------------------------------------- 5. refusals and timers
def test_refusals_leave_the_output_and_the_timers_alone(setups, inputs):
    scene, rt, o, t, (ent, uv, rows) = setups("spheres_opaque")       # it has spheres for a chart to name
    L = rt.L
    p = rt.params(W, H)
    rt.run(W, H, min_samples=1, max_samples=1)
    rt.run_occlusion(W, H, n=1, dirs=2)
    atlas = inputs["atlas"][(8, 8)]
    kw = dict(sh=inputs["sh"], grid_box=be.inner_box(t), chain=inputs["chain"], exponents=be.CHAIN_EXPONENTS)
    good = rt.run_baked_lightmap(W, H, 1, atlas, ent, uv, **kw)
    out = np.full((H, W, 12), -7.0)
    ptr = out.ctypes.data_as(C.c_void_p)
    bp, s, c = rt.baked_params(n=1, lightmap=True, **kw)
    lp, a, e, u = gi.baked_lightmap_params(atlas, ent, uv)
    dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))
    vp = lambda x: x.ctypes.data_as(C.c_void_p)

    def host(bp=bp, lp=lp, s=s, c=c, a=a, e=e, u=u, p=p, ptr=ptr, h=rt.h):
        return L.gi_render_baked_lightmap_host(h, C.byref(p) if p is not None else None, C.byref(bp) if bp is not None else None, C.byref(lp) if lp is not None else None,
                                               dp(s) if s is not None else None, dp(c) if c is not None else None, vp(a) if a is not None else None, 1,
                                               ip(e) if e is not None else None, dp(u) if u is not None else None, ptr, 1)

    def device(bp=bp, lp=lp):
        return L.gi_render_baked_lightmap_device(rt.h, C.byref(p), C.byref(bp), C.byref(lp), C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), 1)

    def variant(src, **fields):
        q = type(src).from_buffer_copy(src)
        for k, v in fields.items():
            if k in ("grid_min", "grid_max"):
                getattr(q, k)[:] = v
            else:
                setattr(q, k, v)
        return q

    ms0, frame_ms, ao_ms = rt.last_baked_ms(), rt.last_render_ms(), rt.last_occlusion_ms()
    assert ms0 > 0 and frame_ms[0] > 0 and ao_ms > 0
    box = be.inner_box(t)
    # what gi_render_baked_* refuses, and the lightmap's own parameters: before a pointer is used, by either entry
    bad_bp = [variant(bp, n_samples=0), variant(bp, terms=0), variant(bp, terms=16), variant(bp, nx=0), variant(bp, grid_max=[box[0], box[4], box[5]]),
              variant(bp, grid_min=[float("nan"), box[1], box[2]]), variant(bp, face=0), variant(bp, levels=13)]
    bad_lp = [variant(lp, width=0), variant(lp, width=8193), variant(lp, height=0), variant(lp, height=-3), variant(lp, height=8193), variant(lp, filter=2),
              variant(lp, filter=-1), variant(lp, n_chart=-1)]
    for q in bad_bp:
        assert host(bp=q) == gi.GI_E_INVALID and b"render_baked_lightmap" in L.gi_last_error(rt.h), bytes(q)[:16]
        assert device(bp=q) == gi.GI_E_INVALID and b"render_baked_lightmap" in L.gi_last_error(rt.h)
    for q in bad_lp:
        assert host(lp=q) == gi.GI_E_INVALID and b"render_baked_lightmap" in L.gi_last_error(rt.h), bytes(q)
        assert device(lp=q) == gi.GI_E_INVALID and b"render_baked_lightmap" in L.gi_last_error(rt.h)
    for kwargs in (dict(a=None), dict(e=None), dict(u=None), dict(c=None), dict(bp=None), dict(lp=None), dict(p=None), dict(ptr=None)):
        assert host(**kwargs) == gi.GI_E_INVALID and b"render_baked_lightmap" in L.gi_last_error(rt.h), kwargs
    assert host(h=None) == gi.GI_E_INVALID
    # the host entry looks at the chart: an entity index out of range, a sphere, a non-finite coordinate
    kind = np.asarray(t["ent_kind"]).reshape(-1)
    assert (kind == 1).any()
    for bad_e in (np.where(np.arange(len(e)) == 3, len(kind), e).astype(np.int32), np.where(np.arange(len(e)) == 3, -1, e).astype(np.int32),
                  np.where(np.arange(len(e)) == 3, int(np.flatnonzero(kind == 1)[0]), e).astype(np.int32)):
        assert host(e=bad_e) == gi.GI_E_INVALID and b"render_baked_lightmap" in L.gi_last_error(rt.h)
    bad_u = u.copy()
    bad_u[2, 1, 1] = np.inf
    assert host(u=bad_u) == gi.GI_E_INVALID and b"render_baked_lightmap" in L.gi_last_error(rt.h)
    assert host(p=rt.params(0, 10)) == gi.GI_E_INVALID
    with pytest.raises(ValueError):
        rt.run_baked_lightmap(W, H, 1, atlas[0], ent, uv)
    with pytest.raises(ValueError):
        rt.run_baked_lightmap(W, H, 1, atlas, ent, uv, filter="cubic")
    empty = gi.RayTracer(0)
    assert host(h=empty.h, p=empty.params(W, H)) == gi.GI_E_STATE
    assert L.gi_render_baked_lightmap_device(empty.h, C.byref(empty.params(W, H)), C.byref(bp), C.byref(lp), *[C.c_void_p(16)] * 6, 1) == gi.GI_E_STATE
    assert empty.last_baked_ms() == 0.0
    assert (out == -7.0).all()
    # no refusal touched a timer: the pass's own keeps the good call's time, the frame's and the occlusion's keep theirs
    assert rt.last_baked_ms() == ms0 and rt.last_render_ms() == frame_ms and rt.last_occlusion_ms() == ao_ms
    # what is allowed: no grid with the diffuse term; no chart pointers without rows or without the diffuse term
    assert host(s=None) == gi.GI_OK and same(out, rt.run_baked_lightmap(W, H, 1, atlas, ent, uv, chain=inputs["chain"], exponents=be.CHAIN_EXPONENTS, terms=15)["baked"])
    assert host(lp=variant(lp, n_chart=0), a=None, e=None, u=None) == gi.GI_OK
    assert host(bp=variant(bp, terms=DIRECT | EMISSIVE), a=None, e=None, u=None, s=None, c=None) == gi.GI_OK
    assert host() == gi.GI_OK and same(out, good["baked"])
    assert rt.last_baked_ms() > 0 and rt.last_render_ms() == frame_ms and rt.last_occlusion_ms() == ao_ms
    # an open progressive session is left alone
    pkw = dict(min_samples=4, max_samples=4)
    before = rt.run(W, H, **pkw)
    with rt.progressive(W, H, **pkw) as sess:
        sess.step(2)
        end = sess.sample_end
        assert same(rt.run_baked_lightmap(W, H, 1, atlas, ent, uv, **kw)["baked"], good["baked"])
        assert host(lp=variant(lp, filter=7)) == gi.GI_E_INVALID
        assert sess.sample_end == end and same(sess.step(2), before)


# ---------------------------------------------------------------------------------------------------------------- 6. end to end
def test_a_baked_lightmap_feeds_the_pass_end_to_end(setups):
    scene, rt, o, t, _ = setups("box")
    ent, uv = bl.packed_quads_chart(6, 3)
    atlas, owner, n_cov = rt.bake_lightmap(ent, uv, 32, 32, 64, dilate=2, want_owner=True)
    assert n_cov > 0 and np.isfinite(atlas).all()
    got = rt.run_baked_lightmap(W, H, N, atlas, ent, uv)
    cov = rt.run_features(W, H, N, want_ids=False)["coverage"]
    assert np.isfinite(got["baked"]).all() and (cov == 1).all()
    assert (got["diffuse"][cov == 1] > 0).all()                       # a white diffuse box, lit from inside: every pixel reads a filled texel
    assert not got["specular"].any()
    box = t["node_bbox"][0]
    sh = rt.bake_probes(gi.probe_grid(box, 2, 2, 2).reshape(-1, 3), 64).reshape(2, 2, 2, 9, 3)
    probes = rt.run_baked(W, H, N, sh=sh, grid_box=box)
    ref = rt.run(W, H, min_samples=16, max_samples=16)
    print(f"closed box: mean diffuse from the 32 x 32 lightmap {got['diffuse'].mean():.6f}, from 2 x 2 x 2 probes {probes['diffuse'].mean():.6f} "
          f"(ratio {got['diffuse'].mean() / probes['diffuse'].mean():.4f}); mean beauty {got['beauty'].mean():.6f}, of the 16-spp path-traced frame {ref.mean():.6f} "
          f"(ratio {got['beauty'].mean() / ref.mean():.4f}); {n_cov} of 1024 texels covered")


def test_cli_writes_the_preview_with_a_lightmap(tmp_path, capsys):
    from gi_raytracer_amd import __main__ as cli
    scn = os.path.join(pc.ROOT, pc.SCN["cornell"])
    assert cli.main([scn, "-o", str(tmp_path / "out.ppm"), "--width", "24", "--height", "16", "--samples", "1", "--photons", "0", "--baked", str(tmp_path / "lit"),
                     "--baked-samples", "2", "--baked-probes", "2", "1", "2", "--baked-lightmap", "16", "8", "--lightmap-samples", "4"]) == 0
    assert sorted(os.listdir(tmp_path)) == ["lit.ppm", "lit_diffuse.pfm", "lit_direct.pfm", "lit_specular.pfm", "out.ppm"]
    text = capsys.readouterr().out
    assert "baked lightmap 16x8" in text and "texels covered" in text and "baked light" in text
    d = fe.read_pfm(tmp_path / "lit_diffuse.pfm")
    assert d.shape == (16, 24, 3) and np.isfinite(d).all()
