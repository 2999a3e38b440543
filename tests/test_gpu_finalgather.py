"""The final-gather pass (gi_render_final_gather_*, k_fg) on the GPU, through the C ABI via the Python mirror.

What is exact and what has an allowance (tests/finalgather_expect.py has the derivation):
 * with DIFFUSE off the pass is run_baked bit for bit, all 12 channels; with it on, direct and specular still are;
 * on the open floor every gather ray misses, in the closed emitting box every ray hits a wall: diffuse is albedo * ambient, albedo * e, bit for bit;
 * the ids tap equals the statement's entities, except for rays that graze an edge within the sampler's ulp: at most 1 ray in 1 000 (the CPU
   test shows that the oracle alone flips none on these frames under a 4-ulp move; the count is printed);
 * pixels whose rays all agree match the statement's diffuse term within fg.ALLOWANCE of the pixel's own value, floored at 1e-6 of the frame's largest;
 * every identity (repetition, f32, stripes, walk variants, the pinhole, the tap, the beauty sum, the first direction) is exact, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import gi_raytracer_amd as gi

import baked_expect as be
import features_expect as fe
import finalgather_expect as fg
import occlusion_expect as oe
import parity_checks as pc

pytestmark = pytest.mark.gpu

SIZES = ((13, 9), (24, 16))         # 13 x 9: no multiple of the 8 x 8 tile and less than one workgroup
DIRS = (1, 4, 5)                    # 5: not a power of two
N = 2
DIRECT, DIFFUSE, SPECULAR, EMISSIVE = be.DIRECT, be.DIFFUSE, be.SPECULAR, be.EMISSIVE
LEVEL_COLOURS = ((0.5, 2.0, 0.125), (1.5, 0.25, 1.0), (0.75, 0.5, 3.0))


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def level_chain():
    """One colour per level, different across levels: a texel flip cannot move a value, a wrong level does."""
    return [np.ascontiguousarray(np.broadcast_to(np.array(c), (6, be.CHAIN_FACE >> l, be.CHAIN_FACE >> l, 3))) for l, c in enumerate(LEVEL_COLOURS)]


@pytest.fixture(scope="module")
def setups():
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
    return {"sh": {g: be.random_sh(g, 100 + k) for k, g in enumerate(be.GRIDS)}, "chain": be.random_chain(7), "levels": level_chain()}


# ---------------------------------------------------------------------------------------------------------------- 1. run_baked where nothing gathers
@pytest.mark.parametrize("name", ["cornell", "spheres_opaque"])
def test_without_diffuse_the_pass_is_run_baked_bit_for_bit(setups, inputs, name):
    scene, rt, o, t = setups(name)
    kw = dict(sh=inputs["sh"][(3, 2, 4)], grid_box=be.inner_box(t), chain=inputs["chain"], exponents=be.CHAIN_EXPONENTS)
    for (w, h) in SIZES:
        for n in (1, N):
            for terms in (DIRECT | SPECULAR | EMISSIVE, SPECULAR, DIRECT):
                lit = rt.run_baked(w, h, n, terms=terms, **kw)["baked"]
                for dirs in (1, 5):
                    got = rt.run_final_gather(w, h, n, dirs=dirs, terms=terms, want_ids=True, **kw)
                    assert same(got["final_gather"], lit), (name, w, h, n, terms, dirs)
                    assert (got["ids"] == fg.ID_NONE).all() and got["ids"].shape == (h, w, n, dirs)
            lit = rt.run_baked(w, h, n, terms=15, **kw)
            got = rt.run_final_gather(w, h, n, dirs=4, terms=15, **kw)
            assert same(np.ascontiguousarray(got["direct"]), np.ascontiguousarray(lit["direct"])) and same(np.ascontiguousarray(got["specular"]), np.ascontiguousarray(lit["specular"]))
            assert not same(np.ascontiguousarray(got["diffuse"]), np.ascontiguousarray(lit["diffuse"])) and (got["direct"] > 0).any()
    if name == "spheres_opaque":                                      # its frame sees past the spheres, and its ambient colour is not 0
        w, h = SIZES[1]
        cov = rt.run_features(w, h, N, want_ids=False)["coverage"]
        got = rt.run_final_gather(w, h, N, dirs=4, terms=15, want_ids=True, **kw)
        miss = cov == 0
        assert miss.any() and t["ambient"].all() and (got["beauty"][miss] == t["ambient"]).all()
        assert not got["final_gather"][miss][:, 3:].any() and (got["ids"][miss] == fg.ID_NONE).all()


# ---------------------------------------------------------------------------------------------------------------- 2. analytic, exact
def test_open_floor_gathers_the_ambient_colour_exactly():
    scene = oe.floor_scene(gi)
    ambient = np.array([0.25, 0.5, 1.5])
    scene.set_ambient(ambient)
    scene = scene.rebuild()
    rt = gi.RayTracer(0).setScene(scene)
    t = scene.tables()
    for (w, h) in SIZES:
        for n in (1, N):
            got = rt.run_final_gather(w, h, n, dirs=4, sh=np.zeros((1, 1, 1, 9, 3)), grid_box=t["node_bbox"][0] + np.array([-1, -1, -1, 1, 1, 1.0]), terms=DIFFUSE, want_ids=True)
            f = rt.run_features(w, h, n, want_ids=False)
            floor = f["coverage"] == 1
            assert floor.any() and (got["ids"][floor] == fg.ID_MISS).all()          # the normal points up and nothing is above the floor
            want = t["mats"][0, 3:6] * (((((0.0 + ambient) + ambient) + ambient) + ambient) / 4.0)
            assert (want == t["mats"][0, 3:6] * ambient).all()       # four equal addends divided by 4: exact
            assert same(np.ascontiguousarray(got["diffuse"][floor]), np.ascontiguousarray(np.broadcast_to(want, got["diffuse"][floor].shape)))


def test_closed_emitting_box_gathers_the_emission_exactly():
    s = gi.Scene()
    e = np.array([0.5, 1.25, 2.0])
    albedo = (0.75, 0.5, 0.25)
    m = s.add_material(1, 1, 1, albedo, e)
    src = oe.closed_box_scene(gi).tables()
    s.add_triangles(src["tri_pos"], mat_idx=[m] * len(src["tri_pos"]))
    s.set_camera((0.3, 0.2, 1.9), (-0.4, -0.1, -2.5))
    scene = s.rebuild()                                              # no light: i_Q = 0
    rt = gi.RayTracer(0).setScene(scene)
    t = scene.tables()
    assert len(t["lights"]) == 0
    for (w, h) in SIZES:
        for n in (1, N):
            got = rt.run_final_gather(w, h, n, dirs=4, sh=np.zeros((2, 2, 2, 9, 3)), grid_box=t["node_bbox"][0], terms=DIFFUSE, want_ids=True)
            assert (got["ids"] >= 0).all()                           # every first hit is diffuse and every ray hits a wall
            L = (e + np.array(albedo) * 0.0) + np.array(albedo) * 0.0
            want = np.array(albedo) * (((((0.0 + L) + L) + L) + L) / 4.0)
            assert (want == np.array(albedo) * e).all()
            assert same(np.ascontiguousarray(got["diffuse"]), np.ascontiguousarray(np.broadcast_to(want, got["diffuse"].shape)))


# ---------------------------------------------------------------------------------------------------------------- 3 and 4. the oracle's secondary hits, the statement's values
@pytest.mark.parametrize("name", ["cornell", "test_scene", "spheres_opaque"])
def test_secondary_hits_and_values_are_the_statement_s(setups, inputs, name):
    scene, rt, o, t = setups(name)
    assert name in fe.DRAW_FREE_SCENES
    box, chain = be.inner_box(t), inputs["levels"]
    differ = asked = 0
    kinds = np.zeros(4, np.int64)
    worst = 0.0
    for gi_, (w, h) in enumerate(fg.FRAMES[name]):
        hits = [be.sample_hits(o, t, w, h, s) for s in range(N)]
        f1, f2 = rt.run_features(w, h, 1), rt.run_features(w, h, N)
        assert np.array_equal(f1["ids"][:, :, 0], hits[0]["ent"].reshape(h, w))                 # identical first hits
        assert np.array_equal(f2["coverage"] * N, sum(g["hit"].reshape(h, w).astype(np.float64) for g in hits))
        sh = inputs["sh"][be.GRIDS[1 + gi_]]                                                     # (frames: fg.FRAMES -- cornell's second is 20 x 14)
        for n in (1, N):
            for dirs in DIRS:
                want = fg.expected_final_gather(o, t, w, h, n, dirs, sh, box, chain, be.CHAIN_EXPONENTS, hits=hits)
                got = rt.run_final_gather(w, h, n, dirs=dirs, sh=sh, grid_box=box, chain=chain, exponents=be.CHAIN_EXPONENTS, terms=DIFFUSE, want_ids=True)
                gathered = want["ids"] != fg.ID_NONE
                assert np.array_equal(got["ids"] != fg.ID_NONE, gathered)
                bad = got["ids"] != want["ids"]
                differ += int(bad.sum()); asked += int(gathered.sum())
                agree = ~bad.any((2, 3))
                top = float(np.abs(want["diffuse"]).max())
                rel = np.abs(got["diffuse"] - want["diffuse"]) / np.maximum(np.abs(want["diffuse"]), 1e-6 * top)
                worst = max(worst, float(rel[agree].max()))
                assert (rel[agree] <= fg.ALLOWANCE).all(), (name, w, h, n, dirs, float(rel[agree].max()))
                assert not got["diffuse"][~gathered.any((2, 3))].any()
                kinds += np.bincount(want["kind"][want["kind"] >= 0], minlength=4)
    print(f"{name}: {differ} of {asked} gather rays hit another entity than the statement's; largest relative difference of an agreeing pixel's diffuse term {worst:.3e} "
          f"(allowance {fg.ALLOWANCE:.3e}); secondary misses / diffuse inside / diffuse outside the grid box / specular: {kinds.tolist()}")
    assert asked > 0 and differ * 1000 <= asked, (differ, asked)
    assert kinds[0] > 0 and kinds[1] + kinds[2] > 0 and kinds[2] > 0 and kinds[3] > 0, kinds      # misses, diffuse-lobe hits, Q outside the grid box, specular hits


# ---------------------------------------------------------------------------------------------------------------- 5. identities, bit for bit
@pytest.mark.parametrize("name", ["cornell", "spheres_opaque"])
def test_identities_bit_for_bit(setups, inputs, name):
    scene, rt, o, t = setups(name)
    kw = dict(dirs=5, sh=inputs["sh"][(3, 2, 4)], grid_box=be.inner_box(t), chain=inputs["chain"], exponents=be.CHAIN_EXPONENTS, terms=15)
    for (w, h) in SIZES:
        full = rt.run_final_gather(w, h, N, want_ids=True, **kw)
        ids, full = full["ids"], full["final_gather"]
        assert np.isfinite(full).all() and (full[:, :, 6:9] > 0).any()
        again = rt.run_final_gather(w, h, N, want_ids=True, **kw)
        assert same(again["final_gather"], full) and same(again["ids"], ids)                     # a repeated call
        assert same(rt.run_final_gather(w, h, N, **kw)["final_gather"], full)                      # the tap does not change out
        f32 = rt.run_final_gather(w, h, N, f64=False, **kw)["final_gather"]
        assert f32.dtype == np.float32 and same(f32, full.astype(np.float32))
        for world in (2, 3):
            frame, fids = np.full_like(full, -7.0), np.full_like(ids, -9)
            for rank in range(world):
                part = rt.run_final_gather(w, h, N, stripe_h=4, rank=rank, world=world, want_ids=True, **kw)
                rows = fe.frame_rows(h, 4, rank, world)
                assert part["final_gather"].shape == (len(rows), w, 12)
                frame[rows], fids[rows] = part["final_gather"], part["ids"]
            assert same(frame, full) and same(fids, ids), (name, w, h, world)
        for switch in (rt.set_wide_nodes, rt.set_content_culling, rt.set_entity_boxes):
            try:
                switch(False)
                off = rt.run_final_gather(w, h, N, want_ids=True, **kw)
            finally:
                switch(True)
            assert same(off["final_gather"], full) and same(off["ids"], ids), (name, w, h, switch.__name__)
        try:
            rt.set_lens(radius=0.0, blades=5)
            assert same(rt.run_final_gather(w, h, N, **kw)["final_gather"], full)                  # a zero-radius lens is the pinhole
        finally:
            rt.set_lens(radius=0.0)
        # beauty = ((direct + diffuse) + specular) + emissive + the miss share of ambient, exact at one and two samples
        one = rt.run_final_gather(w, h, 1, **kw)
        em = rt.run_baked(w, h, 1, terms=EMISSIVE)["beauty"]                                       # emissive, and the ambient colour on the misses
        assert same(np.ascontiguousarray(one["beauty"]), np.ascontiguousarray(((one["direct"] + one["diffuse"]) + one["specular"]) + em))
        two = rt.run_final_gather(w, h, N, **dict(kw, terms=DIFFUSE))                              # one term: halving a sum of two is exact
        misses = 1.0 - rt.run_features(w, h, N, want_ids=False)["coverage"]
        assert same(np.ascontiguousarray(two["beauty"]), np.ascontiguousarray(((two["direct"] + two["diffuse"]) + two["specular"]) + misses[:, :, None] * t["ambient"]))
        # the first direction does not depend on n_dirs
        d1 = rt.run_final_gather(w, h, 1, want_ids=True, **dict(kw, dirs=1))["ids"]
        d5 = rt.run_final_gather(w, h, 1, want_ids=True, **kw)["ids"]
        assert same(np.ascontiguousarray(d1[..., 0]), np.ascontiguousarray(d5[..., 0])) and (d1 >= 0).any()


# ---------------------------------------------------------------------------------------------------------------- 6. refusals and timers
def test_refusals_leave_the_output_and_the_timers_alone(setups, inputs):
    scene, rt, o, t = setups("cornell")
    L = rt.L
    w, h = SIZES[1]
    p = rt.params(w, h)
    sh, box = inputs["sh"][(2, 2, 2)], be.inner_box(t)
    rt.run_baked(w, h, 1, sh=sh, grid_box=box)
    good = rt.run_final_gather(w, h, 1, dirs=4, sh=sh, grid_box=box, chain=inputs["chain"], exponents=be.CHAIN_EXPONENTS)
    fp, s, c = gi.final_gather_params(n=1, dirs=4, sh=sh, grid_box=box, chain=inputs["chain"], exponents=be.CHAIN_EXPONENTS)
    out = np.full((h, w, 12), -7.0)
    ptr = out.ctypes.data_as(C.c_void_p)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ms0, lit_ms = rt.last_final_gather_ms(), rt.last_baked_ms()
    assert ms0 > 0 and lit_ms > 0

    def variant(**kw):
        q = gi.FinalGatherParams.from_buffer_copy(fp)
        for k, v in kw.items():
            setattr(q.baked if k in ("terms", "face", "n_samples") else q, k, v)
        return q

    for q, word in ((variant(n_dirs=0), b"n_dirs"), (variant(n_dirs=65), b"n_dirs"), (variant(reserved=1), b"reserved"), (variant(n_samples=0), b"n_samples"),
                    (variant(terms=DIFFUSE, face=6), b"face")):             # (a chain's face is checked without the SPECULAR bit too)
        assert L.gi_render_final_gather_host(rt.h, C.byref(p), C.byref(q), dp(s), dp(c), ptr, 1, None) == gi.GI_E_INVALID
        err = L.gi_last_error(rt.h)
        assert b"render_final_gather" in err and word in err, err
        assert L.gi_render_final_gather_device(rt.h, C.byref(p), C.byref(q), C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), 1, None) == gi.GI_E_INVALID
    assert L.gi_render_final_gather_host(rt.h, C.byref(p), C.byref(fp), None, dp(c), ptr, 1, None) == gi.GI_E_INVALID      # DIFFUSE without sh
    assert b"probe grid" in L.gi_last_error(rt.h)
    assert L.gi_render_final_gather_host(rt.h, C.byref(p), C.byref(variant(terms=DIFFUSE | SPECULAR)), dp(s), None, ptr, 1, None) == gi.GI_E_INVALID      # SPECULAR without a chain
    assert b"chain" in L.gi_last_error(rt.h)
    assert L.gi_render_final_gather_host(rt.h, C.byref(p), C.byref(fp), dp(s), dp(c), None, 1, None) == gi.GI_E_INVALID   # null output
    assert b"output" in L.gi_last_error(rt.h)
    assert L.gi_render_final_gather_host(rt.h, C.byref(p), None, dp(s), dp(c), ptr, 1, None) == gi.GI_E_INVALID
    assert L.gi_render_final_gather_host(None, C.byref(p), C.byref(fp), dp(s), dp(c), ptr, 1, None) == gi.GI_E_INVALID
    assert L.gi_last_final_gather_ms(rt.h, None) == gi.GI_E_INVALID
    big = rt.params(3840, 2160, stripe_h=8, rank=0, world=270)      # the Halton index: a 3840 x 2160 frame takes 479 samples; refused before the level table is touched
    out_big = np.full((8, 3840, 12), -7.0, np.float32)
    assert L.gi_render_final_gather_host(rt.h, C.byref(big), C.byref(variant(n_samples=480)), dp(s), dp(c), out_big.ctypes.data_as(C.c_void_p), 0, None) == gi.GI_E_INVALID
    assert b"render_final_gather" in L.gi_last_error(rt.h) and b"480" in L.gi_last_error(rt.h) and b"479" in L.gi_last_error(rt.h)
    assert L.gi_render_final_gather_device(rt.h, C.byref(big), C.byref(variant(n_samples=480)), C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), 0, None) == gi.GI_E_INVALID
    assert (out_big == -7.0).all()
    empty = gi.RayTracer(0)
    assert L.gi_render_final_gather_host(empty.h, C.byref(empty.params(w, h)), C.byref(fp), dp(s), dp(c), ptr, 1, None) == gi.GI_E_STATE
    assert b"no scene" in L.gi_last_error(empty.h) and empty.last_final_gather_ms() == 0.0
    for bad in (dict(dirs=0), dict(dirs=65), dict(dirs=2.5)):
        with pytest.raises(ValueError):
            rt.run_final_gather(w, h, 1, sh=sh, grid_box=box, **bad)
    assert (out == -7.0).all()
    assert rt.last_final_gather_ms() == ms0 and rt.last_baked_ms() == lit_ms
    assert L.gi_render_final_gather_host(rt.h, C.byref(p), C.byref(fp), dp(s), dp(c), ptr, 1, None) == gi.GI_OK and same(out, good["final_gather"])
    assert rt.last_final_gather_ms() > 0 and rt.last_baked_ms() == lit_ms
    kw = dict(min_samples=4, max_samples=4)                           # an open progressive session is left alone
    before = rt.run(w, h, **kw)
    with rt.progressive(w, h, **kw) as sess:
        sess.step(2)
        end = sess.sample_end
        assert same(rt.run_final_gather(w, h, 1, dirs=4, sh=sh, grid_box=box, chain=inputs["chain"], exponents=be.CHAIN_EXPONENTS)["final_gather"], good["final_gather"])
        assert sess.sample_end == end and same(sess.step(2), before)
