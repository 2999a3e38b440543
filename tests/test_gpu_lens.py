"""The thin-lens camera (gi_set_lens, include/gi_hip.h) on the GPU, through the C ABI via the Python mirror.

The expectation is tests/lens_expect.py -- the lens restated in numpy from the oracle's Halton sampler and counter RNG -- and the oracle as it is,
applied to those rays: Oracle.radiance for frames, Oracle.trace for features and autofocus, Oracle.visible for the occlusion segments.  Rays are
compared bit for bit; frames with the tolerance tests/parity_checks.py applies to whole frames (RMSE_TOL); features as exactly as
tests/test_gpu_features.py compares the pinhole's (bit for bit); occlusion counts with the allowance of tests/test_gpu_occlusion.py (1 segment in
1 000).  Frames are 7 x 5 and 13 x 9: neither a power of 2 nor of 3, so the Halton scale factors are not trivial; 1 .. 4 samples."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import gi_raytracer_amd as gi

import features_expect as fe
import host_build
import lens_expect as le
import occlusion_expect as oe
import parity_checks as pc

pytestmark = pytest.mark.gpu

W, H, SPP = 13, 9, 4
RADIUS, BLADES, ROTATION = 0.35, 5, 0.3
SEEDS = (le.DEFAULT_SEED, 12345)
# Halton indices whose first lens draw u0 lies in the last 2^-20 of [0, 1), found on the CPU by a search over the counter RNG (the test checks them)
LAST_SLIVER = {le.DEFAULT_SEED: 2039157, 12345: 721123}


def new_rt(name="cornell", photons=None):
    scene = pc.load_scene(name)
    rt = gi.RayTracer(0).setScene(scene)
    if photons is not None:
        scene.build_photon_map(photons)
        rt.upload_photon_map()
    return scene, rt


@pytest.fixture(scope="module")
def cornell():
    scene, rt = new_rt("cornell")
    return scene, rt, pc.oracle_for(scene), scene.tables()


def lens_rays(rt, w, h, idx, lens, seed=le.DEFAULT_SEED):
    return le.rays(le.camera(rt), w, h, idx, lens.radius, gi.lens_vertices(lens) if lens.radius > 0 else None, seed)


def all_indices(w, h, n):
    return np.concatenate([le.frame_indices(w, h, s) for s in range(n)])


# ---------------------------------------------------------------------------------------------------------------- 1. rays
def indices_hitting_every_blade(B, seed):
    """The first Halton index per k = (int)(u0 B), and the one in the last sliver of [0, 1), which lands in k = B - 1 through the min()."""
    got = {}
    i = 0
    while len(got) < B:
        u0 = le.draws([i], seed)[0][0]
        got.setdefault(int(u0 * B), i)
        i += 1
    u0 = le.draws([LAST_SLIVER[seed]], seed)[0][0]
    assert 1.0 - 2.0 ** -20 <= u0 < 1.0 and min(int(u0 * B), B - 1) == B - 1
    return sorted(got.values()) + [LAST_SLIVER[seed]]


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("rotation", [0.0, 0.7])
@pytest.mark.parametrize("blades", [3, 6, 16])
def test_primary_rays_equal_the_numpy_statement_bit_for_bit(cornell, blades, rotation, seed):
    scene, rt, o, t = cornell
    w, h = 7, 5
    lens = gi.lens_params(RADIUS, blades, rotation)
    idx = np.concatenate([all_indices(w, h, 4), np.array(indices_hitting_every_blade(blades, seed), np.uint32)])
    try:
        rt.set_lens(lens=lens)
        got = rt.primary_rays(rt.params(w, h, seed=seed), idx)
    finally:
        rt.set_lens(0.0)
    want = lens_rays(rt, w, h, idx, lens, seed)
    ks = le.lens_points(gi.lens_vertices(lens), *le.draws(idx, seed))[1]
    assert set(ks.tolist()) == set(range(blades))
    assert (got[:, 0:3] != np.array(rt.cam_pos)).any(1).all()                     # every eye left the pinhole
    assert le.same(got, want), (np.abs(got - want).max(), int((got != want).any(1).sum()))
    assert le.same(rt.primary_rays(rt.params(w, h, seed=seed), idx), lens_rays(rt, w, h, idx, gi.lens_params(0.0), seed))      # and the pinhole's, after


# ---------------------------------------------------------------------------------------------------------------- 2. frames
@pytest.mark.parametrize("name", ["cornell", "caustics"])
def test_frame_under_a_lens_is_the_oracle_on_the_lens_rays(name, golden):
    photons = golden("scene_caustics")["photons"] if name == "caustics" else None
    scene, rt = new_rt(name, photons)
    o = pc.oracle_for(scene)
    if photons is not None:
        o.set_photons(photons)
    o.build_photon_map()
    lens = gi.lens_params(RADIUS, BLADES, ROTATION)
    rt.set_lens(lens=lens)
    kw = dict(min_samples=SPP, max_samples=SPP)
    samples = []
    for s in range(SPP):
        idx = le.frame_indices(W, H, s)
        samples.append(o.radiance(lens_rays(rt, W, H, idx, lens), idx, rt.seed))
    want = le.fold(samples).reshape(H, W, 3)
    frames = {}
    for mode in ("wavefront", "megakernel", "rounds"):
        rt.set_render_mode(mode)
        frames[mode], spp = rt.run(W, H, want_spp=True, **kw)
        assert (spp == SPP).all()
    rmse = float(np.sqrt(((frames["wavefront"] - want) ** 2).mean()))
    print(f"{name}: rmse of the lens frame against the oracle on the lens rays {rmse:.3e}")
    assert rmse < pc.RMSE_TOL, rmse
    for mode in ("megakernel", "rounds"):
        assert le.same(frames[mode], frames["wavefront"]), mode
    rt.set_render_mode("wavefront")
    rt.set_lens(0.0)
    pin = rt.run(W, H, **kw)
    assert not le.same(pin, frames["wavefront"])                                   # the lens moved the frame
    # an adaptive frame (synchronous rounds) renders under the lens as well: its first min_samples are the fixed frame's
    rt.set_lens(lens=lens)
    ad, spp = rt.run(W, H, want_spp=True, min_samples=SPP, max_samples=SPP, noise_thresh=1e9)
    assert le.same(ad, frames["wavefront"])


# ---------------------------------------------------------------------------------------------------------------- 3. radius 0 is the pinhole
def test_radius_zero_is_bit_for_bit_the_context_that_never_heard_of_a_lens():
    _, a = new_rt("caustics")
    _, b = new_rt("caustics")
    b.set_lens(0.0, 16, 1.0)
    assert (b.lens.radius, b.lens.blades, b.lens.rotation) == (0.0, 16, 1.0) and (a.lens.radius, a.lens.blades, a.lens.rotation) == (0.0, 6, 0.0)
    for rt in (a, b):
        rt.tracePhotonsOnDevice(2000)
    kw = dict(min_samples=SPP, max_samples=SPP)
    fa, sa = a.run(W, H, want_spp=True, **kw)
    fb, sb = b.run(W, H, want_spp=True, **kw)
    assert le.same(fa, fb) and le.same(sa, sb)
    ga, gb = a.run_features(W, H, 2), b.run_features(W, H, 2)
    assert le.same(ga["features"], gb["features"]) and le.same(ga["ids"], gb["ids"])
    assert le.same(a.run_occlusion(W, H, n=2, dirs=8)["occlusion"], b.run_occlusion(W, H, n=2, dirs=8)["occlusion"])
    blobs = []
    for rt in (a, b):
        with rt.progressive(W, H, **kw) as s:
            s.step(3)
            blobs.append(s.save())
    assert blobs[0] == blobs[1] and gi.parse_checkpoint_header(blobs[0])["lens_tag"] == 0
    idx = all_indices(W, H, 2)
    assert le.same(a.primary_rays(a.params(W, H), idx), b.primary_rays(b.params(W, H), idx))


# ---------------------------------------------------------------------------------------------------------------- 4. focus, exact form
QUAD_HALF, TILES = 40.0, 20          # a 80 x 80 quad of 4 x 4 tiles
FOCUS_RADIUS = 0.5


def checker_scene(dist, cam_pos):
    """A black and white checkerboard quad perpendicular to cam_forward = (0, 0, -1), `dist` in front of z = cam_pos.z."""
    s = gi.Scene()
    tex = s.add_checkerboard((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), TILES)
    none = s.add_color_texture((0.0, 0.0, 0.0))
    m = s.add_material_tex(tex, none, 1.0, 1.0, 1.0)
    z, a = cam_pos[2] - dist, QUAD_HALF
    p = [(-a, -a, z), (a, -a, z), (a, a, z), (-a, a, z)]
    uv = [(0, 0), (1, 0), (1, 1), (0, 1)]
    # vertex normals given: a triangle interpolates its texture coordinates only where it interpolates normals (include/entities.h:478)
    s.add_triangles(np.array([[p[0], p[1], p[2]], [p[0], p[2], p[3]]], float), nrm=np.tile(np.array([0.0, 0.0, 1.0]), (2, 3, 1)), uv=np.array([[uv[0], uv[1], uv[2]], [uv[0], uv[2], uv[3]]], float), mat_idx=[m, m])
    s.add_light((0, 0, cam_pos[2]), (1, 1, 1), 0.1)
    s.set_camera(cam_pos, (cam_pos[0], cam_pos[1], cam_pos[2] - 1.0))
    return s.rebuild()


def edge_distance(hit_xy):
    """Distance of points [n][2] on the quad to the nearest tile edge."""
    tile = 2 * QUAD_HALF / TILES
    q = (hit_xy + QUAD_HALF) / tile
    return (np.abs(q - np.round(q)) * tile).min(1)


def pinhole_hits(cam, n, dist):
    """Where the pinhole rays of samples 0 .. n-1 meet the plane `dist` in front of the camera: [n][H * W][2] (x, y)."""
    out = []
    for s in range(n):
        r = le.rays(cam, W, H, le.frame_indices(W, H, s))
        t = (-dist) / r[:, 5]                                   # cam_forward = (0, 0, -1)
        out.append(r[:, 0:2] + t[:, None] * r[:, 3:5])
    return np.array(out)


def pick_camera(dist):
    """A camera position for which no pinhole hit on the plane at `dist` lies within 1e-9 of a tile edge (so no case has to be left out)."""
    for k in range(20):
        pos = (0.137 + 0.01 * k, -0.211, 5.0)
        scene = checker_scene(dist, pos)
        st = scene.settings
        cam = le.camera({"cam_pos": list(st.cam_pos), "cam_up": list(st.cam_up), "cam_forward": list(st.cam_forward), "sensor_diag": st.sensor_diag, "focal_dist": st.focal_dist})
        hits = pinhole_hits(cam, SPP, dist)
        if edge_distance(hits.reshape(-1, 2)).min() > 1e-9 and np.abs(hits).max() < QUAD_HALF:
            return scene, cam, hits
    raise AssertionError("no camera found")


def albedo_per_sample(rt, n):
    """The albedo (0 or 1) of samples 0 .. n-1 of every pixel, [n][H * W], from the means of run_features at 1 .. n samples (sums of 0s and 1s)."""
    counts = [np.zeros(H * W)]
    for k in range(1, n + 1):
        f = rt.run_features(W, H, k, want_ids=False)
        assert (f["coverage"] == 1).all()
        c = f["albedo"][:, :, 0].reshape(-1) * k
        assert np.abs(c - np.round(c)).max() < 1e-9
        counts.append(np.round(c))
    return np.diff(np.array(counts), axis=0)


def test_focus_sharp_plane_keeps_every_sample_and_blur_stays_within_the_radius():
    focal = gi.Scene().settings.focal_dist
    # the quad at the sharp plane: every lens ray goes through its pixel's point of that plane
    scene, cam, hits = pick_camera(focal)
    rt = gi.RayTracer(0).setScene(scene)
    pin = albedo_per_sample(rt, SPP)
    rt.set_lens(FOCUS_RADIUS, 6, 0.2)
    assert np.array_equal(albedo_per_sample(rt, SPP), pin) and 0 < pin.mean() < 1
    # the quad at twice that distance: a lens ray meets it within `radius` of where the pinhole ray does
    scene, cam, hits = pick_camera(2 * focal)
    rt = gi.RayTracer(0).setScene(scene)
    pin = albedo_per_sample(rt, SPP)
    rt.set_lens(FOCUS_RADIUS, 6, 0.2)
    lens = albedo_per_sample(rt, SPP)
    far = edge_distance(hits.reshape(-1, 2)).reshape(SPP, H * W) > FOCUS_RADIUS * 1.01
    assert far.any() and (~far).any()
    assert np.array_equal(lens[far], pin[far])
    assert (lens[~far] != pin[~far]).any()
    # autofocus (8.): after focus_at(distance of the far quad) the far quad is the sharp plane and every sample is the pinhole's again
    d = rt.focus_distance(W, H, W // 2, H // 2)
    assert abs(d - 2 * focal) <= 4 * np.spacing(2 * focal)
    rt.focus_at(d)
    assert rt.focal_dist == d and abs(rt.sensor_diag / rt.focal_dist - cam["sensor_diag"] / cam["focal_dist"]) < 1e-15
    assert np.array_equal(albedo_per_sample(rt, SPP), pin)


# ---------------------------------------------------------------------------------------------------------------- 5. features and occlusion
def test_features_and_occlusion_start_from_the_lens_rays(cornell):
    scene, rt, o, t = cornell
    lens = gi.lens_params(RADIUS, BLADES, ROTATION)
    dirs = 8
    rays, idxs = [], []
    for s in range(2):
        idxs.append(le.frame_indices(W, H, s))
        rays.append(lens_rays(rt, W, H, idxs[s], lens))
    assert fe.oracle_is_draw_free(o, rays[0])
    try:
        rt.set_lens(lens=lens)
        got = {n: rt.run_features(W, H, n) for n in (1, 2)}
        radius = oe.default_radius(t)
        ao = {n: rt.run_occlusion(W, H, n=n, dirs=dirs, radius=radius) for n in (1, 2)}
    finally:
        rt.set_lens(0.0)
    acc = np.zeros((H * W, 8))
    geo = []
    for s in range(2):
        hit, ent, mat, albedo, normal, depth, tex = fe.sample_features(o, t, rays[s])
        acc = acc + np.concatenate([albedo, normal, depth[:, None], hit.astype(np.float64)[:, None]], 1)
        if s == 0:
            assert np.array_equal(got[1]["ids"].reshape(-1, 2), np.stack([ent, mat], 1))
        assert le.same(got[s + 1]["features"], (acc / float(s + 1)).reshape(H, W, 8)), s      # depth = length(hit - the eye on the lens)
        # occlusion: the geometry dict of occlusion_expect.sample_geometry, from the lens rays
        hitb = hit.astype(bool)
        _, _, res, _ = o.trace(rays[s])
        N = res[:, 3:6]
        with np.errstate(divide="ignore", invalid="ignore"):
            nh = N * (1.0 / np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2]))[:, None]
        dn = (nh[:, 0] * rays[s][:, 3] + nh[:, 1] * rays[s][:, 4]) + nh[:, 2] * rays[s][:, 5]
        nf = np.where(hitb[:, None], np.where((dn > 0)[:, None], -nh, nh), 0.0)
        d = np.zeros((H * W, dirs, 3))
        hi = np.flatnonzero(hitb)
        d[hi] = oe.directions(nf[hi], idxs[s][hi], dirs)
        geo.append({"hit": hitb, "ent": ent, "O": np.where(hitb[:, None], res[:, 0:3] + oe.SHADOW_BIAS * nf, 0.0), "Nf": nf, "d": d})
    assert geo[0]["hit"].sum() > H * W // 2
    want = [oe.sample_values(g, oe.sample_open(o, g, radius))[0].reshape(H, W) for g in geo]
    c0 = ao[1]["open"] * dirs
    c01 = ao[2]["open"] * (dirs * 2)
    assert (c0 == np.round(c0)).all() and (c01 == np.round(c01)).all()
    counts = np.array([c0, c01 - c0]).astype(np.int64)
    differ, asked = int(np.abs(counts - np.array(want)).sum()), int(sum(g["hit"].sum() for g in geo)) * dirs
    print(f"occlusion under a lens: {differ} of {asked} segments differ from the oracle's")
    assert asked > 1000 and differ * 1000 <= asked, (differ, asked)


# ---------------------------------------------------------------------------------------------------------------- 6. sessions
def test_sessions_under_a_lens_and_the_checkpoint_tag():
    _, rt = new_rt("caustics")
    rt.tracePhotonsOnDevice(2000)
    lens = gi.lens_params(RADIUS, BLADES, ROTATION)
    rt.set_lens(lens=lens)
    kw = dict(min_samples=SPP, max_samples=SPP)
    ref = rt.run(W, H, **kw)
    with rt.progressive(W, H, **kw) as s:
        s.step(1)
        with pytest.raises(gi.GiError, match=r"\(-4\)"):
            rt.set_lens(0.1)                                       # refused while the session is open, and the session goes on
        assert rt.lens.radius == RADIUS
        s.step(1)
        blob = s.save()
        assert le.same(s.step(2), ref)
    assert gi.parse_checkpoint_header(blob)["lens_tag"] == gi.lens_tag(lens) != 0
    # a fresh context, the same lens: resume and finish on the same bits
    _, rt2 = new_rt("caustics")
    rt2.tracePhotonsOnDevice(2000)
    for other in (None, gi.lens_params(RADIUS, BLADES + 1, ROTATION), gi.lens_params(RADIUS * 2, BLADES, ROTATION)):
        if other is not None:
            rt2.set_lens(lens=other)
        with pytest.raises(gi.GiError, match=r"\(-2\)"):
            rt2.resume(blob)                                       # the pinhole, another blade count, another radius
    rt2.set_lens(lens=lens)
    with rt2.resume(blob) as s:
        assert s.sample_end == 2 and le.same(s.step(2), ref)
    # a pinhole checkpoint does not resume under a lens either
    rt2.set_lens(0.0)
    with rt2.progressive(W, H, **kw) as s:
        s.step(1)
        pin_blob = s.save()
    rt2.set_lens(lens=lens)
    with pytest.raises(gi.GiError, match=r"\(-2\)"):
        rt2.resume(pin_blob)


# ---------------------------------------------------------------------------------------------------------------- 7. stripes and groups
def test_stripes_and_a_group_assemble_to_the_one_context_lens_frame():
    scene, rt = new_rt("cornell")
    lens = gi.lens_params(RADIUS, BLADES, ROTATION)
    rt.set_lens(lens=lens)
    kw = dict(min_samples=2, max_samples=2)
    full = rt.run(W, H, **kw)
    frame = np.full_like(full, -7.0)
    for rank in range(2):                                          # two ranks, each a context of its own with the lens set
        _, r = new_rt("cornell")
        r.set_lens(lens=lens)
        frame[fe.frame_rows(H, 2, rank, 2)] = r.run(W, H, stripe_h=2, rank=rank, world=2, **kw)
    assert le.same(frame, full)
    grp = gi.RayTracerGroup([0, 0]).setScene(scene).set_lens(lens=lens)
    assert le.same(grp.run(rt.params(W, H, **kw), stripe_h=2), full)
    with pytest.raises(ValueError):
        grp.set_lens(blades=2)
    bad = gi.Lens(-1.0, 0.0, 6, 0)
    assert rt.L.gi_group_set_lens(grp.h, C.byref(bad)) == gi.GI_E_INVALID
    assert le.same(grp.run(rt.params(W, H, **kw), stripe_h=2), full)      # the group's lens stayed
    grp.set_lens(0.0)
    rt.set_lens(0.0)
    assert le.same(grp.run(rt.params(W, H, **kw), stripe_h=2), rt.run(W, H, **kw))


# ---------------------------------------------------------------------------------------------------------------- 8. autofocus
def test_focus_distance_is_the_oracle_on_the_pinhole_centre_ray(cornell):
    scene, rt, o, t = cornell
    cam = le.camera(rt)
    rt.set_lens(RADIUS)                                            # autofocus looks through the pinhole whatever the lens is
    try:
        for (x, y) in ((W // 2, H // 2), (0, 0), (W - 1, H - 1), (3, 7)):
            ray = le.pinhole_centre_ray(cam, W, H, x, y)
            hit, ent, res, _ = o.trace(ray)
            got = rt.focus_distance(W, H, x, y)
            if not hit[0]:
                assert got is None
                continue
            d = res[0, 0:3] - ray[0, 0:3]
            want = float(np.sqrt(le.dot(d, d)) * le.dot(ray[0, 3:6], cam["cam_forward"]))
            assert abs(got - want) <= 4 * np.spacing(want), (x, y, got, want)
    finally:
        rt.set_lens(0.0)
    # a miss: the camera turned away from the scene; the return code is 1 and dist is left alone
    rt2 = gi.RayTracer(0).setScene(scene)
    rt2.cam_forward = [-v for v in rt2.cam_forward]
    p = rt2.params(W, H)
    d = C.c_double(-7.0)
    assert rt2.L.gi_focus_distance(rt2.h, C.byref(p), 3, 3, C.byref(d)) == 1 and d.value == -7.0
    assert rt2.focus_distance(W, H, 3, 3) is None


# ---------------------------------------------------------------------------------------------------------------- 9. refusals
def test_refusals_leave_the_lens_the_timers_and_the_buffers_alone(cornell):
    scene, rt, o, t = cornell
    L = rt.L
    good = gi.lens_params(RADIUS, BLADES, ROTATION)
    rt.set_lens(lens=good)
    try:
        before = rt.run(W, H, min_samples=1, max_samples=1)
        ms = rt.last_render_ms()
        nan, inf = float("nan"), float("inf")
        for bad in (gi.Lens(-1e-9, 0, 6, 0), gi.Lens(nan, 0, 6, 0), gi.Lens(inf, 0, 6, 0), gi.Lens(1, nan, 6, 0), gi.Lens(1, inf, 6, 0), gi.Lens(1, 0, 2, 0),
                    gi.Lens(1, 0, 17, 0), gi.Lens(1, 0, -1, 0), gi.Lens(1, 0, 6, 1), gi.Lens(0, 0, 2, 0)):
            assert L.gi_set_lens(rt.h, C.byref(bad)) == gi.GI_E_INVALID, (bad.radius, bad.rotation, bad.blades, bad.reserved)
            assert b"set_lens" in L.gi_last_error(rt.h)
            xy = np.full((18, 2), -7.0)
            assert L.gi_lens_vertices(C.byref(bad), xy.ctypes.data_as(C.POINTER(C.c_double))) == gi.GI_E_INVALID and (xy == -7.0).all()
        assert L.gi_set_lens(rt.h, None) == gi.GI_E_INVALID and L.gi_set_lens(None, C.byref(good)) == gi.GI_E_INVALID
        assert L.gi_get_lens(rt.h, None) == gi.GI_E_INVALID and L.gi_lens_vertices(C.byref(good), None) == gi.GI_E_INVALID
        l = rt.lens
        assert (l.radius, l.rotation, l.blades, l.reserved) == (RADIUS, ROTATION, BLADES, 0)
        p = rt.params(W, H)
        idx = np.arange(4, dtype=np.uint32)
        rays = np.full((4, 6), -7.0)
        ip, rp = idx.ctypes.data_as(C.POINTER(C.c_uint32)), rays.ctypes.data_as(C.POINTER(C.c_double))
        assert L.gi_debug_primary_rays(rt.h, C.byref(p), -1, ip, rp) == gi.GI_E_INVALID
        assert L.gi_debug_primary_rays(rt.h, C.byref(p), 4, None, rp) == gi.GI_E_INVALID
        assert L.gi_debug_primary_rays(rt.h, None, 4, ip, rp) == gi.GI_E_INVALID
        assert L.gi_debug_primary_rays(rt.h, C.byref(rt.params(0, 5)), 4, ip, rp) == gi.GI_E_INVALID
        d = C.c_double(-7.0)
        for (x, y) in ((-1, 0), (W, 0), (0, H), (0, -1)):
            assert L.gi_focus_distance(rt.h, C.byref(p), x, y, C.byref(d)) == gi.GI_E_INVALID
        assert L.gi_focus_distance(rt.h, C.byref(p), 0, 0, None) == gi.GI_E_INVALID
        assert L.gi_focus_distance(gi.RayTracer(0).h, C.byref(p), 0, 0, C.byref(d)) == gi.GI_E_STATE
        assert (rays == -7.0).all() and d.value == -7.0
        assert rt.last_render_ms() == ms
        assert le.same(rt.run(W, H, min_samples=1, max_samples=1), before)
        for kw in (dict(radius=-1.0), dict(radius=nan), dict(blades=2), dict(blades=17), dict(blades=6.5), dict(rotation=inf)):
            with pytest.raises(ValueError):
                rt.set_lens(**kw)
        assert rt.lens.radius == RADIUS
    finally:
        rt.set_lens(0.0)


def test_cli_renders_under_the_lens_with_the_other_passes(tmp_path, capsys):
    from gi_raytracer_amd import __main__ as cli
    scn = os.path.join(pc.ROOT, pc.SCN["cornell"])
    assert cli.main([scn, "-o", str(tmp_path / "out.ppm"), "--pfm", str(tmp_path / "out.pfm"), "--width", str(W), "--height", str(H), "--samples", "2", "--photons", "0",
                     "--aperture", "0.3", "--blades", "5", "--blade-rotation", "20", "--focus-pixel", "6", "4", "--features", str(tmp_path / "f"), "--feature-samples", "2",
                     "--occlusion", str(tmp_path / "ao"), "--occlusion-samples", "1", "--occlusion-dirs", "4"]) == 0
    assert "lens radius 0.3, 5 blades" in capsys.readouterr().out
    _, rt = new_rt("cornell")
    rt.min_samples = rt.max_samples = 2
    rt.focus_at(rt.focus_distance(W, H, 6, 4))
    rt.set_lens(0.3, 5, math.radians(20.0))
    assert le.same(fe.read_pfm(tmp_path / "out.pfm"), rt.run(W, H, f64=False))
    assert le.same(fe.read_pfm(tmp_path / "f_depth.pfm"), rt.run_features(W, H, 2, f64=False, want_ids=False)["depth"])
    assert le.same(fe.read_pfm(tmp_path / "ao.open.pfm"), rt.run_occlusion(W, H, n=1, dirs=4, f64=False)["open"])
    rt.set_lens(0.0)
    assert not le.same(fe.read_pfm(tmp_path / "out.pfm"), rt.run(W, H, f64=False))
    # progressive, and a checkpoint that resumes only under the lens it was written with
    ck = str(tmp_path / "c.bin")
    common = [scn, "-o", str(tmp_path / "p.ppm"), "--pfm", str(tmp_path / "p.pfm"), "--width", str(W), "--height", str(H), "--samples", "2", "--photons", "0", "--progressive", "1",
              "--checkpoint", ck]
    assert cli.main(common + ["--aperture", "0.3", "--blades", "5", "--blade-rotation", "20", "--focus-pixel", "6", "4"]) == 0
    assert le.same(fe.read_pfm(tmp_path / "p.pfm"), fe.read_pfm(tmp_path / "out.pfm"))
    assert gi.parse_checkpoint_header(open(ck, "rb").read())["lens_tag"] != 0
    with pytest.raises(gi.GiError, match=r"\(-2\)"):
        cli.main(common)


def test_cpp_members_set_the_lens_and_move_the_focus(cornell):
    """RayTracer::setLens and focusAt of the drop-in C++ class (include/gi/raytracer.h) over the C ABI: tests/cpp/test_lens.cpp renders a frame under a
    lens and prints the sum of its depth buffer with all digits, for the Python mirror to match."""
    exe = os.path.join(pc.ROOT, "tests", "cpp", "test_lens")
    host_build.client("tests/cpp/test_lens.cpp", exe, "-O1")
    out = subprocess.run([exe, os.path.join(pc.ROOT, pc.SCN["cornell"]), str(W), str(H)], check=True, capture_output=True, text=True).stdout
    m = re.search(r"lens sum (\S+) pinhole sum (\S+) focused sum (\S+)", out)
    assert m and "bad lens refused 1" in out and "lens kept 1" in out, out
    _, rt = new_rt("cornell")

    def depth_sum():                # the C++ program adds in memory order
        s = 0.0
        for v in np.ascontiguousarray(rt.run_features(W, H, 2, want_ids=False)["depth"]).reshape(-1):
            s += float(v)
        return s
    pin = depth_sum()
    rt.set_lens(0.25, 7, 0.5)
    lens = depth_sum()
    rt.focus_at(6.0)
    focused = depth_sum()
    assert [float(m.group(k)) for k in (1, 2, 3)] == [lens, pin, focused] and len({lens, pin, focused}) == 3
