"""Frames whose sides are no multiple of the 8 x 8 tile, against the CPU oracle.

Every other frame the suite compares with the oracle has a width that is a multiple of 8, and the tests that render ragged shapes compare the
device with itself.  So the two record orders of gi_pixels.inc (st_pixel_xy with its right-edge and bottom-edge branches, tile_pixel_xy with
padding records to the right of the frame), k_render's own bounds test, halton_index where the enumeration's scale changes and global_row with
stripes shorter than a tile were pinned only by "every schedule makes the same mistake".  Here each of them faces the oracle, pixel by pixel.

One context and one oracle per scene (cornell without a photon map, caustics with 3000 photon indices emitted so that the gather and its sort
run); the oracle's frames are computed once per (shape, sample counts) and shared by the schedules and the tests.  No frame is larger than
61 x 47; 4 samples fixed, 4 .. 16 adaptive under check_render's threshold."""
import numpy as np
import pytest

import gi_raytracer_amd as gi

import lens_expect as le
import parity_checks as pc

pytestmark = pytest.mark.gpu

# the smallest shapes that take each branch of the record orders and of the Halton enumeration
SHAPES = [
    (1, 1),      # one pixel
    (1, 17),     # one column: tiles_x = 1, so the last tile is also the first; tw = 1
    (17, 1),     # one row: rows_full = 0, hr = 1; two padding columns per tile in rounds mode
    (7, 5),      # thinner than a tile both ways
    (8, 8),      # exactly one tile (control)
    (9, 8),      # one pixel over in x only
    (8, 9),      # one pixel over in y only
    (13, 9),     # both ragged (the shape the lens, occlusion, baked-light and feature passes use)
    (16, 9),     # width a power of two and height a power of three exactly
    (17, 10),    # one more than either: the Halton scale jumps
    (61, 47),    # several tiles, both ragged (the free-list test's shape)
]
SCENES = {"cornell": 0, "caustics": 3000}      # photon indices emitted; both hold RMSE < 1e-9 at 96 x 54 (test_render_matches_oracle)
MODES = ("wavefront", "rounds", "megakernel")
SPP = 4
TOL = 1e-9                                     # test_render_matches_oracle's bound for these scenes: any larger value means a diverged path
ids = lambda s: f"{s[0]}x{s[1]}"


@pytest.fixture(scope="module")
def ctx():
    """name -> (scene, context, FrameOracle holding the context's photon map), made on first use and kept for the module."""
    made = {}

    def get(name):
        if name not in made:
            scene = pc.load_scene(name)
            rt = gi.RayTracer(0).setScene(scene)
            made[name] = (scene, rt, pc.FrameOracle(rt, scene, SCENES[name]))
        return made[name]

    return get


def rmse(a, b):
    return float(np.sqrt(((a - b) ** 2).mean()))


def reference(o, w, h, adaptive):
    """The oracle's frame and sample counts, as check_render asks for them (so the answer is the kept one)."""
    return o.render(w, h, SPP, 4 * SPP, 0.0015) if adaptive else o.render(w, h, SPP)


# ---------------------------------------------------------------------------------------------------------------- 1. primary rays
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_primary_rays_and_halton_indices_of_every_pixel(ctx, shape):
    """Samples 0 .. 3 of every pixel: the device's Halton index equals the oracle's, and the pinhole ray the device makes for that index equals the
    oracle's bit for bit (the equality of test_gpu_lens.py).  No path is traced.  The indices are also checked without the oracle's enumeration:
    all different, and the two Halton numbers of each, scaled to the frame, fall inside the pixel the index was made for."""
    w, h = shape
    scene, rt, o = ctx("cornell")
    sxy, idx, rays = pc.frame_primary_rays(o, w, h, SPP)
    assert len(np.unique(idx)) == len(idx) == SPP * w * h
    # (the sampler scales its numbers by 1 - 2^-23, so one on a pixel's lower edge comes out some 1e-5 below it at most; samples 0 .. 3 sit at
    # 0, 1/4, 1/2, 3/4 and 0, 1/9, 1/3, 2/3 of a pixel, far from the upper edge)
    dx, dy = le.pixel_offsets(w, h, idx)
    assert np.array_equal(np.floor(dx + 1e-4), sxy[:, 1]) and np.array_equal(np.floor(dy + 1e-4), sxy[:, 2])
    assert np.array_equal(rt.halton_index(w, h, sxy), idx)
    got = rt.primary_rays(rt.params(w, h), idx)
    assert le.same(got, rays), (np.abs(got - rays).max(), int((got != rays).any(1).sum()))
    assert le.same(rays, le.rays(le.camera(rt), w, h, idx))          # and the numpy statement of the camera agrees with both


# ---------------------------------------------------------------------------------------------------------------- 2. frames
@pytest.mark.parametrize("adaptive", [False, True], ids=["fixed", "adaptive"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
@pytest.mark.parametrize("name", list(SCENES))
def test_frame_matches_oracle_in_every_schedule(ctx, name, shape, adaptive):
    """check_render (exact per-pixel sample counts, RMSE) in the three render modes, RMSE < 1e-9 on top, and the three frames the same bits.
    A frame that is self-consistent but wrong -- pixels permuted inside the last tile column, a pixel under another pixel's Halton index --
    differs from the oracle's by ~1e-2."""
    w, h = shape
    scene, rt, o = ctx(name)
    frames = {}
    try:
        for mode in MODES:
            rt.set_render_mode(mode)
            err, img, ref = pc.check_render(rt, scene, w, h, SPP, SCENES[name], adaptive, oracle=o)
            print(f"{name} {w}x{h} {'adaptive' if adaptive else 'fixed'} {mode}: rmse vs oracle {err:.3e}, max |diff| {np.abs(img - ref).max():.3e}")
            assert err < TOL, (mode, err)
            frames[mode] = img
    finally:
        rt.set_render_mode("wavefront")
    assert np.isfinite(frames["wavefront"]).all()
    for mode in MODES[1:]:
        assert le.same(frames[mode], frames["wavefront"]), mode


def test_the_frames_are_not_trivially_equal(ctx):
    """What makes the comparisons above able to fail: the frames have light in them, neighbouring pixels differ, the adaptive rule stops some
    pixels early and lets others go on, and the photon map changes the caustics frame."""
    for name in SCENES:
        scene, rt, o = ctx(name)
        lin = reference(o, 13, 9, False)["lin"]
        assert lin.mean() > 1e-3 and len(np.unique(lin.reshape(-1, 3), axis=0)) > 13 * 9 // 2, name
        assert len(np.unique(reference(o, 61, 47, True)["spp"])) >= 2, name
    scene, rt, o = ctx("caustics")
    assert len(scene.photon_tables()["photons"]) > 1000
    assert not np.array_equal(reference(o, 13, 9, False)["lin"], pc.FrameOracle(rt, scene, 0).render(13, 9, SPP)["lin"])     # (an oracle without the map)


# ---------------------------------------------------------------------------------------------------------------- 3. small pools
@pytest.mark.parametrize("shape", [(17, 1), (7, 5), (13, 9), (61, 47)], ids=ids)
def test_pool_smaller_than_the_frame(ctx, shape):
    """A pool of a third of the padded records' samples, refilled from the free list (wavefront) or worked off in rounds of one sample (rounds):
    the whole-pool frame bit for bit, which test 2 holds against the oracle."""
    w, h = shape
    scene, rt, o = ctx("caustics")
    kw = dict(min_samples=SPP, max_samples=SPP)
    whole, whole_spp = rt.run(w, h, want_spp=True, **kw)
    assert rmse(whole, reference(o, w, h, False)["lin"]) < TOL
    try:
        rt.set_pool_slots(max(64, pc.padded_records(w, h) * SPP // 3))
        for mode in ("wavefront", "rounds"):
            rt.set_render_mode(mode)
            img, spp = rt.run(w, h, want_spp=True, **kw)
            assert le.same(img, whole) and le.same(spp, whole_spp), mode
    finally:
        rt.set_pool_slots(1 << 30)
        rt.set_render_mode("wavefront")


# ---------------------------------------------------------------------------------------------------------------- 4. stripes
STRIPES = [((13, 9), sh, world) for sh in (1, 3, 5) for world in (2, 3)] + [((61, 47), sh, world) for sh in (1, 3, 5) for world in (2, 3)] + [
    ((7, 5), 8, 2),      # one stripe: rank 1 has no rows and returns an empty array
    ((7, 5), 2, 4)]      # three stripes (the last one a single row): rank 3 has none


@pytest.mark.parametrize("shape,stripe_h,world", STRIPES, ids=lambda v: ids(v) if isinstance(v, tuple) else str(v))
def test_stripes_shorter_than_a_tile(ctx, shape, stripe_h, world):
    """global_row with stripes of 1, 3 and 5 rows, a short last stripe and ranks without rows: the stripes assemble to the whole frame
    (check_stripes), and that frame is the oracle's."""
    w, h = shape
    scene, rt, o = ctx("caustics")
    empty = [r for r in range(world) if len(pc.stripe_rows(h, stripe_h, r, world)) == 0]
    assert shape != (7, 5) or len(empty) == 1        # (13 x 9 in stripes of 5 rows over 3 ranks has an idle rank too)
    for r in empty:
        part = rt.run(w, h, min_samples=SPP, max_samples=SPP, stripe_h=stripe_h, rank=r, world=world)
        assert part.shape == (0, w, 3)
    frame, counts = pc.check_stripes(rt, scene, w, h, SPP, world=world, stripe_h=stripe_h)
    assert rmse(frame, reference(o, w, h, False)["lin"]) < TOL and (counts == SPP).all()


def test_adaptive_stripes_keep_the_oracles_sample_counts(ctx):
    w, h = 13, 9
    scene, rt, o = ctx("caustics")
    frame, counts = pc.check_stripes(rt, scene, w, h, SPP, world=2, stripe_h=3, adaptive=True)
    ref = reference(o, w, h, True)
    assert np.array_equal(counts, ref["spp"]) and rmse(frame, ref["lin"]) < TOL


# ---------------------------------------------------------------------------------------------------------------- 5. sessions
@pytest.mark.parametrize("adaptive", [False, True], ids=["fixed", "adaptive"])
@pytest.mark.parametrize("shape", [(17, 1), (7, 5)], ids=ids)
def test_sessions_in_the_rounds_order_with_padding_to_the_right(ctx, shape, adaptive):
    """Progressive sessions whose records are in padded 8 x 8 tiles (render mode rounds; adaptive frames take that order in every mode), at
    shapes with padding records to the right of the frame: the last step leaves the one-shot frame and sample counts (and so the oracle's), and
    the count of pixels still wanting samples never exceeds the frame's pixels -- a padding record k_pix_wanting counted would show there."""
    w, h = shape
    scene, rt, o = ctx("caustics")
    kw = dict(min_samples=SPP, max_samples=4 * SPP, noise_thresh=0.0015) if adaptive else dict(min_samples=SPP, max_samples=SPP)
    ref = reference(o, w, h, adaptive)
    try:
        rt.set_render_mode("rounds")
        one, one_spp = rt.run(w, h, want_spp=True, **kw)
        assert np.array_equal(one_spp, ref["spp"]) and rmse(one, ref["lin"]) < TOL
        with rt.progressive(w, h, **kw) as s:
            img, spp = s.frame(want_spp=True)
            assert (img == 0.5).all() and (spp == 0).all() and s.pixels_wanting == w * h and not s.done
            for n in ((SPP, SPP, 2 * SPP) if adaptive else (2, 2)):
                assert s.pixels_wanting <= w * h              # before the last step
                img, spp = s.step(n, want_spp=True)
                assert s.pixels_wanting == int((ref["spp"] > s.sample_end).sum())     # exactly the pixels the finished frame gives more samples
            assert s.sample_end == kw["max_samples"] and s.pixels_wanting == 0 and s.done
            assert le.same(img, one) and le.same(spp, one_spp)
            assert le.same(s.frame(), one)                    # k_pix_resolve(tiled = 1) alone
    finally:
        rt.set_render_mode("wavefront")


# ---------------------------------------------------------------------------------------------------------------- 6. the f32 write
@pytest.mark.parametrize("mode", MODES)
def test_f32_frame_is_the_rounding_of_the_f64_frame(ctx, mode):
    w, h = 13, 9
    scene, rt, o = ctx("caustics")
    try:
        rt.set_render_mode(mode)
        for kw in (dict(min_samples=SPP, max_samples=SPP), dict(min_samples=SPP, max_samples=4 * SPP, noise_thresh=0.0015)):
            a = rt.run(w, h, **kw)
            b = rt.run(w, h, f64=False, **kw)
            assert b.dtype == np.float32 and le.same(b, a.astype(np.float32)), kw
    finally:
        rt.set_render_mode("wavefront")
