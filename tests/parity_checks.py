"""Backend-agnostic parity checks: the same assertions run on the CPU build of the device functions (not gpu) and on
the HIP library through the C ABI (gpu).  `rt` is a gi_raytracer_amd.RayTracer-like object; the oracle is the checker."""
import os

import numpy as np

import gi_raytracer_amd as gi
import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCN = {"test_scene": "scenes/test_scene/test.scn", "cornell": "scenes/cornell/test.scn", "caustics": "scenes/caustics/caustics.scn", "caustics_02": "scenes/caustics_02/caustics.scn",
       "teapot": "scenes/cornell/teapot.scn", "textures": "scenes/textures/tex.scn", "textures_opaque": "scenes/textures/tex_opaque.scn", "cornell_tex": "scenes/textures/cornell_tex.scn", "spheres": "scenes/spheres/spheres.scn", "spheres_opaque": "scenes/spheres/spheres_opaque.scn", "fog": "scenes/fog/fog.scn"}

# float tolerance of the path (north_star: pixel RMSE < 1e-4 on linear radiance); measured values are ~1e-16
RMSE_TOL = 1e-4


def load_scene(name):
    return gi.Scene.load(os.path.join(ROOT, SCN[name])).rebuild()


def oracle_for(scene):
    t, st = scene.tables(), scene.settings
    o = ol.Oracle().set_scene(t["tri_pos"], t["tri_nrm"], t["tri_uv"], t["tri_mat"], t["mats"], t["lights"][:, :7], t["ambient"], kind=t["ent_kind"])
    o.set_camera(list(st.cam_pos), list(st.cam_up), list(st.cam_forward), st.sensor_diag, st.focal_dist)
    if len(t["tex_kind"]):
        o.set_textures(t["tex_kind"], t["tex_param"], t["mat_tex"], t["tex_pixels"])
    if len(t["fog"]):
        o.set_fog(t["fog"], t["fog_grid_off"], t["fog_grid"])     # the same noise grid the product's loader generated
    return o.build_octree()


def check_halton(rt, golden):
    g = golden("halton")
    idxs, ref = g["halton_sample_idx"], g["halton_sample"]
    dims = np.repeat(np.arange(256, dtype=np.uint32), len(idxs))
    got = rt.halton_sample(dims, np.tile(idxs, 256)).reshape(256, len(idxs))
    assert got.tobytes() == ref.tobytes()                       # bit-exact floats, all 256 dimensions
    sizes = g["halton_enum_params"][:, :2]
    for k in range(len(sizes)):
        rows = g["halton_enum_index"][g["halton_enum_index"][:, 0] == k]
        got = rt.halton_index(int(sizes[k][0]), int(sizes[k][1]), rows[:, 1:4])
        assert np.array_equal(got, rows[:, 4])


def check_kats(rt, golden):
    """a-11: the samplers, fastPow / fastPrecisePow, refr, reflect as the device computes them, against the reference's known answers
    (tests/golden/kat.npz, captured from include/util.h / util.cpp).  fastPow / fastPrecisePow are integer bit manipulation + exact
    products: bit-exact.  The samplers go through sin / cos / acos / sqrt: bit-exact on the CPU build (glibc, like the reference); on the
    GPU the libm is OCML, whose results may differ from glibc's in the last bit, so the bound there is 4 ulp of the result's magnitude
    scale (1.0: these are unit vectors), with the share of bit-exact answers reported."""
    k = golden("kat")
    exact = getattr(rt, "libm_is_glibc", False)

    def close(got, ref, what):
        if exact:
            assert got.tobytes() == np.ascontiguousarray(ref).tobytes(), what
        else:
            assert np.abs(got - ref).max() <= 4 * 2.0 ** -52, (what, np.abs(got - ref).max())
    pw = k["kat_pow"]
    assert rt.kat("fastPow", pw[:, :2])[:, 0].tobytes() == np.ascontiguousarray(pw[:, 2]).tobytes()
    assert rt.kat("fastPrecisePow", pw[:, :2])[:, 0].tobytes() == np.ascontiguousarray(pw[:, 3]).tobytes()
    h = k["kat_hemi"]
    close(rt.kat("hemisphereSample_cos", h[:, :6]), h[:, 6:9], "hemisphereSample_cos")
    ph = k["kat_phong"]
    close(rt.kat("sample_phong", np.concatenate([ph[:, 0:3], ph[:, 6:9]], 1)), ph[:, 9:12], "sample_phong")
    c = k["kat_cap"]
    close(rt.kat("sphereCapSample_cos", c[:, :7]), c[:, 7:10], "sphereCapSample_cos")
    u = k["kat_unitvec"]
    close(rt.kat("randomUnitVec", u[:, :2]), u[:, 2:5], "randomUnitVec")
    r = k["kat_refr"]
    assert rt.kat("refr", r[:, :7]).tobytes() == np.ascontiguousarray(r[:, 7:10]).tobytes()        # +, *, sqrt only: IEEE-exact everywhere
    assert rt.kat("reflect", r[:, :6]).tobytes() == np.ascontiguousarray(r[:, 10:13]).tobytes()


def check_rng(rt):
    """a-16: the counter RNG that stands in for drand() (include/util.h:52-80 is a sequential xorshift64* chain a parallel device cannot replay;
    DESIGN.md "RNG contract"), as the device evaluates it through gi_kat, against the oracle's on a lattice of (seed, stream, depth, purpose, a, b):
    every draw bit-exact (integer mixing + one exact scaling), and the stream key too -- a regression in the key mixing shows here, not as a frame."""
    L = ol.lib()
    rs = np.random.RandomState(16)
    seeds = [0, 1, gi.DEFAULT_SEED, 0xffffffffffffffff, 0x5048544f4e5eed00 ^ gi.DEFAULT_SEED] + [int(v) for v in rs.randint(0, 2**63, 6, dtype=np.int64)]
    streams = [0, 1, 2, 1146617855, 2**31 - 1, 2**31, 2**32 - 1] + [int(v) for v in rs.randint(0, 2**32, 6, dtype=np.int64)]
    depths = [0, 1, 2, 3, 10, 63, 64, 65]
    purposes = [0, 1, 2, 3, 4, 5, 6, 7, 8, 16, 17, 18, 19, 20, 21, 22, 1 | (1 << 8), 2 | (3 << 8), 7 | (255 << 8)]
    ab = [(0, 0), (1, 0), (0, 1), (1557, 2191), (2**32 - 1, 2**32 - 1), (17, 2**31)] + [(int(a), int(b)) for a, b in rs.randint(0, 2**32, (6, 2), dtype=np.int64)]
    rows = [(sd, st, d, pu, a, b) for sd in seeds for st in streams for d in depths for pu in purposes for (a, b) in ab[:4]]
    rows += [(seeds[2], st, 1, pu, a, b) for st in streams for pu in purposes for (a, b) in ab[4:]]
    arg = np.array([[sd >> 32, sd & 0xffffffff, st, d, pu, a, b] for (sd, st, d, pu, a, b) in rows], np.float64)
    got = rt.kat("rng", arg)
    want = np.array([L.gio_counter_rand(sd, st, d, pu, a, b) for (sd, st, d, pu, a, b) in rows])
    assert got[:, 0].tobytes() == want.tobytes()
    assert ((got[:, 0] >= 0) & (got[:, 0] < 1)).all()
    # distinct keys of one seed give distinct draws (across seeds the contract lets (seed, stream) and (seed + golden ratio, stream - 1) coincide)
    for sd in seeds:
        d = got[[r[0] == sd for r in rows], 0]
        assert len(np.unique(d)) == len(d)
    # the stream key alone (what rng_make leaves in the lane's registers): draws of one stream at depth 0, purpose 0 agree => keys agree; and
    # distinct streams of one seed have distinct keys
    keys = got[:, 1] * 2.0 ** 32 + got[:, 2]
    first = {}
    for r, k in zip(rows, keys):
        assert first.setdefault((r[0], r[1]), k) == k
    for sd in seeds:
        ks = [k for (s_, _), k in first.items() if s_ == sd]
        assert len(set(ks)) == len(ks)
    return len(rows)


def check_leaf_order(rt, fx, set_wide=None):
    """a-4: the leaves the device walk meets for a ray, in order, against Octree::intersectSorted's t0-sorted list of the reference
    (leaforder_* of the scene fixtures).  The reference orders leaves with equal t0 by insertion (pre-order DFS, include/octree.cpp:285-313);
    the device's front-to-back order may permute such a group, never anything else -- and the test says how many rays had such a group."""
    rays = fx["rays"][fx["leaforder_ray"]]
    off, node, t0 = fx["leaforder_off"], fx["leaforder_node"], fx["leaforder_t0"]
    out = {}
    for wide in ((True, False) if set_wide is not None else (None,)):
        if wide is not None and set_wide(wide) != wide:
            continue                                     # a tree the wide records do not cover walks per node either way
        got = rt.leaf_order(rays)
        n_exact = n_tie = 0
        for j, g in enumerate(got):
            ref, rt0 = node[off[j]:off[j + 1]], t0[off[j]:off[j + 1]]
            assert len(g) == len(ref), (j, g, ref)
            if np.array_equal(g, ref):
                n_exact += 1
                continue
            # same leaves; every leaf stays inside its group of equal t0
            assert sorted(g) == sorted(ref), (j, g, ref)
            pos = {int(v): i for i, v in enumerate(ref)}
            assert all(rt0[pos[int(v)]] == rt0[i] for i, v in enumerate(g)), (j, g, ref, rt0)
            n_tie += 1
        out[wide] = (n_exact, n_tie)
        assert n_exact > 0.9 * len(got), out
    if set_wide is not None:
        set_wide(True)
    return out


def check_trace_table(rt, fx):
    """RayTracer::trace against the reference's own answers: hit flag / entity index exact, hit point and normal bit-exact."""
    hit, ent, res = rt.trace(fx["rays"])
    assert np.array_equal(hit, fx["trace_hit"])
    assert np.array_equal(ent, fx["trace_ent"])
    assert np.array_equal(res[:, :6], fx["trace_res"][:, :6])


def check_visible_table(rt, fx):
    assert np.array_equal(rt.visible(fx["shadow_q"]), fx["shadow_vis"])


def check_gather_table(rt, scene, fx):
    scene.build_photon_map(fx["photons"])
    rt.upload_photon_map()
    res, nc = rt.samplePhotons(fx["gather_q"])
    assert np.array_equal(nc, fx["gather_ncand"])                # candidate counts exact
    ref = fx["gather_res"]
    assert np.array_equal(res == 0, ref == 0)
    np.testing.assert_allclose(res, ref, rtol=1e-9, atol=1e-300)  # summation order differs (distance-sorted vs leaf order)


def check_emission(rt, scene, n):
    """tracePhotons: identical photon set (every draw is keyed) as the oracle."""
    o = oracle_for(scene)
    ph, tries = rt.tracePhotons(n)
    on, otries = o.emit_photons(n, 5, ol.RNG_COUNTER, rt.seed)
    oph = o.get_photons()
    assert len(ph) == on and tries == otries
    # same photons; refraction through glass amplifies the <=1 ulp differences between OCML and glibc sin/cos/acos
    np.testing.assert_allclose(ph, oph, rtol=1e-9, atol=1e-12)
    return o, ph


class FrameOracle:
    """oracle_for(scene) holding the photon map `rt` holds after tracePhotons(photons) (none for photons = 0), for tests that compare many
    frames of one context with the oracle: check_render(..., oracle=this) emits and builds nothing, and render() keeps its answer per argument
    list (read-only arrays), so that the schedules of one frame share one reference.  Everything else is the oracle's own."""

    def __init__(self, rt, scene, photons):
        self.o = oracle_for(scene)
        if photons > 0 and scene.desc().n_light > 0:
            ph, _ = rt.tracePhotons(photons)
            self.o.set_photons(ph)
        self.o.build_photon_map()
        self._frames = {}

    def render(self, *args):
        if args not in self._frames:
            ref = self.o.render(*args)
            for a in ref.values():
                a.setflags(write=False)
            self._frames[args] = ref
        return self._frames[args]

    def __getattr__(self, name):
        return getattr(self.o, name)


def check_render(rt, scene, w, h, spp, photons, adaptive=False, tol=RMSE_TOL, spp_mismatch=0.0, oracle=None):
    """oracle: a FrameOracle of rt and scene, which holds rt's photon map already; without one, an oracle is built and `photons` emitted here."""
    o = oracle
    if o is None:
        o = oracle_for(scene)
        if photons > 0 and scene.desc().n_light > 0:
            ph, _ = rt.tracePhotons(photons)
            o.set_photons(ph)
        o.build_photon_map()
    if adaptive:
        img, nspp = rt.run(w, h, min_samples=spp, max_samples=4 * spp, noise_thresh=0.0015, want_spp=True)
        ref = o.render(w, h, spp, 4 * spp, 0.0015)
        assert (nspp != ref["spp"]).mean() <= spp_mismatch       # per-pixel sample counts are integer work: exact (spp_mismatch = 0)
    else:
        img, nspp = rt.run(w, h, min_samples=spp, max_samples=spp, want_spp=True)
        ref = o.render(w, h, spp)
        assert (nspp == spp).all(), (np.unique(nspp, return_counts=True), float(img.mean()))
    rmse = float(np.sqrt(((img - ref["lin"]) ** 2).mean()))
    assert rmse < tol, rmse
    return rmse, img, ref["lin"]


def frame_primary_rays(o, w, h, n):
    """The oracle's primary rays of samples 0 .. n-1 of every pixel of a w x h frame, sample after sample and row-major inside one:
    (sxy [m][3] uint32 = sample, x, y; Halton index [m] uint32; rays [m][6] = origin, unit direction)."""
    sxy = np.array([(s, x, y) for s in range(n) for y in range(h) for x in range(w)], np.uint32)
    got = [o.primary_ray(w, h, int(s), int(x), int(y)) for s, x, y in sxy]
    return sxy, np.array([i for i, _ in got], np.uint32), np.array([r for _, r in got])


def padded_records(w, h):
    """Records of the rounds schedule for a w x h frame: whole 8 x 8 tiles (gi_pixels.inc: tile_pixel_xy)."""
    return ((w + 7) // 8) * ((h + 7) // 8) * 64


def two_light_scene(with_glass=True):
    """A floor, a diffuse and a glass (or second diffuse) block, two lights of different colour (no reference scene has more than one): the reference keeps the
    share of the LAST visible light of a vertex (`i = ...` inside its light loop, include/raytracer.h), photons are emitted per (index, light)."""
    s = gi.Scene()
    white = s.add_material(1, 1, 1, (0.8, 0.8, 0.8)); red = s.add_material(1, 1, 1, (0.8, 0.3, 0.2)); glass = s.add_material(0, 0, 1.5, (1, 1, 1))
    quad = lambda a, b, c, d: [[a, b, c], [a, c, d]]
    tris, mats = [], []
    def box(lo, hi, m):
        (x0, y0, z0), (x1, y1, z1) = lo, hi
        f = [((x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0)), ((x0, y0, z1), (x0, y1, z1), (x1, y1, z1), (x1, y0, z1)),
             ((x0, y0, z0), (x0, y1, z0), (x0, y1, z1), (x0, y0, z1)), ((x1, y0, z0), (x1, y0, z1), (x1, y1, z1), (x1, y1, z0)),
             ((x0, y1, z0), (x1, y1, z0), (x1, y1, z1), (x0, y1, z1)), ((x0, y0, z0), (x0, y0, z1), (x1, y0, z1), (x1, y0, z0))]
        for q in f:
            tris.extend(quad(*q)); mats.extend([m, m])
    tris.extend(quad((-4, 0, -4), (-4, 0, 4), (4, 0, 4), (4, 0, -4))); mats.extend([white, white])
    box((-1.6, 0.001, -0.4), (-0.6, 1.0, 0.6), red)
    box((0.5, 0.001, -0.7), (1.5, 1.2, 0.3), glass if with_glass else white)
    s.add_triangles(np.array(tris, float), mat_idx=mats)
    s.add_light((-2.5, 4, 1.5), (9, 7, 5), 0.1)
    s.add_light((3, 3.5, 2), (3, 5, 9), 0.15)
    s.set_camera((0.2, 2.2, 5.5), (0, 0.5, 0))
    return s.rebuild()


# the lights of many_lights_scene: different sides and heights, distinct colours and radii (the first n are used)
MANY_LIGHTS = [((-2.5, 4.0, 1.5), (9, 7, 5), 0.10), ((3.0, 3.5, 2.0), (3, 5, 9), 0.15), ((0.4, 3.0, -3.2), (6, 9, 4), 0.05), ((-3.6, 2.4, -0.8), (8, 3, 7), 0.20),
               ((3.4, 2.0, -1.6), (4, 8, 8), 0.12), ((0.3, 5.0, 3.0), (7, 7, 2), 0.08)]
# thin slabs: a canopy over the front of the left block, one over the right block's front, a wall at the left, a wall at the back; the canopies' tops are the highest y
MANY_LIGHTS_SLABS = [((-2.1, 1.45, 0.2), (-0.2, 1.5, 1.9)), ((0.2, 1.45, -0.1), (2.2, 1.5, 1.6)), ((-2.7, 0.001, -1.6), (-2.65, 1.4, 1.2)), ((-2.2, 0.001, -1.65), (2.4, 1.4, -1.6))]
SHADOW_BIAS = 1e-4      # include/raytracer.h: the shadow segment starts at hit + SHADOW_BIAS * normal


def many_lights_scene(n_lights, emitter=False, fog=False):
    """two_light_scene(False)'s floor and blocks (diffuse only) under the first n_lights of MANY_LIGHTS, with thin slabs between them so that which
    lights a vertex sees differs from vertex to vertex: two canopies whose top faces are the scene's highest (a shadow segment that starts on one
    misses the scene's box), a wall at the left and a mirror wall at the back (no glass: nothing refracts).  The reference keeps the share of the LAST visible light of a vertex, so a walk
    from the last light down stops at another light in every part of the picture (many_lights_census counts the parts).  emitter: the left block
    has diffuse and emissive colour, so a vertex on it carries A0 beside its queries; fog: a HeightFog slab over the right half of the floor, which the
    segments from there cross and the ones from the left do not; it reaches above the right canopy, so that the segments which miss the scene's box are
    answered by the medium."""
    s = gi.Scene()
    white = s.add_material(1, 1, 1, (0.8, 0.8, 0.8)); grey = s.add_material(1, 1, 1, (0.5, 0.5, 0.55))
    red = s.add_material(1, 1, 1, (0.8, 0.3, 0.2), (0.6, 0.45, 0.1) if emitter else (0, 0, 0))
    quad = lambda a, b, c, d: [[a, b, c], [a, c, d]]
    tris, mats = [], []
    def box(lo, hi, m):
        (x0, y0, z0), (x1, y1, z1) = lo, hi
        f = [((x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0)), ((x0, y0, z1), (x0, y1, z1), (x1, y1, z1), (x1, y0, z1)),
             ((x0, y0, z0), (x0, y1, z0), (x0, y1, z1), (x0, y0, z1)), ((x1, y0, z0), (x1, y0, z1), (x1, y1, z1), (x1, y1, z0)),
             ((x0, y1, z0), (x1, y1, z0), (x1, y1, z1), (x0, y1, z1)), ((x0, y0, z0), (x0, y0, z1), (x1, y0, z1), (x1, y0, z0))]
        for a, b, c, d in f:                             # wound so that the normals point outwards (two_light_scene's point inwards: its blocks' faces
            tris.extend(quad(a, d, c, b)); mats.extend([m, m])   # start their shadow segments inside the block and see no light at all)
    tris.extend(quad((-4, 0, -4), (-4, 0, 4), (4, 0, 4), (4, 0, -4))); mats.extend([white, white])
    # a foot under the floor, as in large_alpha_scene: with the floor ON the root box's lower face a vertex there (y = +-1e-16) gathers or not by the last
    # bit of the bounce that led to it (device libm against glibc) -- seen on the MI355X without the foot: 34 of 5 184 pixels, RMSE 6e-5 .. 1.5e-4 with
    # a photon map and 1e-18 without one, the same bits in every schedule
    tris.extend(quad((-0.5, -0.37, -0.5), (-0.5, -0.37, 0.5), (0.5, -0.37, 0.5), (0.5, -0.37, -0.5))); mats.extend([white, white])
    box((-1.6, 0.001, -0.4), (-0.6, 1.0, 0.6), red)
    box((0.5, 0.001, -0.7), (1.5, 1.2, 0.3), white)
    mirror = s.add_material(0, 1, 1, (0.9, 0.9, 0.9))    # opaque; reflect() is +, * only, the same bits with every libm.  The photon map keeps
    for k, (lo, hi) in enumerate(MANY_LIGHTS_SLABS):     # caustic photons only: without a specular surface no photon would be stored at all
        box(lo, hi, mirror if k == 3 else grey)
    s.add_triangles(np.array(tris, float), mat_idx=mats)
    for pos, col, rad in MANY_LIGHTS[:n_lights]:
        s.add_light(pos, col, rad)
    if fog:
        s.add_height_fog((2.0, 1.0, 0.5), (3.6, 2.0, 5.0), (0.8, 0.85, 1.0), 4, 0.5, 4)    # x 0.2 .. 3.8, y 0 .. 2: the right canopy's top lies in it
    s.set_camera((0.2, 2.2, 5.5), (0, 0.5, 0))
    return s.rebuild()


MANY_LIGHTS_NAMES = {"three_lights": (3, False, False), "four_lights": (4, False, False), "five_lights": (5, False, False), "six_lights": (6, False, False),
                     "four_lights_emitter": (4, True, False), "three_lights_fog": (3, False, True)}


def _segment_meets_box(a, b, lo, hi):
    """Whether the segments a[i] -> b[i] touch the box [lo, hi] (slab test in numpy)."""
    d = b - a
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - a) / d, (hi - a) / d
    par = d == 0
    tn = np.where(par, np.where((a >= lo) & (a <= hi), -np.inf, np.inf), np.minimum(t0, t1))
    tf = np.where(par, np.where((a >= lo) & (a <= hi), np.inf, -np.inf), np.maximum(t0, t1))
    return np.maximum(tn.max(axis=1), 0.0) <= np.minimum(tf.min(axis=1), 1.0)


def many_lights_census(scene, w=96, h=54):
    """Which branches of the several-lights shadow path a frame of `scene` reaches, from the oracle alone: the first hits of the w x h sample-0 primary
    rays, and whether the segment from hit + SHADOW_BIAS * normal to each light's centre is free.  Returns the number of hit vertices per class:
      last            the last light is visible (the first query asked answers the item)
      second_last     the last light is hidden, the one before it visible (one step of k_st_shadow's loop)
      earlier         (3+ lights) the last two are hidden and an earlier one is visible (two or more steps)
      light0_only     (4 lights) lights 3, 2 and 1 are hidden, light 0 is visible
      none            every light is hidden
      outside_box     the segment starts outside the scene's root box (above a top face at its highest y): no walk begins
      emitter_lit / emitter_dark   the hit is on an emitting surface, with a visible light / with none
      fog_crossed / fog_missed   the segment to the winning (last visible) light crosses the medium's box / does not
      fog_outside_box            it crosses the medium's box and starts outside the scene's root box"""
    o = oracle_for(scene)
    t = scene.tables()
    lights = t["lights"][:, :3]
    n = len(lights)
    rays = np.array([o.primary_ray(w, h, 0, x, y)[1] for y in range(h) for x in range(w)])
    hit, ent, res, _ = o.trace(rays)
    k = hit > 0
    org = res[k, :3] + SHADOW_BIAS * res[k, 3:6]
    vis = np.stack([o.visible(np.concatenate([org, np.broadcast_to(l, org.shape)], 1))[0] > 0 for l in lights], 1)
    root = o.octree()[0][0]
    assert np.all(lights[:, 1] > root[4])                      # every light hangs above the box: a segment that starts above it never enters it
    out = {"vertices": int(k.sum()), "last": int(vis[:, -1].sum()), "second_last": int((~vis[:, -1] & vis[:, -2]).sum()), "none": int((~vis.any(1)).sum()),
           "outside_box": int((org[:, 1] > root[4]).sum())}
    if n >= 3:
        out["earlier"] = int((~vis[:, -1] & ~vis[:, -2] & vis[:, :-2].any(1)).sum())
    if n == 4:
        out["light0_only"] = int((~vis[:, 1:].any(1) & vis[:, 0]).sum())
    emits = (t["mats"][:, 6:9] != 0).any(1)[t["tri_mat"]][ent[k]]
    if (t["mats"][:, 6:9] != 0).any():
        out["emitter_lit"] = int((emits & vis.any(1)).sum())
        out["emitter_dark"] = int((emits & ~vis.any(1)).sum())
    if len(t["fog"]):
        f = t["fog"][0]
        win = n - 1 - np.argmax(vis[:, ::-1], axis=1)          # the last visible light (rows without one are masked out below)
        crossed = _segment_meets_box(org, lights[win], f[:3] - 0.5 * f[3:6], f[:3] + 0.5 * f[3:6])
        out["fog_crossed"] = int((vis.any(1) & crossed).sum())
        out["fog_missed"] = int((vis.any(1) & ~crossed).sum())
        out["fog_outside_box"] = int((crossed & (org[:, 1] > root[4])).sum())      # no walk begins and the medium alone answers, light after light
    return out


def coplanar_scene():
    """Entities that lie in one plane and overlap (a patch on the floor of a room, a panel in its ceiling -- what a Cornell box's light is): a ray into the
    overlap meets two entities at exactly the same distance and RayTracer::trace keeps the one it asks first (include/raytracer.h:446-472, strict <).
    The large floor triangles reach through many leaves, the patch through few, blocks on the floor make the octree split around them."""
    s = gi.Scene()
    white = s.add_material(1, 1, 1, (0.8, 0.8, 0.8)); red = s.add_material(1, 1, 1, (0.8, 0.3, 0.2)); blue = s.add_material(1, 1, 1, (0.2, 0.3, 0.8))
    quad = lambda a, b, c, d: [[a, b, c], [a, c, d]]
    tris, mats = [], []
    def put(q, m):
        tris.extend(quad(*q)); mats.extend([m, m])
    put(((-4, 0, -4), (-4, 0, 4), (4, 0, 4), (4, 0, -4)), white)                      # floor
    put(((-4, 4, -4), (4, 4, -4), (4, 4, 4), (-4, 4, 4)), white)                      # ceiling
    put(((-1.5, 0, -1.25), (-1.5, 0, 2.5), (2.25, 0, 2.5), (2.25, 0, -1.25)), red)    # patch in the floor's plane
    put(((-1, 4, -1), (1, 4, -1), (1, 4, 1), (-1, 4, 1)), blue)                       # panel in the ceiling's plane
    put(((-1.5, 0, -1.25), (-1.5, 0, 2.5), (2.25, 0, 2.5), (2.25, 0, -1.25)), blue)   # and the patch once more: the very same triangles
    rs = np.random.RandomState(11)
    for k in range(40):                                                               # small blocks standing on the floor
        x, z = rs.uniform(-3.5, 3.3, 2)
        w, h = rs.uniform(0.05, 0.2), rs.uniform(0.1, 0.6)
        (x0, y0, z0), (x1, y1, z1) = (x, 0.0, z), (x + w, h, z + w)
        for q in (((x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0)), ((x0, y0, z1), (x0, y1, z1), (x1, y1, z1), (x1, y0, z1)),
                  ((x0, y0, z0), (x0, y1, z0), (x0, y1, z1), (x0, y0, z1)), ((x1, y0, z0), (x1, y0, z1), (x1, y1, z1), (x1, y1, z0)),
                  ((x0, y1, z0), (x1, y1, z0), (x1, y1, z1), (x0, y1, z1))):
            put(q, white)
    s.add_triangles(np.array(tris, float), mat_idx=mats)
    s.add_light((0, 3.5, 0), (9, 9, 9), 0.1)
    s.set_camera((0.2, 2.2, 5.5), (0, 0.5, 0))
    return s.rebuild()


def check_equal_distance_hits(rt, scene, set_wide):
    """Rays into overlapping coplanar entities: the walk with its short cuts (boxes cut to the leaves, no look behind the best hit) returns the entity
    the plain per-node walk returns -- the one the reference meets first -- bit for bit, also where two or three entities tie."""
    rs = np.random.RandomState(3)
    n = 20000
    o = np.stack([rs.uniform(-3.5, 3.5, n), rs.uniform(0.5, 3.5, n), rs.uniform(-3.5, 3.5, n)], 1)
    tgt = np.stack([rs.uniform(-2.5, 3.0, n), np.where(rs.rand(n) < 0.7, 0.0, 4.0), rs.uniform(-2.0, 3.0, n)], 1)
    d = tgt - o
    d /= np.linalg.norm(d, axis=1)[:, None]
    rays = np.concatenate([o, d], 1)
    assert set_wide(True)
    hit_w, ent_w, res_w = rt.trace(rays)
    set_wide(False)
    hit_n, ent_n, res_n = rt.trace(rays)
    set_wide(True)
    assert np.array_equal(hit_w, hit_n) and np.array_equal(ent_w, ent_n)
    assert np.array_equal(res_w[hit_w > 0].view(np.uint64), res_n[hit_n > 0].view(np.uint64))
    ents = set(ent_w[hit_w > 0].tolist())
    assert ents & {0, 1} and ents & {2, 3} and len(ents) > 20         # floor, ceiling, blocks
    return ents


def _load_png(path):
    """[h][w][4] uint8 and whether the file has an alpha channel, through the product's own decoder (the `imTex` loader)."""
    import ctypes as C
    L = gi.lib()
    w, h, a = C.c_int32(), C.c_int32(), C.c_int32()
    px = C.POINTER(C.c_uint8)()
    err = C.create_string_buffer(256)
    assert L.gih_load_png(os.fsencode(path), C.byref(w), C.byref(h), C.byref(a), C.byref(px), err, 256) == 0, err.value
    arr = np.ctypeslib.as_array(px, (h.value, w.value, 4)).copy()
    L.gih_free(px)
    return arr, bool(a.value)


def alpha_entities(scene):
    """Which entities RayTracer::trace puts to the alpha test (include/raytracer.h:455): opacity below 1 or an image with an alpha channel, and IOR 1."""
    t = scene.tables()
    mats = t["mats"]
    alpha = mats[:, 1] < 1.0
    if len(t["tex_kind"]):
        dt = t["mat_tex"][:, 0]
        alpha |= (dt >= 0) & (t["tex_kind"][np.where(dt >= 0, dt, 0)] == 2) & (t["tex_param"][np.where(dt >= 0, dt, 0), 4] != 0)
    return (alpha & (mats[:, 2] == 1.0))[t["tri_mat"]]


def large_alpha_scene(opacity=0.5, textured=False):
    """Large entities with an alpha test, reaching through many leaves: an 8 x 8 floor (on a small foot), 60 small opaque blocks that make the octree split, and
    12 large triangles of opacity `opacity` and IOR 1 above them (every other one with vertex normals: both kinds of triangle test), a mirror
    wall at one side (opaque; the photon map holds caustic photons only, so without a specular surface a frame would have no gather).  The
    reference draws the alpha test per (leaf, entity) (include/raytracer.h:455): an entity that failed its draw from an early leaf is drawn again
    from every later leaf that refers to it and may win there with a hit NEARER than the best so far, so a closest-hit walk may neither stop
    behind its best hit nor cut an entity's box to a leaf in such a scene.  textured: the large triangles carry scenes/textures/cutout.png (an
    image with an alpha channel) instead of a colour: the alpha then depends on the uv a successful intersect of a smooth triangle left behind."""
    s = gi.Scene()
    if textured:
        black = s.add_color_texture((0, 0, 0))
        white = s.add_material_tex(s.add_color_texture((0.8, 0.8, 0.8)), black, 1, 1, 1)
        red = s.add_material_tex(s.add_checkerboard((0.8, 0.3, 0.2), (0.9, 0.8, 0.2), 6), black, 1, 1, 1)
        rgba, has_alpha = _load_png(os.path.join(ROOT, "scenes", "textures", "cutout.png"))
        assert has_alpha and (rgba[:, :, 3] < 255).any()
        veil = s.add_material_tex(s.add_image_texture(rgba, (2, 2), True), black, 1, opacity, 1)
        mirror = s.add_material_tex(s.add_color_texture((0.9, 0.9, 0.9)), black, 0, 1, 1)
    else:
        white = s.add_material(1, 1, 1, (0.8, 0.8, 0.8)); red = s.add_material(1, 1, 1, (0.8, 0.3, 0.2))
        veil = s.add_material(1, opacity, 1, (0.2, 0.3, 0.8)); mirror = s.add_material(0, 1, 1, (0.9, 0.9, 0.9))
    quad = lambda a, b, c, d: [[a, b, c], [a, c, d]]
    tris, nrms, uvs, mats = [], [], [], []
    def put(q, m):
        tris.extend(quad(*q)); mats.extend([m, m]); nrms.extend([np.zeros((3, 3))] * 2); uvs.extend([[(0, 0), (1, 0), (1, 1)], [(0, 0), (1, 1), (0, 1)]])
    put(((-4, 0, -4), (-4, 0, 4), (4, 0, 4), (4, 0, -4)), white)                      # floor
    put(((-3.9, 0, -2.5), (-3.9, 0, 2.5), (-3.9, 2.5, 2.5), (-3.9, 2.5, -2.5)), mirror)   # a mirror wall (opaque): photons reach the map only off a specular surface
    # A foot under the floor.  The photon map lives in the scene's root box and a gather outside it finds nothing; hit points on a floor at y = 0 come
    # out at y = +-1e-16, so with the floor ON the box's lower face the last bit of a bounce direction (device libm against glibc) would decide
    # whether a floor vertex gathers at all -- a discontinuity of the scene, not of the walk under test (seen on the MI355X: frame RMSE 1e-6 .. 1e-5).
    put(((-0.5, -0.37, -0.5), (-0.5, -0.37, 0.5), (0.5, -0.37, 0.5), (0.5, -0.37, -0.5)), white)
    rs = np.random.RandomState(11)
    for k in range(60):                                                               # small blocks standing on the floor
        x, z = rs.uniform(-3.5, 3.3, 2)
        w, h = rs.uniform(0.05, 0.2), rs.uniform(0.1, 0.6)
        (x0, y0, z0), (x1, y1, z1) = (x, 0.0, z), (x + w, h, z + w)
        for q in (((x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0)), ((x0, y0, z1), (x0, y1, z1), (x1, y1, z1), (x1, y0, z1)),
                  ((x0, y0, z0), (x0, y1, z0), (x0, y1, z1), (x0, y0, z1)), ((x1, y0, z0), (x1, y0, z1), (x1, y1, z1), (x1, y1, z0)),
                  ((x0, y1, z0), (x1, y1, z0), (x1, y1, z1), (x0, y1, z1))):
            put(q, red if k % 3 == 0 else white)
    for k in range(12):                                                               # the large half-transparent triangles
        p = np.stack([rs.uniform(-3.5, 3.5, 3), rs.uniform(0.05, 3.0, 3), rs.uniform(-3.5, 3.5, 3)], 1)
        tris.append(p.tolist()); mats.append(veil); uvs.append([(0, 0), (1, 0), (0.5, 1)])
        if k % 2:                                                                     # a smooth one: vertex normals around the face normal
            fn = np.cross(p[1] - p[0], p[2] - p[0])
            n = fn / np.linalg.norm(fn) + rs.uniform(-0.3, 0.3, (3, 3))
            nrms.append(n / np.linalg.norm(n, axis=1)[:, None])
        else:
            nrms.append(np.zeros((3, 3)))
    s.add_triangles(np.array(tris, float), nrm=np.array(nrms, float), uv=np.array(uvs, float), mat_idx=mats)
    s.add_light((0.3, 3.8, 0.4), (9, 9, 9), 0.1)
    s.set_camera((0.2, 2.6, 5.5), (0, 0.5, 0))
    s.rebuild()
    t = s.tables()
    alpha = alpha_entities(s)
    assert alpha.sum() == (12 if opacity < 1 or textured else 0) and (np.abs(t["tri_nrm"][-12:]).sum(axis=(1, 2)) > 0).sum() == 6
    leaf_has_alpha = [alpha[t["node_ent_idx"][t["node_ent_off"][n]:t["node_ent_off"][n + 1]]].any() for n in range(len(t["node_bbox"]))]
    assert sum(leaf_has_alpha) > 1 or not alpha.any(), "the octree did not split around the large triangles"
    return s


_ALPHA_CASES = {}


def alpha_case(opacity=0.5, textured=False):
    """large_alpha_scene(opacity, textured), built once per session, with the oracle's answers on its rays (alpha_walk_answers) attached."""
    key = (opacity, textured)
    if key not in _ALPHA_CASES:
        scene = large_alpha_scene(opacity, textured)
        scene.alpha_answers = alpha_walk_answers(scene)
        _ALPHA_CASES[key] = scene
    return _ALPHA_CASES[key]


_NAMED = {"large_alpha": lambda: alpha_case(), "large_alpha_tex": lambda: alpha_case(textured=True),
          "two_lights": lambda: two_light_scene(False), "two_lights_glass": lambda: two_light_scene(True)}
_NAMED.update({name: (lambda args=args: many_lights_scene(*args)) for name, args in MANY_LIGHTS_NAMES.items()})


def named_scene(name):
    """A scene file of SCN or one of the scenes built in this module, by name (the GPU tests' scene lists)."""
    return _NAMED[name]() if name in _NAMED else load_scene(name)


def alpha_walk_answers(scene, n=20000, seed=21):
    """Fixed-seed rays from above towards the floor of large_alpha_scene, per ray a segment from where it lands (or starts) to a point of the light,
    and the oracle's answers: {rays, q, hit, ent, res, vis}, read-only.  Checked with the oracle alone, so that a comparison over them cannot pass
    for want of cases: at least 1 % of the rays end on an alpha entity, at least 1 % on an opaque one after crossing a leaf that refers to an alpha
    entity, and the segments are neither all blocked nor all free."""
    oracle = oracle_for(scene)
    rs = np.random.RandomState(seed)
    o = np.stack([rs.uniform(-3.8, 3.8, n), rs.uniform(2.0, 3.9, n), rs.uniform(-3.8, 3.8, n)], 1)
    tgt = np.stack([rs.uniform(-3.8, 3.8, n), np.zeros(n), rs.uniform(-3.8, 3.8, n)], 1)
    d = tgt - o
    d /= np.linalg.norm(d, axis=1)[:, None]
    rays = np.concatenate([o, d], 1)
    alpha = alpha_entities(scene)
    hit, ent, res, _ = oracle.trace(rays)
    _, _, off, idx = oracle.octree()
    node_has_alpha = np.array([alpha[idx[off[k]:off[k + 1]]].any() for k in range(len(off) - 1)])
    crosses = np.array([node_has_alpha[oracle.leaf_order(r)[0]].any() for r in rays])
    on_alpha = (hit > 0) & alpha[np.where(hit > 0, ent, 0)]
    on_opaque = (hit > 0) & ~alpha[np.where(hit > 0, ent, 0)] & crosses
    assert on_alpha.mean() >= 0.01 and on_opaque.mean() >= 0.01, (on_alpha.mean(), on_opaque.mean())
    light = scene.tables()["lights"][0]
    u = rs.randn(n, 3)
    u /= np.linalg.norm(u, axis=1)[:, None]
    start = np.where((hit > 0)[:, None], res[:, :3] + 1e-4 * res[:, 3:6], o)
    q = np.concatenate([start, light[:3] + light[6] * u], 1)
    vis = oracle.visible(q)[0]
    assert 0.05 < vis.mean() < 0.95, vis.mean()
    out = {"rays": rays, "q": q, "hit": hit, "ent": ent, "res": res, "vis": vis}
    for a in out.values():
        a.setflags(write=False)
    return out


def check_alpha_walks(rt, scene, set_wide):
    """Large alpha-tested entities (large_alpha_scene): the wide walk, the per-node walk and the oracle return the same closest hit -- flag and
    entity exact, hit point and normal bit for bit -- and the same visibility of segments that end at the light (the any-hit walk draws per
    (leaf, entity) too, and where the lights hang free k_st_shadow shares the closest-hit walk's boxes: visible_turns on the CPU build).
    Returns the mismatch counts (wide against per-node, per-node against oracle), printed before they are asserted to be 0."""
    a = getattr(scene, "alpha_answers", None) or alpha_walk_answers(scene)
    rays, q, hit_o, ent_o, res_o, vis_o = (a[k] for k in ("rays", "q", "hit", "ent", "res", "vis"))
    assert set_wide(True)
    hit_w, ent_w, res_w = rt.trace(rays)
    vis_w = rt.visible(q)
    turns = rt.visible_turns(q, light_bound=True) if hasattr(rt, "visible_turns") else None
    set_wide(False)
    hit_n, ent_n, res_n = rt.trace(rays)
    vis_n = rt.visible(q)
    set_wide(True)
    n_wn = int(((hit_w != hit_n) | (ent_w != ent_n)).sum())
    n_no = int(((hit_n != hit_o) | (ent_n != ent_o)).sum())
    print(f"alpha walks: {int(hit_o.sum())} hits of {len(rays)} rays; mismatches wide vs per-node {n_wn}, per-node vs oracle {n_no}; "
          f"visibility differs from the oracle's on {int((vis_w != vis_o).sum())} (wide) / {int((vis_n != vis_o).sum())} (per node) of {len(q)} segments")
    assert n_no == 0
    assert np.array_equal(res_n[hit_n > 0, :6].view(np.uint64), res_o[hit_o > 0, :6].view(np.uint64))
    assert n_wn == 0
    assert np.array_equal(res_w[hit_w > 0].view(np.uint64), res_n[hit_n > 0].view(np.uint64))
    assert np.array_equal(vis_n, vis_o) and np.array_equal(vis_w, vis_o)
    if turns is not None:
        assert np.array_equal(turns, vis_o)
    return n_wn, n_no


# Frame of large_alpha_scene with a photon map: 100 x the RMSE the per-node walk with both short cuts off reaches against the oracle on the CPU
# build of the device code (measured 3.95e-18 at opacity 0.5, 2.08e-18 textured, 3.45e-18 at 0.05, 1.27e-18 at 0.95; the largest is taken)
ALPHA_PHOTON_FRAME_TOL = 100 * 3.95e-18


def check_alpha_frames(rt, scene):
    """48 x 32 frames at 4 spp of large_alpha_scene against the oracle: without a photon map (1e-9: a wrong first hit moves the frame by ~1e-4, the
    arithmetic by ~1e-18), then with 2000 photon indices emitted (ALPHA_PHOTON_FRAME_TOL), so that the gather sees the alpha hits too.  `rt` comes
    fresh from setScene (no map loaded).  Returns the two RMSE values, printed before the second is asserted."""
    rmse0, img0, _ = check_render(rt, scene, 48, 32, 4, photons=0, tol=1e-9)
    check_emission(rt, scene, 1000)                  # photon paths cross the alpha triangles too (their own draws, keyed by leaf and entity as well)
    rmse1, img1, _ = check_render(rt, scene, 48, 32, 4, photons=2000, tol=1e-9)
    print(f"alpha frames: rmse vs oracle {rmse0:.3e} without photons, {rmse1:.3e} with")
    assert len(scene.photon_tables()["photons"]) > 1000 and not np.array_equal(img0, img1)      # the map is there and the gather adds to the frame
    assert img0.mean() > 1e-3
    assert rmse1 < ALPHA_PHOTON_FRAME_TOL, rmse1
    return rmse0, rmse1


def check_gather_float_ties(rt_factory):
    """Photons whose squared distances to the query agree to float precision around rank 32: the float-key heap cannot
    separate them, the exact pass must.  40 photons on a ray from the query point, spacing 1e-9."""
    s = gi.Scene()
    m = s.add_material(1.0, 1.0, 1.0, (1, 1, 1))
    s.add_triangles(np.array([[[0, 0, 0], [4, 0, 0], [0, 0, 4]], [[4, 0, 0], [4, 0, 4], [0, 0, 4]], [[0, 4, 0], [4, 4, 0], [0, 4, 4]]], float), mat_idx=[m] * 3)
    s.add_light((2, 3, 2), (1, 1, 1), .05)
    s.rebuild()
    rs = np.random.RandomState(5)
    n = 40
    q = np.array([1.0, 1.0, 1.0]) * 2.0 ** -3
    # 40 photons on a shell of radius 2^-20 (1 + k 2^-30) around q: squared distances differ by ~2e-9 relative, far below
    # float resolution; 10 clearly nearer ones put rank 32 inside that group.  The whole cluster (radius 1e-6) lies inside
    # the +-1e-5 neighbourhood of the leaf that contains q, so all 50 are candidates.
    u = rs.randn(n, 3); u /= np.linalg.norm(u, axis=1)[:, None]
    pos = q + u * (2.0 ** -20 * (1 + rs.permutation(n) * 2.0 ** -30))[:, None]
    d = rs.randn(n, 3); d /= np.linalg.norm(d, axis=1)[:, None]
    ph = np.concatenate([pos, d, rs.rand(n, 3)], axis=1)
    un = rs.randn(10, 3); un /= np.linalg.norm(un, axis=1)[:, None]
    near = np.concatenate([q + un * 2.0 ** -21 * (1 + rs.rand(10, 1)* 0.5), d[:10], rs.rand(10, 3)], axis=1)
    ph = np.concatenate([near, ph])
    rt = rt_factory().setScene(s)
    s.build_photon_map(ph)
    rt.upload_photon_map()
    o = oracle_for(s)
    o.set_photons(ph).build_photon_map()
    qq = np.array([[*q, 0.3, 0.5, 0.8]])
    got, nc = rt.samplePhotons(qq)
    ref, nco = o.gather(qq)
    assert nc[0] == nco[0] == 50
    np.testing.assert_allclose(got, ref, rtol=1e-9)


def check_gather_exact_duplicates(rt_factory):
    """Exact copies of photons (same position, direction and colour) inside a float-key tie group that straddles rank 32: every copy is a
    photon of its own, as in the reference's partial_sort, and the exact pass has to count each.  The layout of check_gather_float_ties with
    copies of every tie-group photon, of the three nearest ones, and a tie group made only of five copies of one photon (28 nearer ones, 10
    farther).  Copies are whole photons, so the answer does not depend on which copy is taken."""
    s = gi.Scene()
    m = s.add_material(1.0, 1.0, 1.0, (1, 1, 1))
    s.add_triangles(np.array([[[0, 0, 0], [4, 0, 0], [0, 0, 4]], [[4, 0, 0], [4, 0, 4], [0, 0, 4]], [[0, 4, 0], [4, 4, 0], [0, 4, 4]]], float), mat_idx=[m] * 3)
    s.add_light((2, 3, 2), (1, 1, 1), .05)
    s.rebuild()
    rs = np.random.RandomState(6)
    q = np.array([1.0, 1.0, 1.0]) * 2.0 ** -3

    def unit(n):
        u = rs.randn(n, 3)
        return u / np.linalg.norm(u, axis=1)[:, None]

    def photons(radius):
        return np.concatenate([q + unit(len(radius)) * radius[:, None], unit(len(radius)), rs.rand(len(radius), 3)], axis=1)

    def d2(ph):
        d = ph[:, :3] - q
        return d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]

    near = photons(2.0 ** -21 * (1 + rs.rand(10) * 0.5))
    shell = photons(2.0 ** -20 * (1 + rs.permutation(40) * 2.0 ** -30))
    shell = shell[np.argsort(d2(shell))]                                      # nearest first: the copies fall among the ones pass 3 takes
    one = photons(np.array([2.0 ** -20]))
    cases = [np.concatenate([near, shell, shell[:20]]),                       # every photon of the tie group taken twice
             np.concatenate([near, shell, shell[:3]]),                        # three of them twice
             np.concatenate([photons(2.0 ** -21 * (1 + rs.rand(28) * 0.5)), np.repeat(one, 5, axis=0), photons(2.0 ** -19 * (1 + rs.rand(10)))])]
    qq = np.concatenate([np.broadcast_to(q, (4, 3)), unit(4)], axis=1)
    for ph in cases:
        key = np.sort(d2(ph).astype(np.float32))
        assert key[31] == key[32]                                             # float keys tie across rank 32: the exact pass runs
        rt = rt_factory().setScene(s)
        s.build_photon_map(ph)
        rt.upload_photon_map()
        o = oracle_for(s)
        o.set_photons(ph).build_photon_map()
        got, nc = rt.samplePhotons(qq)
        ref, nco = o.gather(qq)
        assert (nc == len(ph)).all() and (nco == len(ph)).all()
        np.testing.assert_allclose(got, ref, rtol=1e-9)


def check_stripes(rt, scene, w, h, spp, world, stripe_h, adaptive=False):
    """Row-stripe sharding: rendering the stripes of every rank and interleaving them gives the single-GPU frame exactly, and its per-pixel
    sample counts.  adaptive: spp .. 4 spp samples under check_render's threshold.  A rank without rows returns empty arrays.  Returns the
    assembled (frame, sample counts)."""
    kw = dict(min_samples=spp, max_samples=4 * spp, noise_thresh=0.0015) if adaptive else dict(min_samples=spp, max_samples=spp)
    full, full_spp = rt.run(w, h, want_spp=True, **kw)
    frame, counts = np.full_like(full, np.nan), np.full_like(full_spp, -1)
    seen = np.zeros(h, int)
    for rank in range(world):
        part, part_spp = rt.run(w, h, want_spp=True, stripe_h=stripe_h, rank=rank, world=world, **kw)
        rows = stripe_rows(h, stripe_h, rank, world)
        assert len(rows) == len(part)
        assert part.shape == (len(rows), w, 3) and part_spp.shape == (len(rows), w)
        frame[rows], counts[rows] = part, part_spp
        seen[rows] += 1
    assert (seen == 1).all()                          # every row from exactly one rank
    assert np.array_equal(frame, full)
    assert np.array_equal(counts, full_spp)
    return frame, counts


from gi_raytracer_amd.sharding import stripe_rows  # noqa: E402  (re-exported for the tests)


def adversarial_rays(scene, n=6000, seed=5):
    """Rays that stress the box arithmetic of the octree walk: random ones, axis-parallel ones (a zero direction component makes
    invDir infinite and 0 * inf = NaN when the origin lies on a plane), origins exactly on node planes, and -0.0 components."""
    t = scene.tables()
    bb = t["node_bbox"]
    rs = np.random.RandomState(seed)
    lo, hi = bb[0, :3], bb[0, 3:]
    o = lo + (hi - lo) * (rs.rand(n, 3) * 1.4 - 0.2)
    d = rs.randn(n, 3)
    k = n // 6
    for j in range(k):                              # axis-parallel and plane-parallel directions
        d[j, rs.randint(3)] = 0.0
    for j in range(k, 2 * k):
        a = rs.randint(3)
        d[j] = 0.0
        d[j, a] = rs.choice([-1.0, 1.0])
    for j in range(2 * k, 3 * k):                   # origins on planes of random nodes (min / max / a child's planes)
        nb = bb[rs.randint(len(bb))]
        a = rs.randint(3)
        o[j, a] = nb[a + 3 * rs.randint(2)]
    for j in range(3 * k, 4 * k):                   # both: origin on a plane, direction inside that plane
        nb = bb[rs.randint(len(bb))]
        a = rs.randint(3)
        o[j, a] = nb[a + 3 * rs.randint(2)]
        d[j, a] = rs.choice([0.0, -0.0])
    for j in range(4 * k, 5 * k):                   # negative zeros
        d[j, rs.randint(3)] = -0.0
    nrm = np.sqrt((d * d).sum(1))
    d = d / np.where(nrm == 0, 1, nrm)[:, None]
    return np.concatenate([o, d], 1)


def check_wide_walk(rt, scene, set_wide):
    """The wide-record walk and the per-node walk give identical answers (hit flag, entity, hit point bits, visibility)."""
    rays = adversarial_rays(scene)
    rs = np.random.RandomState(9)
    q = np.concatenate([rays[:, :3], rays[:, :3] + rays[:, 3:] * (rs.rand(len(rays), 1) * 12 + 0.01)], 1)
    if (scene.tables()["node_child"][0] < 0).all():
        assert not set_wide(True)          # the root is a leaf: nothing to walk, the per-node path handles it
        return
    assert set_wide(True), "the scene's octree was not accepted as exact octants"
    hit_w, ent_w, res_w = rt.trace(rays)
    vis_w = rt.visible(q)
    set_wide(False)
    hit_n, ent_n, res_n = rt.trace(rays)
    vis_n = rt.visible(q)
    set_wide(True)
    assert hit_w.sum() > 100
    assert np.array_equal(hit_w, hit_n) and np.array_equal(ent_w[hit_w > 0], ent_n[hit_n > 0])
    assert np.array_equal(res_w[hit_w > 0].view(np.uint64), res_n[hit_n > 0].view(np.uint64))
    assert np.array_equal(vis_w, vis_n)


def check_content_culling(rt, scene, photons=2000, render=True):
    """Content-box culling (a child of the walk is skipped when the ray misses the box of everything referenced below it) changes nothing:
    hit flag, entity, hit point bits, visibility on the adversarial rays, and whole frames bit for bit, with and without."""
    rays = adversarial_rays(scene)
    rs = np.random.RandomState(9)
    q = np.concatenate([rays[:, :3], rays[:, :3] + rays[:, 3:] * (rs.rand(len(rays), 1) * 12 + 0.01)], 1)
    if not rt.set_content_culling(True):
        return False                      # the tree does not take the wide walk: nothing to compare
    a = rt.trace(rays); va = rt.visible(q)
    assert not rt.set_content_culling(False)
    b = rt.trace(rays); vb = rt.visible(q)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64)) and np.array_equal(va, vb)
    if render:
        if scene.desc().n_light:
            rt.tracePhotons(photons)
        fb = rt.run(40, 30, min_samples=4, max_samples=4)
        assert rt.set_content_culling(True)
        fa = rt.run(40, 30, min_samples=4, max_samples=4)
        assert np.array_equal(fa.view(np.uint64), fb.view(np.uint64))
    rt.set_content_culling(True)
    return True


def check_photon_descent(rt, scene, photons=20000):
    """PhotonMap::getBounds walked one record per level (children's boxes from the parent's planes) and two records per level give
    identical gathers: inside, outside and on the faces of the map."""
    rt.tracePhotons(photons)
    t = scene.tables()
    bb = t["node_bbox"][0]
    rs = np.random.RandomState(1)
    pos = bb[:3] + (bb[3:] - bb[:3]) * (rs.rand(20000, 3) * 1.1 - 0.05)
    ph = scene.photon_tables()
    nb = ph["node_bbox"]
    for j in range(2000):                       # queries exactly on planes of photon-map nodes
        b = nb[rs.randint(len(nb))]
        pos[j, rs.randint(3)] = b[rs.randint(6)]
    q = np.concatenate([pos, rs.randn(len(pos), 3)], 1)
    rt.set_wide_nodes(True)
    assert rt.photon_planes, "the photon octree was not accepted for the one-record descent"
    a, na = rt.samplePhotons(q)
    rt.set_wide_nodes(False)
    assert not rt.photon_planes
    b, nbc = rt.samplePhotons(q)
    rt.set_wide_nodes(True)
    assert (na > 0).mean() > 0.1 and (na == 0).any()
    assert np.array_equal(na, nbc) and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ------------------------------------------------------------------------------------------------ rays aimed at the geometry
GI_EPSILON = 1e-5                    # gi_intersect.h / include/entities.h: tri_hit's |det| threshold
EDGE_RAYS_PER_CLASS = 1600           # (at most 4 000 per class and scene; six classes stay below 24 000 rays per launch)


def _unit(v):
    v = np.asarray(v, float)
    n = np.sqrt((v * v).sum(-1, keepdims=True))
    return v / np.where(n == 0, 1.0, n)


def _hair(rs, ext, n):
    """ext * 10**U(-15, -9) with both signs (the range test_quick_descent_of_the_gather_keys_finds_the_same_leaf uses)."""
    return ext * 10.0 ** rs.uniform(-15, -9, n) * rs.choice([-1.0, 1.0], n)


def _edge_origins(rs, lo, hi, n):
    """A third inside the root box, a third on its faces, a third up to 0.2 extents outside it."""
    o = lo + (hi - lo) * rs.rand(n, 3)
    k = np.arange(n) % 3
    ax, side = rs.randint(3, size=n), rs.randint(2, size=n)
    face = np.where(side == 0, lo[ax], hi[ax])
    out = face + (hi - lo)[ax] * rs.uniform(0, 0.2, n) * np.where(side == 0, -1.0, 1.0)
    rows = np.arange(n)
    o[rows[k == 1], ax[k == 1]] = face[k == 1]
    o[rows[k == 2], ax[k == 2]] = out[k == 2]
    return o


def _aim(rs, o, tgt, lo, hi, axis_share=0.2, back_share=0.6):
    """Rays from o to tgt; a share of them reaches the target along an exact axis direction instead (the other two components 0.0 or -0.0).
    back_share of the rays whose origin lies outside the root box run the other way, from the target out to that origin: the aimed-at point is
    then the ray's own origin (t = 0 to rounding), and in a closed room these are the rays that can leave the scene at all."""
    n = len(tgt)
    o = o.copy()
    d = _unit(tgt - o)
    back = ((o < lo) | (o > hi)).any(1) & (rs.rand(n) < back_share)
    d[back] = -d[back]
    o[back] = tgt[back]
    ax = rs.rand(n) < axis_share
    for j in np.nonzero(ax)[0]:
        a, s = rs.randint(3), rs.choice([-1.0, 1.0])
        dist = (hi - lo)[a] * rs.uniform(0.05, 1.2)
        o[j] = tgt[j]
        o[j, a] = tgt[j, a] - s * dist
        d[j] = rs.choice([0.0, -0.0], 3)
        d[j, a] = s
    return np.concatenate([o, d], 1)


def _root_box_entered(rays, lo, hi):
    """BoundingBox::intersect(ray, 0, inf) of the root box as the walks ask it (include/bbox.h:47-73; a NaN from 0 * inf is ignored, and leaving at
    the first tmax <= tmin equals testing the last): a ray for which this is False is never walked, whatever lies on its line."""
    with np.errstate(all="ignore"):
        inv = 1.0 / rays[:, 3:]
        t0, t1 = (lo - rays[:, :3]) * inv, (hi - rays[:, :3]) * inv
    t0, t1 = np.where(inv < 0, t1, t0), np.where(inv < 0, t0, t1)
    tmin, tmax = np.zeros(len(rays)), np.full(len(rays), np.inf)
    ok = np.ones(len(rays), bool)
    for a in range(3):
        tmin = np.where(t0[:, a] > tmin, t0[:, a], tmin)
        tmax = np.where(t1[:, a] < tmax, t1[:, a], tmax)
        ok &= ~(tmax <= tmin)
    return ok


def _with_scene_behind(rs, rays, lo, hi, ext, share=0.12):
    """The same lines with the origin slid forward to where the ray leaves the root box -- on that face to rounding, a hair before or behind it, or up to
    0.2 extents outside: everything aimed at lies behind the origin (t < 0), and whether a walk begins at all hangs on the root box's own slab test.  In a
    closed room these are the rays that leave the scene."""
    rays = rays.copy()
    rows = np.nonzero((rs.rand(len(rays)) < share) & _root_box_entered(rays, lo, hi))[0]
    o, d = rays[rows, :3], rays[rows, 3:]
    with np.errstate(all="ignore"):
        t1 = np.where(d == 0, np.inf, np.maximum((lo - o) / d, (hi - o) / d))
    s = t1.min(1)
    k = np.arange(len(rows)) % 3
    s = s + np.where(k == 0, 0.0, np.where(k == 1, _hair(rs, ext, len(rows)), ext * rs.uniform(0, 0.2, len(rows))))
    rays[rows, :3] = o + d * s[:, None]
    return rays


def _leaf_entities(t):
    """(leaf node, entity) pairs of the scene's octree, grouped per leaf that holds any."""
    off, idx = t["node_ent_off"], t["node_ent_idx"]
    return [(k, idx[off[k]:off[k + 1]]) for k in range(len(off) - 1) if off[k + 1] > off[k]]


def _tri_boundary_targets(rs, t, n, ext):
    tri, kind = t["tri_pos"], t["ent_kind"]
    leaves = [(k, e[kind[e] == 0]) for k, e in _leaf_entities(t)]
    leaves = [(k, e) for k, e in leaves if len(e)]
    out = []
    for j in range(n):
        _, ents = leaves[j % len(leaves)]                      # triangles from every leaf that holds any, in turn
        p0, p1, p2 = tri[ents[rs.randint(len(ents))]]
        e1, e2 = p1 - p0, p2 - p0
        w = rs.uniform(0.03, 0.97)
        what = j // len(leaves) % 6 if n >= 6 * len(leaves) else rs.randint(6)
        u, v = [(0, 0), (1, 0), (0, 1), (w, 0), (0, w), (w, 1 - w)][what]
        p = p0 + u * e1 + v * e2
        move = rs.randint(3)                                   # on the boundary; a hair inwards or outwards in the triangle's plane
        if move:
            c = (p0 + p1 + p2) / 3.0
            if what < 3:
                inward = _unit(c - p)
            else:
                a, b = [(p0, p1), (p0, p2), (p1, p2)][what - 3]
                along = _unit(b - a)
                inward = c - a
                inward = _unit(inward - along * (inward * along).sum())
            p = p + inward * _hair(rs, ext, 1)[0]
        out.append(p)
    return np.array(out)


def _cut_triangle(p, a, c):
    """The two points where the plane x_a = c cuts the triangle p [3][3] (None when it does not cross it)."""
    s = p[:, a] - c
    pts = []
    for i, j in ((0, 1), (1, 2), (2, 0)):
        if (s[i] < 0) != (s[j] < 0):
            pts.append(p[i] + (p[j] - p[i]) * (s[i] / (s[i] - s[j])))
    return pts if len(pts) == 2 else None


def _leaf_plane_targets(rs, t, n, ext):
    """Per target: point, the face's axis (the normal), -1 or the second axis for a target on a leaf edge.  None when no entity crosses a face of
    its leaf (a tree of one leaf)."""
    tri, kind, bb = t["tri_pos"], t["ent_kind"], t["node_bbox"]
    pairs = [(k, e) for k, ents in _leaf_entities(t) for e in ents]
    order = rs.permutation(len(pairs))
    plane, edge = [], []
    want_edge = n // 4
    for rnd in range(8):
        for j in order:
            k, e = pairs[j]
            a = rs.randint(3)
            c = bb[k, a + 3 * rs.randint(2)]
            lo, hi = bb[k, :3], bb[k, 3:]
            if kind[e] == 0:
                cut = _cut_triangle(tri[e], a, c)
                if cut is None:
                    continue
                P, Q = cut
                if len(edge) < want_edge:                       # on a leaf edge: where the cut crosses a plane of a second axis
                    b = (a + 1 + rs.randint(2)) % 3
                    for c2 in (lo[b], hi[b]):
                        sP, sQ = P[b] - c2, Q[b] - c2
                        if (sP < 0) != (sQ < 0):
                            x = P + (Q - P) * (sP / (sP - sQ))
                            x[a], x[b] = c, c2
                            edge.append((x, a, b))
                            break
                for _ in range(6):                                  # a point of the cut, on the leaf's own face when the cut reaches it
                    x = P + (Q - P) * rs.rand()
                    if ((x >= lo - 1e-9) & (x <= hi + 1e-9)).all():
                        break
                x[a] = c
            else:
                ctr, rad = tri[e][0], tri[e][1][0]
                h = c - ctr[a]
                if abs(h) >= rad:
                    continue
                phi, r = rs.uniform(0, 2 * np.pi), np.sqrt(rad * rad - h * h)
                x = ctr.copy()
                x[a] = c
                x[(a + 1) % 3] += r * np.cos(phi)
                x[(a + 2) % 3] += r * np.sin(phi)
            plane.append((x, a, -1))
            if len(plane) >= n - want_edge and len(edge) >= want_edge:
                break
        if not plane or (len(plane) >= n - want_edge and len(edge) >= want_edge):
            break
    if not plane:
        return None
    both = (plane[:n - len(edge[:want_edge])] + edge[:want_edge])[:n]
    return np.array([b[0] for b in both]), np.array([b[1] for b in both]), np.array([b[2] for b in both])


def _leaf_plane_rays(rs, t, n, lo, hi, ext):
    got = _leaf_plane_targets(rs, t, n, ext)
    if got is None:
        return None
    tgt, ax, _ = got
    m = len(tgt)
    rows = np.arange(m)
    plane = tgt[rows, ax].copy()
    k = rs.randint(3, size=m)                                   # on the plane, a hair to either side along its normal
    tgt[rows, ax] += np.where(k == 0, 0.0, _hair(rs, ext, m))
    o = _edge_origins(rs, lo, hi, m)
    side = np.where(rs.rand(m) < 0.5, -1.0, 1.0)                # from both sides of the plane
    o[rows, ax] = plane + side * np.maximum(np.abs(o[rows, ax] - plane), 1e-3 * ext)
    rays = _aim(rs, o, tgt, lo, hi, axis_share=0.0)
    normal = rs.rand(m) < 0.25                                  # along the plane's normal
    for j in np.nonzero(normal)[0]:
        a = ax[j]
        rays[j, :3] = tgt[j]
        rays[j, a] = o[j, a]
        rays[j, 3:] = rs.choice([0.0, -0.0], 3)
        rays[j, 3 + a] = 1.0 if o[j, a] < plane[j] else -1.0
    return rays


def _in_plane_rays(rs, t, n, lo, hi, ext):
    tri, kind = t["tri_pos"], t["ent_kind"]
    tris = np.nonzero(kind == 0)[0]
    rays = []
    for j in range(n):
        p0, p1, p2 = tri[tris[rs.randint(len(tris))]]
        e1, e2 = p1 - p0, p2 - p0
        N = np.cross(e1, e2)
        if not (N * N).sum() > 0:
            continue
        nrm = _unit(N)
        u = rs.uniform(0.05, 0.9); v = rs.uniform(0.02, 0.95 - u)
        tgt = p0 + u * e1 + v * e2
        a, b = rs.uniform(-1.5, 2.5, 2)
        o = p0 + a * e1 + b * e2
        d0 = _unit(tgt - o)
        if j % 3 == 0:                                          # origin and direction in the triangle's plane: det == 0 to rounding
            rays.append(np.concatenate([o, d0]))
            continue
        # tilted out of the plane so that |det| = |d . (e1 x e2)| lands at 1e-3 .. 1e3 times GI_EPSILON, through a point inside the triangle
        det = GI_EPSILON * 10.0 ** rs.uniform(-3, 3)
        s = min(det / np.sqrt((N * N).sum()), 0.9)
        d = _unit(d0 * np.sqrt(1 - s * s) + nrm * s * rs.choice([-1.0, 1.0]))
        rays.append(np.concatenate([tgt - d * ext * rs.uniform(0.02, 0.5), d]))
    return np.array(rays)


def _sphere_rays(rs, t, n, lo, hi, ext):
    tri, kind = t["tri_pos"], t["ent_kind"]
    sph = np.nonzero(kind == 1)[0]
    if not len(sph):
        return None
    org = _edge_origins(rs, lo, hi, n)
    rays = []
    for j in range(n):
        e = sph[rs.randint(len(sph))]
        c, rad = tri[e][0], tri[e][1][0]
        o = org[j]
        rnd = _unit(rs.randn(3))
        what = j % 8
        if what in (0, 1):                                      # tangent (r of ent_hit zero) and a hair either side
            oc = c - o
            L = np.sqrt((oc * oc).sum())
            if L <= rad * 1.001:
                o = c + rnd * rad * rs.uniform(1.5, 4.0); oc = c - o; L = np.sqrt((oc * oc).sum())
            w = _unit(np.cross(oc, rs.randn(3)))
            T = c + rad * (-(rad / L) * _unit(oc) + np.sqrt(1 - (rad / L) ** 2) * w)      # the tangent point seen from o
            if what == 1:
                T = T + _unit(T - c) * _hair(rs, ext, 1)[0]
            rays.append(np.concatenate([o, _unit(T - o)]))
        elif what == 2:                                         # origin on the surface, pointing in / pointing out
            o = c + rad * rnd
            d = _unit(rs.randn(3))
            rays.append(np.concatenate([o, d]))
        elif what == 3:                                         # origin inside, or at the centre
            o = c + rad * rnd * (0.0 if j % 16 == 3 else rs.uniform(0, 1))
            rays.append(np.concatenate([o, _unit(rs.randn(3))]))
        elif what == 4:                                         # the sphere entirely behind the origin
            if np.sqrt(((o - c) ** 2).sum()) <= rad * 1.001:
                o = c + rnd * rad * rs.uniform(1.01, 3.0)
            rays.append(np.concatenate([o, _unit(_unit(o - c) + 0.8 * rs.randn(3) * rs.rand())]))
        elif what == 5:                                         # through both poles (ent_uv: asin of the y component)
            if j % 16 == 5:
                s = rs.choice([-1.0, 1.0])
                rays.append(np.array([c[0], c[1] + s * rad * rs.uniform(1.1, 3.0), c[2], rs.choice([0.0, -0.0]), -s, rs.choice([0.0, -0.0])]))
            else:
                rays.append(np.concatenate([o, _unit(c + np.array([0, rad, 0]) * rs.choice([-1.0, 1.0]) - o)]))
        elif what == 6:                                         # the atan2 seam: hit points with z = centre's z on the +x side
            phi = rs.uniform(-0.5 * np.pi, 0.5 * np.pi)
            T = c + rad * np.array([np.cos(phi), np.sin(phi), 0.0])
            rays.append(np.concatenate([o, _unit(T - o)]))
        else:                                                   # a plain ray at the sphere
            rays.append(np.concatenate([o, _unit(c + rad * rnd * rs.rand() - o)]))
    return np.array(rays)


def segments_as_rays(q):
    """Segments q [n][6] = origin, target as gi_visible_rays' arguments, formed the way k_visible / make_ray form them (IEEE +, *, /, sqrt in the
    same order: the same bits): rays [n][6] = origin, unit direction; mt [n] = squared length.  A segment of length zero has no direction: +x."""
    q = np.asarray(q, float)
    ld = q[:, 3:] - q[:, :3]
    mt = ld[:, 0] * ld[:, 0] + ld[:, 1] * ld[:, 1] + ld[:, 2] * ld[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        d = ld * (1.0 / np.sqrt(mt))[:, None]
    d[mt == 0] = (1.0, 0.0, 0.0)
    return np.concatenate([q[:, :3], d], 1), mt


def entity_edge_rays(scene, seed=1, n=EDGE_RAYS_PER_CLASS):
    """Rays aimed at the geometry instead of at random (adversarial_rays stresses the box arithmetic; these the entity tests and the places where
    the walks' short cuts are tight): named classes, each [m][6] = origin, unit direction (m <= n); "shadow_ends" is [m][6] = origin, target
    (segments_as_rays gives the other form).  Built from scene.tables(); from_hits and shadow_ends start from the ORACLE's hit points.
      tri_boundary  vertices, points on the edges, and the same a hair inwards / outwards in the triangle's plane; triangles of every leaf in turn
      leaf_plane    a point of an entity on a face plane of a leaf that refers to it, and a hair to either side; from both sides, a share along
                    the plane's normal, a share with the target on a leaf edge (two planes)
      in_plane      origin and direction in a triangle's plane (det == 0); tilted so that |det| is 1e-3 .. 1e3 times GI_EPSILON
      sphere        tangents and a hair either side, origins on the surface / inside / at the centre, the sphere behind the origin, poles, seam
      from_hits     origins that ARE hit points (no bias): mirrored on, in a random direction, straight back
      shadow_ends   segments that end at a hit point exactly or a hair before / behind it, that start at one, of length zero and a hair
    Origins: a third inside the root box, a third on its faces, a third up to 0.2 extents outside; a share of the rays reaches its target along an
    exact axis direction, a share runs from the target out to the origin, a share has the scene behind it (_aim, _with_scene_behind).
    A class a scene cannot have (no sphere; a tree of one leaf has no entity crossing a face) is left out."""
    t = scene.tables()
    bb = t["node_bbox"][0]
    lo, hi = bb[:3], bb[3:]
    ext = float((hi - lo).max())
    rs = np.random.RandomState(seed)
    oracle = oracle_for(scene)
    out = {}
    tgt = _tri_boundary_targets(rs, t, n, ext)
    out["tri_boundary"] = _with_scene_behind(rs, _aim(rs, _edge_origins(rs, lo, hi, len(tgt)), tgt, lo, hi), lo, hi, ext)
    lp = _leaf_plane_rays(rs, t, n, lo, hi, ext)
    if lp is not None:
        out["leaf_plane"] = _with_scene_behind(rs, lp, lo, hi, ext)
    out["in_plane"] = _with_scene_behind(rs, _in_plane_rays(rs, t, n, lo, hi, ext), lo, hi, ext)
    sp = _sphere_rays(rs, t, n, lo, hi, ext)
    if sp is not None:
        out["sphere"] = sp
    # the oracle's hit points of the classes so far: on the surface to rounding, so the t of the self-intersection is ~ +-1e-16 and its sign decides
    base = np.concatenate(list(out.values()))
    hit, _, res, _ = oracle.trace(base)
    hp, nrm, din = res[hit > 0, :3], res[hit > 0, 3:6], base[hit > 0, 3:]
    org = base[hit > 0, :3]
    pick = rs.permutation(len(hp))[:n]
    k = np.arange(len(pick)) % 3
    nn = _unit(nrm[pick])
    mirror = _unit(din[pick] - 2.0 * (din[pick] * nn).sum(1, keepdims=True) * nn)
    d = np.where((k == 0)[:, None], mirror, np.where((k == 1)[:, None], _unit(rs.randn(len(pick), 3)), -din[pick]))
    out["from_hits"] = np.concatenate([hp[pick], d], 1)
    # segments
    pick = rs.permutation(len(hp))[:n]
    m = len(pick)
    k = np.arange(m) % 8
    o, tg = org[pick].copy(), hp[pick].copy()
    h = _hair(rs, ext, m)
    tg[(k == 1) | (k == 2)] += (din[pick] * h[:, None])[(k == 1) | (k == 2)]                 # a hair before or behind the hit point
    before = (k == 3)                                                                         # ends a (larger) hair before its first blocker
    tg[before] -= (din[pick] * (ext * 10.0 ** rs.uniform(-9, -3, m))[:, None])[before]
    start = (k == 4) | (k == 5)                                                               # starts at a hit point (ts == 0)
    o[start] = hp[pick][start]
    tg[start] = o[start] + _unit(rs.randn(m, 3))[start] * (ext * rs.uniform(0.01, 1.0, m))[start, None]
    tg[k == 5] = org[pick][k == 5]                                                            # ... and runs straight back to where the ray came from
    tg[k == 6] = o[k == 6]                                                                    # mt zero
    tg[k == 7] = o[k == 7] + (_unit(rs.randn(m, 3)) * np.abs(h)[:, None])[k == 7]             # mt a hair above zero
    far = (k == 7) & (np.arange(m) % 16 == 15)                                                # (and segments through the hit point to twice as far)
    tg[far] = o[far] + 2.0 * (hp[pick][far] - o[far])
    out["shadow_ends"] = np.concatenate([o, tg], 1)
    for a in out.values():
        a.setflags(write=False)
    return out


def _ulp_close(a, b, ulps=4):
    return np.abs(a - b) <= ulps * np.spacing(np.maximum(np.abs(a), np.abs(b)))


def brute_force_closest(t, rays, never=None, drawn=None, chunk=256):
    """Closest hit over ALL entities without an octree, float64 numpy with the formulas of include/entities.h (triangle: :443-490, sphere: :60-101).
    Returns (hit [n], squared distance of the nearest hit [n], tied [n][n_ent] bool: the entities whose hit point lies within 4 ulp, per coordinate,
    of the nearest one's, applies [n]).  never [n_ent]: entities whose alpha test accepts no hit (alpha 0, IOR 1): left out.  drawn [n_ent]: entities
    whose alpha test draws a number per leaf; a ray that meets one of them anywhere is outside what this can say (applies = False)."""
    tri, kind = t["tri_pos"], t["ent_kind"]
    never = np.zeros(len(tri), bool) if never is None else never
    drawn = np.zeros(len(tri), bool) if drawn is None else drawn
    applies = np.ones(len(rays), bool)
    p0, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    is_sph = kind == 1
    rad = tri[:, 1, 0]
    n, E = len(rays), len(tri)
    hit = np.zeros(n, bool); best = np.full(n, np.inf); tied = np.zeros((n, E), bool)
    dot = lambda a, b: a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]
    for s in range(0, n, chunk):
        o, d = rays[s:s + chunk, None, :3], rays[s:s + chunk, None, 3:]
        with np.errstate(all="ignore"):
            p = np.cross(d, e2[None])
            det = dot(e1[None], p)
            ok = ~((det < GI_EPSILON) & (det > -GI_EPSILON))
            inv = 1.0 / det
            tv = o - p0[None]
            u = dot(tv, p) * inv
            ok &= ~((u < 0) | (u > 1))
            qq = np.cross(tv, e1[None])
            v = dot(d, qq) * inv
            ok &= ~((v < 0) | (u + v > 1))
            tt = dot(e2[None], qq) * inv
            ok &= ~(tt <= 0)
            ok &= ~np.isnan(tt)
            if is_sph.any():
                oc = tv[:, is_sph]
                dt = dot(np.broadcast_to(d, oc.shape), oc)
                r = dt * dt - dot(oc, oc) + (rad * rad)[None, is_sph]
                sr = np.sqrt(r)
                t1, t2 = -1 * dt - sr, -1 * dt + sr
                oks = ~(r < 0) & ~((t1 < 0) & (t2 < 0))
                ts = np.where(((t1 < t2) & (t1 > 0)) | (t2 < 0), t1, t2)
                tt[:, is_sph] = ts
                ok[:, is_sph] = oks
            applies[s:s + chunk] = ~(ok & drawn[None]).any(1)
            ok &= ~(never | drawn)[None]
            hp = o + np.where(ok, tt, 0.0)[..., None] * d
            diff = hp - o
            d2 = np.where(ok, dot(diff, diff), np.inf)
        j = d2.argmin(1)
        rows = np.arange(len(j))
        best[s:s + chunk] = d2[rows, j]
        hit[s:s + chunk] = np.isfinite(d2[rows, j])
        near = hp[rows, j][:, None, :]
        tied[s:s + chunk] = ok & _ulp_close(hp, near).all(-1) & hit[s:s + chunk, None]
    return hit, best, tied, applies


_EDGE_CASES = {}


def edge_case(scene, key=None, brute=True):
    """entity_edge_rays(scene) once per session (key: a name to remember it by), with what the CPU alone says about it, read-only: the closest-hit
    classes as ONE array (a ray's index is its RNG stream: the alpha draws of a launch belong to it) with the oracle's answers and the brute
    force's, the segments with the oracle's, and per class the shares of both outcomes -- at least 5 % each, from the oracle, before any device is asked."""
    if key is not None and key in _EDGE_CASES:
        return _EDGE_CASES[key]
    oracle, t = oracle_for(scene), scene.tables()
    sets = entity_edge_rays(scene)
    names = [n for n in sets if n != "shadow_ends"]
    c = {"names": names, "rays": np.concatenate([sets[n] for n in names]), "cls": np.concatenate([np.full(len(sets[n]), i) for i, n in enumerate(names)]),
         "q": sets["shadow_ends"]}
    rays = c["rays"]
    c["hit"], c["ent"], c["res"], n_leaves = oracle.trace(rays)
    c["vis"] = oracle.visible(c["q"])[0]
    c["seg_rays"], c["mt"] = segments_as_rays(c["q"])
    k = c["hit"] > 0
    if brute:
        # the brute force stands on its own: the oracle's hit is the nearest of all entities (a check of the ray set and of the oracle).  Outside its
        # reach: a ray that meets an entity whose alpha test draws a number per leaf, and a ray whose walk asks no entity at all -- it misses the root
        # box by the reference's own slab test or enters no leaf (a ray lying in a face of the root box), whatever lies on its line
        alpha = alpha_entities(scene)
        never = alpha & (t["mats"][t["tri_mat"], 1] == 0)                 # alpha = opacity * texture alpha = 0, IOR 1: no hit is ever accepted
        bh, bd2, tied, applies = brute_force_closest(t, rays, never, alpha & ~never)
        bb = t["node_bbox"][0]
        applies = applies & _root_box_entered(rays, bb[:3], bb[3:]) & (n_leaves > 0)
        od = c["res"][:, :3] - rays[:, :3]
        od2 = od[:, 0] * od[:, 0] + od[:, 1] * od[:, 1] + od[:, 2] * od[:, 2]
        bad = np.nonzero(applies & ((bh != k) | (k & ~_ulp_close(od2, np.where(k, bd2, od2)))))[0]
        assert not len(bad), (len(bad), [(names[c["cls"][i]], rays[i].tolist(), int(c["hit"][i]), int(c["ent"][i]), float(od2[i]), bool(bh[i]), float(bd2[i])) for i in bad[:3]])
        assert tied[k & applies, c["ent"][k & applies]].all()             # the oracle's own entity is one of the tied ones
        c["tied"], c["applies"] = tied, applies
    for i, name in enumerate(names):
        m = c["cls"] == i
        share = float(k[m].mean())
        line = f"  {name:12s} {int(m.sum()):5d} rays: hit {share:.1%}, miss {1 - share:.1%}"
        if brute:
            line += f"; {int((applies[m] & (tied[m].sum(1) > 1)).sum())} tied (more than one entity within 4 ulp of the nearest hit point)"
            line += f"; {int((~applies[m]).sum())} outside the brute force's reach (an alpha draw, or no entity is asked)"
        print(line)
        assert 0.05 <= share <= 0.95, (name, share)
    share = float((c["vis"] > 0).mean())
    print(f"  {'shadow_ends':12s} {len(c['q']):5d} segments: open {share:.1%}, blocked {1 - share:.1%}")
    assert 0.05 <= share <= 0.95, ("shadow_ends", share)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    if key is not None:
        _EDGE_CASES[key] = c
    return c


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def check_entity_edges(rt, scene, forms, what="closest", key=None, brute=True, others=()):
    """Rays aimed at entity edges, leaf planes and tangents (entity_edge_rays) through every form of the walk `rt` has, against the oracle and the
    brute force.  The bound is equality (the walks use IEEE + - * / sqrt only):
      * hit flag and hit point bits equal the oracle's for every ray; visibility equals the oracle's for every segment;
      * the entity is one of the brute force's tied set (hit points within 4 ulp of the nearest), and the oracle's where that set has one member --
        with it normal, u and v (two triangles that share an edge can place the hit at bitwise the same point; the reference keeps the one it met
        first and leaves entered at equal t0 may be met in another order: check_leaf_order);
      * across the device's own forms everything is bit-equal, the entity included: rt.trace / rt.visible / rt.visible_rays with wide records on
        and off, content culling off, entity boxes off, the contexts in `others` ((name, rt) pairs, e.g. made under GI_CLIP_BOXES=0), and
        rt.debug_walk for every (form, lds) of `forms`.
    brute = False (a scene with alpha-tested entities: the draws are per leaf): the oracle and the forms only.  Returns {class: rays compared}."""
    case = edge_case(scene, key, brute)
    wide = rt.set_wide_nodes(True)
    names = ["shadow_ends"] if what == "any" else case["names"]
    rays = case["seg_rays"] if what == "any" else case["rays"]
    assert len(rays) <= 24000
    cls = np.zeros(len(rays), int) if what == "any" else case["cls"]

    def run(r, how):
        if what == "any":
            q, mt = case["q"], case["mt"]
            return {"visible": lambda: (r.visible(q),), "visible_rays": lambda: (r.visible_rays(rays, mt),)}.get(how, lambda: (r.debug_walk(rays, mt, *how),))()
        return r.trace(rays) if how == "trace" else r.debug_walk(rays, None, *how)

    entries = ["visible", "visible_rays"] if what == "any" else ["trace"]
    got = {}
    for e in entries:
        got[("wide", e)] = run(rt, e)
    if wide:
        for f in forms:
            got[("debug_walk", tuple(f))] = run(rt, tuple(f))
        rt.set_wide_nodes(False)
        for e in entries:
            got[("per node", e)] = run(rt, e)
        assert rt.set_wide_nodes(True)
        if rt.set_content_culling(True):
            rt.set_content_culling(False)
            for e in entries:
                got[("no culling", e)] = run(rt, e)
            rt.set_content_culling(True)
        if rt.set_entity_boxes(True):
            rt.set_entity_boxes(False)
            for e in entries:
                got[("no entity boxes", e)] = run(rt, e)
            rt.set_entity_boxes(True)
    else:
        assert (scene.tables()["node_child"][0] < 0).all()        # only a tree of one leaf has no wide records: nothing but the plain walk to ask
        for f in forms:
            try:
                run(rt, tuple(f))
                raise AssertionError("debug_walk answered without wide records")
            except gi.GiError:
                pass
    for name, r in others:
        for e in entries:
            got[(name, e)] = run(r, e)

    def describe(i, k):
        return {"class": names[cls[i]], "row": int(i), "ray": rays[i].tolist(), "form": k, "got": [np.asarray(a)[i].tolist() for a in got[k]]}

    # against the oracle (and the brute force)
    first = next(iter(got))
    if what == "any":
        vis_o = case["vis"]
        for k, (vis,) in got.items():
            bad = np.nonzero(vis != vis_o)[0]
            assert not len(bad), (len(bad), [dict(describe(i, k), oracle=int(vis_o[i])) for i in bad[:3]])
    else:
        hit_o, ent_o, res_o = case["hit"], case["ent"], case["res"]
        tied, applies = (case["tied"], case["applies"]) if brute else (None, None)
        for k, (hit, ent, res) in got.items():
            bad = np.nonzero((hit != hit_o) | (_bits(res[:, :3]) != _bits(res_o[:, :3])).any(1))[0]
            assert not len(bad), (len(bad), [dict(describe(i, k), oracle=[int(hit_o[i]), int(ent_o[i]), res_o[i].tolist()],
                                                  brute=None if tied is None else np.nonzero(tied[i])[0].tolist()) for i in bad[:3]])
            h = hit_o > 0
            if brute:
                unique = h & (~applies | (tied.sum(1) == 1))
                member = tied[np.arange(len(ent)), np.where(h, ent, 0)] | ~h | ~applies
            else:
                unique, member = h, np.ones(len(ent), bool)
            same = (ent == ent_o) & (_bits(res[:, 3:6]) == _bits(res_o[:, 3:6])).all(1)   # (columns 6, 7: the device's barycentric u, v; the oracle's are the texture's)
            bad = np.nonzero(~member | (unique & ~same))[0]
            assert not len(bad), (len(bad), [dict(describe(i, k), oracle=[int(ent_o[i]), res_o[i].tolist()],
                                                  brute=None if tied is None else np.nonzero(tied[i])[0].tolist()) for i in bad[:3]])
    # across the forms: every bit, the entity included
    for k, v in got.items():
        for a, b in zip(v, got[first]):
            bad = np.nonzero((np.asarray(a).reshape(len(rays), -1).view(np.uint64 if a.dtype == np.float64 else a.dtype) !=
                              np.asarray(b).reshape(len(rays), -1).view(np.uint64 if b.dtype == np.float64 else b.dtype)).any(1))[0]
            assert not len(bad), (len(bad), [dict(describe(i, k), other=describe(i, first)) for i in bad[:3]])
    print(f"  {what}: {len(rays)} rays x {len(got)} forms: " + ", ".join(f"{a} {b}" for a, b in got))
    return {n: int((cls == i).sum()) for i, n in enumerate(names)}
