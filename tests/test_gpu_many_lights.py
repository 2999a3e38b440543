"""Three, four, five and six lights on the MI355X: the kernel instances and the host-side switch that exist for scenes with several lights.

With one to four lights the streaming passes put the shadow walks off to k_st_shadow (gi_stream.inc: defers_shadows), k_st_shade<.., 2> writing one
query per light and k_st_shadow<.., MULTI = 1> asking them from the last light down; with five or more they fall back to k_st_shade<.., DEFER = 0>,
which walks every light inline.  The scenes are pc.many_lights_scene's: tests/test_device_logic_cpu.py shows with the oracle alone that their frames
hold every class of vertex these paths treat differently (test_many_lights_scenes_reach_every_branch).  All frames are 96 x 54 at 8 spp with 4000
photon indices unless a test says otherwise."""
import numpy as np
import pytest

import gi_raytracer_amd as gi
import parity_checks as pc

pytestmark = pytest.mark.gpu

W, H, SPP, PHOTONS = 96, 54, 8, 4000
SCENES = ["three_lights", "four_lights", "five_lights", "four_lights_emitter", "three_lights_fog"]
KNOBS = ("GI_DEFER_SHADOWS", "GI_REFILL_MIN", "GI_SORT_SHADE", "GI_COOP_FACTOR")
_CASES = {}


def _case(name):
    """(scene, context with the photon map of PHOTONS indices loaded, those photons), once per scene; the tests leave the context as they found it."""
    if name not in _CASES:
        scene = pc.named_scene(name)
        rt = gi.RayTracer(0).setScene(scene)
        ph, _ = rt.tracePhotons(PHOTONS)
        assert len(ph) > 200 * scene.desc().n_light
        _CASES[name] = (scene, rt, ph)
    scene, rt, ph = _CASES[name]
    scene.build_photon_map(ph)          # (a test that emitted another set puts this one back)
    rt.upload_photon_map()
    return scene, rt, ph


def _frame(rt):
    return rt.run(W, H, min_samples=SPP, max_samples=SPP)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("name", SCENES)
def test_frames_match_oracle_in_every_schedule(name):
    """wavefront (k_st_shade<.., 2> + k_st_shadow<.., 1> up to four lights, the inline walks from five on), rounds and megakernel: the same bits, and
    the oracle's frame to 1e-9, the bound the suite holds glass-free and fog scenes to (no glass here: the arithmetic differs by ~1e-18)."""
    scene, rt, _ = _case(name)
    frames, rmses = {}, {}
    try:
        rmses["wavefront"], frames["wavefront"], ref = pc.check_render(rt, scene, W, H, SPP, PHOTONS, tol=1e-9)
        for mode in ("rounds", "megakernel"):
            rt.set_render_mode(mode)
            frames[mode] = _frame(rt)
            rmses[mode] = float(np.sqrt(((frames[mode] - ref) ** 2).mean()))
    finally:
        rt.set_render_mode("wavefront")
    print(name, "rmse vs oracle", {k: "%.3e" % v for k, v in rmses.items()}, "mean", float(frames["wavefront"].mean()))
    for mode in ("rounds", "megakernel"):
        assert rmses[mode] < 1e-9, (mode, rmses)
        assert _same_bits(frames["wavefront"], frames[mode]), mode
    assert frames["wavefront"].mean() > 1e-3


def test_six_lights_wavefront_equals_megakernel():
    """Nothing is special about five: six lights take the same inline walks."""
    scene, rt, _ = _case("six_lights")
    assert scene.desc().n_light == 6
    try:
        a = _frame(rt)
        rt.set_render_mode("megakernel")
        b = _frame(rt)
    finally:
        rt.set_render_mode("wavefront")
    assert _same_bits(a, b) and a.mean() > 1e-3


def _fresh(name, monkeypatch, env):
    """A context created under `env` (the knobs are read at context creation), with the scene's photon map."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    scene = _case(name)[0]
    rt = gi.RayTracer(0).setScene(scene)
    rt.upload_photon_map()
    return rt


@pytest.mark.parametrize("name", SCENES)
def test_where_the_walk_happens_is_a_schedule(name, monkeypatch):
    """Inside k_st_shade or put off to k_st_shadow, lockstep waves or refills at 5 idle lanes, the shade queue sorted or not, the finisher's form: the
    frame is the same bit for bit (for five lights GI_DEFER_SHADOWS changes nothing by construction; the other knobs still move its walks)."""
    frames = [_frame(_fresh(name, monkeypatch, env)) for env in ({}, {"GI_DEFER_SHADOWS": "0"}, {"GI_REFILL_MIN": "64"}, {"GI_REFILL_MIN": "5"}, {"GI_SORT_SHADE": "0"}, {"GI_COOP_FACTOR": "0"})]
    assert _same_bits(frames[0], _frame(_case(name)[1]))
    for k, f in enumerate(frames[1:]):
        assert _same_bits(frames[0], f), k + 1


def test_shadow_stage_runs_up_to_four_lights_only(monkeypatch):
    """The 1..4 / 5+ split of defers_shadows, seen in the per-kernel device times of the last frame: k_st_shadow has run for four lights, and has
    not for five, nor for four under GI_DEFER_SHADOWS=0.  A pass without it launches one kernel less."""
    def shadow_ms_and_launches(name, env):
        rt = _fresh(name, monkeypatch, env)
        _frame(rt)
        return rt.last_kernel_ms()["shadow"], rt.last_render_ms()[1], rt.last_kernel_ms()["shade"]
    four, four_inline, five = shadow_ms_and_launches("four_lights", {}), shadow_ms_and_launches("four_lights", {"GI_DEFER_SHADOWS": "0"}), shadow_ms_and_launches("five_lights", {})
    three = shadow_ms_and_launches("three_lights", {})
    print("shadow ms, launches, shade ms: three", three, "four", four, "four inline", four_inline, "five", five)
    assert three[0] > 0.0 and four[0] > 0.0
    assert four_inline[0] == 0.0 and five[0] == 0.0
    assert four_inline[2] > 0.0 and five[2] > 0.0
    assert four_inline[1] < four[1]                      # the same passes (the same frame, above), each without its shadow launch


@pytest.mark.parametrize("name", ["four_lights", "four_lights_emitter"])
def test_refills_with_a_stride_of_four(name):
    """Pools of a third and a seventh of the samples: freed slots are handed out again, the shade queue is sorted by slot from the second pass on
    (q_orig names an item's four queries), and an emitting vertex's A0 waits in pool.L while other passes run.  The whole-frame-in-flight frame, bit for bit."""
    scene, rt, _ = _case(name)
    a = _frame(rt)
    try:
        for div in (3, 7):
            rt.set_pool_slots(max(64, W * H * SPP // div))
            assert _same_bits(a, _frame(rt)), div
    finally:
        rt.set_pool_slots(1 << 30)


@pytest.mark.parametrize("name", ["three_lights", "five_lights"])
def test_per_ray_radiance_matches_oracle(name):
    """gi_radiance on 4000 primary rays (samples 0 and 1 of the frame's pixels, their own Halton indices as streams) with the photon map loaded."""
    scene, rt, ph = _case(name)
    o = pc.oracle_for(scene)
    o.set_photons(ph).build_photon_map()
    rs = np.random.RandomState(7)
    rays, stream = [], []
    for k in range(4000):
        i, r = o.primary_ray(W, H, k & 1, int(rs.randint(W)), int(rs.randint(H)))
        rays.append(r); stream.append(i)
    rays, stream = np.array(rays), np.array(stream, np.uint32)
    got, want = rt.radiance(rays, stream), o.radiance(rays, stream, rt.seed)
    assert (want.max(axis=1) > 0).mean() > 0.3
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("name", ["three_lights", "five_lights"])
def test_emission_identical_to_oracle(name):
    scene, rt, _ = _case(name)
    _, ph = pc.check_emission(rt, scene, 2000)
    assert len(ph) > 200 * scene.desc().n_light          # photons of every light reach the map (off the mirror wall)


def test_emission_on_the_device_leaves_the_same_map():
    """gi_trace_photons compacts the photons of (index, light) pairs on the device (k_rs_scan / k_pb_compact_emitted) and builds the map there; the
    host hop reads them back and builds it on the host: the same tables, the same number of tries, with three lights."""
    scene, rt, _ = _case("three_lights")
    ph, tries = rt.tracePhotons(6000)
    host = rt.photon_tables_on_device()
    n, tries_d = rt.tracePhotonsOnDevice(6000)
    dev = rt.photon_tables_on_device()
    assert n == len(ph) > 3 * 1000 and tries_d == tries
    assert len(host["nodes"]) > 10 and all(np.array_equal(host[k], dev[k]) for k in ("nodes", "ranges", "pos", "dircol"))


@pytest.mark.parametrize("name", ["three_lights", "four_lights", "four_lights_emitter"])
def test_shadow_segments_walked_lie_between_one_and_n_per_vertex(name):
    """gi_set_counters(ctx, 2): every shaded vertex puts its queries off (one per light), and k_st_shadow walks at least the last light's segment and at
    most all n of a vertex: v <= s <= n v with v the shaded vertices and s the segments.  The census has vertices whose last light is visible and
    vertices that see no light, so for four lights s lies strictly between the ends.  v is the oracle's count of shaded vertices; counting changes
    no bit of the frame."""
    scene, rt, ph = _case(name)
    n = scene.desc().n_light
    o = pc.oracle_for(scene)
    o.set_photons(ph).build_photon_map()
    oc = o.render(W, H, SPP, want_counters=True)["counters"]       # v_trace, v_shadow, tri, shaded, pcand, traces, shadows, gathers, tri_shadow
    plain = _frame(rt)
    rt.set_counters("stream")
    try:
        counted = _frame(rt)
        c = rt.stream_counters()
    finally:
        rt.set_counters(0)
    v, s = c["shaded"], c["shadow_rays"]
    print(name, "shaded vertices", v, "shadow segments", s, "bounds", v, n * v, "walks begun", c["shadow_walks"], "reference visible() calls", int(oc[6]))
    assert _same_bits(plain, counted)
    assert v == oc[3] and n * v == oc[6]                            # the reference asks every light of every vertex
    assert v <= s <= n * v
    assert c["shadow_walks"] == s                                   # one root-box test per segment, also where the walk then does not begin
    if n == 4:
        assert v < s < n * v
