"""GI_EARLY_MISS: the deferred shade kernel ends a path whose next ray leaves the scene without meeting a leaf (gi_walk.h: ray_leaves_scene), and
with it releases the slot of a path that does not continue even while its gather is pending.  A schedule, not arithmetic: frames with the knob at 0
and at 1 are the same bit for bit.  Open and closed triangle scenes (caustics; cornell, teapot), a textured scene, and three scenes where part or
all of the frame takes the path the knob does not touch: spheres, the medium (the probe is off with fog) and two lights; and large alpha-tested
triangles over an open floor (pc.large_alpha_scene: a path ends or goes on with the draw of a later leaf).  Each as a streaming
frame with every path in flight at once, with a pool so small that slots are handed on from pass to pass (what releasing a slot with its gather
pending has to survive), and in render mode 2 (rounds)."""
import numpy as np
import pytest

import gi_raytracer_amd as gi

import parity_checks as pc

pytestmark = pytest.mark.gpu

W, H, SPP, SEED = 160, 90, 12, 11


def _frames(scene, monkeypatch, knob):
    monkeypatch.setenv("GI_EARLY_MISS", knob)
    rt = gi.RayTracer(0).setScene(scene)          # the knobs are read when the context is created
    if scene.desc().n_light > 0:
        rt.tracePhotons(4000)
    out = {}
    out["whole frame in flight"] = rt.run(W, H, min_samples=SPP, max_samples=SPP, seed=SEED)
    rt.set_pool_slots(max(64, W * H * SPP // 7))   # seven fills of the pool: freed slots take new samples while older paths are still under way
    out["small pool"] = rt.run(W, H, min_samples=SPP, max_samples=SPP, seed=SEED)
    rt.set_pool_slots(1 << 30)
    rt.set_render_mode("rounds")
    out["rounds"] = rt.run(W, H, min_samples=SPP, max_samples=SPP, seed=SEED)
    rt.set_pool_slots(W * H * 2)                   # rounds of two samples per pixel
    out["rounds, small pool"] = rt.run(W, H, min_samples=SPP, max_samples=SPP, seed=SEED)
    rt.set_pool_slots(1 << 30)
    rt.set_render_mode("wavefront")
    return out


@pytest.mark.parametrize("name", ["caustics", "cornell", "teapot", "textures", "spheres", "fog", "two_lights", "large_alpha"])
def test_early_miss_changes_nothing(name, monkeypatch):
    scene = pc.named_scene(name)
    off = _frames(scene, monkeypatch, "0")
    on = _frames(scene, monkeypatch, "1")
    for what in off:
        a, b = off[what].view(np.uint64), on[what].view(np.uint64)
        assert np.array_equal(a, b), (name, what, int((a != b).any(axis=-1).sum()), "pixels differ")
    assert off["whole frame in flight"].any()
    # the small pool and the rounds are schedules too
    for what in off:
        assert np.array_equal(off[what].view(np.uint64), off["whole frame in flight"].view(np.uint64)), (name, what)


def test_probe_depth_is_a_schedule(monkeypatch):
    """GI_EARLY_MISS_TURNS: how many turns the probe may take before it hands the ray to the trace stage decides only WHERE a miss is found."""
    scene = pc.load_scene("caustics")
    frames = []
    for turns in ("1", "2", "4", "64"):
        monkeypatch.setenv("GI_EARLY_MISS", "1")
        monkeypatch.setenv("GI_EARLY_MISS_TURNS", turns)
        rt = gi.RayTracer(0).setScene(scene)
        rt.tracePhotons(4000)
        rt.set_pool_slots(max(64, W * H * SPP // 7))
        frames.append(rt.run(W, H, min_samples=SPP, max_samples=SPP, seed=SEED))
    for f in frames[1:]:
        assert np.array_equal(frames[0].view(np.uint64), f.view(np.uint64))
