"""The free list of the stream passes has one reader: the refill of the next pass, which hands freed slots to samples that have not been started.
From the pass in which the last sample is started (and in every pass of an adaptive round or of render mode 2) nothing reads it, so the kernels get
no free queue, the compaction leaves the queue out and the pass reports 0 freed slots (gi_stream.inc: trace_stage).  GI_KEEP_FREE_LIST=1 writes
it in every pass as before.  Which slots are listed where nobody looks is bookkeeping, not arithmetic: every frame here is compared byte for byte
with the same frame of a context that keeps the list.  What the passes did is read off the per-pass line of GI_DEBUG_WF, so a default context that
quietly kept the list, or one that dropped it while samples were still waiting for a slot, fails here too."""
import os
import re

import numpy as np
import pytest

import gi_raytracer_amd as gi

import parity_checks as pc

pytestmark = pytest.mark.gpu

W, H, SPP, PHOTONS = 64, 48, 8, 4000
SCENES = ["caustics", "cornell", "two_lights_glass"]
_PAIRS = {}


def _context(scene, env):
    """A context created under `env` (the knobs are read when the context is created); the environment is left as it was."""
    keys = ("GI_KEEP_FREE_LIST", "GI_SAMPLE_IDENTITY", "GI_FINISH_THRESHOLD")
    old = {k: os.environ.pop(k, None) for k in keys}
    try:
        os.environ.update(env)
        rt = gi.RayTracer(0).setScene(scene)
        if scene.desc().n_light > 0:
            rt.tracePhotons(PHOTONS)
        return rt
    finally:
        for k in keys:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def _pair(name):
    """(context that drops the list where it has no reader, context that always keeps it) of a scene: made once, shared by the cases."""
    if name not in _PAIRS:
        scene = pc.named_scene(name)
        _PAIRS[name] = (_context(scene, {}), _context(scene, {"GI_KEEP_FREE_LIST": "1"}))
    for rt in _PAIRS[name]:
        rt.set_pool_slots(1 << 30)
        rt.set_render_mode("wavefront")
    return _PAIRS[name]


def _passes(capfd):
    """(new, cont, free) of every pass since the last call, from the library's stderr."""
    return [tuple(int(v) for v in m) for m in re.findall(r"\[st\] new (\d+) cont (\d+) free (\d+)", capfd.readouterr().err)]


def _same(a, b):
    assert a.dtype == np.float64 and a.any()
    assert a.tobytes() == b.tobytes()


def _both(name, capfd, monkeypatch, render, setup=lambda rt: None):
    """render(rt) on both contexts of the scene: the two results and the passes each of them ran."""
    monkeypatch.setenv("GI_DEBUG_WF", "1")         # read at every frame
    out = []
    for rt in _pair(name):
        setup(rt)
        capfd.readouterr()
        res = render(rt)
        out.append((res, _passes(capfd)))
    return out


@pytest.mark.parametrize("name", SCENES)
def test_whole_frame_in_flight(name, capfd, monkeypatch):
    """Default pool: pass 0 starts every sample, so no pass of the frame wants the list."""
    (drop, p_drop), (keep, p_keep) = _both(name, capfd, monkeypatch, lambda rt: rt.run(W, H, min_samples=SPP, max_samples=SPP))
    _same(drop, keep)
    assert [p[:2] for p in p_drop] == [p[:2] for p in p_keep] and p_drop[0][0] == W * H * SPP
    assert all(p[2] == 0 for p in p_drop)           # nothing listed ...
    assert p_keep[0][2] > 0                         # ... where the knob lists the paths that ended


@pytest.mark.parametrize("name", SCENES)
def test_pool_of_a_third_refills_from_the_list(name, capfd, monkeypatch):
    """At least three passes start samples in freed slots; the list is kept for exactly those, and the last refill takes fewer slots than were freed."""
    total = W * H * SPP
    pool = total // 3 + 1
    (drop, p_drop), (keep, p_keep) = _both(name, capfd, monkeypatch, lambda rt: rt.run(W, H, min_samples=SPP, max_samples=SPP), lambda rt: rt.set_pool_slots(pool))
    _same(drop, keep)
    _same(drop, _pair(name)[0].run(W, H, min_samples=SPP, max_samples=SPP))      # and the frame of the whole pool
    for passes in (p_drop, p_keep):
        new = [p[0] for p in passes]
        assert sum(new) == total and new[0] == pool                             # every sample is started, once
        assert sum(1 for n in new if n > 0) >= 3
    assert [p[:2] for p in p_drop] == [p[:2] for p in p_keep]
    last = max(k for k, p in enumerate(p_drop) if p[0] > 0)                      # the pass that starts the last sample: its own list has no reader
    assert all(d[2] == k[2] for d, k in zip(p_drop[:last], p_keep[:last]))        # before it: the list as the knob writes it
    assert all(p[2] == 0 for p in p_drop[last:])
    assert p_drop[last][0] < p_drop[last - 1][2]                                 # the last refill left freed slots unused


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("short", [0, 64])
def test_pool_of_the_frame_and_just_below(name, short, capfd, monkeypatch):
    """The boundary of "the chunk fits the pool": a pool of exactly the frame starts everything in pass 0; 64 slots less, and pass 1 refills 64."""
    total = W * H * SPP
    (drop, p_drop), (keep, p_keep) = _both(name, capfd, monkeypatch, lambda rt: rt.run(W, H, min_samples=SPP, max_samples=SPP), lambda rt: rt.set_pool_slots(total - short))
    _same(drop, keep)
    assert [p[:2] for p in p_drop] == [p[:2] for p in p_keep]
    assert sum(p[0] for p in p_drop) == total and p_drop[0][0] == total - short
    if short:
        assert p_drop[0][2] == p_keep[0][2] > 0 and p_drop[1][0] == short        # pass 0 still lists: pass 1 reads it
        assert all(p[2] == 0 for p in p_drop[1:])
    else:
        assert all(p[2] == 0 for p in p_drop)


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("mode", ["adaptive", "rounds"])
def test_rounds_never_want_the_list(name, mode, capfd, monkeypatch):
    """Adaptive frames (4 .. 16 samples) and render mode 2 go through the same passes and hand no freed slot out again."""
    def setup(rt):
        if mode == "rounds":
            rt.set_render_mode("rounds")
    kw = dict(min_samples=4, max_samples=16) if mode == "adaptive" else dict(min_samples=SPP, max_samples=SPP)
    ((drop, spp_drop), p_drop), ((keep, spp_keep), p_keep) = _both(name, capfd, monkeypatch, lambda rt: rt.run(W, H, want_spp=True, **kw), setup)
    _same(drop, keep)
    assert np.array_equal(spp_drop, spp_keep) and spp_drop.min() >= kw["min_samples"] and spp_drop.max() <= kw["max_samples"]
    assert [p[:2] for p in p_drop] == [p[:2] for p in p_keep]                    # the same paths started and carried on, pass by pass
    started = sum(p[0] for p in p_drop)
    if mode == "rounds":
        assert started == W * H * SPP == int(spp_drop.sum())                     # a fixed count: no sample is started on speculation
    else:
        assert started >= int(spp_drop.sum())                                    # a round may start samples the variance rule then discards (k_ad_gen)
    assert p_drop and all(p[2] == 0 for p in p_drop) and any(p[2] > 0 for p in p_keep)


@pytest.mark.parametrize("name", SCENES)
def test_progressive_steps_with_the_sample_table(name, capfd, monkeypatch):
    """Two steps of a session, each a chunk with a sample0 of its own, with the slot -> sample table kept (GI_SAMPLE_IDENTITY=0)."""
    scene = pc.named_scene(name)
    monkeypatch.setenv("GI_DEBUG_WF", "1")
    frames = []
    for env in ({"GI_SAMPLE_IDENTITY": "0"}, {"GI_SAMPLE_IDENTITY": "0", "GI_KEEP_FREE_LIST": "1"}):
        rt = _context(scene, env)
        capfd.readouterr()
        with rt.progressive(W, H, min_samples=SPP, max_samples=SPP) as s:
            first = s.step(SPP // 2)
            frames.append((first, s.step(SPP // 2), _passes(capfd)))
    (d1, d2, p_drop), (k1, k2, p_keep) = frames
    _same(d1, k1)
    _same(d2, k2)
    _same(d2, _pair(name)[1].run(W, H, min_samples=SPP, max_samples=SPP))        # the one-shot frame
    assert sum(p[0] for p in p_drop) == W * H * SPP and all(p[2] == 0 for p in p_drop) and any(p[2] > 0 for p in p_keep)


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("pool_div", [1, 3])
def test_queue_order_with_ragged_segments(name, pool_div, capfd, monkeypatch):
    """61 x 47, and GI_FINISH_THRESHOLD=0 so that the stragglers stay in the passes: the last passes hold fewer paths than there are producer
    workgroups, so most segments the compaction closes up are empty and the others end ragged.  The order of its output decides the order of the
    shadow queries and what the sorts see: the frame is that of the context that keeps the list, and of the other pool size."""
    w, h = 61, 47
    scene = pc.named_scene(name)
    monkeypatch.setenv("GI_DEBUG_WF", "1")
    frames = []
    for env in ({"GI_FINISH_THRESHOLD": "0"}, {"GI_FINISH_THRESHOLD": "0", "GI_KEEP_FREE_LIST": "1"}):
        rt = _context(scene, env)
        rt.set_pool_slots(max(64, w * h * SPP // pool_div + (1 if pool_div > 1 else 0)))
        capfd.readouterr()
        frames.append((rt.run(w, h, min_samples=SPP, max_samples=SPP), _passes(capfd)))
    (drop, p_drop), (keep, p_keep) = frames
    _same(drop, keep)
    _same(drop, _pair(name)[0].run(w, h, min_samples=SPP, max_samples=SPP))      # whole pool, finisher at its default
    assert sum(p[0] for p in p_drop) == w * h * SPP
    assert [p[:2] for p in p_drop] == [p[:2] for p in p_keep]
    assert len(p_drop) >= 3 and 0 < p_drop[-2][1] < 256                          # a pass with fewer paths than one workgroup of the compaction
