"""GI_SAMPLE_IDENTITY: a chunk whose samples are all in flight at once is started whole by the first pass, slot s carries sample sample0 + s
throughout, and the stream passes are given no slot -> sample table (gi_pool.h: sample_of; gi_stream.inc: stream_samples).  Where the table is kept -- the
knob at 0, a pool smaller than the chunk so that freed slots take new samples -- the frame is the same bit for bit: which table a path's place in the
radiance buffer is read from is bookkeeping, not arithmetic.  Scenes with a medium and with textures run the other kernel instances and the
finisher; a progressive session takes the frame in two chunks with a sample0 of their own.  Which of the two a frame ran with, and the size of its
pool, is read off the per-chunk line of GI_DEBUG_WF: a default frame that quietly kept the table would compare table with table and must fail here."""
import re

import numpy as np
import pytest

import gi_raytracer_amd as gi

import parity_checks as pc

pytestmark = pytest.mark.gpu

W, H, SPP, PHOTONS = 64, 48, 4, 20000


def _rt(scene, monkeypatch, knob):
    if knob is None:
        monkeypatch.delenv("GI_SAMPLE_IDENTITY", raising=False)
    else:
        monkeypatch.setenv("GI_SAMPLE_IDENTITY", knob)
    rt = gi.RayTracer(0).setScene(scene)          # the knobs are read when the context is created
    if scene.desc().n_light > 0:
        rt.tracePhotons(PHOTONS)
    return rt


def _frame(rt, w=W, h=H, spp=SPP):
    return rt.run(w, h, min_samples=spp, max_samples=spp)


def _chunks(capfd):
    """(samples, pool slots, table state) of every chunk since the last call, from the library's stderr."""
    return [(int(a), int(b), c) for a, b, c in re.findall(r"\[st\] chunk of (\d+) samples: pool (\d+) slots, sample table (on|off)", capfd.readouterr().err)]


def test_identity_table_and_reissued_slots_give_one_frame(monkeypatch, capfd):
    scene = pc.load_scene("caustics")
    monkeypatch.setenv("GI_DEBUG_WF", "1")         # read at every frame
    rt0 = _rt(scene, monkeypatch, None)
    capfd.readouterr()
    ident = _frame(rt0)
    assert _chunks(capfd) == [(SPP, W * H * SPP, "off")]            # the whole frame in flight, no table
    rt = _rt(scene, monkeypatch, "0")
    capfd.readouterr()
    table = _frame(rt)
    assert _chunks(capfd) == [(SPP, W * H * SPP, "on")]             # the knob keeps the table and leaves the pool as it was
    rt2 = _rt(scene, monkeypatch, None)
    rt2.set_pool_slots(W * H * SPP // 3)            # three fills of the pool: slots are reissued, so the table it is, and several passes start paths
    capfd.readouterr()
    small = _frame(rt2)
    assert _chunks(capfd) == [(SPP, W * H * SPP // 3, "on")]
    assert ident.dtype == np.float64 and ident.any()
    assert np.array_equal(ident, table)
    assert np.array_equal(ident, small)


@pytest.mark.parametrize("name", ["fog", "textures"])
def test_identity_and_table_agree_on_other_kernel_instances(name, monkeypatch):
    scene = pc.load_scene(name)
    ident = _frame(_rt(scene, monkeypatch, None))
    table = _frame(_rt(scene, monkeypatch, "0"))
    assert ident.any()
    assert np.array_equal(ident, table)


def test_later_passes_without_the_finisher(monkeypatch, capfd):
    """GI_FINISH_THRESHOLD=0: the stragglers of this small frame stay in the stream passes to the end, so the trace, shade and gather kernels of the
    passes after the first read sample_of as well -- with an ambient light, also the trace stage's add for a path that ends in a miss."""
    monkeypatch.setenv("GI_FINISH_THRESHOLD", "0")
    monkeypatch.setenv("GI_DEBUG_WF", "1")
    scene = pc.load_scene("caustics")
    scene.set_ambient((0.25, 0.5, 0.125))
    scene.rebuild()
    rt = _rt(scene, monkeypatch, None)
    capfd.readouterr()
    ident = _frame(rt)
    err = capfd.readouterr().err
    assert "sample table off" in err
    cont = [int(v) for v in re.findall(r"\[st\] new \d+ cont (\d+)", err)]
    assert len(cont) >= 3 and cont[1] > 0            # paths went on past the second pass, in the passes
    table = _frame(_rt(scene, monkeypatch, "0"))
    assert ident.any() and np.array_equal(ident, table)


@pytest.mark.parametrize("knob", [None, "0"])
def test_progressive_steps_match_the_one_shot_frame(knob, monkeypatch):
    scene = pc.load_scene("caustics")
    rt = _rt(scene, monkeypatch, knob)
    oneshot = _frame(rt)
    with rt.progressive(W, H, min_samples=SPP, max_samples=SPP) as s:
        s.step(2)
        img = s.step(2)
    assert np.array_equal(img, oneshot)


@pytest.mark.parametrize("w,h,spp", [(61, 37, 4), (64, 48, 1), (61, 37, 1)])
def test_ragged_tiles_and_one_sample(w, h, spp, monkeypatch):
    """61 x 37: the 8x8 tile order ends in ragged tiles on both sides; spp 1: a chunk of one sample per pixel."""
    scene = pc.load_scene("caustics")
    rt = _rt(scene, monkeypatch, None)
    ident = _frame(rt, w, h, spp)
    rt.set_pool_slots(max(64, w * h * spp // 3))   # the same context falls back to the table when the chunk no longer fits
    small = _frame(rt, w, h, spp)
    table = _frame(_rt(scene, monkeypatch, "0"), w, h, spp)
    assert ident.any()
    assert np.array_equal(ident, table)
    assert np.array_equal(ident, small)
