"""The schedule of the stream passes (gi_stream.inc) against a recording: tests/golden/stream_schedule.json holds, for the three scenes of
test_gpu_free_list at 64 x 48, 8 spp and 4000 photon indices, what the commit before the scheduler was split into stages rendered and how --
the SHA-256 of the f64 frame and of the samples-per-pixel buffer, n_launches of gi_last_render_ms and the (new, cont, free, gather) of every
"[st] new ..." line of GI_DEBUG_WF -- for the default pool, a pool of a third of the frame, an adaptive frame of 2 .. 8 samples, render mode 2
and a progressive session of 3 + 5 samples.  A scheduler that launches one kernel more or less, hands a freed slot out in another pass, sizes
the pool differently or reorders two launches that share a workspace shows up here.  Every comparison is exact.

python tests/test_gpu_stream_schedule.py FILE writes a recording of the library as built (how the fixture was made)."""
import hashlib
import json
import os
import re
import sys
import tempfile

import numpy as np
import pytest

import gi_raytracer_amd as gi

import parity_checks as pc

pytestmark = pytest.mark.gpu

W, H, SPP, PHOTONS = 64, 48, 8, 4000
SCENES = ["caustics", "cornell", "two_lights_glass"]
CASES = ["default", "pool_third", "adaptive", "rounds", "progressive"]
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stream_schedule.json")
_RT = {}


class _Stderr:
    """The library's stderr (file descriptor 2) of the block, as text in .text afterwards."""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode()
        self.tmp.close()


def _context(name):
    """One context per scene, shared by the cases; every case starts from the default pool and mode."""
    if name not in _RT:
        scene = pc.named_scene(name)
        rt = gi.RayTracer(0).setScene(scene)
        if scene.desc().n_light > 0:
            rt.tracePhotons(PHOTONS)
        _RT[name] = rt
    rt = _RT[name]
    rt.set_pool_slots(1 << 30)
    rt.set_render_mode("wavefront")
    return rt


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _call(rt, render):
    """One render call: what it returned and how the passes ran."""
    with _Stderr() as err:
        img, spp = render()
    assert img.dtype == np.float64 and spp.dtype == np.int32
    passes = [[int(v) for v in m] for m in re.findall(r"\[st\] new (\d+) cont (\d+) free (\d+) gather (\d+)", err.text)]
    return {"frame": _sha(img), "spp": _sha(spp), "n_launches": rt.last_render_ms()[1], "passes": passes}


def record(name, case):
    """The calls of a case (one, or the two steps of the session), each as _call describes it."""
    rt = _context(name)
    old = os.environ.get("GI_DEBUG_WF")
    os.environ["GI_DEBUG_WF"] = "1"         # read at every render call
    try:
        if case == "progressive":
            with rt.progressive(W, H, min_samples=SPP, max_samples=SPP) as s:
                return [_call(rt, lambda: s.step(3, want_spp=True)), _call(rt, lambda: s.step(5, want_spp=True))]
        kw = dict(min_samples=2, max_samples=8) if case == "adaptive" else dict(min_samples=SPP, max_samples=SPP)
        if case == "pool_third":
            rt.set_pool_slots(W * H * SPP // 3 + 1)
        if case == "rounds":
            rt.set_render_mode("rounds")
        return [_call(rt, lambda: rt.run(W, H, want_spp=True, **kw))]
    finally:
        os.environ.pop("GI_DEBUG_WF", None)
        if old is not None:
            os.environ["GI_DEBUG_WF"] = old


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("name", SCENES)
def test_schedule_is_the_recorded_one(name, case, recorded):
    want, got = recorded[name][case], record(name, case)
    assert len(got) == len(want) == (2 if case == "progressive" else 1)
    for g, w in zip(got, want):
        assert g["passes"] and g["passes"] == w["passes"]         # the same paths started, carried on, freed and gathered, pass by pass
        assert g["n_launches"] == w["n_launches"]
        assert g["spp"] == w["spp"] and g["frame"] == w["frame"]


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:          # one line per scene and case
        scenes = [",\n".join(f'  "{case}": {json.dumps(record(name, case))}' for case in CASES) for name in SCENES]
        f.write("{\n" + ",\n".join(f' "{name}": {{\n{body}\n }}' for name, body in zip(SCENES, scenes)) + "\n}\n")
