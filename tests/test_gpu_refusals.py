"""How the four auxiliary passes refuse a bad call: gi_render_features_*, gi_render_occlusion_*, gi_denoise_* and gi_upsample_*, device and host form.

A characterisation: tests/golden/refusals.json holds, for every bad call the header names -- one fault at a time and every pair of faults that can be
combined -- the return code, the text gi_last_error gives afterwards and what the pass's gi_last_*_ms reads.  It was recorded once, with collect()
below, from the commit before the context was split into parts, and is not regenerated: the order in which an entry refuses (which of two faults it
names) is part of its behaviour.

How a case runs: a good 8 x 8 host call of the pass first, so that the pass's timer holds a time; then an unrelated refusal with a known text (the
sentinel), so that an entry that returns a bare code shows as "message left alone"; then the bad call.  Nothing larger than an 8 x 8 frame is
allocated, and a bad call never launches: its device pointers are the address 16."""
import ctypes as C
import itertools
import json
import os

import numpy as np
import pytest

import gi_raytracer_amd as gi

import parity_checks as pc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refusals.json")
N = 8                                       # the frame: 8 x 8, one sample
NOWHERE = C.c_void_p(16)                    # a device pointer no refused call may use
NAN = float("nan")


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Pass:
    """One pass: its good arguments by name (host and device form), the faults that apply to it, its timer."""

    def __init__(self, rt, empty):
        self.rt, self.empty, self.L = rt, empty, rt.L
        self.keep = []                      # host arrays the argument lists point into

    def array(self, *shape):
        a = np.full(shape, 0.5)
        self.keep.append(a)
        return a

    def args(self, host):                   # an ordered dict name -> argument, the context first
        raise NotImplementedError

    def call(self, host, a):
        return getattr(self.L, self.entry + ("_host" if host else "_device"))(*[C.byref(v) if isinstance(v, C.Structure) else v for v in a.values()])

    def read_ms(self, h):
        ms = C.c_float(-1.0)
        rc = getattr(self.L, self.timer)(h, C.byref(ms))
        return rc, ms.value

    # faults: name -> (what it replaces, function of the argument dict).  Two faults that replace the same thing, or one a part of the other, do not combine.
    def common_faults(self):
        return {
            "null_context": ("ctx", lambda a: a.update(ctx=None)),
            "null_output": ("out", lambda a: a.update(out=None)),
        }


def _set(name, field, value):
    def apply(a):
        p = type(a[name])()
        C.pointer(p)[0] = a[name]           # a copy: the good arguments stay good
        setattr(p, field, value)
        a[name] = p
    return (name + "." + field, apply)


class FramePass(Pass):
    """The two per-pixel passes over a scene: a frame's parameters, stripes, the Halton limit."""

    def frame_faults(self):
        rt = self.rt
        no_rows = rt.params(N, N, stripe_h=N, rank=1, world=2)      # one stripe, and it is rank 0's
        assert rt.local_rows(no_rows) == 0
        f = self.common_faults()
        f.update({
            "null_frame_parameters": ("p", lambda a: a.update(p=None)),
            "no_scene": ("ctx", lambda a: a.update(ctx=self.empty.h)),
            "width_0": ("p", lambda a: a.update(p=rt.params(0, N))),
            "stripe_without_rows": ("p", lambda a: a.update(p=no_rows)),
        })
        return f


class Features(FramePass):
    entry, timer = "gi_render_features", "gi_last_features_ms"

    def args(self, host):
        return dict(ctx=self.rt.h, p=self.rt.params(N, N), n=1, out=_ptr(self.array(N, N, 8)) if host else NOWHERE, f64=1, ids=None)

    def faults(self):
        f = self.frame_faults()
        f.update({
            "n_samples_0": ("n", lambda a: a.update(n=0)),
            "n_samples_beyond_halton": ("n", lambda a: a.update(n=gi.halton_sample_cap(N, N) + 1)),
        })
        return f


class Occlusion(FramePass):
    entry, timer = "gi_render_occlusion", "gi_last_occlusion_ms"

    def args(self, host):
        return dict(ctx=self.rt.h, p=self.rt.params(N, N), op=gi.OcclusionParams(1, 4, 1.0), out=_ptr(self.array(N, N, 4)) if host else NOWHERE, f64=1)

    def faults(self):
        f = self.frame_faults()
        f["null_parameters"] = ("op", lambda a: a.update(op=None))
        for name, field, value in (("n_samples_0", "n_samples", 0), ("n_samples_beyond_halton", "n_samples", gi.halton_sample_cap(N, N) + 1),
                                   ("n_dirs_0", "n_dirs", 0), ("n_dirs_65", "n_dirs", 65), ("radius_negative", "radius", -1.0), ("radius_nan", "radius", NAN)):
            f[name] = _set("op", field, value)
        return f


class Denoise(Pass):
    entry, timer = "gi_denoise", "gi_last_denoise_ms"

    def args(self, host):
        h = lambda *s: _ptr(self.array(*s)) if host else NOWHERE
        return dict(ctx=self.rt.h, dp=self.rt.denoise_params(N, N, iterations=1), color=h(N, N, 3), color_f64=1, features=h(N, N, 8), features_f64=1, out=h(N, N, 3), f64=1)

    def faults(self):
        f = self.common_faults()
        f["null_parameters"] = ("dp", lambda a: a.update(dp=None))
        for name, field, value in (("width_0", "width", 0), ("sigma_negative", "sigma_color", -1.0), ("sigma_nan", "sigma_depth", NAN)):
            f[name] = _set("dp", field, value)
        return f


class Upsample(Pass):
    entry, timer = "gi_upsample", "gi_last_upsample_ms"

    def args(self, host):
        h = lambda *s: _ptr(self.array(*s)) if host else NOWHERE
        return dict(ctx=self.rt.h, up=self.rt.upsample_params(N, N, 2), low_color=h(N // 2, N // 2, 3), low_color_f64=1, low_features=h(N // 2, N // 2, 8), low_features_f64=1,
                    features=h(N, N, 8), features_f64=1, out=h(N, N, 3), f64=1)

    def faults(self):
        f = self.common_faults()
        f["null_parameters"] = ("up", lambda a: a.update(up=None))
        for name, field, value in (("width_0", "width", 0), ("sigma_negative", "sigma_normal", -1.0), ("sigma_nan", "sigma_depth", NAN)):
            f[name] = _set("up", field, value)
        return f


def _combine(a, b):
    return not (a == b or a.startswith(b + ".") or b.startswith(a + "."))


def collect():
    """{"<entry>: <fault> [+ <fault>]": {"rc", "error", "ms_rc", "ms"}} for every bad call, and the good calls' timers under "good"."""
    rt = gi.RayTracer(0).setScene(pc.named_scene("cornell"))
    empty = gi.RayTracer(0)
    L = rt.L
    counters = (C.c_int64 * 19)()
    out = {"bad": {}, "good": {}}
    for ps in (Features(rt, empty), Occlusion(rt, empty), Denoise(rt, empty), Upsample(rt, empty)):
        faults = ps.faults()
        singles = [(k,) for k in faults]
        pairs = [(a, b) for a, b in itertools.combinations(faults, 2) if _combine(faults[a][0], faults[b][0])]
        for host in (False, True):
            form = ps.entry + ("_host" if host else "_device")
            for names in singles + pairs:
                assert ps.call(True, ps.args(True)) == gi.GI_OK and ps.read_ms(rt.h)[1] > 0                 # the pass's timer holds a time
                a = ps.args(host)
                for k in names:
                    faults[k][1](a)
                h = a["ctx"] if a["ctx"] is not None else rt.h                                              # whose message and timer to look at
                assert L.gi_get_stream_counters(h, counters) == gi.GI_E_STATE                               # the sentinel message
                sentinel = L.gi_last_error(h)
                rc = ps.call(host, a)
                err = L.gi_last_error(h)
                ms_rc, ms = ps.read_ms(h)
                out["bad"][form + ": " + " + ".join(names)] = {"rc": rc, "error": "(left alone)" if err == sentinel else err.decode(), "ms_rc": ms_rc,
                                                               "ms": "0" if ms == 0.0 else "the good call's" if ms > 0 else "?"}
        # one good call per form: the timer reads a positive time, and the same one again
        hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")      # device buffers from the HIP runtime the library itself uses (no second runtime in this process)
        d = C.c_void_p()
        assert hip.hipMalloc(C.byref(d), C.c_size_t(4 * N * N * 8 * 8)) == 0      # room for every argument of a pass, 8 x 8 x 8 doubles apiece
        try:
            assert hip.hipMemset(d, 0, C.c_size_t(4 * N * N * 8 * 8)) == 0
            for host in (False, True):
                a = ps.args(host)
                if not host:
                    slots = [k for k, v in a.items() if v is NOWHERE]
                    for i, k in enumerate(slots):
                        a[k] = C.c_void_p(d.value + i * N * N * 8 * 8)
                rc = ps.call(host, a)
                first, second = ps.read_ms(rt.h), ps.read_ms(rt.h)
                assert hip.hipDeviceSynchronize() == 0
                out["good"][ps.entry + ("_host" if host else "_device")] = {"rc": rc, "ms_rc": first[0], "positive": first[1] > 0, "same_again": first == second}
        finally:
            assert hip.hipFree(d) == 0
    return out


@pytest.fixture(scope="module")
def got():
    return collect()


@pytest.fixture(scope="module")
def want():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_bad_call_is_refused_as_recorded(got, want):
    assert sorted(got["bad"]) == sorted(want["bad"])
    differ = {k: (got["bad"][k], want["bad"][k]) for k in want["bad"] if got["bad"][k] != want["bad"][k]}
    for k, (g, w) in differ.items():
        print(f"{k}\n   now      {g}\n   recorded {w}")
    assert not differ, f"{len(differ)} of {len(want['bad'])} bad calls are refused differently"


def test_the_recording_is_what_the_header_says(want):
    """The recording itself: a bad call is GI_E_INVALID or GI_E_STATE (a stripe without rows alone is no fault: GI_OK and no work), and the pass's time is
    0 after it -- except under a null context, which has no timer to reset."""
    assert len(want["bad"]) == 290
    for k, r in want["bad"].items():
        faults = k.split(": ")[1].split(" + ")
        if faults == ["stripe_without_rows"]:
            assert r["rc"] == gi.GI_OK, k
        else:
            assert r["rc"] in (gi.GI_E_INVALID, gi.GI_E_STATE), k
        if "no_scene" in faults and r["rc"] == gi.GI_E_STATE:
            assert "no scene" in r["error"], k
        assert r["ms_rc"] == gi.GI_OK and r["ms"] == ("the good call's" if "null_context" in faults else "0"), k


def test_a_good_call_times_itself(got, want):
    assert got["good"] == want["good"]
    assert len(got["good"]) == 8
    for k, r in got["good"].items():
        assert r == {"rc": gi.GI_OK, "ms_rc": gi.GI_OK, "positive": True, "same_again": True}, k
