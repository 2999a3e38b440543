"""The pass timers of the C ABI (gi_last_features_ms, gi_last_denoise_ms, gi_last_upsample_ms; one EventTimer each, gi_scratch.h): 0 before any
call, a positive time after a pass, the same time when read again, and 0 again after a call that was rejected for its parameters."""
import numpy as np
import pytest

import gi_raytracer_amd as gi

import parity_checks as pc

pytestmark = pytest.mark.gpu


def test_pass_timers():
    rt = gi.RayTracer(0).setScene(pc.load_scene("test_scene"))
    w = h = 16
    reads = {"features": rt.last_features_ms, "denoise": rt.last_denoise_ms, "upsample": rt.last_upsample_ms}
    for name, read in reads.items():
        assert read() == 0.0, name                                   # before any call

    full = rt.run_features(w, h, 2)
    low = rt.run_features(w // 2, h // 2, 2)
    color = np.full((h // 2, w // 2, 3), 0.5)
    passes = {"features": lambda **kw: rt.run_features(w, h, kw.get("n", 2)),
              "denoise": lambda **kw: rt.denoise(color, low, **kw),
              "upsample": lambda **kw: rt.upsample(color, low, full, 2, **kw)}
    rejected = {"features": dict(n=0), "denoise": dict(iterations=99), "upsample": dict(sigma_normal=-1.0)}
    for name, read in reads.items():
        passes[name]()
        t = read()
        print(f"{name}: {t:.4f} ms")
        assert t > 0.0, name                                         # after a pass
        assert read() == t, name                                     # read again
        others = {k: r() for k, r in reads.items() if k != name}
        with pytest.raises(gi.GiError):
            passes[name](**rejected[name])
        assert read() == 0.0, name                                   # a rejected call did no work
        assert {k: r() for k, r in reads.items() if k != name} == others, name   # and every pass keeps its own time
