"""What the occlusion pass costs, on the benchmark frame (caustics, 1920 x 1080):

  gi_last_occlusion_ms at n samples x dirs segments (warm-up, then the median of --reps calls), and per segment;
  gi_last_features_ms at n samples of the same frame, the first-hit half of the pass on its own;
  k_st_shadow's time per segment in a frame of the beauty pass: gi_last_kernel_ms[8] of an uncounted frame over gi_get_stream_counters[13]
  (shadow segments) of a counted frame of the same parameters.

    python tools/occlusion_probe.py [--scene caustics] [--width 1920 --height 1080] [--n 16 --dirs 16] [--spp 64] [--photons 200000] [--reps 5] [--out FILE.json]

Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gi_raytracer_amd as gi  # noqa: E402


def median_ms(run, read, reps):
    run()                                          # warm-up: code load, LDS attribute, clocks
    out = []
    for _ in range(reps):
        run()
        out.append(read())
    return statistics.median(out), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="caustics")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--dirs", type=int, default=16)
    ap.add_argument("--radius", type=float, default=0.0)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--photons", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import ctypes as C
    import numpy as np
    hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")      # the HIP runtime the library itself uses

    def device(nbytes):
        d = C.c_void_p()
        assert hip.hipMalloc(C.byref(d), C.c_size_t(nbytes)) == 0
        return d

    def download(d, shape):
        a = np.zeros(shape, np.float32)
        assert hip.hipDeviceSynchronize() == 0 and hip.hipMemcpy(a.ctypes.data_as(C.c_void_p), d, C.c_size_t(a.nbytes), 2) == 0
        return a
    scn = {"caustics": "scenes/caustics/caustics.scn", "cornell": "scenes/cornell/test.scn", "teapot": "scenes/cornell/teapot.scn"}[a.scene]
    scene = gi.Scene.load(os.path.join(ROOT, scn)).rebuild()
    rt = gi.RayTracer(0).setScene(scene)
    w, h = a.width, a.height
    p = rt.params(w, h, min_samples=a.spp, max_samples=a.spp)
    op = rt.occlusion_params(n=a.n, dirs=a.dirs, radius=a.radius, width=w, height=h)
    ao, feat, frame = device(h * w * 4 * 4), device(h * w * 8 * 4), device(h * w * 3 * 4)
    ao_ms, ao_all = median_ms(lambda: rt.run_occlusion_device(p, op, ao.value), rt.last_occlusion_ms, a.reps)
    ft_ms, ft_all = median_ms(lambda: rt.run_features_device(p, a.n, feat.value), rt.last_features_ms, a.reps)
    o = download(ao, (h, w, 4))
    cov = float(download(feat, (h, w, 8))[:, :, 7].mean(dtype=np.float64))
    segments = cov * w * h * a.n * a.dirs          # segments the pass walked: hits x dirs
    if a.photons > 0:
        rt.tracePhotonsOnDevice(a.photons)
    sh_ms, sh_all = median_ms(lambda: rt.run_device(p, frame.value), lambda: rt.last_kernel_ms()["shadow"], max(1, a.reps // 2))
    rt.set_counters("stream")
    rt.run_device(p, frame.value)
    assert hip.hipDeviceSynchronize() == 0
    sc = rt.stream_counters()
    rt.set_counters(0)
    sh_seg = sc["shadow_rays"]
    res = {"scene": a.scene, "frame": [w, h], "n": a.n, "dirs": a.dirs, "radius": a.radius, "occlusion_ms": ao_ms, "occlusion_ms_all": ao_all,
           "features_ms": ft_ms, "features_ms_all": ft_all, "coverage": cov, "segments": segments,
           "occlusion_ns_per_segment": 1e6 * ao_ms / max(segments, 1), "segments_only_ns_per_segment": 1e6 * (ao_ms - ft_ms) / max(segments, 1),
           "mean_openness": float(o[:, :, 0].mean()),
           "beauty_spp": a.spp, "k_st_shadow_ms": sh_ms, "k_st_shadow_ms_all": sh_all, "k_st_shadow_segments": sh_seg,
           "k_st_shadow_ns_per_segment": 1e6 * sh_ms / max(sh_seg, 1),
           "shadow_walk_per_segment": {k: sc[k] / max(sh_seg, 1) for k in ("shadow_records", "shadow_leaves", "shadow_tris")}}
    res["ratio_per_segment"] = res["segments_only_ns_per_segment"] / res["k_st_shadow_ns_per_segment"] if sh_seg else None
    for d in (ao, feat, frame):
        hip.hipFree(d)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
