"""What the guided upsampler costs at the benchmark frame size (caustics, 1920 x 1080, 200 k photon indices, 64 spp, 64 feature samples; f32 colour,
f32 features, f32 out, device buffers), in device time from the context's HIP events, next to what it replaces and what it needs:

  per factor S in 2, 4:  the reduced-size frame (gi_last_render_ms), its feature pass (gi_last_features_ms) and the upsampler (gi_last_upsample_ms);
  once:                  the full-size frame, the full-size feature pass, and the denoiser on the full-size frame with 1 and 2 levels
                         (gi_last_denoise_ms; one level more = their difference, the pack pass is in both).

Every figure is the median of --repeats calls after a warm-up call; the upsampled frame of every factor is compared with a second call (same bytes).
Next to each upsampler time: the bytes it must move per full pixel, derived from the kernels (see bytes_per_pixel), and the fraction of the 6.29 TB/s
a copy reaches on this device that this comes to.  No pass marks: the JSON (--out) records what was measured.

    python tools/upsample_probe.py [--out profiles/NAME.json] [--repeats 5]

Each measurement runs in a process of its own under a time limit, one at a time; the first that fails ends the probe (exit status 1)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, FEATURE_SPP, PHOTONS = 1920, 1080, 64, 64, 200000
FACTORS = (2, 4)
COPY_TBPS = 6.29            # HBM bandwidth a float4 copy reaches on the MI355X (8.0 TB/s peak)
STEP_TIMEOUT = 240


def bytes_per_pixel(S):
    """Bytes per FULL pixel the two kernels must move with f32 buffers, each datum once.  k_dn_pack, per low pixel: reads 12 B colour + 32 B features,
    writes 24 B colour + 64 B guides (f64).  k_up_sample: reads those 88 B per low pixel (the halo of a tile comes again, from L2: not counted), the
    32 B guide record per full pixel, writes 12 B."""
    return {"pack": (12 + 32 + 24 + 64) / (S * S), "sample": 88 / (S * S) + 32 + 12}


def child(what, repeats):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import torch
    import gi_raytracer_amd as gi
    import parity_checks as pc
    rt = gi.RayTracer(0).setScene(pc.load_scene("caustics"))
    rt.tracePhotonsOnDevice(PHOTONS)                                       # as bench.py builds the map
    dev = "cuda:0"

    def frame(w, h):
        p = rt.params(w, h, min_samples=SPP, max_samples=SPP)
        color = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
        feat = torch.empty((h, w, 8), dtype=torch.float32, device=dev)

        def render():
            rt.run_device(p, color.data_ptr())
            torch.cuda.synchronize()
            return rt.last_render_ms()[0]

        def features():
            rt.run_features_device(p, FEATURE_SPP, feat.data_ptr())
            torch.cuda.synchronize()
            return rt.last_features_ms()

        return color, feat, render, features

    def timed(fn):
        fn()                                                               # warm-up: code objects, scratch at its final size
        v = [fn() for _ in range(repeats)]
        return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "ms": v}

    res = {"device": torch.cuda.get_device_name(0)}
    if what == "full":
        color, feat, render, features = frame(W, H)
        res["frame"] = timed(render)
        res["features"] = timed(features)
        out = torch.empty_like(color)
        for levels in (1, 2):
            dp = rt.denoise_params(W, H, iterations=levels)

            def denoise():
                rt.denoise_device(dp, color.data_ptr(), feat.data_ptr(), out.data_ptr())
                torch.cuda.synchronize()
                return rt.last_denoise_ms()
            res[f"denoise_{levels}_level"] = timed(denoise)
        res["denoise_one_more_level_ms"] = res["denoise_2_level"]["median_ms"] - res["denoise_1_level"]["median_ms"]
    else:
        S = int(what)
        wl, hl = gi.low_frame_size(W, H, S)
        low, low_feat, render, features = frame(wl, hl)
        res["low_size"] = [wl, hl]
        res["low_frame"] = timed(render)
        res["low_features"] = timed(features)
        _, feat, _, full_features = frame(W, H)
        full_features()
        out = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
        up = rt.upsample_params(W, H, S)

        def upsample():
            rt.upsample_device(up, low.data_ptr(), low_feat.data_ptr(), feat.data_ptr(), out.data_ptr())
            torch.cuda.synchronize()
            return rt.last_upsample_ms()
        res["upsample"] = timed(upsample)
        first = out.clone()
        upsample()
        assert torch.equal(first, out) and bool(torch.isfinite(out).all()), "two calls on the same buffers must give the same, finite frame"
        b = bytes_per_pixel(S)
        total = (b["pack"] + b["sample"]) * W * H
        res["bytes_per_full_pixel"] = dict(b, total=b["pack"] + b["sample"])
        res["bytes_total"] = total
        res["tb_per_s"] = total / (res["upsample"]["median_ms"] * 1e-3) / 1e12
        res["fraction_of_copy_bandwidth"] = res["tb_per_s"] / COPY_TBPS
    print("PROBE " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.repeats < 3:
        ap.error("--repeats: at least 3")
    if a.child:
        return child(a.child, a.repeats)
    out = {"workload": f"scenes/caustics {W}x{H} {SPP} spp, {FEATURE_SPP} feature samples, {PHOTONS} photon indices; f32 colour, features and output in device memory",
           "method": f"one process on the device at a time, each under a limit of {STEP_TIMEOUT} s; median of {a.repeats} calls after a warm-up call; device time from the context's HIP events",
           "copy_bandwidth_tb_per_s": COPY_TBPS}
    for what in ("full",) + tuple(str(S) for S in FACTORS):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, "--repeats", str(a.repeats)], capture_output=True, text=True, timeout=STEP_TIMEOUT)
        except subprocess.TimeoutExpired:
            print(f"FAIL step {what}: no result within {STEP_TIMEOUT} s; nothing further is started", flush=True)
            return 1
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("PROBE ")]
        if r.returncode != 0 or not lines:
            print(f"FAIL step {what} ({r.returncode}); nothing further is started\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", flush=True)
            return 1
        out["full_size" if what == "full" else f"factor_{what}"] = json.loads(lines[-1][6:])
    full = out["full_size"]
    for S in FACTORS:
        r = out[f"factor_{S}"]
        r["preview_ms"] = r["low_frame"]["median_ms"] + r["low_features"]["median_ms"] + full["features"]["median_ms"] + r["upsample"]["median_ms"]
        r["upsample_over_one_denoiser_level"] = r["upsample"]["median_ms"] / full["denoise_one_more_level_ms"]
        print(f"factor {S}: upsample {r['upsample']['median_ms']:.3f} ms ({r['bytes_per_full_pixel']['total']:.1f} B per full pixel, {r['tb_per_s']:.2f} TB/s, "
              f"{r['fraction_of_copy_bandwidth']:.2f} of a copy); low frame {r['low_frame']['median_ms']:.1f} ms + features {r['low_features']['median_ms']:.1f} + "
              f"{full['features']['median_ms']:.1f} ms = preview {r['preview_ms']:.1f} ms against the frame's {full['frame']['median_ms']:.1f} ms", flush=True)
    print(f"full size: frame {full['frame']['median_ms']:.1f} ms, features {full['features']['median_ms']:.1f} ms, denoiser 1 level {full['denoise_1_level']['median_ms']:.3f} ms, "
          f"one level more {full['denoise_one_more_level_ms']:.3f} ms", flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
