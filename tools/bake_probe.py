"""What a bake costs, against the path a caller had before there was one:

  bake      gi_bake_host of --probes light probes x --samples rays (GI_BAKE_SH9) on the caustics scene with the golden photon set: the device time
            (gi_last_bake_ms, HIP events around the pass) and the host's wall time around the call (upload of the points, the pass, the result back);
  baseline  gi_radiance on the very same rays (gi_bake_rays) -- one path per lane, rays up, a radiance per ray back -- plus the fold on the host
            (numpy, vectorised): wall time around the two.  Making the rays is NOT counted, though such a caller would have to make them too.

One warm-up of each, then --reps timed runs of each, alternating; medians and the run-to-run spread (min .. max).  The probes are the cell centres of
a regular grid in the octree's root box.

    python tools/bake_probe.py [--probes 4096] [--samples 256] [--reps 5] [--out FILE.json]

Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gi_raytracer_amd as gi  # noqa: E402


def host_fold_sh9(L, d, n_samples):
    """The SH9 fold of the header on the host, vectorised (the sum's order is numpy's: a caller after speed would not add one sample at a time)."""
    import numpy as np
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    Y = np.stack([np.full(x.shape, 0.28209479177387814), 0.4886025119029199 * y, 0.4886025119029199 * z, 0.4886025119029199 * x,
                  1.0925484305920792 * (x * y), 1.0925484305920792 * (y * z), 0.31539156525252005 * (3.0 * (z * z) - 1.0),
                  1.0925484305920792 * (x * z), 0.5462742152960396 * (x * x - y * y)], -1)
    return (np.einsum("nkj,nkc->njc", Y, L) * 12.566370614359172) / float(n_samples)


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--probes", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    scene = gi.Scene.load(os.path.join(ROOT, "scenes/caustics/caustics.scn")).rebuild()
    rt = gi.RayTracer(0).setScene(scene)          # raises without a GPU: nothing here is measured on a CPU
    photons = np.load(os.path.join(ROOT, "tests", "golden", "scene_caustics.npz"))["photons"]
    scene.build_photon_map(photons)
    rt.upload_photon_map()
    side = max(1, round(a.probes ** (1.0 / 3.0)))
    grid = gi.probe_grid(scene.tables()["node_bbox"][0], side, side, -(-a.probes // (side * side))).reshape(-1, 3)[:a.probes]
    n, ns = len(grid), a.samples
    rays, streams = rt.bake_rays(grid, None, ns)
    dirs = rays[:, 3:6].reshape(n, ns, 3)

    def bake():
        t0 = time.perf_counter()
        out = rt.bake_probes(grid, ns)
        return out, 1e3 * (time.perf_counter() - t0), rt.last_bake_ms()

    def baseline():
        t0 = time.perf_counter()
        L = rt.radiance(rays, streams)
        t1 = time.perf_counter()
        out = host_fold_sh9(L.reshape(n, ns, 3), dirs, ns)
        return out, 1e3 * (time.perf_counter() - t0), 1e3 * (t1 - t0)

    sh, _, _ = bake()                              # warm-up: code load, LDS attributes, workspaces, clocks
    ref, _, _ = baseline()
    bake_wall, bake_dev, base_wall, base_rad = [], [], [], []
    for _ in range(a.reps):                        # alternating: both see the same neighbours on the machine
        _, w, d = bake()
        bake_wall.append(w); bake_dev.append(d)
        _, w, r = baseline()
        base_wall.append(w); base_rad.append(r)
    res = {"scene": "caustics", "photons": int(len(photons)), "probes": n, "samples": ns, "paths": n * ns, "reps": a.reps,
           "bake_device_ms": spread(bake_dev), "bake_wall_ms": spread(bake_wall),
           "baseline_wall_ms": spread(base_wall), "baseline_radiance_call_ms": spread(base_rad),
           "baseline_over_bake_wall": statistics.median(base_wall) / statistics.median(bake_wall),
           "max_abs_difference": float(np.abs(sh - ref).max()), "max_abs_coefficient": float(np.abs(ref).max())}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
