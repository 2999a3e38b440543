"""What a lightmap atlas costs, against the only way a caller had before there was one:

  lightmap  gi_lightmap_host of a --size x --size atlas of the caustics scene's floor material (material 0, the scene's own texture coordinates as the
            chart: chart_of_material) at --samples rays per covered texel, with the golden photon set: the three stage times of gi_last_lightmap_ms
            (raster + rank, bake, scatter + dilate; HIP events), the device time of the whole pass and the host's wall time around the call;
  baseline  the numpy statement for the texel table (tests/lightmap_expect.py: every texel against every chart row), RayTracer.bake_texels on it,
            numpy scatter and dilation: wall time around the three, and of each.

One small warm-up of each (code load, workspaces), then one timed run of each.  max_abs_difference between the two atlases must be 0.0.

    python tools/lightmap_probe.py [--size 1024] [--samples 64] [--dilate 2] [--out FILE.json]

Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gi_raytracer_amd as gi  # noqa: E402
import lightmap_expect as le  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--dilate", type=int, default=2)
    ap.add_argument("--material", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    scene = gi.Scene.load(os.path.join(ROOT, "scenes/caustics/caustics.scn")).rebuild()
    rt = gi.RayTracer(0).setScene(scene)          # raises without a GPU: nothing here is measured on a CPU
    photons = np.load(os.path.join(ROOT, "tests", "golden", "scene_caustics.npz"))["photons"]
    scene.build_photon_map(photons)
    rt.upload_photon_map()
    tables = scene.tables()
    ent, uv = gi.chart_of_material(scene, a.material)

    def lightmap(size, ns):
        t0 = time.perf_counter()
        atlas, _, n = rt.bake_lightmap(ent, uv, size, size, ns, dilate=a.dilate, want_owner=True)
        wall = 1e3 * (time.perf_counter() - t0)
        ms, stages = rt.last_lightmap_ms()
        return atlas, n, wall, ms, stages

    def baseline(size, ns):
        t0 = time.perf_counter()
        _, P, N, texel = le.texel_table(tables, ent, uv, size, size)
        t1 = time.perf_counter()
        rows = rt.bake_texels(P, N, ns)
        t2 = time.perf_counter()
        atlas = le.dilate(*le.scatter(rows, texel, size, size), a.dilate)[0]
        t3 = time.perf_counter()
        return atlas, len(texel), {"wall_ms": 1e3 * (t3 - t0), "texels_numpy_ms": 1e3 * (t1 - t0), "bake_texels_ms": 1e3 * (t2 - t1), "scatter_dilate_numpy_ms": 1e3 * (t3 - t2)}

    lightmap(64, 4)
    baseline(64, 4)
    atlas, n, wall, ms, stages = lightmap(a.size, a.samples)
    ref, n_ref, base = baseline(a.size, a.samples)
    res = {"scene": "caustics", "photons": int(len(photons)), "material": a.material, "chart_rows": int(len(ent)), "width": a.size, "height": a.size,
           "samples": a.samples, "dilate": a.dilate, "n_covered": int(n), "paths": int(n) * a.samples,
           "stage_ms": {k: round(v, 4) for k, v in stages.items()}, "device_ms": ms, "wall_ms": wall, "baseline": base,
           "baseline_over_lightmap_wall": base["wall_ms"] / wall, "n_covered_baseline": int(n_ref),
           "max_abs_difference": float(np.abs(atlas - ref).max()), "max_abs_value": float(np.abs(ref).max())}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    assert res["max_abs_difference"] == 0.0 and n == n_ref, "the atlas is not the statement's"


if __name__ == "__main__":
    main()
