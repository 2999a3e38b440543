"""What a progressive session costs on the benchmark frame (caustics, 1920 x 1080, 200 k photon indices, 64 spp), in device time from gi_last_render_ms:

  (a) the one-shot gi_render_device, REPEATS times, with the spread between them;
  (b) a session that takes all 64 samples in one step -- the launches of (a) less k_pix_init, which gi_progressive_begin ran before the step;
  (c) sessions in steps of 1, 4 and 16 samples: sum of the step times and time per step.

Pass marks (the exit status is 1 and a FAIL line is printed when one is missed; the JSON is written either way): the median of (b) lies within
min .. max of (a) on this build (two-sided: a session faster than every frame fails it too); with --parent-tree, the median of this build's (a)
over all its processes is not above the maximum of the other build's, i.e. the frame costs nothing beyond that spread (one-sided).  (c) has none.

    python tools/progressive_probe.py [--out profiles/NAME.json] [--parent-tree DIR] [--repeats 5]

--parent-tree DIR: a directory that holds another build's gi_raytracer_amd package (for instance the parent commit's, built next to this tree);
its one-shot frame is timed in processes of its own, alternating with this build's, so that the two (a) figures come from the same minutes on the
same device.  One process uses the GPU at a time; every process warms up before it times; the builds are named by the hash of their library."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, PHOTONS = 1920, 1080, 64, 200000


def child(tree, mode, repeats):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, tree)
    import torch
    import gi_raytracer_amd as gi
    import parity_checks as pc
    rt = gi.RayTracer(0).setScene(pc.load_scene("caustics"))
    rt.tracePhotonsOnDevice(PHOTONS)                                       # as bench.py builds the map
    p = rt.params(W, H, min_samples=SPP, max_samples=SPP)
    buf = torch.empty((H, W, 3), dtype=torch.float32, device="cuda:0")
    spp = torch.zeros((H, W), dtype=torch.int32, device="cuda:0")
    res = {"library": os.path.relpath(gi.LIB_PATH, tree), "library_sha256_16": hashlib.sha256(open(gi.LIB_PATH, "rb").read()).hexdigest()[:16], "device": torch.cuda.get_device_name(0)}

    def oneshot():
        rt.run_device(p, buf.data_ptr(), spp_ptr=spp.data_ptr())
        torch.cuda.synchronize()
        return rt.last_render_ms()

    for _ in range(2):                                                     # warm-up: code objects, the pool and the queues at their final size
        oneshot()
    res["oneshot_ms"] = [oneshot()[0] for _ in range(repeats)]
    res["oneshot_launches"] = rt.last_render_ms()[1]
    if mode == "full":
        ref = buf.clone()

        def session(step):
            times, launches = [], 0
            with rt.progressive(W, H, min_samples=SPP, max_samples=SPP) as s:
                while s.sample_end < SPP:
                    s.step_device(step, buf.data_ptr(), spp_ptr=spp.data_ptr())
                    torch.cuda.synchronize()
                    ms, n = rt.last_render_ms()
                    times.append(ms)
                    launches += n
            assert torch.equal(buf, ref) and int(spp.min()) == SPP == int(spp.max()), "a frame built in steps must have the bits of the one-shot frame"
            return times, launches

        session(SPP)                                                       # warm-up of the session's own buffer
        one = [session(SPP) for _ in range(repeats)]
        res["session_one_step_ms"] = [t[0][0] for t in one]
        res["session_one_step_launches"] = one[-1][1]
        res["oneshot_ms_after_sessions"] = [oneshot()[0] for _ in range(repeats)]   # (a) again, after (b): drift of the device within the process
        res["steps"] = {}
        for step in (1, 4, 16):
            times, launches = session(step)
            res["steps"][str(step)] = {"n_steps": len(times), "sum_ms": sum(times), "ms_per_step_mean": statistics.mean(times), "ms_per_step_min": min(times),
                                       "ms_per_step_max": max(times), "launches": launches, "step_ms": times}
    print("PROBE " + json.dumps(res), flush=True)


def within(v, ref):
    """The mark of (b): the median of v lies within the run-to-run spread min .. max of ref.  Two-sided: a median below min(ref) fails too."""
    return min(ref) <= statistics.median(v) <= max(ref)


def not_above(v, ref):
    """The mark against the other build: the median of v costs nothing beyond the spread of ref, i.e. it is not above max(ref); faster is no cost."""
    return statistics.median(v) <= max(ref)


def spread(v):
    return {"n": len(v), "min": min(v), "max": max(v), "median": statistics.median(v), "mean": statistics.mean(v), "spread_max_minus_min": max(v) - min(v)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats: at least 5")
    if a.child:
        return child(a.tree, a.child, a.repeats)

    def run(tree, mode):                                                   # a fresh process per measurement, one at a time
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--tree", tree, "--repeats", str(a.repeats)], capture_output=True, text=True, timeout=900)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("PROBE ")]
        if r.returncode != 0 or not lines:
            raise SystemExit(f"probe process failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        return json.loads(lines[-1][6:])

    plan = [("this", ROOT, "full")]
    if a.parent_tree:
        plan = [("parent", a.parent_tree, "oneshot"), ("this", ROOT, "full"), ("parent", a.parent_tree, "oneshot"), ("this", ROOT, "oneshot")]
    runs = []
    for name, tree, mode in plan:
        r = run(tree, mode)
        r["build"] = name
        runs.append(r)
        print(name, mode, "one-shot ms", [round(v, 2) for v in r["oneshot_ms"]], flush=True)
    full = next(r for r in runs if "steps" in r)
    a_ms, b_ms = full["oneshot_ms"] + full["oneshot_ms_after_sessions"], full["session_one_step_ms"]
    out = {"workload": f"scenes/caustics {W}x{H} {SPP} spp, {PHOTONS} photon indices; device time of gi_last_render_ms (HIP events on the launch stream)",
           "method": "one process on the device at a time; 2 warm-up frames per process; (b) and (c) verified bit-equal to (a) in the same process",
           "a_oneshot": spread(a_ms), "b_session_one_step": spread(b_ms),
           "b_minus_a_median_ms": statistics.median(b_ms) - statistics.median(a_ms),
           "b_within_spread_of_a": within(b_ms, a_ms),
           "launches": {"oneshot": full["oneshot_launches"], "session_one_step": full["session_one_step_launches"]},
           "c_steps": {k: {kk: vv for kk, vv in v.items() if kk != "step_ms"} for k, v in full["steps"].items()},
           "runs": runs}
    if a.parent_tree:
        this_all = [v for r in runs if r["build"] == "this" for v in r["oneshot_ms"]]
        parent_all = [v for r in runs if r["build"] == "parent" for v in r["oneshot_ms"]]
        out["a_this_build_all_processes"] = spread(this_all)
        out["a_parent_build_all_processes"] = spread(parent_all)
        out["this_minus_parent_median_ms"] = statistics.median(this_all) - statistics.median(parent_all)
        out["a_this_not_above_spread_of_parent"] = not_above(this_all, parent_all)
    failed = []
    if not out["b_within_spread_of_a"]:
        failed.append(f"(b) median {statistics.median(b_ms):.3f} ms outside the spread of (a) {min(a_ms):.3f} .. {max(a_ms):.3f} ms")
    if a.parent_tree and not out["a_this_not_above_spread_of_parent"]:
        failed.append(f"(a) median {statistics.median(this_all):.3f} ms above the spread of the other build's (a) {min(parent_all):.3f} .. {max(parent_all):.3f} ms")
    out["failed"] = failed
    print(json.dumps({k: v for k, v in out.items() if k != "runs"}, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    for msg in failed:
        print("FAIL " + msg, flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
