"""The probe of the next ray in the deferred shade kernel (gi_walk.h: ray_leaves_scene), on the CPU.

ray_leaves_scene is GI_HD: tests/cpp/early_miss.cpp compiles it for the host next to the host emulator's trace, with the emulator's flags.  The
probe is a SUFFICIENT condition for a miss: whenever it says "leaves", trace() must find no hit -- over the wide records (the walk the streaming
kernels run) and over the per-node links (the reference's order of box tests).  An implication, not a tolerance: zero exceptions, on random
rays, axis-parallel ones, origins on octree planes, +-0 direction components (parity_checks.adversarial_rays) and on the next rays of real
paths (every vertex of a small frame that continues), for 1, 2, 4 and 64 turns."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gi_raytracer_amd as gi

import host_build
import parity_checks as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TURNS = (1, 2, 4, 64)
N_ADVERSARIAL, N_NEXT = 36000, 30000     # at least 50 000 rays per scene


@pytest.fixture(scope="module")
def em(tmp_path_factory):
    lib = tmp_path_factory.mktemp("early_miss") / "libearly_miss.so"
    subprocess.run([os.environ.get("CXX", "g++")] + host_build.flags() + ["-shared", os.path.join(ROOT, "tests", "cpp", "early_miss.cpp"), "-o", str(lib)], check=True)
    L = C.CDLL(str(lib))
    vp = C.c_void_p
    L.emul_create.restype = vp
    L.emul_destroy.argtypes = [vp]
    L.emul_error.argtypes = [vp]
    L.emul_error.restype = C.c_char_p
    L.emul_upload_scene.argtypes = [vp, C.POINTER(gi.SceneDesc)]
    L.em_probe.argtypes = [vp, C.c_int, gi._dp, C.c_int, gi._ip, gi._ip, gi._ip]
    L.em_next_rays.argtypes = [vp, C.POINTER(gi.RenderParams), C.c_int, gi._dp]
    return L


class Probe:
    def __init__(self, L, scene):
        self.L, self.scene = L, scene
        self.h = C.c_void_p(L.emul_create())
        d = scene.desc()
        rc = L.emul_upload_scene(self.h, C.byref(d))
        assert rc == 0, L.emul_error(self.h).decode()

    def close(self):
        self.L.emul_destroy(self.h)

    def probe(self, rays, turns):
        rays = gi._f64(rays).reshape(-1, 6)
        n = len(rays)
        leaves, hw, hn = (np.zeros(n, np.int32) for _ in range(3))
        assert self.L.em_probe(self.h, n, gi._p(rays), turns, gi._p(leaves, gi._ip), gi._p(hw, gi._ip), gi._p(hn, gi._ip)) == 0, "no wide records"
        return leaves.astype(bool), hw.astype(bool), hn.astype(bool)

    def next_rays(self, w, h, spp, cap):
        rt = gi.RayTracer.__new__(gi.RayTracer)       # params() only: the camera and sampling settings of the scene, no device
        st = self.scene.settings
        rt.photons, rt.photon_depth = st.photons, st.photon_depth
        rt.min_samples, rt.max_samples, rt.noise_thresh = st.min_samples, st.max_samples, st.noise_thresh
        rt.cam_pos, rt.cam_up, rt.cam_forward = list(st.cam_pos), list(st.cam_up), list(st.cam_forward)
        rt.sensor_diag, rt.focal_dist = st.sensor_diag, st.focal_dist
        rt.seed = gi.DEFAULT_SEED
        p = rt.params(w, h, min_samples=spp, max_samples=spp)
        out = np.zeros((cap, 6))
        n = self.L.em_next_rays(self.h, C.byref(p), cap, gi._p(out))
        assert n >= 0, self.L.emul_error(self.h).decode()
        return out[:n].copy()


@pytest.mark.parametrize("name", ["caustics", "cornell", "teapot"])
def test_leaves_implies_no_hit(em, name):
    scene = pc.load_scene(name)
    P = Probe(em, scene)
    try:
        adv = pc.adversarial_rays(scene, n=N_ADVERSARIAL, seed=11)
        nxt = P.next_rays(96, 54, 8, N_NEXT)
        assert len(nxt) >= 14000, len(nxt)            # the frame gave the rays it was sized for
        assert len(adv) + len(nxt) >= 50000
        prev = None
        for turns in TURNS:
            shares = []
            for what, rays in (("adversarial", adv), ("next rays of real paths", nxt)):
                leaves, hit_wide, hit_nodes = P.probe(rays, turns)
                assert np.array_equal(hit_wide, hit_nodes)
                bad = np.nonzero(leaves & (hit_wide | hit_nodes))[0]
                assert len(bad) == 0, (name, what, turns, len(bad), rays[bad[:3]])
                miss = ~hit_wide
                shares.append((what, len(rays), int(miss.sum()), int(leaves.sum())))
                print(f"{name}: {turns:2d} turns, {what}: {len(rays)} rays, {miss.sum()} miss, probe decides {leaves.sum()} "
                      f"({100.0 * leaves.sum() / max(1, len(rays)):.1f} % of the rays, {100.0 * leaves.sum() / max(1, miss.sum()):.1f} % of the misses)")
            decided = np.concatenate([P.probe(r, turns)[0] for r in (adv, nxt)])
            if prev is not None:
                assert not (prev & ~decided).any()    # more turns never take a decision back
            prev = decided
        if name == "caustics":
            # an open scene: most reflected rays leave it, and the probe has to see a real share of them (a probe that always says "goes on" passes
            # the implication above and must fail here)
            leaves, hit_wide, _ = P.probe(nxt, 4)
            print(f"caustics: the probe decides {100.0 * leaves.mean():.1f} % of the next rays of real paths at 4 turns ({100.0 * (~hit_wide).mean():.1f} % miss)")
            assert leaves.sum() > 0
            assert leaves.mean() > 0.25
    finally:
        P.close()
