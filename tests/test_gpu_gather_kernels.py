"""The stream passes' gather kernels query by query (gi_debug_gather_pass): k_st_gather and k_st_gather_wave, the plain and the counting
instance of each, launched as the stream passes launch them, on synthetic photon clusters with chosen candidate counts and key patterns.
Every instance, with the queries in leaf order and in the caller's order, returns the caustic term of k_gather (samplePhotons) bit for bit
(same arithmetic, same order), the oracle's to rtol 1e-9, and the counting instances count the oracle's candidates."""
import os

import numpy as np
import pytest

import gi_raytracer_amd as gi
import parity_checks as pc
from gather_clusters import REQUIRED, TIES, build as _build     # the clusters and their queries (shared with test_gather_forms_cpu.py)

pytestmark = pytest.mark.gpu

KERNELS = ("gather", "gather_count", "wave", "wave_count")


def _rt(scene, ph, flat):
    old = os.environ.pop("GI_FLAT_CANDIDATES", None)
    try:
        if not flat:
            os.environ["GI_FLAT_CANDIDATES"] = "0"     # read when the context is created: k_st_gather walks the leaf's range list
        rt = gi.RayTracer(0).setScene(scene)
    finally:
        os.environ.pop("GI_FLAT_CANDIDATES", None)
        if old is not None:
            os.environ["GI_FLAT_CANDIDATES"] = old
    scene.build_photon_map(ph)
    rt.upload_photon_map()
    return rt


@pytest.fixture(scope="module")
def case():
    scene, ph, q, placed, cl = _build()
    o = pc.oracle_for(scene)
    o.set_photons(ph).build_photon_map()
    ref, nco = o.gather(q)
    rt = _rt(scene, ph, True)
    base, nc = rt.samplePhotons(q)                   # k_gather: gather_in_leaf per lane
    assert np.array_equal(nc, nco)
    return {"scene": scene, "ph": ph, "q": q, "placed": placed, "cl": cl, "ref": ref, "nco": nco, "base": base, "rt": rt}


@pytest.fixture(scope="module")
def rt_range_walk(case):
    return _rt(case["scene"], case["ph"], False)


SUBSETS = ("all", 1, 63, 65)


def _subset(case, which):
    n = len(case["q"]) if which == "all" else which
    return np.arange(n)


def _check_pass(case, rt, kernel, sort, which):
    idx = _subset(case, which)
    q, ref, nco, base = case["q"][idx], case["ref"][idx], case["nco"][idx], case["base"][idx]
    res, keys, order, cnt = rt.gather_pass(q, kernel, sort=sort)
    assert np.array_equal(np.sort(order), np.arange(len(q)))
    if sort:
        assert (np.diff(keys.astype(np.int64)) >= 0).all()
    # bit for bit the caustic term of k_gather, and the oracle's to rtol 1e-9 (summation order differs: leaf order vs distance order)
    assert np.array_equal(res.view(np.uint64), base.view(np.uint64)), (kernel, sort, which, np.argwhere(res != base)[:5])
    assert np.array_equal(res == 0, ref == 0)
    np.testing.assert_allclose(res, ref, rtol=1e-9, atol=1e-300)
    if kernel.endswith("_count"):
        assert cnt == (len(q), int(nco.sum()))
    return keys, order


def _waves(keys, n):
    return [keys[w:min(w + 64, n)] for w in range(0, n, 64)]


def test_clusters_reach_the_candidate_counts_and_key_patterns(case):
    q, nco, cl, placed = case["q"], case["nco"], case["cl"], case["placed"]
    reached = set()
    for j, (n, p, c) in enumerate(placed):
        assert (nco[cl == j] == n).all(), (n, p, np.unique(nco[cl == j]))
        reached.add(n)
        if p in TIES and n > 32:                      # the query at the centre: float keys tie across rank 32 (the exact pass runs)
            ph = case["ph"][:, :3]
            near = np.abs(ph - c).max(1) < 1e-5
            d = ph[near] - c
            key = np.sort((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).astype(np.float32))
            assert len(key) == n and key[31] == key[32], (n, p)
    assert REQUIRED <= reached and max(reached) > 1000
    assert len(case["q"]) > 4 * 256 and len(case["q"]) % 64 != 0
    assert (nco[cl < 0] == 0).sum() >= 6            # outside the map, in a leaf without candidates


@pytest.mark.parametrize("which", SUBSETS)
@pytest.mark.parametrize("sort", [True, False])
@pytest.mark.parametrize("kernel", KERNELS)
def test_gather_kernels_match_k_gather_and_oracle(case, kernel, sort, which):
    keys, order = _check_pass(case, case["rt"], kernel, sort, which)
    if which != "all":
        return
    n = len(keys)
    if sort:
        # at least one wave of 64 sorted queries of ONE leaf with candidates: the cooperative path (LDS staging, ksel_tau)
        nothing = keys.max()
        assert any(len(w) == 64 and (w == w[0]).all() and w[0] != nothing for w in _waves(keys, n))
    else:
        # every cluster's run is a wave of one leaf; the queries behind the runs give waves that straddle leaves (per-lane heap)
        runs = _waves(keys, n)[:len(case["placed"])]
        assert all((w == w[0]).all() for w in runs)
        assert any(len(np.unique(w)) > 1 for w in _waves(keys, n)[len(runs):])


@pytest.mark.parametrize("which", SUBSETS)
@pytest.mark.parametrize("sort", [True, False])
@pytest.mark.parametrize("kernel", ["gather", "gather_count"])
def test_range_walk_staging_matches(case, rt_range_walk, kernel, sort, which):
    """GI_FLAT_CANDIDATES=0: k_st_gather finds a leaf's k-th candidate through its range list; same numbers bit for bit."""
    _check_pass(case, rt_range_walk, kernel, sort, which)


def test_wave_kernel_needs_flat_candidates(case, rt_range_walk):
    with pytest.raises(gi.GiError, match=r"\(-4\)"):
        rt_range_walk.gather_pass(case["q"][:64], "wave")
