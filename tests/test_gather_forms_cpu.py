"""The CPU build of gather() (tests/host_emul: the per-lane form, gather_in_leaf, with the selection steps and the exact pass g_exact that the
wave forms of the GPU share with it, gi_gather.h) on the queries of tests/test_gpu_gather_kernels.py: synthetic photon clusters with candidate
counts around every staging boundary and the key patterns random, shell, tie, dup and dupgroup, against the oracle."""
import numpy as np
import pytest

import emul_lib as el
import gather_clusters as gc
import parity_checks as pc


@pytest.fixture(scope="module")
def case():
    scene, ph, q, placed, cl = gc.build()
    o = pc.oracle_for(scene)
    o.set_photons(ph).build_photon_map()
    ref, nco = o.gather(q)
    rt = el.EmulRayTracer().setScene(scene)
    scene.build_photon_map(ph)
    rt.upload_photon_map()
    res, nc = rt.samplePhotons(q)
    return {"ph": ph, "q": q, "placed": placed, "cl": cl, "ref": ref, "nco": nco, "res": res, "nc": nc}


def test_candidate_counts_equal_the_oracles(case):
    assert np.array_equal(case["nc"], case["nco"])
    reached = set()
    for j, (n, p, c) in enumerate(case["placed"]):
        assert (case["nc"][case["cl"] == j] == n).all(), (n, p)
        reached.add(n)
    assert gc.REQUIRED <= reached and max(reached) > 1000
    assert (case["nc"][case["cl"] < 0] == 0).sum() >= 6            # outside the map, in a leaf without candidates


def test_tie_patterns_tie_across_rank_32(case):
    """The query at the centre of every such cluster has key[31] == key[32] in float: g_end declines and the exact pass runs."""
    n_ties = 0
    for n, p, c in case["placed"]:
        if p in gc.TIES and n > 32:
            key = gc.float_keys(case["ph"], c)
            assert len(key) == n and key[31] == key[32], (n, p)
            n_ties += 1
    assert n_ties == 4 * sum(1 for n in gc.BIG if n > 32)


def test_gather_matches_the_oracle(case):
    res, ref = case["res"], case["ref"]
    assert np.array_equal(res == 0, ref == 0)
    # rtol 1e-9: the summation order differs (leaf order here, distance order in the oracle)
    np.testing.assert_allclose(res, ref, rtol=1e-9, atol=1e-300)
    # and the queries at the centres of the tie clusters are among the non-zero ones: the exact pass returned a value
    for j, (n, p, c) in enumerate(case["placed"]):
        if p in gc.TIES and n > 32:
            assert (res[case["cl"] == j] != 0).any(), (n, p)
