"""k_st_gather on waves that hold the queries of several photon-map leaves (gi_debug_gather_pass): a wave takes its leaves one run after the other
through the cooperative path, up to GI_GATHER_RUNS of them, and falls back to the per-lane heap walk beyond that.  The caustics scene with its
20 000 photons plus two small clusters (a float-tie group across rank 32, copies of one photon); queries sit on the photons, jittered, so the
leaves a wave of 64 sorted queries spans are chosen by the test.  Every case returns the caustic term of k_gather (samplePhotons) on the same
positions and directions bit for bit, from the plain and from the counting instance; the latter counts k_gather's candidates."""
import os
import re

import numpy as np
import pytest

import gi_raytracer_amd as gi
import parity_checks as pc
from gather_clusters import R, cluster, float_keys
from test_gpu_gather_kernels import _waves

pytestmark = pytest.mark.gpu

KERNELS = ("gather", "gather_count")
LEAVES = (2, 3, 4, 5, 8, 9, 16, 17)         # leaves in one wave: the values the limit was swept over and one more than each


def _limit():
    with open(os.path.join(os.path.dirname(gi.__file__), "csrc", "gi_gather.inc")) as f:
        return int(re.search(r"^#define GI_GATHER_RUNS (\d+)", f.read(), re.M).group(1))


@pytest.fixture(scope="module")
def pool():
    """The query pool Q (position, direction), k_gather's answer to each, its candidate count, leaf and sort key.  Computed once, read only."""
    scene = pc.load_scene("caustics")
    rt = gi.RayTracer(0).setScene(scene)
    ph, _ = rt.tracePhotons(20000)
    rs = np.random.RandomState(5)
    box = scene.photon_tables()["node_bbox"][0]
    lo, ext = box[:3], box[3:] - box[:3]
    # two clusters beside photons of the map: 48 photons with a float-tie group across rank 32, 40 with five copies of one photon at ranks 29 .. 33
    c_tie, c_dup = ph[1000, :3] + 64 * R, ph[7000, :3] + 64 * R
    ph = np.concatenate([ph, cluster("tie", 48, c_tie, rs), cluster("dupgroup", 40, c_dup, rs)])
    scene.build_photon_map(ph)
    rt.upload_photon_map()
    n_ph = len(ph)
    on = ph[:, :3] + ext * 1e-9 * rs.uniform(-1, 1, (n_ph, 3))          # on the photons, jittered
    exact = ph[rs.choice(20000, 64, replace=False), :3]                 # on a photon: distance 0
    rnd = lo + ext * (rs.rand(4000, 3) * 1.2 - 0.1)                     # anywhere: outside the map, leaves without candidates
    pos = np.concatenate([on, exact, c_tie[None], c_dup[None], rnd])
    Q = np.concatenate([pos, rs.randn(len(pos), 3)], 1)
    base, nc = rt.samplePhotons(Q)                                       # k_gather: gather_in_leaf per lane
    _, leaf = rt.find_leaves(pos)
    res, keys, _, _ = rt.gather_pass(Q, "gather", sort=False)           # keys in the caller's order: the leaf rank of every query
    assert np.array_equal(res.view(np.uint64), base.view(np.uint64))
    nothing = int(keys.max())
    assert ((keys == nothing) == (nc == 0)).all() and (nc == 0).any() and (leaf[nc == 0] < 0).any()
    by_leaf = {}
    for i in np.flatnonzero(nc > 0):
        by_leaf.setdefault(int(leaf[i]), []).append(int(i))
    i_exact = n_ph + np.arange(64)
    return {"rt": rt, "ph": ph, "Q": Q, "base": base, "nc": nc, "leaf": leaf, "keys": keys, "by_leaf": by_leaf, "nothing": nothing,
            "i_exact": i_exact[nc[i_exact] > 0], "i_tie": n_ph + 64, "i_dup": n_ph + 65, "c_tie": c_tie, "c_dup": c_dup,
            "i_none": np.concatenate([np.flatnonzero((nc == 0) & (leaf < 0))[:6], np.flatnonzero((nc == 0) & (leaf >= 0))[:4]])}


def _of_leaf(pool, leaf, n):
    ids = pool["by_leaf"][leaf]
    return [ids[k % len(ids)] for k in range(n)]                        # (a leaf with fewer positions than n gives some of them twice)


def _leaves(pool, k, want=lambda nc: True, seed=0):
    """k leaves with candidates, in rank order"""
    nc, keys = pool["nc"], pool["keys"]
    ok = sorted(lf for lf, ids in pool["by_leaf"].items() if want(nc[ids[0]]))
    pick = [ok[j] for j in np.random.RandomState(100 * seed + k).choice(len(ok), k, replace=False)]
    return sorted(pick, key=lambda lf: keys[pool["by_leaf"][lf][0]])


def _check(pool, idx, sort=True, runs_per_wave=None):
    idx = np.asarray(idx)
    q, base, nc = pool["Q"][idx], pool["base"][idx], pool["nc"][idx]
    keys = None
    for kernel in KERNELS:
        res, keys, order, cnt = pool["rt"].gather_pass(q, kernel, sort=sort)
        assert np.array_equal(np.sort(order), np.arange(len(q)))
        assert np.array_equal(res.view(np.uint64), base.view(np.uint64)), (kernel, np.argwhere(res != base)[:5])
        if kernel.endswith("_count"):
            assert cnt == (len(q), int(nc.sum()))                       # a query per valid lane, the candidates of its own leaf per query
    if runs_per_wave is not None:                                       # the waves hold the leaves the case is about
        got = [len(np.unique(w[w != pool["nothing"]])) for w in _waves(keys, len(keys))]
        assert got == list(runs_per_wave), got
    return keys


def _run_lengths(k):
    """64 lanes in k runs of unequal length, one of them a single lane: 64 - k (k - 1) / 2, 1, 2, ..., k - 1"""
    rest = list(range(1, k))
    return [64 - sum(rest)] + rest


def test_the_swept_limits_and_the_built_one_are_covered():
    lim = _limit()
    assert lim >= 64 or (lim in LEAVES and lim + 1 in LEAVES)            # (d): exactly the limit, and one more


def test_one_leaf_is_the_uniform_wave(pool):
    (lf,) = _leaves(pool, 1, lambda nc: nc >= 64)
    _check(pool, _of_leaf(pool, lf, 64), runs_per_wave=[1])


@pytest.mark.parametrize("k", LEAVES)
def test_leaves_in_one_wave(pool, k):
    """(b), (d): k runs of unequal length, among them a run of one lane; k = limit takes the runs, k = limit + 1 the heaps"""
    lens = _run_lengths(k) if k <= 8 else [64 - 2 * (k - 1)] + [2] * (k - 3) + [1, 3]
    assert sum(lens) == 64 and 1 in lens and len(lens) == k
    idx = sum((_of_leaf(pool, lf, n) for lf, n in zip(_leaves(pool, k), lens)), [])
    _check(pool, idx, runs_per_wave=[k])


def test_64_leaves_take_the_heaps(pool):
    idx = [pool["by_leaf"][lf][0] for lf in _leaves(pool, 64)]
    _check(pool, idx, runs_per_wave=[64])


def test_last_wave_with_invalid_lanes(pool):
    """(e): n = 70: a wave of three leaves, then 6 queries of 2 leaves and 58 lanes without a query"""
    lv = _leaves(pool, 5)
    idx = sum((_of_leaf(pool, lf, n) for lf, n in zip(lv, (40, 23, 1, 2, 4))), [])
    _check(pool, idx, runs_per_wave=[3, 2])


@pytest.mark.parametrize("sort", [True, False])
def test_queries_with_nothing_to_gather_between_runs(pool, sort):
    """(f): outside the map or in a leaf without candidates (key n_pleaf); in the caller's order they stand between the runs"""
    lv = _leaves(pool, 3)
    none = [int(i) for i in pool["i_none"][[0, 1, -1, 2, -2]]]              # outside the map; the last ones in a leaf without candidates, if the map has one
    idx = _of_leaf(pool, lv[0], 20) + none[:3] + _of_leaf(pool, lv[1], 20) + none[3:] + _of_leaf(pool, lv[2], 19)
    assert len(idx) == 64
    _check(pool, idx, sort=sort, runs_per_wave=[3])
    _check(pool, none + _of_leaf(pool, lv[2], 3) + none, sort=sort, runs_per_wave=[1])
    _check(pool, none, sort=sort, runs_per_wave=[0])


def test_short_candidate_list_inside_a_wave_of_several_leaves(pool):
    """(g): fewer than 32 candidates: K = ncand, ksel_tau's short first group, from a run that is not the first"""
    short = [lf for lf, ids in pool["by_leaf"].items() if pool["nc"][ids[0]] < 32]
    if not short:
        pytest.skip("the map has no leaf with fewer than 32 candidates")
    key = lambda lf: pool["keys"][pool["by_leaf"][lf][0]]
    s = max(short, key=key)
    before = [lf for lf in _leaves(pool, 40) if key(lf) < key(s)][:2]
    assert len(before) == 2
    idx = _of_leaf(pool, before[0], 30) + _of_leaf(pool, before[1], 14) + _of_leaf(pool, s, 20)
    keys = _check(pool, idx, runs_per_wave=[3])
    assert keys[-1] == key(s)


def test_ties_and_distance_zero_from_a_later_run(pool):
    """(h): queries on a photon (distance 0, given several times) and at the centres of the tie clusters (float keys tied across rank 32: the exact
    pass) behind a run of another leaf, so that g_exact is reached from a run that is not the wave's first"""
    kt = float_keys(pool["ph"], pool["c_tie"])
    kd = float_keys(pool["ph"], pool["c_dup"])
    assert len(kt) >= 48 and kt[31] == kt[32] and len(kd) >= 40 and kd[31] == kd[32]
    keys = pool["keys"]
    special = [int(pool["i_tie"])] * 6 + [int(pool["i_dup"])] * 6 + [int(i) for i in pool["i_exact"][:4]] * 3
    assert pool["nc"][pool["i_tie"]] >= 48 and pool["nc"][pool["i_dup"]] >= 40 and len(pool["i_exact"]) >= 4
    first = min(pool["by_leaf"], key=lambda lf: keys[pool["by_leaf"][lf][0]])       # the leaf of the lowest rank: the wave's first run
    assert keys[pool["by_leaf"][first][0]] < keys[special].min()
    n_leaves = len(np.unique(keys[special]))
    idx = _of_leaf(pool, first, 64 - len(special)) + special
    _check(pool, idx, runs_per_wave=[1 + n_leaves])
    # and with the special leaves alone: the tie group in the first run, the copies behind it or the other way round
    _check(pool, special, runs_per_wave=[n_leaves])


def test_many_waves_of_few_queries_per_leaf(pool):
    """a late pass in small: 256 queries drawn over the whole map, a handful per leaf, sorted"""
    with_c = np.flatnonzero(pool["nc"] > 0)
    idx = np.random.RandomState(9).choice(with_c, 256, replace=False)
    _check(pool, idx)
    lv = _leaves(pool, 40)
    _check(pool, sum((_of_leaf(pool, lf, 6) for lf in lv), []) + [int(i) for i in pool["i_none"]])
