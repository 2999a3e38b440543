"""CPU check of the selection networks behind pass 1 of k_st_gather (gi_gather.h, through gi_device.h: ksort, kmerge32, ksel_tau).

The GI_HD helpers are compiled for the host with the host emulator's flags (tests/host_emul/Makefile) and driven in the
kernel's order: chunks of 64 from the last to the first, groups of 32 from the last to the first, the short group sized to
ncand % 32.  tau must equal, bit for bit, the K-th smallest float key (K = min(32, ncand)) that numpy.partition finds."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import host_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHIM = r"""
#define GI_HD static inline
#define GI_HDM inline
#include "gi_raytracer_amd/csrc/gi_layout.h"
using namespace gi;
template <int N> static void sort_n(float* v) { float a[N]; for (int k = 0; k < N; k++) a[k] = v[k]; ksort<N>(a); for (int k = 0; k < N; k++) v[k] = a[k]; }
extern "C" void sel_sort(float* v, int n) { if (n == 8) sort_n<8>(v); else if (n == 16) sort_n<16>(v); else sort_n<32>(v); }
extern "C" void sel_merge32(float* v) { float a[32]; for (int k = 0; k < 32; k++) a[k] = v[k]; kmerge32(a); for (int k = 0; k < 32; k++) v[k] = a[k]; }
extern "C" float sel_tau(const float* keys, int ncand, int* staged)
{
    int c = 0, n_staged = 0;
    const float t = ksel_tau(ncand, [&](int c0, int m) { c = c0; staged[n_staged++] = c0; staged[n_staged++] = m; }, [&](int k) { return keys[c + k]; });
    staged[n_staged] = -1;
    return t;
}
"""


@pytest.fixture(scope="module")
def sel(tmp_path_factory):
    d = tmp_path_factory.mktemp("gather_select")
    src, lib = d / "sel.cpp", d / "libsel.so"
    src.write_text(SHIM)
    subprocess.run([os.environ.get("CXX", "g++")] + host_build.flags() + ["-I", ROOT, "-shared", str(src), "-o", str(lib)], check=True)
    h = ctypes.CDLL(str(lib))
    fp = ctypes.POINTER(ctypes.c_float)
    h.sel_sort.argtypes = [fp, ctypes.c_int]
    h.sel_merge32.argtypes = [fp]
    h.sel_tau.argtypes = [fp, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    h.sel_tau.restype = ctypes.c_float
    return h


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _tau(sel, keys):
    keys = np.ascontiguousarray(keys, dtype=np.float32)
    staged = np.zeros(2 * (len(keys) // 64 + 2) + 1, dtype=np.int32)
    t = sel.sel_tau(_fp(keys), len(keys), staged.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    return np.float32(t), staged[:np.argmax(staged < 0)].reshape(-1, 2)


def _expected(keys):
    """What the heap root of gather_in_leaf holds: the K-th smallest key; below 32 keys the largest finite one (0 if none)."""
    n = len(keys)
    if n < 32:
        fin = keys[np.isfinite(keys)]
        return np.float32(fin.max()) if len(fin) else np.float32(0.0)
    return np.partition(keys, 31)[31]


def _key_sets(n, rng):
    yield "random", rng.random(n, dtype=np.float32) * np.float32(1e-2)
    yield "all_equal", np.full(n, 3.0e-4, dtype=np.float32)
    yield "zeros", np.zeros(n, dtype=np.float32)
    few = np.array([1e-5, 2e-5, 3e-5], dtype=np.float32)                     # many ties everywhere
    yield "few_values", rng.choice(few, n).astype(np.float32)
    if n >= 32:                                                                 # a tie group exactly across rank 32
        k = np.sort(rng.random(n, dtype=np.float32))
        k[28:min(n, 36)] = k[28]
        yield "tie_at_32", rng.permutation(k)
        k = rng.random(n, dtype=np.float32)                                    # INFINITY among the keys (beyond rank 32)
        k[rng.choice(n, (n - 32) // 2, replace=False)] = np.inf
        yield "with_inf", k
    yield "sorted", np.sort(rng.random(n, dtype=np.float32))
    yield "reversed", np.sort(rng.random(n, dtype=np.float32))[::-1].copy()


@pytest.mark.parametrize("n", [8, 16, 32])
def test_networks_sort(sel, n):
    rng = np.random.default_rng(n)
    for _ in range(200):
        v = rng.choice(rng.random(4 + n // 2, dtype=np.float32), n).astype(np.float32) if rng.random() < 0.5 else rng.random(n, dtype=np.float32)
        w = v.copy()
        sel.sel_sort(_fp(w), n)
        assert np.array_equal(w, np.sort(v))


def test_merge32_sorts_bitonic(sel):
    rng = np.random.default_rng(7)
    for _ in range(200):
        up, down = np.sort(rng.random(32, dtype=np.float32)), np.sort(rng.random(32, dtype=np.float32))
        v = np.minimum(up, down[::-1])        # the fold of ksel_tau: the 32 smallest of 64, bitonic
        w = v.copy()
        sel.sel_merge32(_fp(w))
        assert np.array_equal(w, np.sort(np.concatenate([up, down]))[:32])


def test_tau_matches_partition(sel):
    rng = np.random.default_rng(12345)
    for n in range(1, 129):
        for name, keys in _key_sets(n, rng):
            t, _ = _tau(sel, keys)
            want = _expected(keys)
            assert t.tobytes() == want.tobytes(), (n, name, t, want)


def test_chunks_staged_last_first(sel):
    # chunk 0 is staged last, so pass 2 finds it in LDS; every chunk exactly once, m <= 64
    for n in range(1, 200):
        _, staged = _tau(sel, np.ones(n, dtype=np.float32))
        starts = list(range(0, n, 64))[::-1]
        assert staged[:, 0].tolist() == starts
        assert staged[:, 1].tolist() == [min(64, n - c0) for c0 in starts]
