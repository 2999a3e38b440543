"""The pool budget of a fixed-spp call (gi_layout.h: plan_pool, called by stream_samples) through the CPU build of the host headers
(tests/host_emul): P, the paths in flight, and chunk, the samples per pixel the radiance buffer takes at a time.  The expected values are the
expressions stream_samples held before the budget became a function of its own, spelled out here in integers (one float multiply for the
0.90 of free memory) -- _parent() below never calls the function under test -- and, for the cases with a round answer, the number itself.
The benchmark frame's P decides its speed, so every comparison is exact."""
import ctypes as C

import pytest

import emul_lib

GIB = 1 << 30
POOL_RECORD = 64 + 48 + 48 + 48 + 24        # PoolRay, PoolHit, PoolThru, PoolGath, 24 bytes of smaller fields: GI_POOL_BYTES_PER_SLOT
SHADOW_Q = 96                               # sizeof(ShadowQ)
SLOTS_MAX, LBUF_MAX = 1 << 30, 16 * GIB     # the context's defaults: pool_slots_max, lbuf_bytes_max
BENCH = dict(n_pix=1920 * 1080, spp=256, lights=1)
SMALL = dict(n_pix=64 * 48, spp=8, lights=1)


def _parent(mem_known, free_b, held_b, n_pix, spp, slots_max, lbuf_max, lights):
    """(P, chunk) as the expressions of stream_samples gave them."""
    budget = slots_max
    if mem_known:
        per_slot = POOL_RECORD + 8 + 13 * 4 + 24 + 40 + SHADOW_Q * lights
        lbuf = n_pix * min(spp, lbuf_max // (n_pix * 24)) * 24
        avail = int(float(free_b + held_b) * 0.90)
        budget = min(budget, (avail - lbuf) // per_slot) if avail > lbuf else min(budget, 1 << 20)
    return max(64, min(budget, 0xFFFFFFF0, n_pix * spp)), max(1, min(spp, lbuf_max // (n_pix * 24)))


def _plan(mem_known=True, free_b=280 * GIB, held_b=0, n_pix=0, spp=0, slots_max=SLOTS_MAX, lbuf_max=LBUF_MAX, lights=1):
    out = (C.c_int64 * 2)()
    emul_lib.lib().emul_pool_plan(1 if mem_known else 0, free_b, held_b, n_pix, spp, slots_max, lbuf_max, lights, out)
    assert (out[0], out[1]) == _parent(mem_known, free_b, held_b, n_pix, spp, slots_max, lbuf_max, lights)
    return out[0], out[1]


def test_benchmark_frame_with_280_gib_free():
    """1920 x 1080 x 256 spp, one deferred light, 16 GiB radiance cap, nothing held: 452 bytes per slot, a 12.7 GB radiance buffer.  With 280 GiB
    free the budget is 570 448 542 slots, just above the frame's 530 841 600 samples: the whole frame is in flight (the 530 841 600 new paths
    of pass 0 that GI_DEBUG_WF shows on the benchmark), and the formula is what keeps it so."""
    assert POOL_RECORD + 124 + SHADOW_Q == 452
    assert (int(float(280 * GIB) * 0.90) - 1920 * 1080 * 256 * 24) // 452 == 570448542
    assert _plan(**BENCH) == (530841600, 256)


@pytest.mark.parametrize("free_gib, held_gib", [(256, 0), (200, 0), (100, 156), (128, 0)])
def test_benchmark_frame_bound_by_memory(free_gib, held_gib):
    """Less free memory, or part of it held by the context already: P is what the budget leaves, below n_pix x spp."""
    P, chunk = _plan(free_b=free_gib * GIB, held_b=held_gib * GIB, **BENCH)
    assert P == (int(float((free_gib + held_gib) * GIB) * 0.90) - 1920 * 1080 * 256 * 24) // 452 < 1920 * 1080 * 256 and chunk == 256
    if free_gib + held_gib == 256:
        assert P == 519136986


def test_benchmark_frame_with_four_deferred_lights_bound_by_memory():
    """Four lights put off four ShadowQ per slot: 356 + 4 x 96 = 740 bytes instead of 452.  With 128 GiB free the benchmark frame is bound by memory
    (149 938 999 slots of its 530 841 600 samples), and by fewer slots than with one light (245 475 353, the case above): the stride of d_shq is in the budget."""
    assert POOL_RECORD + 124 + 4 * SHADOW_Q == 740
    P, chunk = _plan(free_b=128 * GIB, **dict(BENCH, lights=4))
    assert (P, chunk) == _parent(True, 128 * GIB, 0, 1920 * 1080, 256, SLOTS_MAX, LBUF_MAX, 4)
    assert P == (int(float(128 * GIB) * 0.90) - 1920 * 1080 * 256 * 24) // 740 == 149938999 < 1920 * 1080 * 256 and chunk == 256
    assert P < _plan(free_b=128 * GIB, **BENCH)[0] == 245475353
    assert P * 740 + 1920 * 1080 * 256 * 24 <= int(float(128 * GIB) * 0.90)          # the pool and the radiance buffer fit what was offered


def test_small_frame_and_a_pool_of_a_third():
    assert _plan(**SMALL) == (24576, 8)
    assert _plan(slots_max=24576 // 3 + 1, **SMALL) == (8193, 8)
    assert _plan(**dict(SMALL, lights=0)) == _plan(**dict(SMALL, lights=4)) == (24576, 8)


def test_memory_query_failing():
    """No figure for free memory: the caller's bound and the frame decide alone."""
    assert _plan(mem_known=False, free_b=0, **BENCH) == (530841600, 256)
    assert _plan(mem_known=False, free_b=0, slots_max=1000000, **BENCH) == (1000000, 256)
    assert _plan(mem_known=False, free_b=0, **SMALL) == (24576, 8)


def test_available_memory_below_the_radiance_buffer():
    """90 % of 8 GiB is less than the 12.7 GB radiance buffer of the benchmark frame: a pool of 1 << 20 slots, or the caller's smaller bound."""
    assert _plan(free_b=8 * GIB, **BENCH) == (1 << 20, 256)
    assert _plan(free_b=8 * GIB, slots_max=4096, **BENCH) == (4096, 256)
    assert _plan(free_b=0, **SMALL) == (24576, 8)            # the cap is above this frame's samples


def test_floor_of_64_slots():
    assert _plan(n_pix=2 * 2, spp=4) == (64, 4)
    assert _plan(slots_max=64, **SMALL) == (64, 8)
    assert _plan(free_b=86440, n_pix=64 * 48, spp=1) == (64, 1)         # 90 % of it: the 73 728-byte radiance buffer and 9 slots of 452 bytes


def test_more_samples_than_the_radiance_cap_allows():
    """The radiance buffer holds 3 samples of every pixel: chunks of 3, and the budget counts a buffer of that size only."""
    assert _plan(lbuf_max=64 * 48 * 24 * 3, **SMALL) == (24576, 3)
    assert _plan(lbuf_max=64 * 48 * 24 * 3 + 23, **SMALL) == (24576, 3)
    assert _plan(lbuf_max=100, **SMALL) == (24576, 1)        # not even one: a chunk is at least a sample
    P, chunk = _plan(free_b=8 * GIB, lbuf_max=4 * GIB, **BENCH)
    assert chunk == (4 * GIB) // (1920 * 1080 * 24) == 86 and P == (int(float(8 * GIB) * 0.90) - 1920 * 1080 * 86 * 24) // 452 == 7635023
