"""CPU: the task table of the wide AIS half-generation kernel (csrc/ais_kernels.hpp wide_deal_mask, the
function the kernel runs once per launch), through kabc_ais_wide_deal -- no device needed.  The GPU
tests cannot choose where the hardware places a wave, so the placement classes are covered here:
the expected placement in its four rotations, both consumers on one SIMD, three producers beside one
consumer, every wave on one SIMD, and seeded random placements; for 8 and 12 waves."""
import ctypes as C
import random

import pytest

ROTATIONS = [(0, 2, 1, 3), (3, 0, 2, 1), (2, 1, 3, 0), (1, 3, 0, 2)]   # SIMD of waves 0..3, then repeating


@pytest.fixture(scope="module")
def lib(k):
    from kissabc_jl_amd import _lib
    return _lib.load()


def _shipped(lib):
    geom = (C.c_int32 * 3)()
    lib.kabc_ais_wide_shipped(geom)
    return tuple(int(v) for v in geom)


def _deal(lib, simd, K, nc):
    W = len(simd)
    masks = (C.c_uint32 * (W - 2))()
    assert lib.kabc_ais_wide_deal((C.c_int32 * W)(*simd), W, K, nc, masks) == 0, lib.kabc_last_error()
    return [int(m) for m in masks]


def _each_task_once(masks, K):
    seen = 0
    for m in masks:
        assert m & seen == 0, "a task dealt twice"
        seen |= m
    assert seen == (1 << (2 * K)) - 1, "a task dealt to nobody"


def _round_robin(cap, K):
    """the dealing order: task 0, 1, ... to the next producer that still has room"""
    cap, masks, p = list(cap), [0] * len(cap), 0
    assert sum(cap) == 2 * K
    for task in range(2 * K):
        while cap[p] == 0:
            p = (p + 1) % len(cap)
        masks[p] |= 1 << task
        cap[p] -= 1
        p = (p + 1) % len(cap)
    return masks


def _parent_table(simd, K, nc):
    """the table the eight-wave kernel built before the dealing moved into wide_deal_mask: one producer
    beside each consumer takes nc, the other four split the rest, the first ones taking the remainder;
    any other placement: equal shares"""
    nprod, nt = 6, 2 * K
    sc0, sc1, prod = simd[0], simd[1], simd[2:]
    cot = [s in (sc0, sc1) for s in prod]
    if nc >= 0 and sc0 != sc1 and prod.count(sc0) == 1 and prod.count(sc1) == 1:
        rest, others, seen, cap = nt - 2 * nc, nprod - 2, 0, []
        for p in range(nprod):
            if cot[p]:
                cap.append(nc)
            else:
                cap.append(rest // others + (1 if seen < rest % others else 0))
                seen += 1
    else:
        cap = [nt // nprod + (1 if p < nt % nprod else 0) for p in range(nprod)]
    return _round_robin(cap, K)


def _geometries(lib):
    W0, K0, c0 = _shipped(lib)
    out = {(W, K0, c0) for W in (8, 12)}
    out |= {(W, K, c) for W in (8, 12) for K in (4, 5, 6) for c in (-1, 0, 1, 2)}
    return sorted(out)


def _placements(W):
    exp = [tuple(r[w % 4] for w in range(W)) for r in ROTATIONS]
    one_simd = [tuple(r[0] if w < 2 else r[w % 4] for w in range(W)) for r in ROTATIONS[:2]]   # both consumers
    three = [tuple([0, 1] + [0] * 3 + [2, 3] * ((W - 5) // 2) + [1] * ((W - 5) % 2))]          # three beside wave 0
    flat = [(2,) * W]
    rng = random.Random(20260 + W)
    rnd = [tuple(rng.randrange(4) for _ in range(W)) for _ in range(300)]
    return exp, one_simd + three + flat + rnd


def test_shipped_geometry(lib):
    W, K, c = _shipped(lib)
    assert W in (8, 12) and 1 <= K <= 8 and c <= K


def test_every_task_has_one_owner(lib):
    for W, K, c in _geometries(lib):
        exp, other = _placements(W)
        for simd in exp + other:
            masks = _deal(lib, simd, K, c)
            assert len(masks) == W - 2
            _each_task_once(masks, K)


def test_shares_of_the_expected_placement(lib):
    """each consumer's SIMD gets c tasks per chunk, handed one at a time to its first producer, then its
    second; the producer-only waves split 2K - 2c, the first ones taking the remainder"""
    for W, K, c in _geometries(lib):
        if c < 0:
            continue
        beside = W // 4 - 1
        for simd in _placements(W)[0]:
            prod, seen, k_beside, cap = simd[2:], 0, {simd[0]: 0, simd[1]: 0}, []
            rest, others = 2 * K - 2 * c, (W - 2) - 2 * beside
            for s in prod:
                if s in k_beside:
                    cap.append(c // beside + (1 if k_beside[s] < c % beside else 0))
                    k_beside[s] += 1
                else:
                    cap.append(rest // others + (1 if seen < rest % others else 0))
                    seen += 1
            masks = _deal(lib, simd, K, c)
            assert [bin(m).count("1") for m in masks] == cap, (W, K, c, simd)
            assert masks == _round_robin(cap, K)
            # what a SIMD carries: c beside a consumer, the rest in two halves on the producer-only SIMDs
            per_simd = {s: 0 for s in range(4)}
            for s, m in zip(prod, masks):
                per_simd[s] += bin(m).count("1")
            assert per_simd[simd[0]] == per_simd[simd[1]] == c
            assert sorted(v for s, v in per_simd.items() if s not in simd[:2]) == [rest // 2, rest - rest // 2]


def test_other_placements_get_equal_shares(lib):
    for W, K, c in _geometries(lib):
        nprod, beside = W - 2, W // 4 - 1
        equal = _round_robin([2 * K // nprod + (1 if p < 2 * K % nprod else 0) for p in range(nprod)], K)
        for simd in _placements(W)[1]:
            expected = c >= 0 and simd[0] != simd[1] and all(simd[2:].count(simd[i]) == beside for i in (0, 1))
            if not expected:
                assert _deal(lib, simd, K, c) == equal, (W, K, c, simd)
        assert _deal(lib, _placements(W)[0][0], K, -1) == equal     # n_c < 0: equal shares whatever the placement


def test_eight_waves_match_the_parent_table(lib):
    for W, K, c in _geometries(lib):
        if W != 8:
            continue
        exp, other = _placements(8)
        for simd in exp + other:
            assert _deal(lib, simd, K, c) == _parent_table(list(simd), K, c), (K, c, simd)
    # the shipped eight-wave shares as the notes state them: 1 beside a consumer, 2 2 1 1 on the others
    assert [bin(m).count("1") for m in _deal(lib, (0, 2, 1, 3, 0, 2, 1, 3), 4, 1)] == [2, 2, 1, 1, 1, 1]


def test_bad_arguments_are_refused(lib):
    from kissabc_jl_amd import _cdefs as cd
    masks, simd = (C.c_uint32 * 10)(), (C.c_int32 * 12)()
    for s, W, K, c, m in [(None, 8, 4, 1, masks), (simd, 8, 4, 1, None), (simd, 10, 4, 1, masks),
                          (simd, 8, 0, 0, masks), (simd, 8, 9, 1, masks), (simd, 12, 4, 5, masks)]:
        assert lib.kabc_ais_wide_deal(s, W, K, c, m) == cd.KABC_ERR_INVALID_ARG
        assert b"kabc_ais_wide_deal" in lib.kabc_last_error()
    simd[3] = 16
    assert lib.kabc_ais_wide_deal(simd, 8, 4, 1, masks) == cd.KABC_ERR_INVALID_ARG
