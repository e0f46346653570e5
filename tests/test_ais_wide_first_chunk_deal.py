"""CPU: what the wide AIS half-generation kernel's short first chunk and its compile-time task table
rest on (csrc/ais_kernels.hpp ais_half_body ch0, wide_placement_expected, WideDealTable), through
kabc_ais_wide_deal and kabc_ais_wide_deal_table -- no device needed.  For the two geometries the
library ships, (waves, chunk, n_c) = (12, 6, 2) and (8, 4, 1), and the four placement rotations
recorded in profiles/ais_wide3.md:
  * a first chunk of r sub-steps (tasks 2 si + b, si < r) is ONE task per producer -- pairwise
    different owners -- for every r with 2 r <= the number of producers: the consumers then leave
    the prologue after one fill;
  * the table the kernel takes in the expected placement equals wide_deal_mask for every wave, and
    the kernel's test accepts exactly the placements whose table that is."""
import ctypes as C
import random

import pytest

ROTATIONS = [(0, 2, 1, 3), (3, 0, 2, 1), (2, 1, 3, 0), (1, 3, 0, 2)]   # SIMD of waves 0..3, then repeating
SHIPPED = [(12, 6, 2), (8, 4, 1)]


@pytest.fixture(scope="module")
def lib(k):
    from kissabc_jl_amd import _lib
    return _lib.load()


def _deal(lib, simd, K, nc):
    W = len(simd)
    masks = (C.c_uint32 * (W - 2))()
    assert lib.kabc_ais_wide_deal((C.c_int32 * W)(*simd), W, K, nc, masks) == 0, lib.kabc_last_error()
    return [int(m) for m in masks]


def _table(lib, simd, K, nc):
    W = len(simd)
    masks, expected = (C.c_uint32 * (W - 2))(), C.c_int32(-1)
    st = lib.kabc_ais_wide_deal_table((C.c_int32 * W)(*simd), W, K, nc, masks, C.byref(expected))
    assert st == 0, lib.kabc_last_error()
    return [int(m) for m in masks], int(expected.value)


def _placed(rot, W):
    return tuple(rot[w % 4] for w in range(W))


def _is_expected(simd):
    """the issue's definition: consumers on two SIMDs, exactly W/4 - 1 producers beside each, and
    wave w on the SIMD of wave w mod 4"""
    W = len(simd)
    return (simd[0] != simd[1] and all(simd[2:].count(simd[i]) == W // 4 - 1 for i in (0, 1))
            and all(simd[w] == simd[w % 4] for w in range(W)))


def test_the_shipped_geometries_are_the_tested_ones(lib):
    geom = (C.c_int32 * 3)()
    lib.kabc_ais_wide_shipped(geom)
    assert tuple(int(v) for v in geom) in SHIPPED


@pytest.mark.parametrize("W,K,nc", SHIPPED)
def test_a_short_first_chunk_is_one_task_per_producer(lib, W, K, nc):
    nprod = W - 2
    lengths = [r for r in range(1, K + 1) if 2 * r <= nprod]
    assert lengths and lengths[-1] >= min(K, nprod // 2)
    for rot in ROTATIONS:
        masks = _deal(lib, _placed(rot, W), K, nc)
        for r in lengths:
            first = (1 << (2 * r)) - 1          # tasks 2 si + b with si < r
            owners = [p for p, m in enumerate(masks) for _ in range(bin(m & first).count("1"))]
            assert len(owners) == 2 * r                       # every task of the chunk has an owner
            assert len(set(owners)) == 2 * r, (W, K, nc, rot, r, masks)


@pytest.mark.parametrize("W,K,nc", SHIPPED)
def test_the_compile_time_table_is_the_deal(lib, W, K, nc):
    for rot in ROTATIONS:
        simd = _placed(rot, W)
        table, expected = _table(lib, simd, K, nc)
        assert expected == 1, (W, rot)
        assert table == _deal(lib, simd, K, nc), (W, K, nc, rot)
        assert len(table) == W - 2


@pytest.mark.parametrize("W,K,nc", SHIPPED)
def test_the_placement_test_accepts_what_the_table_serves(lib, W, K, nc):
    """every placement the kernel's scalar test accepts gets the table's masks from the function too;
    what it refuses goes through the function in the kernel (nothing to compare)"""
    rng = random.Random(4100 + W)
    cases = [tuple(rng.randrange(4) for _ in range(W)) for _ in range(300)]
    # near misses of the expected placement: one wave moved, the consumers together, a producer of
    # the first four beside a consumer, SIMD ids beyond 3
    base = _placed(ROTATIONS[0], W)
    for w in range(W):
        for s in range(4):
            cases.append(base[:w] + (s,) + base[w + 1:])
    cases += [tuple(r[0] if w < 2 else r[w % 4] for w in range(W)) for r in ROTATIONS]
    cases += [tuple([0, 1, 0, 2][w % 4] for w in range(W)), tuple([0, 1, 2, 1][w % 4] for w in range(W)),
              tuple([0, 1, 2, 2][w % 4] for w in range(W)), tuple([4, 9, 15, 7][w % 4] for w in range(W))]
    cases += [_placed(r, W) for r in ROTATIONS]
    seen = {0: 0, 1: 0}
    for simd in cases:
        table, expected = _table(lib, simd, K, nc)
        assert expected == (1 if _is_expected(simd) else 0), simd
        seen[expected] += 1
        if expected:
            assert table == _deal(lib, simd, K, nc), simd
    assert seen[0] > 100 and seen[1] >= 6


def test_bad_arguments_are_refused(lib):
    from kissabc_jl_amd import _cdefs as cd
    masks, simd, exp = (C.c_uint32 * 10)(), (C.c_int32 * 12)(), C.c_int32()
    for s, W, K, c, m, e in [(None, 12, 6, 2, masks, exp), (simd, 12, 6, 2, None, exp), (simd, 12, 6, 2, masks, None),
                             (simd, 12, 4, 1, masks, exp), (simd, 8, 6, 2, masks, exp), (simd, 8, 4, 0, masks, exp)]:
        assert lib.kabc_ais_wide_deal_table(s, W, K, c, m, C.byref(e) if e is not None else None) \
            == cd.KABC_ERR_INVALID_ARG
        assert b"kabc_ais_wide_deal_table" in lib.kabc_last_error()
    simd[3] = 16
    assert lib.kabc_ais_wide_deal_table(simd, 12, 6, 2, masks, C.byref(exp)) == cd.KABC_ERR_INVALID_ARG
