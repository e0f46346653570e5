"""-m gpu: the wide AIS half-generation kernel runs its SHORT chunk first (csrc/ais_kernels.hpp
ais_half_body, ch0, split_full).  With K the shipped chunk, read from the library, a launch of nt
sub-steps is cut into
  nt <= K                    one chunk of nt,
  nt no multiple of K        ((nt - 1) mod K) + 1 sub-steps first, then full chunks of K,
  nt = m K, m > 1            K - 2 first, m - 1 full chunks, 2 last (one chunk more).
Every first-chunk length and its neighbours:
  nt = 1 .. K                a single chunk,
  nt = K + 1 .. 2K - 1       first chunks of 1 .. K - 1 with exactly one full chunk behind,
  nt = 2K                    K - 2, K, 2,
  nt = 2K + 1, 3K, 5K - 2    1 + K + K;  (K - 2) + K + K + 2;  (K - 2) + four full chunks.
BOX prior, D = 8 (the headline's kernel) and D = 2; 128 rows per half (one workgroup, both batches
full) and 128 + 37 (a second workgroup whose second batch is absent and whose first is ragged); two
seeds.  Each case against
  (a) the CPU oracle's sync schedule: trace, state, counters, per-transition debug records,
  (b) the existing geometry (KABC_AIS_WIDE=0) on the same,
  (c) itself: one handle advanced in two calls against one call,
all bit for bit.  The debug records are indexed by the absolute sub-step: a chunk that starts at the
wrong one, or a record filled for another sub-step than the consumer reads, shows there.  Every run
has KABC_AIS_WIDE=2 (a launch that cannot take the wide kernel is an error), KABC_AIS_SMALL=0 and
KABC_SPECIALIZE=0, the way test_gpu_ais_wide3.py runs its cases."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS = (128, 128 + 37)
SEEDS = (1, 2)
# the sub-step counts of a group of cases, from the shipped chunk K
GROUPS = {
    "single_chunk": lambda K: list(range(1, K + 1)),
    "one_full_chunk_behind": lambda K: list(range(K + 1, 2 * K + 1)),   # (2K: K - 2, K, 2)
    "more_chunks_behind": lambda K: [2 * K + 1, 3 * K, 4 * K + K - 2],
}


def _chunk():
    from kissabc_jl_amd import _lib
    geom = (C.c_int32 * 3)()
    _lib.load().kabc_ais_wide_shipped(geom)
    assert geom[0] in (8, 12) and 1 <= geom[1] <= 8
    return int(geom[1])


def _model(k, d):
    return k.ApproxKernelizedPosterior(k.Factored(*[k.Uniform(-5, 5)] * d), k.costs.Rosenbrock(), 1.0)


def _run(k, monkeypatch, model, N, nt, seed, wide, split=False):
    monkeypatch.setenv("KABC_AIS_WIDE", wide)
    ens = k.AisEnsemble(model, N, seed=seed).init()
    assert ens.driver == "halves"
    ens.set_debug(nt)
    g1 = ens.advance(1, nt, collect=True)
    dbg = ens.get_debug(nt)
    ens.set_debug(0)
    if split:
        g2 = np.concatenate([ens.advance(1, nt, collect=True), ens.advance(1, nt, collect=True)])
    else:
        g2 = ens.advance(2, nt, collect=True)
    xs, lps, lls, t = ens.state()
    out = {"g1": g1, "dbg": dbg, "g2": g2, "x": xs, "lp": lps, "ll": lls, "t": t, "stats": ens.stats()}
    ens.close()
    return out


def _same(a, b, what):
    for key in ("g1", "dbg", "g2", "x", "lp", "ll"):
        assert np.array_equal(a[key], b[key]), (what, key)
    assert a["t"] == b["t"] and a["stats"] == b["stats"], what


@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("d", [8, 2])
def test_first_chunk_lengths(k, orc, gpu_ctx, monkeypatch, d, rows, group):
    monkeypatch.setenv("KABC_AIS_SMALL", "0")
    monkeypatch.setenv("KABC_SPECIALIZE", "0")
    model, N = _model(k, d), 2 * rows
    for nt in GROUPS[group](_chunk()):
        for seed in SEEDS:
            what = f"D {d}, nt {nt}, {rows} rows per half, seed {seed}"
            wide = _run(k, monkeypatch, model, N, nt, seed, "2")
            # (b) the existing geometry, (c) two calls against one
            _same(wide, _run(k, monkeypatch, model, N, nt, seed, "0"), "wide != existing: " + what)
            _same(wide, _run(k, monkeypatch, model, N, nt, seed, "2", split=True), "two calls != one: " + what)
            # (a) the oracle
            o = orc.OracleAIS(model, N, seed=seed).init()
            ref, tr = o.generations_sync(1, nt, trace=True)
            dbg = wide["dbg"]
            assert dbg.shape[1] == nt, what
            assert np.array_equal(wide["g1"], ref), what
            for col in (0, 1, 5):   # move id, accepted, evaluated -- per absolute sub-step
                assert np.array_equal(dbg[:, :, col], tr[0, :, :, col]), (what, col)
            base = np.where(np.arange(N) < rows, rows, 0)[:, None]
            for col in (2, 3, 4):   # partner rows
                v = dbg[:, :, col].astype(np.int64)
                assert np.array_equal(np.where(v >= 0, v + base, -1), tr[0, :, :, col].astype(np.int64)), (what, col)
            assert np.array_equal(wide["g2"], o.generations_sync(2, nt)), what
            xo, lpo, llo, to = o.state()
            assert wide["t"] == to == 3 * nt, what
            assert np.array_equal(wide["x"], xo) and np.array_equal(wide["lp"], lpo), what
            assert np.array_equal(wide["ll"], llo), what
            assert wide["stats"] == o.stats(), what
