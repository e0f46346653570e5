"""-m gpu: the wide AIS half-generation kernel the library ships, whatever its wave count
(csrc/ais_kernels.hpp WideGeom<K, n_c, W>: W = 8 or 12 waves, kabc_ais_wide_shipped), against
  (a) the CPU oracle's sync schedule, bit for bit,
  (b) the existing geometry (KABC_AIS_WIDE=0) on trace, state, counters and the per-transition
      debug records, bit for bit,
  (c) itself: one handle advanced in two calls against one call.
Every case runs with KABC_AIS_WIDE=2 (a launch that cannot take the wide kernel is an error),
KABC_AIS_SMALL=0 and KABC_SPECIALIZE=0.  Shapes follow the SHIPPED chunk K, read from the library:
rows per half around the two-batch workgroup, sub-steps around the chunk.  What a 12-wave
workgroup changes and the eight-wave tests do not reach: the consumer with ONE set of partner-row
registers below D = 11 (BOX, D = 2, 5, 8), the log table staged by 512 of 768 threads, a
NegativeBinomial table staged by the first 256 of them (GENERAL class, ntransitions >= 8), and
producers that may hold no task of a chunk.  The task table itself is tested on the CPU
(test_ais_wide_deal.py): no test controls where the hardware places a wave."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _chunk(k):
    from kissabc_jl_amd import _lib
    geom = (C.c_int32 * 3)()
    _lib.load().kabc_ais_wide_shipped(geom)
    assert geom[0] in (8, 12) and 1 <= geom[1] <= 8
    return int(geom[1])


def _models(k):
    box = lambda d: k.ApproxKernelizedPosterior(k.Factored(*[k.Uniform(-5, 5)] * d), k.costs.Rosenbrock(), 1.0)  # noqa: E731
    return {
        "box2": box(2), "box5": box(5), "box8": box(8),
        "normal4": k.ApproxKernelizedPosterior(k.Factored(*[k.Normal(0, 2)] * 4), k.costs.Rosenbrock(), 1.0),
        "simple4": k.ApproxKernelizedPosterior(
            k.Factored(k.Uniform(-3, 3), k.Normal(0, 2), k.TruncatedNormal(0, 2, -3, 3), k.Uniform(-4, 4)),
            k.costs.Rosenbrock(), 1.0),
        # GENERAL class with a NegativeBinomial component: its lgamma table (launches of >= 8 sub-steps)
        # (two parameters: the dimensions up to which the GENERAL class takes the 12-wave kernel)
        "negbin2": k.ApproxKernelizedPosterior(
            k.Factored(k.NegativeBinomial(4.0, 0.4), k.Gamma(2.5, 0.7)), k.costs.Rosenbrock(), 50.0),
        # GENERAL class beyond them: the eight-wave kernel the library keeps there
        "general4": k.ApproxKernelizedPosterior(
            k.Factored(k.Gamma(2.5, 0.7), k.LogNormal(0.3, 0.6), k.Exponential(2.0), k.Beta(2, 3)),
            k.costs.Rosenbrock(), 2.0),
        # a discrete component: push_p rounds it (BOX class)
        "discrete3": k.ApproxKernelizedPosterior(
            k.Factored(k.Uniform(-3, 3), k.DiscreteUniform(-3, 3), k.Uniform(-3, 3)), k.costs.Rosenbrock(), 2.0),
        # ApproxPosterior (threshold acceptance, posterior kind 2)
        "threshold2": k.ApproxPosterior(k.Factored(*[k.Uniform(-5, 5)] * 2), k.costs.Rosenbrock(), 30.0),
    }


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


def _check(k, orc, monkeypatch, name, rows, nt, seeds=(1, 2)):
    monkeypatch.setenv("KABC_AIS_SMALL", "0")
    monkeypatch.setenv("KABC_SPECIALIZE", "0")   # the prebuilt kernels: the model's own have one geometry
    model, N = _models(k)[name], 2 * rows
    for seed in seeds:
        wide = _run(k, monkeypatch, model, N, nt, seed, "2")
        # (b) the existing geometry, (c) two calls against one
        _same(wide, _run(k, monkeypatch, model, N, nt, seed, "0"), f"wide != existing, seed {seed}")
        _same(wide, _run(k, monkeypatch, model, N, nt, seed, "2", split=True), f"resume, seed {seed}")
        # (a) the oracle: trace, move ids, accept and evaluated flags, partner rows, state, counters
        o = orc.OracleAIS(model, N, seed=seed).init()
        ref, tr = o.generations_sync(1, nt, trace=True)
        dbg = wide["dbg"]
        assert np.array_equal(wide["g1"], ref)
        for col in (0, 1, 5):
            assert np.array_equal(dbg[:, :, col], tr[0, :, :, col]), col
        base = np.where(np.arange(N) < rows, rows, 0)[:, None]
        for col in (2, 3, 4):
            d = dbg[:, :, col].astype(np.int64)
            assert np.array_equal(np.where(d >= 0, d + base, -1), tr[0, :, :, col].astype(np.int64)), col
        assert np.array_equal(wide["g2"], o.generations_sync(2, nt))
        xo, lpo, llo, to = o.state()
        assert wide["t"] == to == 3 * nt
        assert np.array_equal(wide["x"], xo) and np.array_equal(wide["lp"], lpo) and np.array_equal(wide["ll"], llo)
        assert wide["stats"] == o.stats()
        # the records cover stretch, DE and walk
        assert set(np.unique(dbg[:, :, 0]).tolist()) == {1, 2, 3}


@pytest.mark.parametrize("rows", [128, 129, 192, 193, 255])
def test_wide3_rows_per_half(k, orc, gpu_ctx, monkeypatch, rows):
    """the second batch of the last workgroup absent, one row, full, ragged; K + 1 sub-steps"""
    _check(k, orc, monkeypatch, "box8", rows, _chunk(k) + 1)


@pytest.mark.parametrize("nt", ["1", "K-1", "K", "2K", "2K+1"])
def test_wide3_substeps_around_the_chunk(k, orc, gpu_ctx, monkeypatch, nt):
    """K the shipped chunk; 1 and 2K + 1 end on a single-sub-step chunk"""
    K = _chunk(k)
    n = {"1": 1, "K-1": K - 1, "K": K, "2K": 2 * K, "2K+1": 2 * K + 1}[nt]
    _check(k, orc, monkeypatch, "box8", 193, max(n, 1))


@pytest.mark.parametrize("name", ["box2", "box5", "box8"])
def test_wide3_one_row_set_small_dimensions(k, orc, gpu_ctx, monkeypatch, name):
    """BOX prior, D = 2, 5, 8: with 12 waves the consumer reuses one set of partner-row registers"""
    _check(k, orc, monkeypatch, name, 129, _chunk(k) + 1)


@pytest.mark.parametrize("name", ["normal4", "simple4", "negbin2", "general4", "discrete3", "threshold2"])
def test_wide3_prior_classes_and_kinds(k, orc, gpu_ctx, monkeypatch, name):
    K = _chunk(k)
    _check(k, orc, monkeypatch, name, 129, max(8, 2 * K + 1) if name == "negbin2" else K + 1)


def test_wide3_placement_independence(k, orc, gpu_ctx, monkeypatch):
    """one case twice in one process (the hardware may place the waves differently): equal"""
    monkeypatch.setenv("KABC_AIS_SMALL", "0")
    monkeypatch.setenv("KABC_SPECIALIZE", "0")
    model, nt = _models(k)["box8"], 2 * _chunk(k) + 1
    first = _run(k, monkeypatch, model, 386, nt, 1, "2")
    _same(first, _run(k, monkeypatch, model, 386, nt, 1, "2"), "second run")
