"""GPU: the autocorrelation of a summarised AIS trace on the device (kabc_ais_autocorr_begin / _get;
AisEnsemble.summary_begin(autocorr=...), sample(..., summary=True, autocorr=...)).

Like the moments, the lagged products and everything derived from them are a fixed order of fp64 operations
(include/kabc.h), so every case compares lagsum, first, last, acov, rho, tau, ess and window BIT FOR BIT with
the numpy restatement (tests/ais_autocorr_oracle.py) applied to the collect=True trace of a second handle
with the same seed, and the moments with those of a summary opened without autocorr: on the one-workgroup
drivers and the launch per half-generation, with lags that reach across blocks, chunks and calls, per chain
of a batch handle, beyond KABC_MAX_DIM parameters, after a cancel, and on recycled accumulators."""
import threading
import time

import numpy as np
import pytest

import ais_autocorr_oracle as ao
import ais_summary_oracle as so

pytestmark = pytest.mark.gpu


def _box(k, D, cost=None):
    return k.ApproxKernelizedPosterior(k.Factored(*[k.Uniform(-5, 5)] * D), cost or k.costs.Rosenbrock(), 1.0)


def _gauss2(k):
    return _box(k, 2, k.costs.GaussDist([1.0, -0.5]))


def _d20(k):
    return k.ApproxKernelizedPosterior(k.Factored(*[k.Normal(0, 3)] * 20), k.costs.GaussDist(np.zeros(20)), 1.0)


def _asdict(s):
    return {f: getattr(s, f) for f in so.FIELDS}


def _ac_dict(s):
    d = _asdict(s)
    d.update({f: getattr(s, attr) for f, attr in ao.AC_FIELDS.items()}, converged=s.tau_converged)
    return d


def _summary(k, model, N, gens, nt, L=None, cov=None, driver=None, **kw):
    e = k.AisEnsemble(model, N, **kw).init()
    if driver is not None:
        assert e.driver == driver
    e.summary_begin(cov, autocorr=L)
    assert e.advance(gens, nt, summary=True) is None
    s = e.summary()
    e.close()
    return s


def _trace(k, model, N, gens, nt, **kw):
    e = k.AisEnsemble(model, N, **kw).init()
    tr = e.advance(gens, nt, collect=True)
    e.close()
    return tr


def _check(k, model, N, gens, nt, driver, L, cov=None, seed=5):
    s = _summary(k, model, N, gens, nt, L, cov=cov, driver=driver, seed=seed)
    plain = _summary(k, model, N, gens, nt, None, cov=cov, driver=driver, seed=seed)
    tr = _trace(k, model, N, gens, nt, seed=seed)
    full = cov != "diag" and len(model) <= k.KABC_MAX_DIM
    want = ao.summarize(tr, L, full=full)
    assert ao.mismatches(s, want) == []
    assert so.mismatches(plain, _asdict(s)) == []           # the moments are those of a plain summary
    assert plain.tau is None and plain.acf is None
    Lm = min(L, gens - 1)
    assert s.maxlag == L and s.acf.shape == (len(model), Lm + 1) == s.acov.shape
    assert s.n == gens * N
    return s, tr


# ---- the one-workgroup driver ----------------------------------------------------------------------

@pytest.mark.parametrize("L", [8, 64])                      # steady state; G <= L
def test_small_driver(k, L):
    s, _ = _check(k, _gauss2(k), 12, 37, 2, "small", L)
    assert s.acf.shape == (2, min(L, 36) + 1)


def test_small_driver_three_blocks_of_the_device_buffer(k, monkeypatch):
    monkeypatch.setenv("KABC_TRACE_CHUNK_MIB", "1")          # 32 KiB per generation: blocks of 32, 32 and 6
    _check(k, _box(k, 8), 512, 70, 1, "small", 40)           # (lags reach across a block boundary)


# ---- the launch per half-generation ----------------------------------------------------------------

@pytest.mark.parametrize("L", [70, 1])                      # across two chunk boundaries; the shortest
def test_half_generation_course_odd_rows_several_chunks(k, monkeypatch, L):
    monkeypatch.setenv("KABC_TRACE_CHUNK_MIB", "1")          # 15 384 B per generation: chunks of 68, 68 and 14
    _check(k, _box(k, 3), 641, 150, 1, "halves", L)


@pytest.mark.parametrize("N", [513, 1025])
def test_row_tree_last_tile_of_one_entry(k, N):
    """N = 512 j + 1: the last tile of the row tree's first level holds a single entry, and at 1025 the second
    level combines an odd number (3) of run values; D = 3 keeps the planes' element stride in play"""
    _check(k, _box(k, 3), N, 5, 1, "halves", 4)


def test_row_tree_three_levels(k):
    """N = 512 * 512 + 1: the first shape whose tree has three levels, and so reads back from both scratch levels
    (a trace of 12.6 MB, planes of 25 MB)"""
    _check(k, _gauss2(k), 512 * 512 + 1, 3, 1, "halves", 2)


def test_both_drivers_give_the_same_bits(k, monkeypatch):
    a, _ = _check(k, _gauss2(k), 100, 25, 2, "small", 8)
    monkeypatch.setenv("KABC_AIS_SMALL", "0")
    b, _ = _check(k, _gauss2(k), 100, 25, 2, "halves", 8)
    assert ao.mismatches(a, _ac_dict(b)) == []


# ---- splitting over calls --------------------------------------------------------------------------

@pytest.mark.parametrize("N,driver", [(100, "small"), (641, "halves")])
def test_split_over_calls(k, N, driver):
    model, nt, L = _gauss2(k), 2, 5
    tr = _trace(k, model, N, 20, nt, seed=8)
    e = k.AisEnsemble(model, N, seed=8).init()
    assert e.driver == driver
    e.summary_begin(autocorr=L)
    done = 0
    for piece in (7, 1, 12):                                 # (longer than L, one generation, the rest)
        e.advance(piece, nt, summary=True)
        done += piece
        got = e.summary()                                    # (reading leaves the accumulators alone)
        assert ao.mismatches(got, ao.summarize(tr[:done], L)) == [], done
    e.close()


# ---- beyond KABC_MAX_DIM parameters, batch handles ---------------------------------------------------

def test_beyond_16_parameters_diag(k):
    s, _ = _check(k, _d20(k), 64, 12, 2, None, 4, cov="diag")
    assert s.diag and s.tau.shape == (20,)


def test_batch_handle_each_chain_is_its_own_run(k):
    from kissabc_jl_amd.api import chain_seeds
    seeds, model, L = chain_seeds(3, 3), _gauss2(k), 6
    both = _summary(k, model, 12, 20, 2, L, seeds=seeds)
    tr = _trace(k, model, 12, 20, 2, seeds=seeds)            # [gen][chain][N][D]
    assert both.nchains == 3 and both.tau.shape == (3, 2) and both.acf.shape == (3, 2, L + 1)
    for c, sd in enumerate(seeds):
        one = _summary(k, model, 12, 20, 2, L, seed=sd)
        assert ao.mismatches(both.chain(c), _ac_dict(one)) == [], c
        assert ao.mismatches(both.chain(c), ao.summarize(tr[:, c], L)) == [], c


# ---- cancel ----------------------------------------------------------------------------------------

def test_cancel_small_driver(k):
    """tests/test_gpu_ais_summary.py's cancel case on the one-workgroup driver: the kernel leaves its block
    early and only the device knows how many generations ran -- the lagged products, the windows and the
    generation count behind the ring are those of exactly the generations the summary's n reports"""
    model, N, nt, L = _gauss2(k), 50, 64, 8
    ctx = k.Context(0)
    try:
        ens = k.AisEnsemble(model, N, seed=11, ctx=ctx).init()
        assert ens.driver == "small"
        ens.summary_begin(autocorr=L)
        t0 = time.perf_counter()
        ens.advance(500, nt, summary=True)
        dt = (time.perf_counter() - t0) / 500
        G = min(max(int(5.0 / dt), 2), 80000)               # ~5 s if the cancel were ignored; one launch block
        ens.summary_begin(autocorr=L)                        # (starts over)
        x0, lp0, ll0, t_before = ens.state()
        tm = threading.Timer(0.3, ctx.cancel)
        tm.start()
        with pytest.raises(k.Cancelled):
            ens.advance(G, nt, summary=True)
        tm.join()
        kg = (ens.state()[3] - t_before) // nt
        assert 0 < kg < G, (kg, G)
        got = ens.summary()
        assert got.n == N * kg
        ref = k.AisEnsemble(model, N, seed=11, ctx=ctx)
        ref.set_state(x0, lp0, ll0, t_before)
        tr = ref.advance(kg, nt, collect=True)
        assert ao.mismatches(got, ao.summarize(tr, L)) == []
        # the handle keeps working, and so do its lagged products (the ring goes on from generation kg)
        ens.advance(3, nt, summary=True)
        tr = np.concatenate([tr, ref.advance(3, nt, collect=True)])
        assert ao.mismatches(ens.summary(), ao.summarize(tr, L)) == []
        ref.close()
        ens.close()
    finally:
        ctx.close()


# ---- recycled memory, refusals -----------------------------------------------------------------------

def test_begin_twice_on_one_handle_takes_dirty_buffers(k):
    model, N, nt, L = _box(k, 3), 641, 1, 6
    ctx = k.Context(0)
    try:
        tr = _trace(k, model, N, 12, nt, seed=2, ctx=ctx)
        e = k.AisEnsemble(model, N, seed=2, ctx=ctx).init()
        e.summary_begin(autocorr=L)
        e.advance(5, nt, summary=True)
        assert ao.mismatches(e.summary(), ao.summarize(tr[:5], L)) == []
        e.summary_begin(autocorr=L)                          # (the first summary's buffers come back dirty)
        e.advance(7, nt, summary=True)
        assert ao.mismatches(e.summary(), ao.summarize(tr[5:], L)) == []
        e.summary_begin()                                    # (starts over WITHOUT the lagged products)
        assert e.advance(0, nt, summary=True) is None
        e.close()
    finally:
        ctx.close()


def test_refusals_on_a_live_handle(k):
    from kissabc_jl_amd import _cdefs as cd
    lib = k._lib.load()
    e = k.AisEnsemble(_gauss2(k), 30, seed=1).init()
    assert lib.kabc_ais_autocorr_begin(e._h, 8) == cd.KABC_ERR_INVALID_STATE          # no summary open
    assert lib.kabc_ais_autocorr_get(e._h, *[None] * 10) == cd.KABC_ERR_INVALID_STATE
    e.summary_begin()
    assert lib.kabc_ais_autocorr_get(e._h, *[None] * 10) == cd.KABC_ERR_INVALID_STATE  # no autocorr on it
    for bad in (0, -1, cd.KABC_AUTOCORR_MAX_LAG + 1):
        assert lib.kabc_ais_autocorr_begin(e._h, bad) == cd.KABC_ERR_INVALID_ARG
    e.summary_begin(autocorr=cd.KABC_AUTOCORR_MAX_LAG)
    with pytest.raises(k.KabcError, match="n = 0") as ei:                              # nothing folded yet
        e.summary()
    assert ei.value.status == cd.KABC_ERR_INVALID_STATE
    e.advance(3, 1, summary=True)
    s = e.summary()
    assert s.n == 90 and s.acf.shape == (2, 3) and s.maxlag == cd.KABC_AUTOCORR_MAX_LAG
    assert lib.kabc_ais_autocorr_begin(e._h, 8) == cd.KABC_ERR_INVALID_STATE          # generations folded
    assert b"already holds" in lib.kabc_last_error()
    e.summary_end()
    assert lib.kabc_ais_autocorr_get(e._h, *[None] * 10) == cd.KABC_ERR_INVALID_STATE
    e.close()


# ---- sample ----------------------------------------------------------------------------------------

def test_sample_reports_tau_ess_and_mcse(k):
    model, N = _gauss2(k), 50
    s = k.sample(model, k.AIS(N), 5000, summary=True, autocorr=True, seed=9)
    x = k.sample(model, k.AIS(N), 5000, return_array=True, seed=9)
    assert ao.mismatches(s, ao.summarize(x.reshape(100, N, 2), 64)) == []
    assert s.n == 5000 and s.maxlag == 64
    assert np.all(1.0 <= s.tau) and np.all(s.ess <= s.n)
    assert np.array_equal(s.mcse, s.std * np.sqrt(s.tau / s.n))
    assert np.array_equal(s.ess, s.n / s.tau)
    # three chains: per-chain values, the chains' ess add up, the pooled moments carry no tau
    cs = k.sample(model, k.AIS(N), k.MCMCThreads(), 1000, 3, summary=True, autocorr=16, seed=9)
    assert np.array_equal(cs.ess, (cs[0].ess + cs[1].ess) + cs[2].ess) and cs.pooled.tau is None
    assert all(c.maxlag == 16 and c.tau.shape == (2,) for c in cs)
    out = k.sample_batch(model, k.AIS(N), 1000, nruns=2, summary=True, autocorr=16, seed=9)
    assert all(o.tau.shape == (2,) and o.acf.shape == (2, 17) for o in out)
