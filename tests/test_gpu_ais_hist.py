"""GPU: marginal histograms of a summarised AIS trace on the device (kabc_ais_hist_begin / _get;
AisEnsemble.summary_begin(hist=...), sample(..., summary=True, hist=...)) and the quantiles read from them.

Counts are integers, so every case compares them BIT FOR BIT with the numpy restatement
(tests/ais_hist_oracle.py) applied to the collect=True trace of a second handle with the same seed, checks
that every parameter's counts add up to n, and compares the moments (and the lagged products, where autocorr
is open) bit for bit with a summary opened without hist: on the one-workgroup drivers and the launch per
half-generation, on both counting kernels, across blocks, chunks and calls, at the ends of the range, per
chain of a batch handle, beyond 16 parameters, after a cancel, and on recycled buffers."""
import ctypes as C
import math
import threading
import time

import numpy as np
import pytest

import ais_autocorr_oracle as ao
import ais_hist_oracle as ho
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


def _summary(k, model, N, gens, nt, hist=None, cov=None, driver=None, autocorr=None, **kw):
    e = k.AisEnsemble(model, N, **kw).init()
    if driver is not None:
        assert e.driver == driver
    e.summary_begin(cov, autocorr=autocorr, hist=hist)
    assert e.advance(gens, nt, summary=True) is None
    s = e.summary()
    e.close()
    return s


_REF = {}


def _reference(k, name, model, N, gens, nt, cov=None, seed=5):
    """the collect=True trace of a twin handle and the summary without hist, computed once per shape"""
    if name not in _REF:
        e = k.AisEnsemble(model, N, seed=seed).init()
        tr = e.advance(gens, nt, collect=True)
        e.close()
        tr.setflags(write=False)
        _REF[name] = (tr, _summary(k, model, N, gens, nt, cov=cov, seed=seed))
    return _REF[name]


def _check(k, name, model, N, gens, nt, driver, hist, cov=None, seed=5):
    tr, plain = _reference(k, name, model, N, gens, nt, cov, seed)
    s = _summary(k, model, N, gens, nt, hist, cov=cov, driver=driver, seed=seed)
    lo, hi, B = hist
    assert ho.mismatches(s, tr, lo, hi, B) == []
    assert so.mismatches(plain, _asdict(s)) == []           # the moments are those of a plain summary
    assert plain.hist is None and plain.median is None
    assert s.n == gens * N and s.hist.shape == (len(model), B) and s.nbins == B
    return s, tr


# ---- the one-workgroup driver ----------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 7, 1024])
def test_small_driver(k, B):
    _check(k, "gauss2-12", _gauss2(k), 12, 37, 2, "small", (-5.0, 5.0, B))


def test_small_driver_three_blocks_of_the_device_buffer(k, monkeypatch):
    monkeypatch.setenv("KABC_TRACE_CHUNK_MIB", "1")          # 32 KiB per generation: blocks of 32, 32 and 6
    s, _ = _check(k, "box8-512", _box(k, 8), 512, 70, 1, "small", (-5.0, 5.0, 33))
    assert np.count_nonzero(s.hist) > 8 * 5                  # (a spread-out posterior: many bins in use)


# ---- the launch per half-generation ----------------------------------------------------------------

def test_half_generation_course_odd_rows_several_chunks(k, monkeypatch):
    monkeypatch.setenv("KABC_TRACE_CHUNK_MIB", "1")          # 15 384 B per generation: chunks of 68, 68 and 14
    _check(k, "box3-641", _box(k, 3), 641, 150, 1, "halves", ([-5.0, -4.0, -1.0], [5.0, 4.5, 1.0], 50))


def test_both_drivers_give_the_same_bits(k, monkeypatch):
    hist = (-5.0, 5.0, 40)
    a, _ = _check(k, "gauss2-100", _gauss2(k), 100, 25, 2, "small", hist)
    monkeypatch.setenv("KABC_AIS_SMALL", "0")
    b = _summary(k, _gauss2(k), 100, 25, 2, hist, driver="halves", seed=5)
    assert np.array_equal(a.histogram["counts"], b.histogram["counts"])
    assert so.mismatches(a, _asdict(b)) == []


@pytest.mark.parametrize("name,D,N,gens,driver", [("gauss2-100", 2, 100, 25, "small"),    # N D < 256: direct by rule
                                                  ("box3-641", 3, 641, 150, "halves")])   # LDS by rule
def test_both_counting_kernels_give_the_same_counts(k, monkeypatch, name, D, N, gens, driver):
    model = _gauss2(k) if D == 2 else _box(k, 3)
    nt = 2 if D == 2 else 1
    got = {}
    for path in ("lds", "direct"):
        monkeypatch.setenv("KABC_HIST_PATH", path)
        got[path], _ = _check(k, name, model, N, gens, nt, driver, (-5.0, 5.0, 21))
    assert np.array_equal(got["lds"].histogram["counts"], got["direct"].histogram["counts"])


# ---- the ends of the range -------------------------------------------------------------------------

def test_exact_minimum_lands_in_bin_0_and_exact_maximum_in_the_overflow(k):
    tr, plain = _reference(k, "gauss2-100", _gauss2(k), 100, 25, 2)
    cols = tr.reshape(-1, 2)
    lo, hi = cols.min(axis=0), cols.max(axis=0)
    assert np.array_equal(lo, plain.min) and np.array_equal(hi, plain.max)
    for B in (5, 1024):
        s, _ = _check(k, "gauss2-100", _gauss2(k), 100, 25, 2, "small", (lo, hi, B))
        assert np.all(s.underflow == 0) and np.all(s.hist[:, 0] >= 1)
        assert np.array_equal(s.overflow, (cols == hi).sum(axis=0).astype(np.uint64)) and np.all(s.overflow >= 1)


def test_narrow_range_most_samples_outside(k):
    tr, plain = _reference(k, "gauss2-100", _gauss2(k), 100, 25, 2)
    lo, hi = plain.mean - 0.02 * plain.std, plain.mean + 0.03 * plain.std
    s, _ = _check(k, "gauss2-100", _gauss2(k), 100, 25, 2, "small", (lo, hi, 16))
    assert np.all(s.underflow + s.overflow > 0.9 * s.n)


@pytest.mark.parametrize("name,D,N,gens,driver", [("gauss2-100", 2, 100, 25, "small"),
                                                  ("box8-512b", 8, 512, 20, "small")])
def test_wide_range_every_sample_in_one_bin(k, name, D, N, gens, driver):
    """the worst case for the atomics: every lane of a wave adds to the same word of its parameter"""
    model = _gauss2(k) if D == 2 else _box(k, 8)
    s, _ = _check(k, name, model, N, gens, 2 if D == 2 else 1, driver, (-1e6, 1e6, 7))
    assert np.all(s.hist[:, 3] == s.n) and s.hist.sum() == D * s.n


def test_discrete_parameter_on_an_integer_aligned_range_is_bincount(k):
    K = 12
    prior = k.Factored(k.Laplace(0.5, 1.5), k.Poisson(3.0))
    model = k.ApproxKernelizedPosterior(prior, k.costs.NoisyQuadDU(5.5), 1.0)
    s, tr = _check(k, "poisson", model, 60, 40, 1, None, (-0.5, K + 0.5, K + 1))
    x = tr.reshape(-1, 2)[:, 1]
    assert np.array_equal(x, np.rint(x)) and x.min() >= 0 and len(np.unique(x)) > 1
    xi = x.astype(np.int64)
    want = np.bincount(xi[xi <= K], minlength=K + 1)
    assert np.array_equal(s.hist[1], want.astype(np.uint64))
    assert s.underflow[1] == 0 and s.overflow[1] == np.count_nonzero(xi > K)
    assert np.array_equal(s.edges[1], np.arange(K + 2) - 0.5)


# ---- splitting over calls, cancel ------------------------------------------------------------------

@pytest.mark.parametrize("N,driver", [(100, "small"), (641, "halves")])
def test_split_over_calls(k, N, driver):
    model, nt, hist = _gauss2(k), 2, (-5.0, 5.0, 30)
    e = k.AisEnsemble(model, N, seed=8).init()
    tr = e.advance(20, nt, collect=True)
    e.close()
    e = k.AisEnsemble(model, N, seed=8).init()
    assert e.driver == driver
    e.summary_begin(hist=hist)
    done = 0
    for piece in (7, 1, 12):
        e.advance(piece, nt, summary=True)
        done += piece
        for _ in range(2):                                   # (reading leaves the counts alone)
            assert ho.mismatches(e.summary(), tr[:done], *hist) == [], done
    e.close()


def test_cancel_small_driver(k):
    """the one-workgroup kernel leaves its block early and only the device knows how many generations ran:
    the counts are those of exactly the generations the summary's n reports"""
    model, N, nt, hist = _gauss2(k), 50, 64, (-5.0, 5.0, 64)
    ctx = k.Context(0)
    try:
        ens = k.AisEnsemble(model, N, seed=11, ctx=ctx).init()
        assert ens.driver == "small"
        ens.summary_begin(hist=hist)
        t0 = time.perf_counter()
        ens.advance(500, nt, summary=True)
        dt = (time.perf_counter() - t0) / 500
        G = min(max(int(5.0 / dt), 2), 80000)               # ~5 s if the cancel were ignored; one launch block
        ens.summary_begin(hist=hist)                         # (starts over)
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
        assert ho.mismatches(got, tr, *hist) == []
        ens.advance(3, nt, summary=True)                     # the handle keeps working, and so do its counts
        tr = np.concatenate([tr, ref.advance(3, nt, collect=True)])
        assert ho.mismatches(ens.summary(), tr, *hist) == []
        ref.close()
        ens.close()
    finally:
        ctx.close()


# ---- beyond 16 parameters, batch handles -------------------------------------------------------------

@pytest.mark.parametrize("B", [9, 1024])                     # (1024: a full slab of 16 fills the larger LDS table)
def test_beyond_16_parameters_two_slabs(k, B):
    lo, hi = np.linspace(-9.0, -5.0, 20), np.linspace(4.0, 8.0, 20)
    s, _ = _check(k, "d20", _d20(k), 64, 12, 2, None, (lo, hi, B), cov="diag")
    assert s.diag and s.hist.shape == (20, B) and s.median.shape == (20,)


def test_batch_handle_per_chain_ranges_each_chain_is_its_own_run(k):
    from kissabc_jl_amd.api import chain_seeds
    seeds, model, B = chain_seeds(3, 3), _gauss2(k), 25
    lo = np.array([[-5.0, -5.0], [-1.0, -2.0], [0.5, -0.75]])
    hi = np.array([[5.0, 5.0], [3.0, 1.0], [1.5, 0.0]])
    both = _summary(k, model, 12, 20, 2, (lo, hi, B), seeds=seeds)
    e = k.AisEnsemble(model, 12, seeds=seeds).init()
    tr = e.advance(20, 2, collect=True)                      # [gen][chain][N][D]
    e.close()
    assert both.nchains == 3 and both.hist.shape == (3, 2, B) and both.edges.shape == (3, 2, B + 1)
    for c, sd in enumerate(seeds):
        one = _summary(k, model, 12, 20, 2, (lo[c], hi[c], B), seed=sd)
        assert np.array_equal(both.chain(c).histogram["counts"], one.histogram["counts"]), c
        assert ho.mismatches(both.chain(c), tr[:, c], lo[c], hi[c], B) == [], c
        assert so.mismatches(both.chain(c), _asdict(one)) == [], c


# ---- with the autocorrelation, recycled memory, refusals ---------------------------------------------

@pytest.mark.parametrize("hist_first", [False, True])
def test_stacked_with_autocorr_in_either_order(k, hist_first):
    from kissabc_jl_amd import _cdefs as cd
    lib = k._lib.load()
    model, N, gens, nt, L, B = _gauss2(k), 100, 25, 2, 8, 40
    tr, _ = _reference(k, "gauss2-100", model, N, gens, nt)
    lo, hi = np.full((1, 2), -5.0), np.full((1, 2), 5.0)
    e = k.AisEnsemble(model, N, seed=5).init()
    e.summary_begin()
    p = lambda a: a.ctypes.data_as(cd.c_double_p)           # noqa: E731
    calls = [lambda: lib.kabc_ais_autocorr_begin(e._h, L), lambda: lib.kabc_ais_hist_begin(e._h, B, p(lo), p(hi))]
    for call in (calls[::-1] if hist_first else calls):
        assert call() == cd.KABC_OK
    e._summary_maxlag, e._summary_hist = L, B
    e.advance(gens, nt, summary=True)
    s = e.summary()
    e.close()
    assert ho.mismatches(s, tr, -5.0, 5.0, B) == []
    assert ao.mismatches(s, ao.summarize(tr, L)) == []
    only_ac = _summary(k, model, N, gens, nt, autocorr=L, seed=5)
    assert ao.mismatches(s, _ac_dict(only_ac)) == []        # moments and lagged products of a run without hist


def test_recycled_count_buffers_are_zeroed(k):
    model, N, nt, hist = _box(k, 3), 641, 1, (-5.0, 5.0, 60)
    ctx = k.Context(0)
    try:
        e = k.AisEnsemble(model, N, seed=2, ctx=ctx).init()
        tr = e.advance(12, nt, collect=True)
        e.close()
        e = k.AisEnsemble(model, N, seed=2, ctx=ctx).init()
        e.summary_begin(hist=hist)
        e.advance(5, nt, summary=True)
        assert ho.mismatches(e.summary(), tr[:5], *hist) == []
        e.summary_end()                                      # (the counts go back to the pool, dirty)
        e.summary_begin(hist=hist)
        e.advance(7, nt, summary=True)
        assert ho.mismatches(e.summary(), tr[5:], *hist) == []
        e.summary_begin(hist=hist)                           # (begin again without an end)
        e.summary_begin()                                    # (starts over WITHOUT the histograms)
        assert e.advance(0, nt, summary=True) is None
        e.close()
        e2 = k.AisEnsemble(model, N, seed=2, ctx=ctx).init()
        e2.summary_begin(hist=hist)
        e2.advance(5, nt, summary=True)
        assert ho.mismatches(e2.summary(), tr[:5], *hist) == []
        e2.close()
    finally:
        ctx.close()


def test_refusals_on_a_live_handle(k):
    from kissabc_jl_amd import _cdefs as cd
    lib = k._lib.load()
    p = lambda a: a.ctypes.data_as(cd.c_double_p)           # noqa: E731
    lo, hi = np.full(2, -5.0), np.full(2, 5.0)
    e = k.AisEnsemble(_gauss2(k), 30, seed=1).init()
    assert lib.kabc_ais_hist_begin(e._h, 8, p(lo), p(hi)) == cd.KABC_ERR_INVALID_STATE     # no summary open
    assert lib.kabc_ais_hist_get(e._h, None, None, None, None) == cd.KABC_ERR_INVALID_STATE
    e.summary_begin()
    assert lib.kabc_ais_hist_get(e._h, None, None, None, None) == cd.KABC_ERR_INVALID_STATE  # no histogram on it
    for bad in (0, -1, cd.KABC_HIST_MAX_BINS + 1):
        assert lib.kabc_ais_hist_begin(e._h, bad, p(lo), p(hi)) == cd.KABC_ERR_INVALID_ARG
    assert lib.kabc_ais_hist_begin(e._h, 8, None, p(hi)) == cd.KABC_ERR_INVALID_ARG
    for blo, bhi in (([-5.0, 5.0], [5.0, 5.0]), ([-5.0, np.nan], [5.0, 5.0]), ([-5.0, -5.0], [5.0, np.inf]),
                     ([-5.0, -1e308], [5.0, 1e308])):        # (the last: hi - lo overflows, the scale is 0)
        assert lib.kabc_ais_hist_begin(e._h, 8, p(np.array(blo)), p(np.array(bhi))) == cd.KABC_ERR_INVALID_ARG
        assert b"chain 0, parameter 1" in lib.kabc_last_error()
    e.summary_begin(hist=(lo, hi, cd.KABC_HIST_MAX_BINS))
    counts = np.full((2, cd.KABC_HIST_MAX_BINS + 2), 99, dtype=np.uint64)
    assert lib.kabc_ais_hist_get(e._h, None, counts.ctypes.data_as(C.POINTER(C.c_uint64)), None,
                                 None) == cd.KABC_ERR_INVALID_STATE                        # nothing folded yet
    assert b"n = 0" in lib.kabc_last_error() and np.all(counts == 99)
    e.advance(3, 1, summary=True)
    s = e.summary()
    assert s.n == 90 and s.hist.shape == (2, 1024) and np.all(s.hist.sum(axis=1) + s.underflow + s.overflow == 90)
    assert lib.kabc_ais_hist_begin(e._h, 8, p(lo), p(hi)) == cd.KABC_ERR_INVALID_STATE     # generations folded
    assert b"already holds" in lib.kabc_last_error()
    e.summary_end()
    assert lib.kabc_ais_hist_get(e._h, None, None, None, None) == cd.KABC_ERR_INVALID_STATE
    e.close()


# ---- sample, quantiles -----------------------------------------------------------------------------

def test_sample_hist_automatic_range_quantiles_and_interval(k):
    from kissabc_jl_amd.api import _hist_auto_range
    model, N, gk = _gauss2(k), 50, 100
    kw = dict(ntransitions=2, discard_initial=150, seed=9)
    s = k.sample(model, k.AIS(N), gk * N, summary=True, hist=True, **kw)
    x = k.sample(model, k.AIS(N), gk * N, return_array=True, **kw)
    e = k.AisEnsemble(model, N, seed=9).init()               # the walkers after discard_initial
    e.advance(3, 2)
    lo, hi = _hist_auto_range(e.state()[0])
    e.close()
    assert s.nbins == 128 and ho.mismatches(s, x.reshape(gk, N, 2), lo, hi, 128) == []
    assert np.all(s.underflow + s.overflow < 0.05 * s.n)     # (the convention holds here; it is no guarantee)
    xs, w = np.sort(x, axis=0), (hi - lo) / 128
    for q in ho.QS:
        stat = xs[max(math.ceil(q * s.n), 1) - 1]
        inside = (lo <= stat) & (stat < hi)
        assert inside.any() or q in (0.0, 1.0)
        slack = 8 * np.spacing(np.maximum(np.abs(lo), np.abs(hi)))
        assert np.all(np.abs(s.quantile(q) - stat)[inside] <= (w + slack)[inside]), q
    assert np.array_equal(s.quantile(0.0), xs[0]) and np.array_equal(s.quantile(1.0), xs[-1])
    assert np.array_equal(s.interval(0.95), s.quantile([0.025, 0.975])) and s.interval().shape == (2, 2)
    assert np.array_equal(s.median, s.quantile(0.5))
    # an int: that many bins, the same automatic range
    s16 = k.sample(model, k.AIS(N), gk * N, summary=True, hist=16, **kw)
    assert ho.mismatches(s16, x.reshape(gk, N, 2), lo, hi, 16) == []


def test_sample_mcmcthreads_pooled_counts_and_sample_batch(k):
    model, N, Nc, gk = _gauss2(k), 50, 3, 20
    kw = dict(ntransitions=2, seed=9)
    hist = ([-5.0, -4.0], [5.0, 4.0], 32)
    cs = k.sample(model, k.AIS(N), k.MCMCThreads(), gk * N, Nc, summary=True, hist=hist, **kw)
    x = k.sample(model, k.AIS(N), k.MCMCThreads(), gk * N, Nc, return_array=True, **kw).reshape(Nc, gk, N, 2)
    for c in range(Nc):
        assert ho.mismatches(cs[c], x[c], *hist) == [], c
    assert ho.mismatches(cs.pooled, x.reshape(Nc * gk, N, 2), *hist) == []
    assert cs.pooled.n == Nc * gk * N and cs.pooled.median.shape == (2,)
    auto = k.sample(model, k.AIS(N), k.MCMCThreads(), gk * N, Nc, summary=True, hist=True, **kw)
    assert all(c.hist.shape == (2, 128) for c in auto) and auto.pooled.hist is None
    with pytest.raises(ValueError, match=r"hist=\(lo, hi\)"):
        auto.pooled.quantile(0.5)
    out = k.sample_batch(model, k.AIS(N), gk * N, nruns=2, summary=True, hist=16, **kw)
    assert all(o.hist.shape == (2, 16) and np.all(o.hist.sum(axis=1) + o.underflow + o.overflow == o.n) for o in out)
    assert not np.array_equal(out[0].hist, out[1].hist)
