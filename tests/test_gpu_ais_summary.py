"""GPU: posterior summaries on the device (kabc_ais_summary_begin / kabc_ais_advance_summary /
kabc_ais_summary_get; AisEnsemble.summary_begin, advance(summary=True), summary; sample(summary=True)).

The summary is defined by a fixed order of fp64 operations (include/kabc.h), so every case compares
summary() BIT FOR BIT -- n, pivot, sum1, sum2, min, max, mean, cov -- with the numpy restatement
(tests/ais_summary_oracle.py) applied to the collect=True trace of a second handle with the same seed:
on the one-workgroup drivers and the launch per half-generation, over several blocks / chunks of the
device trace, split over calls, per chain of a batch handle, beyond KABC_MAX_DIM parameters, after a
cancel, and on accumulators that come back dirty from the context's pool."""
import copy
import threading

import numpy as np
import pytest

import ais_summary_oracle as so

pytestmark = pytest.mark.gpu


def _box(k, D, cost=None):
    return k.ApproxKernelizedPosterior(k.Factored(*[k.Uniform(-5, 5)] * D), cost or k.costs.Rosenbrock(), 1.0)


def _d20(k):
    return k.ApproxKernelizedPosterior(k.Factored(*[k.Normal(0, 3)] * 20), k.costs.GaussDist(np.zeros(20)), 1.0)


def _asdict(s):
    return {f: getattr(s, f) for f in so.FIELDS}


def _summary(k, model, N, gens, nt, cov=None, driver=None, **kw):
    e = k.AisEnsemble(model, N, **kw).init()
    if driver is not None:
        assert e.driver == driver
    e.summary_begin(cov)
    assert e.advance(gens, nt, summary=True) is None
    s = e.summary()
    e.close()
    return s


def _trace(k, model, N, gens, nt, **kw):
    e = k.AisEnsemble(model, N, **kw).init()
    tr = e.advance(gens, nt, collect=True)
    e.close()
    return tr


def _check(k, model, N, gens, nt, driver, cov=None, seed=5):
    s = _summary(k, model, N, gens, nt, cov=cov, driver=driver, seed=seed)
    tr = _trace(k, model, N, gens, nt, seed=seed)
    full = cov != "diag" and len(model) <= k.KABC_MAX_DIM
    want = so.summarize(tr, full=full)
    assert so.mismatches(s, want) == []
    assert s.n == gens * N and s.diag == (not full)
    return s, tr


# ---- the one-workgroup driver ----------------------------------------------------------------------

def test_small_driver_odd_shape(k):
    _check(k, _box(k, 2, k.costs.GaussDist([1.0, -0.5])), 12, 37, 2, "small")


def test_small_driver_three_blocks_of_the_device_buffer(k, monkeypatch):
    monkeypatch.setenv("KABC_TRACE_CHUNK_MIB", "1")          # 32 KiB per generation: blocks of 32, 32 and 6
    _check(k, _box(k, 8), 512, 70, 1, "small")


# ---- the launch per half-generation ----------------------------------------------------------------

def test_half_generation_course_odd_rows_several_chunks(k, monkeypatch):
    monkeypatch.setenv("KABC_TRACE_CHUNK_MIB", "1")          # 15 384 B per generation: chunks of 68, 68 and 14
    _check(k, _box(k, 3), 641, 150, 1, "halves")


def test_half_generation_course_ragged(k):
    _check(k, _box(k, 3), 1000, 7, 3, "halves")


def test_half_generation_course_widest_full_shape(k):
    s, _ = _check(k, _box(k, 16), 600, 6, 2, "halves")
    assert s.cov.shape == (16, 16) and s.sum2.shape == (16, 16)


@pytest.mark.parametrize("N", [513, 1025])
def test_row_tree_last_tile_of_one_entry(k, N):
    """N = 512 j + 1: the last tile of the row tree's first level holds a single entry, and at 1025 the second
    level combines an odd number (3) of run values"""
    _check(k, _box(k, 3), N, 5, 1, "halves")


def test_row_tree_three_levels(k):
    """N = 512 * 512 + 1: the first shape whose tree has three levels, and so reads back from both scratch levels"""
    _check(k, _box(k, 2, k.costs.GaussDist([1.0, -0.5])), 512 * 512 + 1, 3, 1, "halves")


def test_diag_below_the_full_limit(k):
    s, _ = _check(k, _box(k, 3), 641, 9, 1, "halves", cov="diag")
    assert s.cov.shape == (3,)
    _check(k, _box(k, 2, k.costs.GaussDist([1.0, -0.5])), 12, 9, 1, "small", cov="diag")


def test_both_drivers_give_the_same_bits(k, monkeypatch):
    model = _box(k, 2, k.costs.GaussDist([1.0, -0.5]))
    a, _ = _check(k, model, 100, 25, 2, "small")
    monkeypatch.setenv("KABC_AIS_SMALL", "0")
    b, _ = _check(k, model, 100, 25, 2, "halves")
    assert so.mismatches(a, _asdict(b)) == []


# ---- splitting over calls --------------------------------------------------------------------------

@pytest.mark.parametrize("N,driver", [(100, "small"), (641, "halves")])
def test_split_over_calls(k, N, driver):
    model, nt = _box(k, 2, k.costs.GaussDist([1.0, -0.5])), 2
    whole = _summary(k, model, N, 20, nt, driver=driver, seed=8)
    e = k.AisEnsemble(model, N, seed=8).init()
    e.summary_begin()
    e.advance(7, nt, summary=True)
    part = e.summary()                                       # (reading leaves the accumulators alone)
    e.advance(13, nt, summary=True)
    assert so.mismatches(e.summary(), _asdict(whole)) == []
    assert part.n == 7 * N
    e.close()
    # a collect=True advance in between does not feed the summary; the chain goes on from it
    e = k.AisEnsemble(model, N, seed=8).init()
    e.summary_begin()
    e.advance(7, nt, summary=True)
    assert so.mismatches(e.summary(), _asdict(part)) == []
    mid = e.advance(5, nt, collect=True)
    e.advance(13, nt, summary=True)
    got = e.summary()
    e.close()
    r = k.AisEnsemble(model, N, seed=8).init()
    t1 = r.advance(7, nt, collect=True)
    t2 = r.advance(5, nt, collect=True)
    t3 = r.advance(13, nt, collect=True)
    r.close()
    assert np.array_equal(mid, t2)
    assert so.mismatches(got, so.summarize(np.concatenate([t1, t3]))) == []
    assert got.n == 20 * N


# ---- batch handles ---------------------------------------------------------------------------------

def test_batch_handle_per_chain_costs(k):
    seeds = [3, 977, 2 ** 40 + 3]
    costs = [k.costs.GaussDist(np.array([1.0, -0.5]) + 0.3 * c) for c in range(3)]
    model = k.ApproxKernelizedPosterior(k.Factored(k.Normal(0, 5), k.Normal(0, 5)), costs[0], 0.5)
    both = _summary(k, model, 20, 11, 2, seeds=seeds, costs=costs)
    tr = _trace(k, model, 20, 11, 2, seeds=seeds, costs=costs)         # [gen][chain][N][D]
    assert both.nchains == 3 and both.mean.shape == (3, 2) and both.cov.shape == (3, 2, 2)
    for c, sd in enumerate(seeds):
        m = copy.copy(model)
        m.cost = costs[c]
        one = _summary(k, m, 20, 11, 2, seed=sd)
        assert so.mismatches(both.chain(c), _asdict(one)) == [], c
        assert so.mismatches(both.chain(c), so.summarize(tr[:, c])) == [], c


def test_batch_handle_on_the_half_generation_course(k):
    seeds = [11, 12]
    model = _box(k, 3)
    both = _summary(k, model, 641, 5, 1, driver="halves", seeds=seeds)
    tr = _trace(k, model, 641, 5, 1, seeds=seeds)
    for c in range(2):
        assert so.mismatches(both.chain(c), so.summarize(tr[:, c])) == [], c


# ---- beyond KABC_MAX_DIM parameters ----------------------------------------------------------------

@pytest.mark.parametrize("N,driver", [(50, "small"), (600, "halves")])
def test_beyond_16_parameters_diag(k, N, driver):
    for cov in ("diag", None):
        s, _ = _check(k, _d20(k), N, 6, 2, driver, cov=cov)
        assert s.diag and s.cov.shape == (20,) and s.sum2.shape == (20,)
    e = k.AisEnsemble(_d20(k), N, seed=5).init()
    from kissabc_jl_amd import _cdefs as cd
    with pytest.raises(k.KabcError, match="diag") as ei:
        e.summary_begin("full")
    assert ei.value.status == cd.KABC_ERR_UNSUPPORTED
    e.close()


# ---- a discrete component: integer rows, exact sums ------------------------------------------------

def test_discrete_component_sums_are_exact(k):
    """Factored(Normal(1, 0.5), DiscreteUniform(1, 10)) with NoisyQuadDU(5.5), the pfilter tests' problem: the
    second column holds push_p'ed integers, whose sums are exact -- they also equal integer arithmetic"""
    prior = k.Factored(k.Normal(1, 0.5), k.DiscreteUniform(1, 10))
    model = k.ApproxKernelizedPosterior(prior, k.costs.NoisyQuadDU(5.5), 1.0)
    s, tr = _check(k, model, 60, 40, 1, "small")
    x = tr.reshape(-1, 2)[:, 1]
    assert np.array_equal(x, np.rint(x)) and x.min() >= 1 and x.max() <= 10
    xi = x.astype(np.int64)
    d = xi - xi[0]
    assert s.sum1[1] == float(d.sum()) and s.sum2[1, 1] == float((d * d).sum())
    assert s.min[1] == xi.min() and s.max[1] == xi.max()
    assert len(np.unique(xi)) > 1


# ---- sample / sample_batch -------------------------------------------------------------------------

def test_sample_summary_is_the_summary_of_samples_generations(k):
    model, N = _box(k, 2, k.costs.GaussDist([1.0, -0.5])), 100
    kw = dict(ntransitions=3, discard_initial=250, seed=9)
    s = k.sample(model, k.AIS(N), 5 * N, summary=True, **kw)
    x = k.sample(model, k.AIS(N), 5 * N, return_array=True, **kw)
    assert so.mismatches(s, so.summarize(x.reshape(5, N, 2))) == []
    # Ns that N does not divide: the kept generations whole
    s2 = k.sample(model, k.AIS(N), 4 * N + 1, summary=True, **kw)
    assert s2.n == 5 * N and so.mismatches(s2, _asdict(s)) == []
    assert "±" in repr(s) and s.isapprox([1.0, -0.5], nsigma=4.0).all()


def test_sample_mcmcthreads_summary_pooled_and_rhat(k):
    model, N, Nc, gk = _box(k, 2, k.costs.GaussDist([1.0, -0.5])), 100, 3, 6
    kw = dict(ntransitions=2, discard_initial=200, seed=4)
    out = k.sample(model, k.AIS(N), k.MCMCThreads(), gk * N, Nc, summary=True, **kw)
    x = k.sample(model, k.AIS(N), k.MCMCThreads(), gk * N, Nc, return_array=True, **kw).reshape(Nc, gk * N, 2)
    assert isinstance(out, k.ChainSummaries) and len(out) == Nc
    for c in range(Nc):
        assert so.mismatches(out[c], so.summarize(x[c].reshape(gk, N, 2))) == [], c
    flat = x.reshape(-1, 2)
    n = gk * N
    assert out.pooled.n == Nc * n
    # (host double arithmetic on ~2000 values of order 1: far inside 1e-12)
    assert np.allclose(out.pooled.mean, flat.mean(axis=0), rtol=0, atol=1e-12)
    assert np.allclose(out.pooled.cov, np.cov(flat, rowvar=False, ddof=1), rtol=0, atol=1e-12)
    assert np.array_equal(out.pooled.min, flat.min(axis=0)) and np.array_equal(out.pooled.max, flat.max(axis=0))
    W = x.var(axis=1, ddof=1).mean(axis=0)
    rhat = np.sqrt(((n - 1) / n * W + x.mean(axis=1).var(axis=0, ddof=1)) / W)
    assert np.allclose(out.rhat, rhat, rtol=1e-12, atol=0)


@pytest.mark.parametrize("course", ["grid", "sequential"])
def test_sample_batch_summary(k, course):
    N, gk = 60, 4
    models = [k.ApproxKernelizedPosterior(k.Factored(k.Normal(0, 5), k.Normal(0, 5)),
                                          k.costs.GaussDist(np.array([1.0, -0.5]) + 0.3 * r), 0.5) for r in range(3)]
    kw = dict(seeds=[5, 6, 7], ntransitions=2, discard_initial=60, course=course)
    out = k.sample_batch(models, k.AIS(N), gk * N, summary=True, **kw)
    ref = k.sample_batch(models, k.AIS(N), gk * N, return_array=True, **kw)
    assert out.info["course"] == course == ref.info["course"] and len(out) == 3
    for r in range(3):
        assert isinstance(out[r], k.PosteriorSummary)
        assert so.mismatches(out[r], so.summarize(ref[r].reshape(gk, N, 2))) == [], r


# ---- refusals on a live handle ---------------------------------------------------------------------

def test_refusals_on_a_live_handle(k):
    from kissabc_jl_amd import _cdefs as cd
    model = _box(k, 2, k.costs.GaussDist([1.0, -0.5]))
    e = k.AisEnsemble(model, 30, seed=1)
    with pytest.raises(k.KabcError, match="kabc_ais_init") as ei:       # not initialised
        e.summary_begin()
    assert ei.value.status == cd.KABC_ERR_INVALID_STATE
    e.init()
    for call in (lambda: e.advance(2, 1, summary=True), e.summary):     # without begin
        with pytest.raises(k.KabcError, match="kabc_ais_summary_begin") as ei:
            call()
        assert ei.value.status == cd.KABC_ERR_INVALID_STATE
    with pytest.raises(k.KabcError, match="cov_mode") as ei:
        k._lib.check(k._lib.load().kabc_ais_summary_begin(e._h, 7))
    assert ei.value.status == cd.KABC_ERR_INVALID_ARG
    e.summary_begin()
    with pytest.raises(k.KabcError, match="n = 0") as ei:               # nothing summarised yet
        e.summary()
    assert ei.value.status == cd.KABC_ERR_INVALID_STATE
    e.advance(0, 1, summary=True)
    with pytest.raises(k.KabcError, match="n = 0"):
        e.summary()
    e.advance(3, 1, summary=True)
    assert e.summary().n == 90
    e.summary_end()
    e.summary_end()                                                     # (nothing open: fine)
    with pytest.raises(k.KabcError, match="kabc_ais_summary_begin"):
        e.summary()
    assert e.advance(2, 1, collect=True).shape == (2, 30, 2)            # the handle goes on
    e.close()


# ---- cancel ----------------------------------------------------------------------------------------

CANCEL_AFTER = 0.3
TARGET_S = 5.0      # what the cancelled call would take if the cancel were ignored


def _cancel_case(k, model, N, nt, cal, driver, max_gens=None):
    """tests/test_gpu_cancel.py's pattern: a call sized from a calibration run to ~5 s, a host cancel request
    from a timer after 0.3 s; the summary then holds the generations that completed, exactly"""
    import time
    ctx = k.Context(0)
    try:
        ens = k.AisEnsemble(model, N, seed=11, ctx=ctx).init()
        assert ens.driver == driver
        ens.summary_begin()
        t0 = time.perf_counter()
        ens.advance(cal, nt, summary=True)
        dt = (time.perf_counter() - t0) / cal
        G = max(int(TARGET_S / dt), 2)
        if max_gens is not None:
            G = min(G, max_gens)
        ens.summary_begin()                                  # (starts over)
        x0, lp0, ll0, t_before = ens.state()
        tm = threading.Timer(CANCEL_AFTER, ctx.cancel)
        tm.start()
        with pytest.raises(k.Cancelled):
            ens.advance(G, nt, summary=True)
        tm.join()
        t_after = ens.state()[3]
        assert (t_after - t_before) % nt == 0
        kg = (t_after - t_before) // nt
        assert 0 < kg < G, (kg, G)
        got = ens.summary()
        assert got.n == N * kg
        ref = k.AisEnsemble(model, N, seed=11, ctx=ctx)
        ref.set_state(x0, lp0, ll0, t_before)
        ref.summary_begin()
        ref.advance(kg, nt, summary=True)
        assert so.mismatches(got, _asdict(ref.summary())) == []
        # the handle keeps working, and so does its summary
        ens.advance(3, nt, summary=True)
        ref.advance(3, nt, summary=True)
        assert so.mismatches(ens.summary(), _asdict(ref.summary())) == []
        assert ens.summary().n == N * (kg + 3)
        ref.close()
        ens.close()
    finally:
        ctx.close()


def test_cancel_small_driver(k):
    # <= 80 000 generations of 50 x 2 doubles: one launch block, left early by the kernel itself
    _cancel_case(k, _box(k, 2, k.costs.GaussDist([1.0, -0.5])), 50, 64, 500, "small", max_gens=80000)


def test_cancel_half_generation_course(k):
    _cancel_case(k, _box(k, 8), 65536, 100, 20, "halves")


# ---- recycled memory -------------------------------------------------------------------------------

def test_accumulators_are_zeroed_not_assumed_zero(k):
    """begin -> advance -> end -> begin on one handle takes the first summary's buffers back from the
    context's pool, dirty; so does a second handle on the context.  Both give the bits of a first run."""
    model, N, nt = _box(k, 3), 641, 1
    ctx = k.Context(0)
    try:
        tr = _trace(k, model, N, 12, nt, seed=2, ctx=ctx)
        first = so.summarize(tr[:5])
        e = k.AisEnsemble(model, N, seed=2, ctx=ctx).init()
        e.summary_begin()
        e.advance(5, nt, summary=True)
        assert so.mismatches(e.summary(), first) == []
        e.summary_end()
        e.summary_begin()
        e.advance(7, nt, summary=True)
        assert so.mismatches(e.summary(), so.summarize(tr[5:])) == []
        e.summary_begin("diag")                              # (begin again, another layout in the same buffers)
        e.close()
        e2 = k.AisEnsemble(model, N, seed=2, ctx=ctx).init()
        e2.summary_begin()
        e2.advance(5, nt, summary=True)
        assert so.mismatches(e2.summary(), first) == []
        e2.close()
    finally:
        ctx.close()
