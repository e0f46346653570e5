"""GPU: user-defined derived quantities g(θ) of a summarised AIS trace on the device (kabc_compile_derived,
kabc_derived_eval, kabc_ais_derived_begin; Derived, summary_begin(derived=...), sample(..., derived=...)).

The snippets are made of + - * /, comparisons and constants and are compiled without contraction, so every
value has one fp64 result: d(theta) is compared BIT FOR BIT with the numpy restatements of
tests/ais_derived_oracle.py, and the derived summary with the composed oracle -- the summary, autocorrelation
and histogram oracles applied to restatement(trace) of the collect=True trace of a twin handle.  The identity
snippet needs no oracle: its derived summary must equal the parameters' own in every field."""
import ctypes as C
import threading
import time

import numpy as np
import pytest

import ais_autocorr_oracle as ao
import ais_derived_oracle as do
import ais_summary_oracle as so

pytestmark = pytest.mark.gpu

ALL_FIELDS = tuple(so.FIELDS) + tuple(ao.AC_FIELDS.values()) + ("tau_converged",)


def _box(k, D, cost=None):
    return k.ApproxKernelizedPosterior(k.Factored(*[k.Uniform(-5, 5)] * D), cost or k.costs.Rosenbrock(), 1.0)


def _gauss2(k):
    return _box(k, 2, k.costs.GaussDist([1.0, -0.5]))


def _d20(k):
    return k.ApproxKernelizedPosterior(k.Factored(*[k.Normal(0, 3)] * 20), k.costs.GaussDist(np.zeros(20)), 1.0)


def _derived(k, name, G=None, **kw):
    src, D, G0, params, _ = do.SNIPPETS[name]
    return k.Derived(src, G0 or G, params=params, **kw)


def _same(a, b, fields, equal_nan=True):
    """the fields in which two PosteriorSummary differ bit for bit (a NaN equals a NaN)"""
    bad = []
    for f in fields:
        x, y = getattr(a, f), getattr(b, f)
        if f == "n":
            if x != y:
                bad.append(f)
            continue
        x, y = np.asarray(x), np.asarray(y)
        if x.shape != y.shape or not np.array_equal(x, y, equal_nan=equal_nan and x.dtype.kind == "f"):
            bad.append(f)
    return bad


def _summary(k, model, N, gens, nt, derived=None, driver=None, autocorr=None, hist=None, pieces=None, **kw):
    e = k.AisEnsemble(model, N, **kw).init()
    if driver is not None:
        assert e.driver == driver
    e.summary_begin(autocorr=autocorr, hist=hist, derived=derived)
    for g in (pieces or (gens,)):
        assert e.advance(g, nt, summary=True) is None
    s = e.summary()
    e.close()
    return s


_TR = {}


def _trace(k, name, model, N, gens, nt, seed=5):
    """the collect=True trace of a twin handle, computed once per shape and left unchanged"""
    if name not in _TR:
        e = k.AisEnsemble(model, N, seed=seed).init()
        tr = e.advance(gens, nt, collect=True)
        e.close()
        tr.setflags(write=False)
        _TR[name] = tr
    return _TR[name]


# ---- d(theta) ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["A", "C", "D"])
def test_eval_equals_the_restatement_across_launch_sizes(k, gpu_ctx, monkeypatch, name):
    src, D, G, params, _ = do.SNIPPETS[name]
    d = _derived(k, name)
    rng = np.random.default_rng(ord(name))
    x = rng.normal(0.0, 2.0, size=(389, D))
    x[3] = 0.0
    x[5, 0] = x[5, 1]                                            # (x0 > x1 is false on a tie)
    want = do.restate(name, x)
    got = d(x)
    assert got.shape == (389, G) and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    monkeypatch.setenv("KABC_EVAL_ROWS", "64")                   # 7 launches, the last of 5 rows
    assert np.array_equal(d(x).view(np.uint64), want.view(np.uint64))
    monkeypatch.setenv("KABC_EVAL_ROWS", "1")
    assert np.array_equal(d(x[:9]).view(np.uint64), want[:9].view(np.uint64))
    monkeypatch.delenv("KABC_EVAL_ROWS")
    assert np.array_equal(d(x[100:237]), want[100:237]) and np.array_equal(d(x[7]), want[7])
    for path in ("lds", "direct"):                               # either form of the kernel by name: the same bits
        monkeypatch.setenv("KABC_DERIVED_PATH", path)
        assert np.array_equal(d(x).view(np.uint64), want.view(np.uint64)), path


def test_eval_on_a_sampled_trace_keeps_the_leading_axes(k):
    tr = _trace(k, "gauss2-100", _gauss2(k), 100, 25, 2)
    d = _derived(k, "A")
    g = d(tr)
    assert g.shape == (25, 100, 3) and np.array_equal(g, do.restate("A", tr))
    x = k.sample(_gauss2(k), k.AIS(100), 700, ntransitions=2, seed=5, return_array=True)
    assert np.array_equal(d(x), do.restate("A", x)) and np.array_equal(x, tr.reshape(-1, 2)[:700])


# ---- the identity: the derived set is the parameters' set ------------------------------------------------

@pytest.mark.parametrize("N,gens,driver", [(100, 25, "small"), (641, 30, "halves")])
def test_identity_snippet_gives_the_parameter_summary_in_every_field(k, monkeypatch, N, gens, driver):
    if driver == "halves":
        monkeypatch.setenv("KABC_TRACE_CHUNK_MIB", "1")          # 10 256 B per generation at D = 2: several chunks
        monkeypatch.setenv("KABC_DERIVED_MIB", "1")
    lo, hi = [-5.0, -4.0], [5.0, 4.5]
    d = _derived(k, "B", G=2, hist_range=(lo, hi))
    s = _summary(k, _gauss2(k), N, gens, 2, d, driver=driver, autocorr=8, hist=(lo, hi, 7), seed=5)
    assert s.derived is not None and s.derived.names == ("g0", "g1") and s.names is None
    assert _same(s, s.derived, ALL_FIELDS + ("hist", "underflow", "overflow", "edges", "median")) == []
    assert s.derived.n == gens * N and not s.derived.diag and s.derived.nbins == 7
    assert np.array_equal(s.derived.quantile([0.1, 0.9]), s.quantile([0.1, 0.9]))


@pytest.mark.parametrize("N,driver", [(100, "small"), (641, "halves")])
def test_both_forms_of_the_map_kernel_fold_to_the_same_bits(k, monkeypatch, N, driver):
    d = _derived(k, "A", hist_range=(-30.0, 30.0))
    got = {}
    for path in ("direct", "lds"):
        monkeypatch.setenv("KABC_DERIVED_PATH", path)
        got[path] = _summary(k, _gauss2(k), N, 25, 2, d, driver=driver, autocorr=4, hist=16, seed=5)
    assert _same(got["direct"].derived, got["lds"].derived, ALL_FIELDS + ("hist", "underflow", "overflow")) == []
    if N == 100:
        tr = _trace(k, "gauss2-100", _gauss2(k), 100, 25, 2)
        assert do.mismatches(got["direct"].derived, do.summarize("A", tr, L=4, hist=(-30.0, 30.0, 16)), L=4,
                             hist=(-30.0, 30.0, 16)) == []


# ---- snippet A against the composed oracle, on both drivers ----------------------------------------------

def test_snippet_a_against_the_composed_oracle_on_both_drivers(k, monkeypatch):
    model, N, gens, nt, L, B = _gauss2(k), 100, 25, 2, 8, 16
    tr = _trace(k, "gauss2-100", model, N, gens, nt)
    rng_d = ([-30.0, -6.0, -0.5], [30.0, 6.0, 1.5])
    d = _derived(k, "A", hist_range=rng_d, names=["prod", "ratio", "first_larger"])
    want = do.summarize("A", tr, L=L, hist=(*rng_d, B))
    plain = _summary(k, model, N, gens, nt, None, driver="small", autocorr=L, hist=B, seed=5)
    got = {}
    for driver in ("small", "halves"):
        if driver == "halves":
            monkeypatch.setenv("KABC_AIS_SMALL", "0")
        s = got[driver] = _summary(k, model, N, gens, nt, d, driver=driver, autocorr=L, hist=B, seed=5)
        assert do.mismatches(s.derived, want, L=L, hist=(*rng_d, B)) == [], driver
        assert s.derived.names == ("prod", "ratio", "first_larger") and s.derived.cov.shape == (3, 3)
        # the parameters' summary is that of a call without derived=
        assert _same(s, plain, ALL_FIELDS + ("hist", "underflow", "overflow", "edges")) == [], driver
        assert plain.derived is None
        # the indicator's mean is the fraction of rows with x0 > x1, its histogram two spikes
        frac = np.count_nonzero(tr[..., 0] > tr[..., 1]) / s.n
        assert abs(s.derived.mean[2] - frac) < 1e-12 and s.derived.hist[2].sum() == s.n
    assert _same(got["small"].derived, got["halves"].derived,
                 ALL_FIELDS + ("hist", "underflow", "overflow", "edges")) == []


def test_automatic_derived_range_is_the_convention_on_d_of_the_walkers(k):
    from kissabc_jl_amd.api import _hist_auto_range
    model, N, gens, nt = _gauss2(k), 100, 25, 2
    tr = _trace(k, "gauss2-100", model, N, gens, nt)
    d = _derived(k, "A")
    e = k.AisEnsemble(model, N, seed=5).init()
    lo, hi = _hist_auto_range(do.restate("A", e.state()[0]))
    e.summary_begin(hist=16, derived=d)
    e.advance(gens, nt, summary=True)
    s = e.summary()
    e.close()
    assert do.mismatches(s.derived, do.summarize("A", tr, hist=(lo, hi, 16)), hist=(lo, hi, 16)) == []
    assert np.array_equal(s.derived.histogram["lo"], lo) and np.array_equal(s.derived.histogram["hi"], hi)


# ---- splitting --------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,driver", [(100, "small"), (641, "halves")])
def test_split_over_calls_blocks_and_the_derived_buffer(k, monkeypatch, N, driver):
    model, gens, nt, L, B = _box(k, 8), 70, 1, 8, 16
    d = _derived(k, "B", G=8, hist_range=(-5.0, 5.0))
    kw = dict(derived=d, driver=driver, autocorr=L, hist=(-5.0, 5.0, B), seed=8)
    whole = _summary(k, model, N, gens, nt, **kw)
    fields = ALL_FIELDS + ("hist", "underflow", "overflow")
    assert _same(whole, whole.derived, fields) == []
    # three advance calls
    s = _summary(k, model, N, gens, nt, pieces=(7, 1, 62), **kw)
    assert _same(s.derived, whole.derived, fields) == [] and _same(s, whole, fields) == []
    # the device trace buffer at its smallest, 1 MiB: at N = 641 (41 024 B per generation) chunks of 25, 25 and
    # 20; at N = 100 the 70 generations still fit one block -- the one-workgroup driver's three blocks are
    # test_small_driver_three_blocks_of_the_device_buffer's, at N = 512
    monkeypatch.setenv("KABC_TRACE_CHUNK_MIB", "1")
    s = _summary(k, model, N, gens, nt, **kw)
    assert _same(s.derived, whole.derived, fields) == []
    monkeypatch.delenv("KABC_TRACE_CHUNK_MIB")
    # the derived buffer's own cap forced small: sub-blocks of whole generations inside one trace block
    monkeypatch.setenv("KABC_DERIVED_MIB", "1")
    d17 = _derived(k, "D")
    model2 = _gauss2(k)
    a = _summary(k, model2, N, 200, 1, d17, driver=driver, autocorr=4, seed=8)        # 200 generations x N x 17 x 8 B > 1 MiB
    monkeypatch.delenv("KABC_DERIVED_MIB")
    b = _summary(k, model2, N, 200, 1, d17, driver=driver, autocorr=4, seed=8)
    assert 200 * N * 17 * 8 > 2 * (1 << 20)
    assert _same(a.derived, b.derived, ALL_FIELDS) == [] and a.derived.diag


def test_small_driver_three_blocks_of_the_device_buffer(k, monkeypatch):
    monkeypatch.setenv("KABC_TRACE_CHUNK_MIB", "1")              # 32 KiB per generation: blocks of 32, 32 and 6
    model, N, gens = _box(k, 8), 512, 70
    d = _derived(k, "B", G=8)
    s = _summary(k, model, N, gens, 1, d, driver="small", autocorr=8, seed=5)
    assert _same(s, s.derived, ALL_FIELDS) == [] and s.n == gens * N
    monkeypatch.delenv("KABC_TRACE_CHUNK_MIB")
    one = _summary(k, model, N, gens, 1, d, driver="small", autocorr=8, seed=5)
    assert _same(s.derived, one.derived, ALL_FIELDS) == []


def test_cancel_small_driver(k):
    """the one-workgroup kernel leaves its block early and only the device knows how many generations ran: the
    map and the derived folds take exactly those"""
    model, N, nt, L = _gauss2(k), 50, 64, 4
    rng_d = ([-30.0, -6.0, -0.5], [30.0, 6.0, 1.5])
    d = _derived(k, "A", hist_range=rng_d)
    ctx = k.Context(0)
    try:
        ens = k.AisEnsemble(model, N, seed=11, ctx=ctx).init()
        assert ens.driver == "small"
        ens.summary_begin(autocorr=L, hist=16, derived=d)
        t0 = time.perf_counter()
        ens.advance(500, nt, summary=True)
        dt = (time.perf_counter() - t0) / 500
        G = min(max(int(5.0 / dt), 2), 80000)               # ~5 s if the cancel were ignored; one launch block
        ens.summary_begin(autocorr=L, hist=16, derived=d)    # (starts over)
        x0, lp0, ll0, t_before = ens.state()
        tm = threading.Timer(0.3, ctx.cancel)
        tm.start()
        with pytest.raises(k.Cancelled):
            ens.advance(G, nt, summary=True)
        tm.join()
        kg = (ens.state()[3] - t_before) // nt
        assert 0 < kg < G, (kg, G)
        got = ens.summary()
        assert got.n == N * kg and got.derived.n == got.n
        ref = k.AisEnsemble(model, N, seed=11, ctx=ctx)
        ref.set_state(x0, lp0, ll0, t_before)
        tr = ref.advance(kg, nt, collect=True)
        assert do.mismatches(got.derived, do.summarize("A", tr, L=L, hist=(*rng_d, 16)), L=L, hist=(*rng_d, 16)) == []
        ens.advance(3, nt, summary=True)                     # the handle keeps working, and so does the derived set
        tr = np.concatenate([tr, ref.advance(3, nt, collect=True)])
        assert do.mismatches(ens.summary().derived, do.summarize("A", tr, L=L, hist=(*rng_d, 16)), L=L,
                             hist=(*rng_d, 16)) == []
        ref.close()
        ens.close()
    finally:
        ctx.close()


# ---- beyond 16 on either side --------------------------------------------------------------------------

def test_snippet_c_twenty_parameters_one_derived_value(k):
    model, N, gens, nt = _d20(k), 64, 12, 2
    tr = _trace(k, "d20", model, N, gens, nt)
    d = _derived(k, "C", hist_range=(0.0, 400.0))
    s = _summary(k, model, N, gens, nt, d, autocorr=4, hist=9, seed=5)
    assert s.diag and s.cov.shape == (20,) and not s.derived.diag and s.derived.cov.shape == (1, 1)
    assert do.mismatches(s.derived, do.summarize("C", tr, L=4, hist=(0.0, 400.0, 9)), L=4, hist=(0.0, 400.0, 9)) == []


def test_snippet_d_seventeen_derived_values_variances_and_two_slabs(k):
    model, N, gens, nt = _gauss2(k), 100, 25, 2
    tr = _trace(k, "gauss2-100", model, N, gens, nt)
    lo, hi = np.linspace(-6.0, -40.0, 17), np.linspace(6.0, 40.0, 17)
    d = _derived(k, "D", hist_range=(lo, hi))
    for B in (9, 1024):
        s = _summary(k, model, N, gens, nt, d, autocorr=4, hist=B, seed=5)
        assert not s.diag and s.derived.diag and s.derived.cov.shape == (17,) and s.derived.hist.shape == (17, B)
        assert do.mismatches(s.derived, do.summarize("D", tr, L=4, hist=(lo, hi, B)), L=4, hist=(lo, hi, B)) == []
    assert _same(s, _summary(k, model, N, gens, nt, None, autocorr=4, hist=B, seed=5), ALL_FIELDS + ("hist",)) == []


# ---- batch handles, MCMCThreads ----------------------------------------------------------------------

def test_batch_handle_with_per_chain_costs_each_chain_is_its_own_run(k):
    from kissabc_jl_amd.api import _hist_auto_range, chain_seeds
    seeds, N, gens, nt = chain_seeds(3, 3), 12, 20, 2
    costs = [k.costs.GaussDist([1.0, -0.5]), k.costs.GaussDist([-2.0, 0.0]), k.costs.GaussDist([0.0, 3.0])]
    d = _derived(k, "A")
    both = _summary(k, _box(k, 2, costs[0]), N, gens, nt, d, autocorr=4, hist=16, seeds=seeds, costs=costs)
    assert both.nchains == 3 and both.derived.nchains == 3 and both.derived.mean.shape == (3, 3)
    assert both.derived.hist.shape == (3, 3, 16)
    for c, sd in enumerate(seeds):
        model = _box(k, 2, costs[c])
        one = _summary(k, model, N, gens, nt, d, autocorr=4, hist=16, seed=sd)
        fields = ALL_FIELDS + ("hist", "underflow", "overflow", "edges")
        assert _same(both.chain(c).derived, one.derived, fields) == [], c
        assert _same(both.chain(c), one, fields) == [], c
        e = k.AisEnsemble(model, N, seed=sd).init()
        lo, hi = _hist_auto_range(do.restate("A", e.state()[0]))           # the convention on d(state), per chain
        tr = e.advance(gens, nt, collect=True)
        e.close()
        assert np.array_equal(both.derived.histogram["lo"][c], lo) and np.array_equal(both.derived.histogram["hi"][c], hi)
        assert do.mismatches(both.chain(c).derived, do.summarize("A", tr, L=4, hist=(lo, hi, 16)), L=4,
                             hist=(lo, hi, 16)) == [], c
    out = k.sample_batch([_box(k, 2, c) for c in costs], k.AIS(N), gens * N, seeds=seeds, ntransitions=nt, summary=True,
                         autocorr=4, hist=16, derived=d)
    assert out.info["course"] == "grid"
    for c in range(3):
        assert _same(out[c].derived, both.chain(c).derived, ALL_FIELDS + ("hist",)) == [], c


def test_mcmcthreads_pools_the_derived_set_with_the_parameters_code(k):
    from kissabc_jl_amd.api import _pool_summaries, _rhat
    model, N, Nc, gk = _gauss2(k), 50, 3, 20
    d = _derived(k, "A", hist_range=(-30.0, 30.0))
    kw = dict(ntransitions=2, seed=9)
    cs = k.sample(model, k.AIS(N), k.MCMCThreads(), gk * N, Nc, summary=True, hist=16, derived=d, **kw)
    x = k.sample(model, k.AIS(N), k.MCMCThreads(), gk * N, Nc, return_array=True, **kw).reshape(Nc, gk, N, 2)
    for c in range(Nc):
        assert do.mismatches(cs[c].derived, do.summarize("A", x[c], hist=(-30.0, 30.0, 16)), hist=(-30.0, 30.0, 16)) == [], c
    ders = [c.derived for c in cs]
    want = _pool_summaries(ders)
    assert cs.pooled.derived.n == Nc * gk * N and cs.pooled.derived.names == d.names
    assert _same(cs.pooled.derived, want, ("n", "mean", "cov", "min", "max", "hist")) == []
    assert np.array_equal(cs.derived.rhat, _rhat(ders)) and cs.derived.rhat.shape == (3,)
    # the host formulas themselves, on the per-chain values
    g = do.restate("A", x)                                           # [Nc][gk][N][3]
    flat = g.reshape(Nc * gk * N, 3)
    assert np.allclose(cs.pooled.derived.mean, flat.mean(axis=0), rtol=1e-12, atol=1e-13)
    assert np.allclose(cs.pooled.derived.cov, np.cov(flat.T), rtol=1e-10, atol=1e-13)
    n = gk * N
    means, W = np.stack([c.mean for c in ders]), np.mean(np.stack([c.var for c in ders]), axis=0)
    assert np.allclose(cs.derived.rhat, np.sqrt(((n - 1) / n * W + np.var(means, axis=0, ddof=1)) / W), rtol=1e-13)
    assert np.array_equal(cs.pooled.derived.hist, np.sum([c.hist for c in ders], axis=0).astype(np.uint64))


# ---- values that are not finite ------------------------------------------------------------------------

def test_snippet_e_nan_and_infinities_go_where_the_kernels_send_them(k):
    model, N, gens, nt = _gauss2(k), 100, 25, 2
    tr = _trace(k, "gauss2-100", model, N, gens, nt)
    hist = (-5.0, 5.0, 8)
    d = _derived(k, "E", hist_range=hist[:2])
    s = _summary(k, model, N, gens, nt, d, autocorr=4, hist=8, seed=5)
    want = do.summarize("E", tr, L=4, hist=hist)
    assert do.mismatches(s.derived, want, L=4, hist=hist, equal_nan=True) == []
    g = want["g"]
    npos = np.count_nonzero(tr[..., 0] > 0)
    assert 0 < npos < s.n
    der = s.derived
    assert der.overflow[1] == npos and der.underflow[1] == s.n - npos and der.hist[1].sum() == 0   # +inf / -inf
    assert der.overflow[0] == np.count_nonzero(np.isnan(g[..., 0]) | (g[..., 0] >= 5.0))            # every NaN
    assert np.all(der.hist.sum(axis=1) + der.underflow + der.overflow == s.n)
    assert np.isnan(der.mean[0]) and np.isnan(der.mean[1]) and np.all(np.isnan(der.cov))
    # the parameters of the same call are untouched by it
    assert _same(s, _summary(k, model, N, gens, nt, None, autocorr=4, hist=8, seed=5), ALL_FIELDS + ("hist",)) == []
    assert np.all(np.isfinite(s.mean)) and np.all(np.isfinite(s.cov))


# ---- recycled memory, refusals ---------------------------------------------------------------------------

def test_recycled_derived_buffers_start_from_zero(k):
    model, N, nt, L = _box(k, 3), 641, 1, 4
    src = do.SRC_B
    ctx = k.Context(0)
    try:
        d = k.Derived(src, 3, hist_range=(-5.0, 5.0))
        e = k.AisEnsemble(model, N, seed=2, ctx=ctx).init()
        tr = e.advance(12, nt, collect=True)
        e.close()
        hist = (-5.0, 5.0, 60)

        def check(s, part):
            want = do.summarize("B", part, L=L, hist=hist)
            assert do.mismatches(s.derived, want, L=L, hist=hist) == []

        e = k.AisEnsemble(model, N, seed=2, ctx=ctx).init()
        e.summary_begin(autocorr=L, hist=hist, derived=d)
        e.advance(5, nt, summary=True)
        check(e.summary(), tr[:5])
        e.summary_end()                                      # (every buffer of the set goes back to the pool, dirty)
        e.summary_begin(autocorr=L, hist=hist, derived=d)
        e.advance(7, nt, summary=True)
        check(e.summary(), tr[5:])
        e.summary_begin(autocorr=L, hist=hist, derived=d)    # (begin again without an end)
        e.summary_begin()                                    # (starts over WITHOUT the derived set)
        assert e.advance(0, nt, summary=True) is None
        assert k._lib.load().kabc_ais_derived_summary_get(e._h, *([None] * 8)) != 0
        e.close()
        e2 = k.AisEnsemble(model, N, seed=2, ctx=ctx).init()
        e2.summary_begin(autocorr=L, hist=hist, derived=d)
        e2.advance(5, nt, summary=True)
        check(e2.summary(), tr[:5])
        e2.close()
    finally:
        ctx.close()


def test_refusals_on_a_live_handle(k):
    from kissabc_jl_amd import _cdefs as cd
    lib = k._lib.load()
    p = lambda a: a.ctypes.data_as(cd.c_double_p)           # noqa: E731
    d = _derived(k, "A")
    par = np.array([0.25])
    lo, hi = np.full(3, -5.0), np.full(3, 5.0)
    begin = lambda G=3, nb=0, lo_=None, hi_=None, id=d.id, L=0, cov=0: lib.kabc_ais_derived_begin(   # noqa: E731
        e._h, id, G, p(par), 1, cov, L, nb, lo_, hi_)
    err = lambda: lib.kabc_last_error()                     # noqa: E731
    e = k.AisEnsemble(_gauss2(k), 30, seed=1).init()
    assert begin() == cd.KABC_ERR_INVALID_STATE and b"no summary is open" in err()
    for get in (lambda: lib.kabc_ais_derived_summary_get(e._h, *([None] * 8)),
                lambda: lib.kabc_ais_derived_autocorr_get(e._h, *([None] * 10)),
                lambda: lib.kabc_ais_derived_hist_get(e._h, None, None, None, None)):
        assert get() == cd.KABC_ERR_INVALID_STATE and b"no summary is open" in err()
    e.summary_begin()
    for get, who in ((lambda: lib.kabc_ais_derived_summary_get(e._h, *([None] * 8)), b"kabc_ais_derived_summary_get"),
                     (lambda: lib.kabc_ais_derived_autocorr_get(e._h, *([None] * 10)), b"kabc_ais_derived_autocorr_get"),
                     (lambda: lib.kabc_ais_derived_hist_get(e._h, None, None, None, None), b"kabc_ais_derived_hist_get")):
        assert get() == cd.KABC_ERR_INVALID_STATE
        assert who in err() and b"no derived set is open" in err()
    for G in (0, -1, 257):
        assert begin(G=G) == cd.KABC_ERR_INVALID_ARG and b"outside 1..256" in err()
    assert begin(nb=8) == cd.KABC_ERR_INVALID_ARG and b"lo and hi must be non-NULL" in err()
    assert begin(nb=8, lo_=p(lo)) == cd.KABC_ERR_INVALID_ARG
    assert begin(id=0) == cd.KABC_ERR_INVALID_ARG and b"not a registered" in err()
    assert begin(L=-1) == cd.KABC_ERR_INVALID_ARG and begin(L=cd.KABC_AUTOCORR_MAX_LAG + 1) == cd.KABC_ERR_INVALID_ARG
    assert begin(G=17, cov=cd.SUMMARY_FULL) == cd.KABC_ERR_UNSUPPORTED and b"derived values" in err()
    bad_hi = hi.copy()
    bad_hi[2] = -5.0
    assert begin(nb=8, lo_=p(lo), hi_=p(bad_hi)) == cd.KABC_ERR_INVALID_ARG and b"chain 0, derived value 2" in err()
    assert lib.kabc_ais_derived_summary_get(e._h, *([None] * 8)) == cd.KABC_ERR_INVALID_STATE    # none of them opened one
    assert begin(nb=8, lo_=p(lo), hi_=p(hi)) == cd.KABC_OK
    mean = np.full(3, 99.0)
    assert lib.kabc_ais_derived_summary_get(e._h, None, None, None, None, p(mean), None, None,
                                            None) == cd.KABC_ERR_INVALID_STATE                    # nothing folded yet
    assert b"n = 0" in err() and np.all(mean == 99.0)
    assert lib.kabc_ais_derived_autocorr_get(e._h, *([None] * 10)) == cd.KABC_ERR_INVALID_STATE
    assert b"maxlag > 0" in err()                                                              # opened without it
    e._summary_derived, e._summary_hist = d, 0
    e.advance(3, 1, summary=True)
    n = C.c_int64()
    assert lib.kabc_ais_derived_summary_get(e._h, C.byref(n), None, None, None, p(mean), None, None, None) == cd.KABC_OK
    assert n.value == 90 and np.all(mean != 99.0)
    assert begin() == cd.KABC_ERR_INVALID_STATE and b"already holds" in err()                   # after a fold
    e.summary_end()
    assert lib.kabc_ais_derived_summary_get(e._h, *([None] * 8)) == cd.KABC_ERR_INVALID_STATE
    e.close()
