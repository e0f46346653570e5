"""CPU: the parts of the derived quantities g(θ) that need no device -- Derived's own validation, the refusals of
derived= outside a summary, kabc_compile_derived (hipRTC is a compiler: it runs without a GPU, as the cost
plugin's registration test does), kabc_derived_eval's argument checks, and the numpy restatements of the test
snippets (tests/ais_derived_oracle.py) against rows computed by hand."""
import ctypes as C

import numpy as np
import pytest

import ais_derived_oracle as do


def _model(k, D=2):
    return k.ApproxKernelizedPosterior(k.Factored(*[k.Uniform(-5, 5)] * D), k.costs.GaussDist([1.0, -0.5][:D]), 1.0)


# ---- Derived ---------------------------------------------------------------------------------------

def test_derived_keeps_what_it_is_given(k):
    d = k.Derived(do.SRC_A, 3, params=[0.25], names=["prod", "ratio", "first_larger"], hist_range=(-1.0, [1.0, 2.0, 3.0]))
    assert d.G == 3 and d.names == ("prod", "ratio", "first_larger") and d.id >= 1
    assert d.params.dtype == np.float64 and d.params.tolist() == [0.25]
    assert d.hist_range[0].tolist() == [-1.0] * 3 and d.hist_range[1].tolist() == [1.0, 2.0, 3.0]
    assert k.Derived(do.SRC_A, 3, params=[0.5]).id == d.id         # (the same snippet is the same map)
    assert k.Derived(do.SRC_B, 2).names == ("g0", "g1") and k.Derived(do.SRC_B, 2).hist_range is None
    assert "ratio" in repr(d)


@pytest.mark.parametrize("G", [0, -1, 257, 2.0, "3", None, True])
def test_derived_refuses_a_bad_G(k, G):
    with pytest.raises(ValueError, match="G must be an int in 1 ... 256"):
        k.Derived(do.SRC_A, G, params=[0.25])


def test_derived_refuses_bad_params_names_and_source(k):
    with pytest.raises(ValueError, match="params must be a sequence of numbers"):
        k.Derived(do.SRC_A, 3, params=["c"])
    with pytest.raises(ValueError, match="flat sequence"):
        k.Derived(do.SRC_A, 3, params=[[1.0, 2.0], [3.0, 4.0]])
    with pytest.raises(ValueError, match="names must be 3 strings"):
        k.Derived(do.SRC_A, 3, params=[0.25], names=["a", "b"])
    with pytest.raises(ValueError, match="names must be 3 strings"):
        k.Derived(do.SRC_A, 3, params=[0.25], names=["a", "b", 3])
    with pytest.raises(ValueError, match="source must be the C text"):
        k.Derived("  ", 3)


@pytest.mark.parametrize("rng,msg", [
    ((0.0,), r"None or \(lo, hi\)"), (5.0, r"None or \(lo, hi\)"),
    (([0.0, 0.0], 1.0), r"lo must be a scalar or \[G\] = \[3\]"),
    ((0.0, np.inf), "hi must be finite"), ((np.nan, 1.0), "lo must be finite"),
    ((0.0, [1.0, 0.0, 1.0]), "derived value 1: lo = 0.0 is not below hi = 0.0"),
    (("a", 1.0), "lo must be a scalar"),
])
def test_derived_refuses_a_bad_hist_range(k, rng, msg):
    with pytest.raises(ValueError, match=msg):
        k.Derived(do.SRC_A, 3, params=[0.25], hist_range=rng)


# ---- derived= needs a summary ------------------------------------------------------------------------

def test_derived_without_summary_is_refused_before_anything_runs(k):
    d = k.Derived(do.SRC_A, 3, params=[0.25])
    for call in (lambda **kw: k.sample(_model(k), k.AIS(10), 100, **kw),
                 lambda **kw: k.sample(_model(k), k.AIS(10), k.MCMCThreads(), 100, 2, **kw),
                 lambda **kw: k.sample_batch(_model(k), k.AIS(10), 100, nruns=2, **kw)):
        with pytest.raises(ValueError, match="derived= needs summary=True"):
            call(derived=d)
        with pytest.raises(ValueError, match="derived= needs summary=True"):
            call(derived=d, return_array=True)
        with pytest.raises(TypeError, match="derived must be a Derived"):
            call(derived=do.SRC_A, summary=True)


def test_derived_on_a_sharded_ensemble_says_why(k):
    from kissabc_jl_amd.api import _derived_check
    d = k.Derived(do.SRC_A, 3, params=[0.25])
    with pytest.raises(ValueError, match="sharded ensemble has no streamed trace"):
        _derived_check(d, "summary_begin", sharded=True)
    _derived_check(None, "sample", summary=False)                   # (no derived: nothing to refuse)


def test_summary_classes_carry_the_derived_set(k):
    """PosteriorSummary.chain and ChainSummaries pass the derived set through the code that serves the parameters"""
    from kissabc_jl_amd.api import ChainSummaries, PosteriorSummary, _pool_summaries, _rhat
    rng = np.random.default_rng(3)

    def one(D, shift):
        x = rng.normal(shift, 1.0, size=(40, D))
        return PosteriorSummary(40, x.mean(axis=0), np.cov(x.T).reshape(D, D), x.min(axis=0), x.max(axis=0))

    chains = []
    for c in range(3):
        s = one(2, c)
        s.derived = one(3, -c)
        s.derived.names = ("a", "b", "c")
        chains.append(s)
    cs = ChainSummaries(chains)
    ders = [c.derived for c in chains]
    assert cs.pooled.derived is cs.derived.pooled and cs.pooled.derived.names == ("a", "b", "c")
    want = _pool_summaries(ders)
    assert np.array_equal(cs.pooled.derived.mean, want.mean) and np.array_equal(cs.pooled.derived.cov, want.cov)
    assert cs.pooled.derived.n == 120 and np.array_equal(cs.derived.rhat, _rhat(ders)) and cs.derived.rhat.shape == (3,)
    assert cs.rhat.shape == (2,)
    plain = ChainSummaries([one(2, 0), one(2, 1)])
    assert plain.derived is None and plain.pooled.derived is None
    both = PosteriorSummary(40, np.zeros((2, 2)), np.zeros((2, 2, 2)), np.zeros((2, 2)), np.zeros((2, 2)))
    both.derived = PosteriorSummary(40, np.arange(6.0).reshape(2, 3), np.zeros((2, 3, 3)), np.zeros((2, 3)),
                                    np.zeros((2, 3)))
    both.derived.names = ("a", "b", "c")
    assert both.chain(1).derived.mean.tolist() == [3.0, 4.0, 5.0] and both.chain(1).derived.names == ("a", "b", "c")


# ---- kabc_compile_derived, kabc_derived_eval ---------------------------------------------------------

def test_compile_derived_checks_the_snippet_at_once(k):
    from kissabc_jl_amd import _cdefs as cd
    lib = k._lib.load()
    out = C.c_int32(-7)
    assert lib.kabc_compile_derived(do.SRC_C.encode(), C.byref(out)) == cd.KABC_OK and out.value >= 1
    good = out.value
    assert lib.kabc_compile_derived(do.SRC_C.encode(), C.byref(out)) == cd.KABC_OK and out.value == good
    # a snippet that lacks the function
    out = C.c_int32(-7)
    st = lib.kabc_compile_derived(b"KABC_HD void kabc_user_derive(const double* x, double* g) { g[0] = x[0]; }\n",
                                  C.byref(out))
    assert st == cd.KABC_ERR_INVALID_ARG and out.value == -7
    assert b"kabc_user_derived" in lib.kabc_last_error() and b"undeclared" in lib.kabc_last_error()
    # a syntax error: the compiler's message, with the line
    st = lib.kabc_compile_derived(do.SRC_A.replace("x[0] * x[1];", "x[0] * x[1]").encode(), C.byref(out))
    assert st == cd.KABC_ERR_INVALID_ARG and out.value == -7
    assert b"expected ';'" in lib.kabc_last_error()
    with pytest.raises(k.KabcError, match="expected ';'"):
        k.Derived(do.SRC_A.replace("x[0] * x[1];", "x[0] * x[1]"), 3)
    # a wrong signature is a compile error too: the function is called the way the kernel calls it
    st = lib.kabc_compile_derived(b"KABC_HD void kabc_user_derived(const double* x, double* g) { g[0] = x[0]; }\n",
                                  C.byref(out))
    assert st == cd.KABC_ERR_INVALID_ARG
    assert lib.kabc_compile_derived(None, C.byref(out)) == cd.KABC_ERR_INVALID_ARG
    assert lib.kabc_compile_derived(do.SRC_C.encode(), None) == cd.KABC_ERR_INVALID_ARG


@pytest.mark.parametrize("name", sorted(do.SNIPPETS))
def test_map_kernel_compiles_with_every_test_snippet(k, name):
    """The kernel itself, from the library's own headers under hipRTC (no system headers there): on a box
    without a GPU the code object is produced and only its load fails; with one it loads."""
    from kissabc_jl_amd import _cdefs as cd
    lib = k._lib.load()
    src, D, G, params, _ = do.SNIPPETS[name]
    d = k.Derived(src, G or 8, params=params)
    st = lib.kabc_derived_precompile(d.id)
    msg = lib.kabc_last_error().decode()
    assert st == cd.KABC_OK or (st == cd.KABC_ERR_DEVICE and "the kernels compiled (" in msg), msg[:2000]
    assert lib.kabc_derived_precompile(0) == cd.KABC_ERR_INVALID_ARG


def test_derived_eval_argument_checks_need_no_device(k):
    from kissabc_jl_amd import _cdefs as cd
    lib = k._lib.load()
    d = k.Derived(do.SRC_A, 3, params=[0.25])
    x, out, par = np.zeros((4, 2)), np.zeros((4, 3)), np.array([0.25])
    p = lambda a: a.ctypes.data_as(cd.c_double_p)           # noqa: E731
    call = lambda id=d.id, D=2, G=3, n=4, th=p(x), pp=p(par), npar=1, o=p(out): lib.kabc_derived_eval(   # noqa: E731
        None, id, D, G, n, th, pp, npar, o)
    for kw, msg in (({"th": None}, b"NULL argument"), ({"o": None}, b"NULL argument"), ({"D": 0}, b"D = 0 outside"),
                    ({"D": 257}, b"D = 257 outside"), ({"G": 0}, b"G = 0 outside 1..256"), ({"G": 257}, b"G = 257"),
                    ({"n": -1}, b"n = -1 rows"), ({"pp": None}, b"NULL params"), ({"npar": -1}, b"negative length"),
                    ({"id": 0}, b"not a registered"), ({"id": 10 ** 6}, b"not a registered"), ({}, b"ctx is NULL")):
        assert call(**kw) == cd.KABC_ERR_INVALID_ARG, kw
        assert msg in lib.kabc_last_error(), (kw, lib.kabc_last_error())
    with pytest.raises(ValueError, match="one row"):
        d(np.float64(1.0))


# ---- the restatements, against rows computed by hand ----------------------------------------------------

def test_restatements_on_hand_computed_rows():
    x = np.array([[3.0, 2.0], [-1.0, 0.5], [0.0, 0.0], [2.0, 2.0]])
    a = do.restate("A", x, [1.0])
    assert a.tolist() == [[6.0, 2.0 / 5.0, 1.0], [-0.5, -2.0 / 1.25, 0.0], [0.0, -1.0, 0.0], [4.0, 1.0 / 5.0, 0.0]]
    assert np.array_equal(do.restate("B", x), x) and do.restate("B", x) is not x
    c = do.restate("C", np.array([[1.0, 2.0, 3.0], [0.5, -0.5, 0.0]]))
    assert c.tolist() == [[14.0], [0.5]]
    # in index order, and the order is part of the definition: with a^2 = 2^-54, a quarter of 1's last place,
    # ((1 + a^2) + a^2) + a^2 stays 1 while ((a^2 + a^2) + a^2) + 1 rounds up
    a = 2.0 ** -27
    assert do.restate("C", np.array([[1.0, a, a, a]]))[0, 0] == 1.0
    assert do.restate("C", np.array([[a, a, a, 1.0]]))[0, 0] == 1.0 + 2.0 ** -52
    d = do.restate("D", x)
    assert d.shape == (4, 17) and d[0].tolist() == [3.0 + 2.0 * j for j in range(17)]
    assert d[1].tolist() == [-1.0 + 0.5 * j for j in range(17)]
    e = do.restate("E", x)
    assert np.isnan(e[1, 0]) and np.isnan(e[2, 0]) and e[0, 0] == 2.0 and e[3, 0] == 2.0
    assert e[:, 1].tolist() == [np.inf, -np.inf, -np.inf, np.inf]
    # leading axes are kept: a trace [gens][N][D] maps to [gens][N][G]
    assert do.restate("A", x.reshape(2, 2, 2), [1.0]).shape == (2, 2, 3)


def test_composed_oracle_is_the_three_oracles_on_the_mapped_trace():
    import ais_autocorr_oracle as ao
    import ais_hist_oracle as ho
    import ais_summary_oracle as so
    rng = np.random.default_rng(1)
    tr = rng.normal(size=(9, 7, 2))
    w = do.summarize("A", tr, L=4, hist=(-2.0, 2.0, 5))
    g = do.restate("A", tr)
    assert np.array_equal(w["g"], g) and w["n"] == 63 and w["cov"].shape == (3, 3)
    assert ao.mismatches(ao.summarize(g, 4), w) == [] and np.array_equal(w["counts"], ho.histogram(g, -2.0, 2.0, 5))
    assert so.mismatches(so.summarize(g), do.summarize("A", tr)) == []
    assert do.summarize("D", tr)["cov"].shape == (17,)                 # beyond KABC_MAX_DIM: the variances
    e = do.summarize("E", tr, hist=(-1.0, 1.0, 4))
    assert np.all(e["counts"].sum(axis=1) == 63)
    npos = np.count_nonzero(tr[..., 0] > 0)
    assert e["counts"][1, -1] == npos and e["counts"][1, 0] == 63 - npos   # +inf: overflow, -inf: underflow
    assert e["counts"][0, -1] >= 63 - npos                                 # every NaN in the overflow
