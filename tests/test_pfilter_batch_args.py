"""CPU: pfilter_batch's argument checks (all before the library runs anything) and the C entry point's
own refusals."""
import ctypes as C

import pytest


@pytest.fixture
def prob(k):
    prior = k.Factored(k.Normal(0, 5), k.Normal(0, 5))
    return prior, k.costs.GaussDist([1.0, -0.5])


def test_costs_must_share_id_and_lengths(k, prob):
    prior, g = prob
    with pytest.raises(ValueError, match="cost 1 differs"):
        k.pfilter_batch(prior, [g, k.costs.Rosenbrock()], 100)
    with pytest.raises(ValueError, match="cost 2 differs"):
        k.pfilter_batch(prior, [g, k.costs.GaussDist([0.0, 1.0]), k.costs.GaussDist([0.0, 1.0, 2.0])], 100)
    with pytest.raises(ValueError, match="cost 1 differs"):
        k.pfilter_batch(prior, [k.costs.HierGaussSim([1.0, 2.0]), k.costs.HierGaussSim([1.0, 2.0, 3.0])], 100)
    with pytest.raises(TypeError):
        k.pfilter_batch(prior, [g, lambda x: 0.0], 100)
    with pytest.raises(ValueError, match="2 costs for nruns = 3"):
        k.pfilter_batch(prior, [g, g], 100, 3)


def test_seeds_and_nruns(k, prob):
    prior, g = prob
    with pytest.raises(ValueError, match=r"len\(seeds\) = 2 != nruns = 3"):
        k.pfilter_batch(prior, g, 100, 3, seeds=[1, 2])
    with pytest.raises(ValueError, match="nruns must be >= 1"):
        k.pfilter_batch(prior, g, 100, 0)
    with pytest.raises(ValueError, match="nruns must be >= 1"):
        k.pfilter_batch(prior, [], 100)
    with pytest.raises(ValueError, match="nruns is required"):
        k.pfilter_batch(prior, g, 100)


def test_refused_keywords(k, prob):
    """verbose, q outside (0, 1] and N < 1 are refused in Python, before a context is asked for"""
    prior, g = prob
    with pytest.raises(ValueError, match="verbose"):
        k.pfilter_batch(prior, g, 100, 2, verbose=True)
    for q in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError) as ei:
            k.pfilter_batch(prior, g, 100, 2, q=q)
        assert str(ei.value) == "pfilter needs 0 < q <= 1 and N >= 1"
    for n in (0, -3):
        with pytest.raises(ValueError) as ei:
            k.pfilter_batch(prior, g, n, 2)
        assert str(ei.value) == "pfilter needs 0 < q <= 1 and N >= 1"


def test_signature_follows_pfilter(k):
    import inspect
    p = inspect.signature(k.pfilter_batch).parameters
    q = inspect.signature(k.pfilter).parameters
    assert p["seed"].default == 0 and p["nruns"].default is None and p["seeds"].default is None
    for name in ("q", "eff_tol", "epstol", "max_iters", "proposal_width", "parallel", "verbose", "ctx",
                 "return_array"):
        assert p[name].default == q[name].default, name
    assert "pfilter_batch" in k.__all__


def test_c_entry_point_refuses_null_arguments(k):
    from kissabc_jl_amd import _cdefs as cd, _lib
    lib = _lib.load()
    res = (cd.PfilterResult * 2)()
    st = (C.c_int * 2)()
    seeds = (C.c_uint64 * 2)(1, 2)
    o = cd.PfilterOpts()
    lib.kabc_pfilter_default_opts(C.byref(o))
    rc = lib.kabc_pfilter_run_batch(None, None, 2, None, 2, seeds, C.byref(o), res, st)
    assert rc == cd.KABC_ERR_INVALID_ARG
    assert b"kabc_pfilter_run_batch: NULL argument" in lib.kabc_last_error()
    stats = (C.c_int64 * 4)(9, 9, 9, 9)
    lib.kabc_pfilter_batch_stats(stats)
    assert list(stats) == [0, 0, 0, 0]
