"""CPU: ABCDE_batch's argument checks (all before the library runs anything) and the C entry point's
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
        k.ABCDE_batch(prior, [g, k.costs.Rosenbrock()], 0.1)
    with pytest.raises(ValueError, match="cost 2 differs"):
        k.ABCDE_batch(prior, [g, k.costs.GaussDist([0.0, 1.0]), k.costs.GaussDist([0.0, 1.0, 2.0])], 0.1)
    with pytest.raises(ValueError, match="cost 1 differs"):
        k.ABCDE_batch(prior, [k.costs.HierGaussSim([1.0, 2.0]), k.costs.HierGaussSim([1.0, 2.0, 3.0])], 0.1)
    with pytest.raises(TypeError):
        k.ABCDE_batch(prior, [g, lambda x: 0.0], 0.1)
    with pytest.raises(ValueError, match="2 costs for nruns = 3"):
        k.ABCDE_batch(prior, [g, g], 0.1, 3)


def test_seeds_and_nruns(k, prob):
    prior, g = prob
    with pytest.raises(ValueError, match=r"len\(seeds\) = 2 != nruns = 3"):
        k.ABCDE_batch(prior, g, 0.1, 3, seeds=[1, 2])
    with pytest.raises(ValueError, match="nruns must be >= 1"):
        k.ABCDE_batch(prior, g, 0.1, 0)
    with pytest.raises(ValueError, match="nruns must be >= 1"):
        k.ABCDE_batch(prior, [], 0.1)
    with pytest.raises(ValueError, match="nruns is required"):
        k.ABCDE_batch(prior, g, 0.1)


def test_refused_keywords(k, prob):
    prior, g = prob
    with pytest.raises(ValueError, match="verbose"):
        k.ABCDE_batch(prior, g, 0.1, 2, verbose=True)
    for a in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="α must be in 0 <= α < 1."):
            k.ABCDE_batch(prior, g, 0.1, 2, α=a)
    with pytest.raises(ValueError, match="α must be in 0 <= α < 1."):
        k.ABCDE_batch(prior, g, 0.1, 2, alpha=1.5)


def test_signature_follows_abcde(k):
    import inspect
    p = inspect.signature(k.ABCDE_batch).parameters
    q = inspect.signature(k.ABCDE).parameters
    assert p["seed"].default == 0 and p["nruns"].default is None and p["seeds"].default is None
    for name in ("nparticles", "generations", "α", "alpha", "earlystop", "proposal_width", "parallel"):
        assert p[name].default == q[name].default, name


def test_c_entry_point_refuses_null_arguments(k):
    from kissabc_jl_amd import _cdefs as cd, _lib
    lib = _lib.load()
    res = (cd.AbcdeResult * 2)()
    st = (C.c_int * 2)()
    seeds = (C.c_uint64 * 2)(1, 2)
    o = cd.AbcdeOpts()
    lib.kabc_abcde_default_opts(C.byref(o))
    rc = lib.kabc_abcde_run_batch(None, None, 2, None, 2, seeds, C.byref(o), res, st)
    assert rc == cd.KABC_ERR_INVALID_ARG
    assert b"NULL argument" in lib.kabc_last_error()
    stats = (C.c_int64 * 4)(9, 9, 9, 9)
    lib.kabc_abcde_batch_stats(stats)
    assert list(stats) == [0, 0, 0, 0]
