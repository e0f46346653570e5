"""CPU: sample_batch's argument checks (all before the library runs anything) and the C entry point
kabc_ais_create_batch_costs's own refusals, which need no device."""
import ctypes as C
import inspect

import pytest


@pytest.fixture
def prob(k):
    prior = k.Factored(k.Normal(0, 5), k.Normal(0, 5))
    return prior, k.ApproxKernelizedPosterior(prior, k.costs.GaussDist([1.0, -0.5]), 0.1)


def test_models_must_differ_in_their_cost_values_only(k, prob):
    prior, m = prob
    g = k.costs.GaussDist([0.0, 1.0])
    cases = [
        (k.ApproxKernelizedPosterior(prior, k.costs.Rosenbrock(), 0.1), "model 1 differs from model 0 in its cost id"),
        (k.ApproxKernelizedPosterior(prior, k.costs.GaussDist([0.0, 1.0, 2.0]), 0.1), "in its cost's params / data"),
        (k.ApproxKernelizedPosterior(k.Factored(k.Normal(0, 4), k.Normal(0, 5)), g, 0.1), "in its prior"),
        (k.ApproxKernelizedPosterior(k.Factored(k.Normal(0, 5)), k.costs.GaussDist([0.0]), 0.1), "in its prior"),
        (k.ApproxKernelizedPosterior(prior, g, 0.2), "in its eps"),
        (k.ApproxPosterior(prior, g, 0.1), "in its class"),
    ]
    for other, msg in cases:
        with pytest.raises(ValueError, match=msg):
            k.sample_batch([m, other], k.AIS(12), 10)
    h = [k.ApproxKernelizedPosterior(prior, k.costs.HierGaussSim([1.0, 2.0]), 0.1),
         k.ApproxKernelizedPosterior(prior, k.costs.HierGaussSim([1.0, 2.0]), 0.1),
         k.ApproxKernelizedPosterior(prior, k.costs.HierGaussSim([1.0, 2.0, 3.0]), 0.1)]
    with pytest.raises(ValueError, match="model 2 differs from model 0 in its cost's params / data lengths"):
        k.sample_batch(h, k.AIS(12), 10)
    with pytest.raises(TypeError):
        k.sample_batch([m, k.costs.GaussDist([0.0, 1.0])], k.AIS(12), 10)
    with pytest.raises(ValueError, match="2 models for nruns = 3"):
        k.sample_batch([m, m], k.AIS(12), 10, 3)


def test_seeds_and_nruns(k, prob):
    _, m = prob
    with pytest.raises(ValueError, match=r"len\(seeds\) = 2 != nruns = 3"):
        k.sample_batch(m, k.AIS(12), 10, 3, seeds=[1, 2])
    with pytest.raises(ValueError, match="nruns must be >= 1"):
        k.sample_batch(m, k.AIS(12), 10, 0)
    with pytest.raises(ValueError, match="nruns must be >= 1"):
        k.sample_batch([], k.AIS(12), 10)
    with pytest.raises(ValueError, match="nruns is required"):
        k.sample_batch(m, k.AIS(12), 10)


def test_sampler_must_be_ais(k, prob):
    _, m = prob
    with pytest.raises(TypeError, match=r"sampler must be AIS\(nparticles\)"):
        k.sample_batch(m, 12, 10, 2)
    with pytest.raises(TypeError, match=r"sampler must be AIS\(nparticles\)"):
        k.sample_batch([m, m], k.MCMCThreads(), 10)


def test_keyword_defaults_follow_sample(k):
    p = inspect.signature(k.sample_batch).parameters
    q = inspect.signature(k.sample).parameters
    assert p["seed"].default == 0 and p["nruns"].default is None and p["seeds"].default is None
    for name in ("ntransitions", "discard_initial", "retry_sampling", "seed", "ctx", "return_array"):
        assert p[name].default == q[name].default, name


def test_ensemble_costs_need_one_seed_each(k, prob):
    _, m = prob
    g = k.costs.GaussDist([0.0, 1.0])
    with pytest.raises(ValueError, match="costs needs seeds"):
        k.AisEnsemble(m, 12, costs=[g, g])
    with pytest.raises(ValueError, match="3 costs for 2 seeds"):
        k.AisEnsemble(m, 12, seeds=[1, 2], costs=[g, g, g])
    with pytest.raises(TypeError, match="DeviceCosts"):
        k.AisEnsemble(m, 12, seeds=[1, 2], costs=[g, None])


def _c_args(k, m, costs):
    from kissabc_jl_amd import _cdefs as cd
    model = m.to_c()
    ccs = (cd.Cost * len(costs))(*[c.to_c() for c in costs])
    seeds = (C.c_uint64 * len(costs))(*range(1, len(costs) + 1))
    return model, ccs, seeds


def test_c_entry_point_refusals(k, prob):
    from kissabc_jl_amd import _cdefs as cd, _lib
    lib = _lib.load()
    _, m = prob
    keep = [k.costs.GaussDist([0.0, 1.0]), k.costs.GaussDist([2.0, 1.0])]
    model, ccs, seeds = _c_args(k, m, keep)
    out = C.c_void_p()
    f = lib.kabc_ais_create_batch_costs
    for args in ((None, 12, 2, seeds, ccs, C.byref(out)), (C.byref(model), 12, 2, None, ccs, C.byref(out)),
                 (C.byref(model), 12, 2, seeds, ccs, None)):
        assert f(None, *args) == cd.KABC_ERR_INVALID_ARG
        assert b"NULL argument" in lib.kabc_last_error()
    # the checks on the costs come before the context's
    assert f(None, C.byref(model), 12, 0, seeds, ccs, C.byref(out)) == cd.KABC_ERR_INVALID_ARG
    assert b"nchains must be 1..65535" in lib.kabc_last_error()
    assert f(None, C.byref(model), 12, 2, seeds, ccs, C.byref(out)) == cd.KABC_ERR_INVALID_ARG
    assert b"NULL argument" in lib.kabc_last_error()
    for bad, msg in (([keep[0], k.costs.Rosenbrock()], b"costs[1] differs from model->cost in its id"),
                     ([keep[0], k.costs.GaussDist([0.0, 1.0, 2.0])], b"costs[1] differs from model->cost"),
                     ([k.costs.HierGaussSim([1.0]), k.costs.HierGaussSim([1.0])], b"costs[0] differs")):
        model, ccs, seeds = _c_args(k, m, bad)
        assert f(None, C.byref(model), 12, 2, seeds, ccs, C.byref(out)) == cd.KABC_ERR_INVALID_ARG
        assert msg in lib.kabc_last_error(), lib.kabc_last_error()
    # a NULL params array behind a non-zero length
    model, ccs, seeds = _c_args(k, m, keep)
    ccs[1].params = None
    assert f(None, C.byref(model), 12, 2, seeds, ccs, C.byref(out)) == cd.KABC_ERR_INVALID_ARG
    assert b"costs[1] has a NULL params / data array" in lib.kabc_last_error()
    assert not out.value
