"""GPU: one AIS model fitted to many datasets in one handle (kabc_ais_create_batch_costs,
AisEnsemble(costs=...), sample_batch).

Chain c of a handle with per-chain costs must be bit-identical to a single-chain handle on the model
with its cost replaced by costs[c] and seeded seeds[c]: the trace, the state, the ensemble and the
counters -- on the one-workgroup driver (N <= 512) and on the launch per half-generation, with the
costs' params or their data differing from chain to chain."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEEDS5 = [1, 977, 2 ** 40 + 3, 123456789, 0x9E3779B97F4A7C15 % (1 << 63)]
NT, GD, GK = 3, 2, 3   # ntransitions, discarded generations, kept generations

USER_LPI = """
KABC_HD double kabc_user_cost(const double* x, int D, const double* params, const double* data,
                              int64_t ndata, kabc_cost_rng_t* rng) {
    double s = 0.0;
    for (int k = 0; k < D; ++k) {
        const double d = (x[k] - params[k]) / data[k];
        s += d * d;
    }
    return -0.5 * s;
}
"""


def _with_cost(model, cost):
    m = copy.copy(model)
    m.cost = cost
    return m


def _gauss(k, D, box=False):
    prior = k.Factored(*([k.Uniform(-5, 5)] * D if box else [k.Normal(0, 5)] * D))
    costs = [k.costs.GaussDist(np.linspace(-1.0, 1.0, D) + 0.3 * r) for r in range(5)]
    return k.ApproxKernelizedPosterior(prior, costs[0], 0.5), costs


def _hier(k):
    prior = k.Factored(k.Normal(0, 5), k.Uniform(0, 5), *[k.Normal(0, 1)] * 4)
    costs = [k.costs.HierGaussSim(np.array([0.9, 1.3, 0.2, 1.1]) + 0.1 * r) for r in range(5)]
    return k.ApproxKernelizedPosterior(prior, costs[0], 0.3), costs


def _readme(k, n=(1000,) * 5):
    prior = k.Factored(k.Uniform(1, 3), k.Truncated(k.Normal(0, 0.1), 0, 100))
    costs = [k.costs.NormalMeanStdSim(n[r], 2.0 + 0.01 * r, 0.04 + 0.002 * r) for r in range(5)]
    return k.ApproxKernelizedPosterior(prior, costs[0], 0.005), costs


def _run(ens):
    ens.init()
    ens.advance(GD, NT)
    tr = ens.advance(GK, NT, collect=True)
    return tr, ens.state(), ens.ensemble(), ens.stats()


def _check(k, model, costs, N, driver, seeds=SEEDS5, batch=None):
    """the batch handle against single-chain handles on each chain's model; returns the batch's trace"""
    b = batch or k.AisEnsemble(model, N, seeds=seeds, costs=costs)
    assert b.driver == driver
    trb, (xb, lpb, llb, tb), eb, sb = _run(b)
    tot = {"proposals": 0, "cost_evals": 0, "accepted": 0}
    for c, (seed, cost) in enumerate(zip(seeds, costs)):
        e = k.AisEnsemble(_with_cost(model, cost), N, seed=seed)
        assert e.driver == driver
        tr, (x, lp, ll, t), en, st = _run(e)
        e.close()
        assert np.array_equal(trb[:, c].view(np.uint64), tr.view(np.uint64)), c
        assert np.array_equal(xb[c], x) and np.array_equal(lpb[c], lp) and np.array_equal(llb[c], ll), c
        assert np.array_equal(eb[c], en) and tb == t, c
        for kk, v in st.items():
            tot[kk] += v
    assert sb == tot
    b.close()
    return trb


@pytest.mark.parametrize("D,box,N,small,driver", [
    (2, False, 64, "1", "small"), (8, True, 200, "1", "small"),
    (8, True, 4096, "1", "halves"), (2, False, 300, "0", "halves")])
def test_per_chain_params_gauss(k, gpu_ctx, monkeypatch, D, box, N, small, driver):
    monkeypatch.setenv("KABC_AIS_SMALL", small)
    model, costs = _gauss(k, D, box)
    tr = _check(k, model, costs, N, driver)
    assert not np.array_equal(tr[:, 0], tr[:, 1])


@pytest.mark.parametrize("N,small,driver", [(100, "1", "small"), (4096, "1", "halves"), (100, "0", "halves")])
def test_per_chain_data_hier(k, gpu_ctx, monkeypatch, N, small, driver):
    monkeypatch.setenv("KABC_AIS_SMALL", small)
    model, costs = _hier(k)
    _check(k, model, costs, N, driver)


@pytest.mark.parametrize("N,small,driver,n", [(10, "1", "small", (1000,) * 5), (10, "0", "halves", (1000,) * 5),
                                              (30, "1", "small", (100, 120, 140, 160, 180))])
def test_readme_problem_per_run_observations(k, gpu_ctx, monkeypatch, N, small, driver, n):
    """the aux pre-pass reads each chain's params, including a draw count of its own"""
    monkeypatch.setenv("KABC_AIS_SMALL", small)
    model, costs = _readme(k, n)
    _check(k, model, costs, N, driver)


def test_threshold_posterior(k, gpu_ctx):
    model, costs = _gauss(k, 2)
    model = k.ApproxPosterior(model.prior, costs[0], 1.5)
    _check(k, model, costs, 50, "small")


@pytest.mark.parametrize("N,driver", [(40, "small"), (1024, "halves")])
def test_common_log_density_user_cost_reads_params_and_data(k, gpu_ctx, N, driver):
    costs = [k.costs.UserCost(USER_LPI, dims=[2], params=[0.5 * r, -0.25 * r], data=[1.0 + 0.1 * r, 0.5],
                              name="lpi_pd", posteriors=["common"]) for r in range(5)]
    assert len({c.id for c in costs}) == 1
    model = k.CommonLogDensity(2, k.Factored(k.Uniform(-3, 3), k.Uniform(-3, 3)), costs[0])
    _check(k, model, costs, N, driver)


def test_specialised_model(k, gpu_ctx):
    model = k.ApproxKernelizedPosterior(k.Factored(k.Normal(0.1, 5), k.Normal(0, 4), k.Uniform(-6, 6)),
                                        k.costs.GaussDist([0.0, 0.0, 0.0]), 0.4)
    costs = [k.costs.GaussDist([0.2 * r, -0.1 * r, 0.3]) for r in range(5)]
    k.set_specialize("blocking")
    try:
        b = k.AisEnsemble(model, 100, seeds=SEEDS5, costs=costs)
        assert b.spec_state()[0] == "active"
        _check(k, model, costs, 100, "small", batch=b)
    finally:
        k.set_specialize("env")


@pytest.mark.parametrize("N", [64, 4096])
def test_shared_cost_is_the_plain_batch(k, gpu_ctx, N):
    """costs that are all equal (distinct objects): stride 0, exactly kabc_ais_create_batch"""
    model, _ = _gauss(k, 2)
    costs = [k.costs.GaussDist([0.4, -0.2]) for _ in range(5)]
    model = _with_cost(model, k.costs.GaussDist([0.4, -0.2]))
    got = _run(k.AisEnsemble(model, N, seeds=SEEDS5, costs=costs))
    ref = _run(k.AisEnsemble(model, N, seeds=SEEDS5))
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2]) and got[3] == ref[3]
    for a, b in zip(got[1][:3], ref[1][:3]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("which", ["gauss_small", "hier_halves"])
def test_chains_against_the_oracle(k, orc, gpu_ctx, which):
    model, costs = _gauss(k, 2) if which == "gauss_small" else _hier(k)
    N = 64 if which == "gauss_small" else 2048
    b = k.AisEnsemble(model, N, seeds=SEEDS5, costs=costs).init()
    b.advance(GD, NT)
    trb = b.advance(GK, NT, collect=True)
    b.close()
    for c, (seed, cost) in enumerate(zip(SEEDS5, costs)):
        o = orc.OracleAIS(_with_cost(model, cost), N, seed).init()
        o.generations_sync(GD, NT, collect=False)
        assert np.array_equal(trb[:, c], o.generations_sync(GK, NT)), c


def test_sample_batch_grid_is_sample(k, gpu_ctx):
    model, costs = _gauss(k, 2)
    models = [_with_cost(model, c) for c in costs]
    kw = dict(ntransitions=4, discard_initial=30, retry_sampling=50)
    out = k.sample_batch(models, k.AIS(12), 50, seeds=SEEDS5, return_array=True, **kw)
    assert out.info["course"] == "grid" and out.info["driver"] == "small" and out.info["nruns"] == 5
    for r, m in enumerate(models):
        ref = k.sample(m, k.AIS(12), 50, seed=SEEDS5[r], return_array=True, **kw)
        assert np.array_equal(out[r], ref), r
    # one model, runs differing by seed only; Particles like sample()'s
    one = k.sample_batch(models[1], k.AIS(12), 30, 3, seed=5, ntransitions=2)
    seeds = k.api.chain_seeds(5, 3)
    for r in range(3):
        ref = k.sample(models[1], k.AIS(12), 30, seed=seeds[r], ntransitions=2)
        assert all(np.array_equal(np.asarray(a), np.asarray(b_)) for a, b_ in zip(one[r], ref))


def test_sample_batch_sequential_beyond_16_parameters(k, gpu_ctx):
    prior = k.Factored(*[k.Normal(0, 3)] * 20)
    models = [k.ApproxKernelizedPosterior(prior, k.costs.GaussDist(np.full(20, 0.1 * r)), 1.0) for r in range(3)]
    out = k.sample_batch(models, k.AIS(60), 60, seeds=SEEDS5[:3], ntransitions=2, discard_initial=60,
                         return_array=True)
    assert out.info["course"] == "sequential"
    for r, m in enumerate(models):
        ref = k.sample(m, k.AIS(60), 60, seed=SEEDS5[r], ntransitions=2, discard_initial=60, return_array=True)
        assert np.array_equal(out[r], ref), r


def test_failed_initial_draw_names_its_run(k, gpu_ctx):
    """run 3's cost is +Inf everywhere on the prior's support (its centre's square overflows)"""
    prior = k.Factored(k.Uniform(-1, 1), k.Uniform(-1, 1))
    costs = [k.costs.GaussDist([0.1 * r, 0.0]) for r in range(5)]
    costs[3] = k.costs.GaussDist([1e200, 0.0])
    models = [k.ApproxPosterior(prior, c, 0.5) for c in costs]
    with pytest.raises(k.KabcError) as e:
        k.sample_batch(models, k.AIS(20), 20, seeds=SEEDS5, retry_sampling=5)
    assert str(e.value) == ("run 3: Prior leads to ∞ costs too often, tune the prior or increase "
                            "`retry_sampling`.")
    ens = k.AisEnsemble(models[0], 20, seeds=SEEDS5, costs=costs)
    with pytest.raises(k.KabcError, match=r"^chain 3: Prior leads to ∞ costs too often"):
        ens.init(5)
    ens.close()
    ok = models[:3] + models[4:]
    out = k.sample_batch(ok, k.AIS(20), 20, seeds=SEEDS5[:4], retry_sampling=5, return_array=True)
    assert out.info["course"] == "grid" and len(out) == 4
