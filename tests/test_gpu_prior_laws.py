"""-m gpu: the law of DEVICE prior draws (tests/helpers.py check_law, as test_prior_laws.py runs it on the
oracle) on every sampler branch that was fixed, plus one case per other branch; the device log-density
at the truncated Normal's edges; every init path of a model whose components hit those branches, bit-exact
against the oracle; and the Dirichlet support test on the device along a chain's proposals."""
import numpy as np
import pytest

from helpers import check_law, make_dist, prior_law
from test_prior_laws import DIR_ALPHA, _dirichlet_chain_proposals, _isprobvec

pytestmark = pytest.mark.gpu

INF = float("inf")
N_DEVICE = 1_000_000

DEVICE_GRID = [
    ("TruncNormal", (0, 0.1, 0, 100)),            # parent Normal (the README / bench prior)
    ("TruncNormal", (0, 1, -0.004, 0.006)),       # uniform, across the mean
    ("TruncNormal", (0, 1, 3, 3 + 1e-6)),         # uniform, narrow tail window
    ("TruncNormal", (0, 1, 8, INF)),              # exponential, one-sided
    ("TruncNormal", (0, 1, -38, -37)),            # exponential, two-sided, mirrored
    ("Beta", (1e-3, 1e-3)),                       # both Gammas underflow: the log-space ratio
    ("Beta", (2, 1e-3)),                          # one underflows
    ("Beta", (0.5, 0.5)),                         # the plain ratio
    ("Gamma", (1e-3, 1.0)),                       # the a < 1 boost into the subnormals
    ("Gamma", (1.000001, 1.0)),
    ("NegativeBinomial", (2.0, 1e-9)),            # PTRS at lambda ~ 1e9
    ("DiscreteUniform", (0, 2 ** 32)),            # the 64-bit index
]


@pytest.mark.parametrize("case", DEVICE_GRID, ids=lambda c: f"{c[0]}{tuple(c[1])}")
def test_device_draws_follow_the_reference_law(k, orc, gpu_ctx, case):
    kind, params = case
    d = k.Factored(make_dist(k, kind, params))
    got = d.rand(N_DEVICE, seed=31)
    assert np.array_equal(got, orc.push_p(d, orc.factored_rand(d, N_DEVICE, seed=31)))
    check_law(got[:, 0], prior_law(kind, params), f"device {kind}{params}")


def test_device_truncnormal_logpdf_beyond_erfc_underflow(k, orc, gpu_ctx):
    d = k.Factored(k.TruncatedNormal(0, 1, 40, 41))
    x = np.array([[40.0], [40.5], [41.0]])
    got = d.logpdf(x)
    assert np.all(np.isfinite(got)) and np.array_equal(got, orc.factored_logpdf(d, x))


def _edge_prior(k, D=4):
    comps = [k.TruncatedNormal(0, 1, 8, INF), k.TruncatedNormal(0, 1, 3, 3 + 1e-6), k.Beta(1e-3, 1e-3),
             k.Normal(0, 1)]
    return k.Factored(*(comps + [k.Normal(0, 1)] * (D - len(comps))))


def _check_init_draws(x):
    assert not np.isnan(x).any()
    assert np.all(x[:, 0] > 8.0) and np.all((x[:, 1] > 3.0) & (x[:, 1] < 3 + 1e-6))


# the one-workgroup driver, the half-generation kernels (prebuilt and the model's own unit: one size
# is enough, a compilation each), the run-time-dimension kernels
@pytest.mark.parametrize("N,D,spec", [(100, 4, "0"), (4096, 4, "0"), (4096, 4, "1"), (300, 20, "0")],
                         ids=["small", "halves", "halves_spec", "dyn_d20"])
def test_ais_init_on_the_edges_bit_exact(k, orc, gpu_ctx, monkeypatch, tmp_path, N, D, spec):
    monkeypatch.setenv("KABC_RTC_CACHE_DIR", str(tmp_path))
    monkeypatch.setenv("KABC_SPECIALIZE", spec)
    model = k.ApproxKernelizedPosterior(_edge_prior(k, D), k.costs.GaussDist(np.full(D, 0.5)), 1e9)
    e = k.AisEnsemble(model, N, seed=13).init()
    o = orc.OracleAIS(model, N, seed=13).init()
    for got, ref in zip(e.state()[:3], o.state()[:3]):
        assert np.array_equal(got, ref)
    _check_init_draws(e.state()[0])


@pytest.mark.parametrize("nparticles", [200, 5000, 70000])
def test_smc_init_on_the_edges_bit_exact(k, orc, gpu_ctx, monkeypatch, nparticles):
    monkeypatch.setenv("KABC_SPECIALIZE", "0")
    prior, cost = _edge_prior(k), k.costs.GaussDist(np.full(4, 0.5))
    kw = dict(nparticles=nparticles, alpha=0.9, epstol=1e9)       # stops at its first eps: the draws
    got = k.smc(prior, cost, seed=6, return_array=True, **kw)
    ref = orc.smc(prior, cost, seed=6, **kw)
    assert got.eps == ref["eps"] and np.array_equal(got.info["theta_all"], ref["theta_all"])
    _check_init_draws(got.info["theta_all"])


def test_smc_dyn_dim_init_on_the_edges_bit_exact(k, orc, gpu_ctx, monkeypatch):
    monkeypatch.setenv("KABC_SPECIALIZE", "0")
    prior, cost = _edge_prior(k, 20), k.costs.GaussDist(np.full(20, 0.5))
    kw = dict(nparticles=3000, alpha=0.9, epstol=1e9)
    got = k.smc(prior, cost, seed=6, return_array=True, **kw)
    ref = orc.smc(prior, cost, seed=6, **kw)
    assert got.eps == ref["eps"] and np.array_equal(got.info["theta_all"], ref["theta_all"])
    _check_init_draws(got.info["theta_all"])


def test_abcde_init_on_the_edges_bit_exact(k, orc, gpu_ctx, monkeypatch):
    monkeypatch.setenv("KABC_SPECIALIZE", "0")
    prior, cost = _edge_prior(k), k.costs.GaussDist(np.full(4, 0.5))
    got = k.ABCDE(prior, cost, 1e9, seed=9, return_array=True, nparticles=300, generations=1)
    ref = orc.abcde(prior, cost, 1e9, seed=9, nparticles=300, generations=1)
    assert np.array_equal(got.P, ref["P"]) and np.array_equal(got.C, ref["C"])
    _check_init_draws(got.P.reshape(-1, 4))


def test_device_dirichlet_chain_proposals(k, orc, gpu_ctx):
    d = k.Dirichlet(DIR_ALPHA)
    P = _dirichlet_chain_proposals(DIR_ALPHA)
    ok, _ = _isprobvec(P)
    got = d.logpdf(P)
    assert np.array_equal(np.isfinite(got), ok)
    assert np.array_equal(got, orc.factored_logpdf(d, P))
