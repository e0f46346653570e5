"""-m gpu: DeviceCost.evaluate / prior_predictive (kabc_cost_eval, kabc_prior_predictive; the kernel of
csrc/cost_eval_kernel.hpp) against the CPU oracle's orc_cost_eval, bit for bit.

Every comparison is on the bit patterns (view(np.uint64)): +-Inf compare too (NoisyBanana(0.5) returns
Inf half the time).  Stream contract under test: out[i, j] is the cost of row i under
(seed, walker = first_row + i, t = j, DOM_EVAL_COST) and depends on nothing else."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIRST_ROWS = (0, (1 << 31) + 5)
SEEDS = (3, 0x9E3779B97F4A7C15)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        raise AssertionError(f"{what}: {bad.shape[0]} of {g.size} differ, first at {bad[0].tolist()}: "
                             f"{np.asarray(got).reshape(g.shape)[tuple(bad[0])]!r} != "
                             f"{np.asarray(want).reshape(w.shape)[tuple(bad[0])]!r}")


def _oracle_table(orc, cost, theta, seed, first_row, nrep, pairs=None):
    """orc.cost_eval(cost, theta[i], seed, walker=first_row+i, t=j, domain=DOM_EVAL_COST) for every (i, j)
    (or for the listed pairs only: NaN elsewhere), through the oracle's C entry point directly"""
    from kissabc_jl_amd import _cdefs as cd
    f = orc.load().orc_cost_eval
    cc = cost.to_c()
    ref = C.byref(cc)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    n, D = theta.shape
    out = np.full((n, nrep), np.nan)
    rows = [theta[i].ctypes.data_as(cd.c_double_p) for i in range(n)]
    if pairs is None:
        for i in range(n):
            xi, w = rows[i], first_row + i
            for j in range(nrep):
                out[i, j] = f(ref, D, xi, seed, w, j, cd.DOM_EVAL_COST)
    else:
        for i, j in pairs:
            out[i, j] = f(ref, D, rows[i], seed, first_row + i, j, cd.DOM_EVAL_COST)
    return out


def _cases(k):
    rng = np.random.default_rng(5)
    c = []
    for D in (2, 20, 128):
        c.append((f"GaussDist/{D}", k.costs.GaussDist(rng.normal(size=D)), D))
    for D in (2, 17):
        c.append((f"Rosenbrock/{D}", k.costs.Rosenbrock(), D))
    for D in (3, 34):
        c.append((f"HierGaussSim/{D}", k.costs.HierGaussSim(rng.normal(size=D - 2)), D))
    c.append(("NormalMeanStdSim/2", k.costs.NormalMeanStdSim(1000, 2.0, 0.04), 2))
    c.append(("DiracSq/1", k.costs.DiracSq(1.5), 1))
    c.append(("AbsDiff/1", k.costs.AbsDiff(1.5), 1))
    for D in (1, 5, 24):
        c.append((f"NormShell/{D}", k.costs.NormShell(1.5), D))
    c.append(("NoisyQuadDU/2", k.costs.NoisyQuadDU(5.5), 2))
    c.append(("Mixture/1", k.costs.Mixture(0.0), 1))
    c.append(("NoisyBanana/2", k.costs.NoisyBanana(0.5), 2))
    c.append(("WienerRms/2", k.costs.WienerRms(np.sqrt(0.25 * np.arange(31.0) ** 2 + 4.0 * np.arange(31.0))), 2))
    return c


# ---- 1. oracle parity, every built-in cost --------------------------------------------------------
def test_every_builtin_cost_matches_the_oracle(k, orc, gpu_ctx):
    cases = _cases(k)
    assert sorted({c.id for _, c, _ in cases}) == list(range(1, 12))
    rng = np.random.default_rng(17)
    for name, cost, D in cases:
        theta = rng.normal(size=(1000, D)) * 1.5
        sim = cost.id == 4        # NormalMeanStdSim(1000, ...): 2000 pairs keep the oracle loop short
        for seed, first_row in zip(SEEDS, FIRST_ROWS):
            pairs = None
            if sim:
                pairs = sorted({(int(i), int(j)) for i, j in zip(rng.integers(0, 1000, 2000), rng.integers(0, 64, 2000))}
                               | {(0, 0), (0, 63), (62, 2), (999, 0), (999, 63)})
            want = _oracle_table(orc, cost, theta, seed, first_row, 64, pairs)
            mask = ~np.isnan(want) if sim else np.ones_like(want, dtype=bool)
            for n in (1, 63, 1000):
                for nrep in (None, 3, 64):
                    got = cost.evaluate(theta[:n], nrep=nrep, seed=seed, first_row=first_row)
                    R = 1 if nrep is None else nrep
                    assert got.shape == ((n,) if nrep is None else (n, nrep)), (name, n, nrep, got.shape)
                    g2, w2, m2 = got.reshape(n, R), want[:n, :R], mask[:n, :R]
                    _same(g2[m2], w2[m2], (name, n, nrep, seed, first_row))
            if sim:
                assert mask.sum() >= 1900


def test_nonfinite_rows_go_to_the_cost(k, orc, gpu_ctx):
    """no look at the values of a row: an Inf coordinate reaches the formula like any other"""
    theta = np.array([[0.5, -0.25], [np.inf, 0.0], [1.0, -np.inf], [-np.inf, np.inf]])
    for cost in (k.costs.GaussDist([0.0, 1.0]), k.costs.NoisyQuadDU(5.5)):
        got = cost.evaluate(theta, nrep=2, seed=1)
        _same(got, _oracle_table(orc, cost, theta, 1, 0, 2), cost.name)
    assert np.isinf(k.costs.GaussDist([0.0, 1.0]).evaluate([np.inf, 0.0]))
    assert np.isnan(k.costs.GaussDist([0.0, 1.0]).evaluate([np.nan, 0.0]))


# ---- 2. known answers without the oracle ----------------------------------------------------------
def test_closed_forms(k, gpu_ctx):
    rng = np.random.default_rng(0)
    for D in (1, 2, 5, 16, 40):
        c = rng.normal(size=D)
        X = rng.normal(size=(20, D)) * 3
        want = []
        for x in X:
            s = 0.0
            for kk in range(D):
                s += (x[kk] - c[kk]) ** 2
            want.append(np.sqrt(s))
        _same(k.costs.GaussDist(c).evaluate(X), np.array(want), ("GaussDist", D))
    for D in (2, 3, 8, 16, 17):
        X = rng.uniform(-5, 5, size=(20, D))
        want = []
        for x in X:
            s = 0.0
            for kk in range(D - 1):
                a, b = x[kk + 1] - x[kk] * x[kk], 1.0 - x[kk]
                s += 100.0 * a * a + b * b
            want.append(np.sqrt(s))
        _same(k.costs.Rosenbrock().evaluate(X), np.array(want), ("Rosenbrock", D))
    assert k.costs.Rosenbrock().evaluate(np.ones(8)) == 0.0
    xs = rng.normal(size=(50, 1)) * 2
    _same(k.costs.DiracSq(1.5).evaluate(xs), np.abs(xs[:, 0] * xs[:, 0] + 1.0 - 1.5), "DiracSq")
    _same(k.costs.AbsDiff(1.5)(xs), np.abs(xs[:, 0] - 1.5), "AbsDiff")
    for D in (1, 4, 9, 24):
        x = rng.normal(size=D)
        s = 0.0
        for v in x:
            s += v * v
        got = k.costs.NormShell(1.5)(x)
        assert isinstance(got, float) and got == abs(np.sqrt(s) - 1.5), (D, got)


# ---- 3. geometry independence ---------------------------------------------------------------------
def test_value_does_not_depend_on_the_call_geometry(k, gpu_ctx, monkeypatch):
    rng = np.random.default_rng(2)
    for cost, D in ((k.costs.NoisyBanana(0.5), 2), (k.costs.HierGaussSim(rng.normal(size=18)), 20),
                    (k.costs.GaussDist(rng.normal(size=128)), 128)):
        theta = rng.normal(size=(4097, D))
        full = cost.evaluate(theta, seed=9)
        assert full.shape == (4097,)
        for a, b in ((0, 1), (100, 163), (1000, 4097), (4096, 4097)):
            _same(cost.evaluate(theta[a:b], seed=9, first_row=a), full[a:b], (cost.name, a, b))
        five = cost.evaluate(theta, nrep=5, seed=9)
        assert five.shape == (4097, 5)
        _same(five[:, 0], full, (cost.name, "column 0 of nrep=5"))
        _same(cost.evaluate(theta[7], nrep=5, seed=9, first_row=7), five[7], (cost.name, "one row"))
        assert cost.evaluate(theta[7], seed=9, first_row=7) == full[7] or np.isinf(full[7])
        # the same input cut into launches of 1500 rows (three launches), and of 64
        for rows in ("1500", "64"):
            monkeypatch.setenv("KABC_EVAL_ROWS", rows)
            _same(cost.evaluate(theta, nrep=5, seed=9), five, (cost.name, "KABC_EVAL_ROWS=" + rows))
            monkeypatch.delenv("KABC_EVAL_ROWS")
    # the launches are counted where the call reports them
    monkeypatch.setenv("KABC_EVAL_ROWS", "1500")
    prior = k.Factored(k.Normal(0, 1), k.Normal(0, 1))
    r = k.prior_predictive(prior, k.costs.NoisyBanana(0.5), 4097, seed=4, return_array=True)
    assert r.info["launches"] == 3 and r.info["rows_per_launch"] == 1500, r.info
    monkeypatch.delenv("KABC_EVAL_ROWS")
    r1 = k.prior_predictive(prior, k.costs.NoisyBanana(0.5), 4097, seed=4, return_array=True)
    assert r1.info["launches"] == 1
    _same(r.P, r1.P, "P across launch sizes")
    _same(r.C, r1.C, "C across launch sizes")
    _same(r.logprior, r1.logprior, "logprior across launch sizes")


# ---- 4. user costs --------------------------------------------------------------------------------
L1_SRC = """
KABC_HD double kabc_user_cost(const double* x, int D, const double* params, const double* data,
                              int64_t ndata, kabc_cost_rng_t* rng) {
    double z0, z1;
    kabc_cost_rng_normal2(rng, &z0, &z1);
    return kabc_fabs(x[0] - params[0]) + kabc_fabs(x[1] - params[1]) + 0.01 * kabc_fabs(z0);
}
"""
D20_SRC = """
KABC_HD double kabc_user_cost(const double* x, int D, const double* params,
                              const double* data, int64_t ndata, kabc_cost_rng_t* rng) {
    double z0, z1, s = 0.0;
    kabc_cost_rng_normal2(rng, &z0, &z1);
    for (int k = 0; k < D; ++k) s += (x[k] - params[0]) * (x[k] - params[0]);
    return kabc_sqrt(s) + 0.01 * kabc_fabs(z0);
}"""


def test_user_costs_hiprtc(k, orc, gpu_ctx, monkeypatch):
    monkeypatch.setenv("KABC_USER_PLUGIN", "hiprtc")
    rng = np.random.default_rng(8)
    for cost, D in ((k.costs.UserCost(L1_SRC, dims=[2], params=[1.0, -0.5], name="l1_noisy_eval"), 2),
                    (k.costs.UserCost(D20_SRC, dims=[20], params=[0.25], name="dyn_user_eval"), 20)):
        orc.register_user_cost(cost)
        theta = rng.normal(size=(300, D))
        for seed, first_row in zip(SEEDS, FIRST_ROWS):
            for nrep in (None, 7):
                got = cost.evaluate(theta, nrep=nrep, seed=seed, first_row=first_row)
                want = _oracle_table(orc, cost, theta, seed, first_row, 1 if nrep is None else nrep)
                _same(got.reshape(want.shape), want, (cost.name, nrep, seed, first_row))
    # a dimension the snippet does not list
    cost = k.costs.UserCost(L1_SRC, dims=[2], params=[1.0, -0.5], name="l1_noisy_eval")
    with pytest.raises(k.KabcError) as ei:
        cost.evaluate(np.zeros((4, 3)))
    assert ei.value.status == 5, str(ei.value)          # KABC_ERR_UNSUPPORTED


def test_user_cost_hipcc_form_is_refused(k, gpu_ctx, monkeypatch):
    """include/kabc.h: a cost plugin .so built by hipcc carries no evaluation kernel -- KABC_ERR_UNSUPPORTED,
    and the message names the hipRTC form.  (The snippet, dims and posteriors of tests/test_gpu_dyn_dim.py's
    hipcc case: one plugin build serves both files.)"""
    monkeypatch.setenv("KABC_USER_PLUGIN", "hipcc")
    cost = k.costs.UserCost(D20_SRC, dims=[20], params=[0.25], name="dyn_user_hipcc", posteriors=["kernelized"])
    with pytest.raises(k.KabcError) as ei:
        cost.evaluate(np.zeros((4, 20)))
    assert ei.value.status == 5 and "kabc_compile_cost_plugin" in str(ei.value), str(ei.value)
    with pytest.raises(k.KabcError) as ei:
        k.prior_predictive(k.Factored(*[k.Normal(0, 1)] * 20), cost, 10)
    assert ei.value.status == 5


# ---- 5. prior_predictive --------------------------------------------------------------------------
def test_prior_predictive_is_the_three_calls_composed(k, orc, gpu_ctx):
    from kissabc_jl_amd import _cdefs as cd
    rng = np.random.default_rng(4)
    A = rng.normal(size=(4, 4))
    problems = [
        ("mixed", k.Factored(k.Normal(0, 2), k.DiscreteUniform(-3, 3), k.Beta(2.0, 3.0)),
         k.costs.GaussDist([0.5, 1.0, 0.25])),
        ("mvnormal", k.MvNormal(rng.normal(size=4), A @ A.T + 0.4 * np.eye(4)), k.costs.Rosenbrock()),
        ("user family", k.Factored(k.Laplace(0.5, 1.5), k.Poisson(3.0)), k.costs.NoisyQuadDU(5.5)),
        ("factored/20", k.Factored(*[k.Normal(0, 1)] * 19, k.DiscreteUniform(-2, 2)),
         k.costs.HierGaussSim(rng.normal(size=18))),
    ]
    for name, prior, cost in problems:
        for n, nrep, seed, first_row in ((257, None, SEEDS[0], 0), (1000, 3, SEEDS[1], FIRST_ROWS[1])):
            r = k.prior_predictive(prior, cost, n, nrep=nrep, seed=seed, first_row=first_row, return_array=True)
            D = len(k.distributions.as_factored(prior))
            assert r.P.shape == (n, D) and r.logprior.shape == (n,), (name, r.P.shape)
            assert r.C.shape == ((n,) if nrep is None else (n, nrep)), (name, r.C.shape)
            P = orc.push_p(prior, orc.factored_rand(prior, n, seed, domain=cd.DOM_EVAL_DRAW, first_walker=first_row))
            _same(r.P, P, (name, "P"))
            _same(r.logprior, orc.factored_logpdf(prior, P), (name, "logprior"))
            want = _oracle_table(orc, cost, P, seed, first_row, 1 if nrep is None else nrep)
            _same(r.C.reshape(want.shape), want, (name, "C"))
            _same(cost.evaluate(r.P, nrep=nrep, seed=seed, first_row=first_row), r.C, (name, "C == evaluate(P)"))
    # bundled like smc's P; a univariate prior gives one Particles
    r = k.prior_predictive(problems[0][1], problems[0][2], 50, seed=1)
    assert isinstance(r.P, list) and len(r.P) == 3 and isinstance(r.P[0], k.Particles)
    r = k.prior_predictive(k.Normal(0, 1), k.costs.Mixture(0.0), 50, nrep=4, seed=1)
    assert isinstance(r.P, k.Particles) and r.C.shape == (50, 4)
    # n = 0 touches nothing
    r = k.prior_predictive(problems[0][1], problems[0][2], 0, return_array=True)
    assert r.P.shape == (0, 3) and r.C.shape == (0,)


# ---- 6. posterior predictive on a real result -----------------------------------------------------
def test_posterior_predictive_of_an_smc_result(k, gpu_ctx):
    N2 = k.Factored(k.Normal(0, 5), k.Normal(0, 5))
    cost = k.costs.GaussDist([1.0, -0.5])
    r = k.smc(N2, cost, nparticles=100, return_array=True, seed=3)
    # a deterministic cost: the sampler stored exactly these values
    _same(cost.evaluate(r.info["theta_all"]), r.C, "cost.evaluate(theta_all) == r.C")
    _same(cost(r.info["theta_all"]), r.C, "cost(theta_all) == r.C")
    sim = k.costs.NormalMeanStdSim(1000, 2.0, 0.04)
    prior = k.Factored(k.Uniform(1, 3), k.Uniform(0, 0.1))
    rs = k.smc(prior, sim, nparticles=100, return_array=True, seed=3)
    pp = sim.evaluate(rs.info["theta_all"], nrep=16, seed=5)
    assert pp.shape == (100, 16) and np.all(np.isfinite(pp))
    for row in pp:
        assert np.unique(_bits(row)).size == 16          # all replicates of a row distinct


# ---- 7. cancel ------------------------------------------------------------------------------------
def test_cancel(k, gpu_ctx):
    rng = np.random.default_rng(6)
    theta = rng.normal(size=(500, 2))
    cost = k.costs.NoisyBanana(0.5)
    want = cost.evaluate(theta, nrep=3, seed=2)          # an undisturbed call (the default context)
    ctx = k.Context(0)
    try:
        ctx.cancel()                                     # on an idle context: cancels the next call
        with pytest.raises(k.Cancelled):
            cost.evaluate(theta, nrep=3, seed=2, ctx=ctx)
        _same(cost.evaluate(theta, nrep=3, seed=2, ctx=ctx), want, "the call after a cancelled one")
        ctx.cancel()
        with pytest.raises(k.Cancelled):
            k.prior_predictive(k.Factored(k.Normal(0, 1), k.Normal(0, 1)), cost, 100, ctx=ctx)
        r = k.prior_predictive(k.Factored(k.Normal(0, 1), k.Normal(0, 1)), cost, 100, seed=2, ctx=ctx, return_array=True)
        _same(r.C, k.prior_predictive(k.Factored(k.Normal(0, 1), k.Normal(0, 1)), cost, 100, seed=2,
                                      return_array=True).C, "prior_predictive after a cancelled one")
    finally:
        ctx.close()
