"""GPU: abc_pmc / kabc_abc_pmc against tests/abc_pmc_oracle.py, the numpy restatement of include/kabc.h's definition.

1. bit for bit against the oracle: theta, w, C, logprior, index and, per generation, eps, draws and ess -- one
   wavefront (N = 64), one lane past the 256-lane tile and a one-ancestor tail chunk (257), a partial third chunk
   (600); D = 1, 3, 16; both kernels; explicit and adaptive schedules; proposals outside a bounded prior's support;
   a stochastic cost, +Inf costs, the prepared cost;
2. invariants without the oracle: generation 0 is abc_reject, every cost is reproduced by cost.evaluate, sum w = 1;
3. the same bits under KABC_EVAL_ROWS, KABC_REJECT_CAPACITY (the overflow repeat), KABC_PMC_COURSE=phases,
   KABC_PMC_WEIGHT_SPLIT=0|1, and for an MvNormal prior and a UserCost (the phases course by themselves);
4. kabc_pmc_kernel_sums against numpy, underflow to S = 0 and zero weights included;
5. the stops; 6. cancel; 7. the known answer of tests/test_abc_pmc_known_answer.py on the device."""
import ctypes as C
import math
import threading

import numpy as np
import pytest

import abc_pmc_oracle as po
from test_abc_pmc_known_answer import EPS as KA_EPS, N as KA_N, SEED as KA_SEED, check_known_answer, known_answer_case

pytestmark = pytest.mark.gpu


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


def _same_run(r, o, what):
    """a PmcResult against the oracle's dict"""
    assert r.info["stop"] == o["stop"] and r.info["generations_run"] == o["generations_run"], (what, r.info, o["stop"])
    assert len(r.info["log"]) == len(o["log"]), what
    for g, (a, b) in enumerate(zip(r.info["log"], o["log"])):
        _same([a["eps"]], [b["eps"]], (what, "eps of generation", g))
        assert a["draws"] == b["draws"], (what, "draws of generation", g, a, b)
        _same([a["ess"]], [b["ess"]], (what, "ess of generation", g))
        assert a["launches"] >= 1
    _same(r.theta, o["theta"], (what, "theta"))
    _same(r.C, o["C"], (what, "C"))
    _same(r.logprior, o["logprior"], (what, "logprior"))
    _same(r.w, o["w"], (what, "w"))
    assert np.array_equal(r.info["index"], o["index"]), (what, "index")
    if o["generations_run"]:
        _same([r.eps], [o["eps"]], (what, "eps"))
        mu, c = po.moments(o["theta"], o["w"])
        _same(r.mean, mu, (what, "mean"))
        _same(r.cov, c, (what, "cov"))


def _cases(k):
    rng = np.random.default_rng(8)
    c16 = rng.normal(size=16) * 0.3
    return {
        # name: (prior, cost, N, keywords)
        "mixture_d1_n64": (k.Normal(0, 3), k.costs.Mixture(0.0), 64, dict(eps=[3.0, 1.5, 0.8], seed=1)),
        "bounded_d3_n257_full": (k.Factored(k.Uniform(-1, 1), k.Uniform(0, 2), k.Uniform(-3, 0.2)),
                                 k.costs.GaussDist([0.9, 0.1, 0.1]), 257, dict(eps=[1.5, 0.9, 0.5, 0.3], seed=2)),
        "bounded_d3_n257_diag": (k.Factored(k.Uniform(-1, 1), k.Uniform(0, 2), k.Uniform(-3, 0.2)),
                                 k.costs.GaussDist([0.9, 0.1, 0.1]), 257,
                                 dict(q=0.4, generations=4, kernel="diag", scale=1.5, seed=3)),
        "banana_inf_d2_n600": (k.Factored(k.Normal(0, 5), k.Normal(0, 5)), k.costs.NoisyBanana(0.2), 600,
                               dict(q=0.5, generations=3, seed=4)),
        "gauss_d16_n64": (k.Factored(*[k.Normal(0, 1)] * 16), k.costs.GaussDist(c16), 64,
                          dict(q=0.5, generations=3, eps0=6.0, seed=5)),
        "meanstd_sim_d2_n64": (k.Factored(k.Uniform(1, 3), k.Uniform(0, 0.1)), k.costs.NormalMeanStdSim(100, 2.0, 0.04), 64,
                               dict(eps=[1.0, 0.3, 0.1], kernel="diag", seed=6)),
    }


_ORACLE = {}


def _oracle(orc, k, name):
    """the oracle's run of a case: computed once, shared, never changed"""
    if name not in _ORACLE:
        prior, cost, N, kw = _cases(k)[name]
        _ORACLE[name] = po.oracle_pmc(orc, prior, cost, N, **kw)
    return _ORACLE[name]


# ---- 1. bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixture_d1_n64", "bounded_d3_n257_full", "bounded_d3_n257_diag", "banana_inf_d2_n600",
                                  "gauss_d16_n64", "meanstd_sim_d2_n64"])
def test_bit_for_bit_against_the_oracle(k, orc, gpu_ctx, name):
    prior, cost, N, kw = _cases(k)[name]
    o = _oracle(orc, k, name)
    r = k.abc_pmc(prior, cost, N, **kw)
    assert r.info["course"] == "fused" and o["generations_run"] >= 3, (r.info, o["stop"])
    _same_run(r, o, name)
    if name.startswith("bounded"):
        # proposals left the support and were counted as draws: the last generation's draws exceed the rows whose
        # log-prior is finite, which the oracle's own table shows
        assert r.info["log"][-1]["draws"] > N
    if name == "banana_inf_d2_n600":
        assert math.isinf(r.info["log"][0]["eps"]) and np.isfinite(r.C).all()


# ---- 2. invariants without the oracle -------------------------------------------------------------------
def test_invariants(k, gpu_ctx):
    prior, cost, N, kw = _cases(k)["bounded_d3_n257_full"]
    seed = kw["seed"]
    r0 = k.abc_pmc(prior, cost, N, eps=kw["eps"][:1], seed=seed)
    a = k.abc_reject(prior, cost, kw["eps"][0], N, seed=seed, return_array=True)
    _same(r0.theta, a.P, "generation 0 is abc_reject: theta")
    _same(r0.C, a.C, "generation 0 is abc_reject: C")
    _same(r0.logprior, a.logprior, "generation 0 is abc_reject: logprior")
    assert np.array_equal(r0.info["index"], a.info["index"]) and r0.info["log"][0]["draws"] == a.info["draws"]
    assert np.all(r0.w == 1.0 / N) and r0.info["stop"] == "done"
    r = k.abc_pmc(prior, cost, N, **kw)
    g = r.info["generations_run"] - 1
    assert g == 3 and np.all(np.diff(r.info["index"]) > 0)
    for i in (0, 1, 100, 255, 256):
        got = cost.evaluate(r.theta[i], nrep=g + 1, seed=seed, first_row=int(r.info["index"][i]))[g]
        _same([r.C[i]], [got], ("cost of particle", i))
    assert np.all(r.C <= kw["eps"][-1]) and np.all(np.isfinite(r.logprior)) and np.all(r.w > 0)
    assert abs(float(np.sum(r.w)) - 1.0) <= N * 2.0 ** -52
    assert 1.0 <= r.ess <= N and r.ess == pytest.approx(r.info["log"][-1]["ess"], rel=1e-12)
    # the stochastic cost the same way: replicate g of row index_i
    prior, cost, N, kw = _cases(k)["mixture_d1_n64"]
    r = k.abc_pmc(prior, cost, N, **kw)
    assert r.theta.shape == (N, 1)
    for i in (0, 31, 63):
        got = cost.evaluate(r.theta[i], nrep=3, seed=kw["seed"], first_row=int(r.info["index"][i]))[2]
        _same([r.C[i]], [got], ("stochastic cost of particle", i))
    assert len(r.resample(100, seed=1)) == 100             # (a scalar prior: one Particles)


# ---- 3. the same bits whatever the launches look like -----------------------------------------------------
@pytest.mark.parametrize("env", [("KABC_EVAL_ROWS", "256"), ("KABC_REJECT_CAPACITY", "64"), ("KABC_PMC_COURSE", "phases"),
                                 ("KABC_PMC_WEIGHT_SPLIT", "0"), ("KABC_PMC_WEIGHT_SPLIT", "1")],
                         ids=lambda e: "=".join(e))
@pytest.mark.parametrize("name", ["bounded_d3_n257_full", "banana_inf_d2_n600"])
def test_same_bits_under(k, orc, gpu_ctx, monkeypatch, name, env):
    prior, cost, N, kw = _cases(k)[name]
    monkeypatch.setenv(*env)
    r = k.abc_pmc(prior, cost, N, **kw)
    _same_run(r, _oracle(orc, k, name), (name, env))
    assert r.info["course"] == ("phases" if env[0] == "KABC_PMC_COURSE" else "fused")
    if env[0] == "KABC_REJECT_CAPACITY":                    # 64 records: the first look of every generation overflows
        assert all(rec["launches"] >= 3 for rec in r.info["log"])


L1_SRC = """
KABC_HD double kabc_user_cost(const double* x, int D, const double* params, const double* data,
                              int64_t ndata, kabc_cost_rng_t* rng) {
    double z0, z1;
    kabc_cost_rng_normal2(rng, &z0, &z1);
    return kabc_fabs(x[0] - params[0]) + kabc_fabs(x[1] - params[1]) + kabc_fabs(x[2]) + 0.01 * kabc_fabs(z0);
}
"""


def test_phases_course_by_itself(k, orc, gpu_ctx, monkeypatch):
    """an MvNormal prior and a user cost (hipRTC form) take the phases course without being asked to"""
    monkeypatch.setenv("KABC_USER_PLUGIN", "hiprtc")
    A = np.array([[1.0, 0.0, 0.0], [0.6, 0.8, 0.0], [-0.3, 0.2, 0.5]])
    prior = k.MvNormal([0.5, -0.5, 0.0], A @ A.T)
    cost = k.costs.GaussDist([0.2, -0.1, 0.3])
    kw = dict(q=0.5, generations=3, seed=9)
    r = k.abc_pmc(prior, cost, 65, **kw)
    assert r.info["course"] == "phases"
    _same_run(r, po.oracle_pmc(orc, prior, cost, 65, **kw), "MvNormal prior")
    monkeypatch.setenv("KABC_REJECT_COURSE", "phases")      # (generation 0 on the evaluation kernel too: one compilation)
    ucost = k.costs.UserCost(L1_SRC, dims=[3], params=[1.0, -0.5], name="l1_noisy_pmc")
    orc.register_user_cost(ucost)
    prior = k.Factored(k.Normal(0, 2), k.Uniform(-2, 2), k.Normal(0, 1))
    kw = dict(eps=[3.0, 1.5, 0.8], seed=10)
    r = k.abc_pmc(prior, ucost, 65, **kw)
    assert r.info["course"] == "phases"
    _same_run(r, po.oracle_pmc(orc, prior, ucost, 65, **kw), "UserCost")


# ---- 4. the weight kernel alone -----------------------------------------------------------------------
def _kernel_sums(k, ctx, y_new, y_anc, w_anc):
    from kissabc_jl_amd import _cdefs as cd, _lib
    y_new, y_anc, w_anc = (np.ascontiguousarray(a, dtype=np.float64) for a in (y_new, y_anc, w_anc))
    S = np.full(y_new.shape[0], np.nan)
    dp = lambda a: a.ctypes.data_as(cd.c_double_p)
    _lib.check(_lib.load().kabc_pmc_kernel_sums(ctx.handle, y_new.shape[1], y_new.shape[0], dp(y_new), y_anc.shape[0],
                                                dp(y_anc), dp(w_anc), dp(S)))
    return S


@pytest.mark.parametrize("split", [None, "0", "1"])
@pytest.mark.parametrize("D", [1, 2, 7, 16])
def test_kernel_sums_against_numpy(k, orc, gpu_ctx, monkeypatch, D, split):
    if split is not None:
        monkeypatch.setenv("KABC_PMC_WEIGHT_SPLIT", split)
    rng = np.random.default_rng(100 + D)
    for n_anc in (1, 255, 256, 257, 513):
        y_anc = rng.normal(size=(n_anc, D))
        w_anc = rng.random(n_anc)
        w_anc[rng.random(n_anc) < 0.2] = 0.0                  # zero weights
        for n_new in (1, 65, 300):
            y_new = rng.normal(size=(n_new, D)) * 1.5
            y_new[0] = 60.0                                   # so far away that every term underflows: S = 0, not hidden
            if n_new > 2:
                y_new[2] = y_anc[n_anc - 1]                   # on top of the last ancestor (the tail chunk)
            S = _kernel_sums(k, gpu_ctx, y_new, y_anc, w_anc)
            _same(S, po.kernel_sums(orc, y_new, y_anc, w_anc), ("S", D, n_anc, n_new, split))
            assert S[0] == 0.0 and np.all(S >= 0.0)
            if n_new > 2:
                assert S[2] >= w_anc[n_anc - 1]


# ---- 5. the stops -------------------------------------------------------------------------------------
def test_stops(k, orc, gpu_ctx):
    prior, cost = known_answer_case(k)
    # exhausted in generation 0: nothing comes back, KABC_OK
    r = k.abc_pmc(prior, cost, 64, eps=[1e-9], max_draws=64, seed=1)
    assert r.info["stop"] == "exhausted" and r.info["generations_run"] == 0 and r.theta.shape == (0, 1)
    # ... and in generation 1: generation 0 is intact
    kw = dict(eps=[4.0, 1e-9], max_draws=400, seed=1)
    _same_run(k.abc_pmc(prior, cost, 64, **kw), po.oracle_pmc(orc, prior, cost, 64, **kw), "exhausted")
    r = k.abc_pmc(prior, cost, 64, **kw)
    a = k.abc_reject(prior, cost, 4.0, 64, seed=1, return_array=True)
    assert r.info["stop"] == "exhausted" and r.info["generations_run"] == 1
    _same(r.theta, a.P, "the generation before an exhausted one")
    # target
    kw = dict(q=0.5, eps_target=0.5, generations=12, seed=1)
    r = k.abc_pmc(prior, cost, 64, **kw)
    _same_run(r, po.oracle_pmc(orc, prior, cost, 64, **kw), "target")
    assert r.info["stop"] == "target" and r.eps == 0.5
    # stalled: a cost with two kinds of values -- a fifth of NoisyBanana's costs are +Inf, so the 0.95-quantile of a
    # generation run at eps = +Inf is +Inf again: the threshold does not fall
    pb, cb = k.Factored(k.Normal(0, 5), k.Normal(0, 5)), k.costs.NoisyBanana(0.2)
    kw = dict(q=0.95, generations=8, seed=2)
    r = k.abc_pmc(pb, cb, 64, **kw)
    _same_run(r, po.oracle_pmc(orc, pb, cb, 64, **kw), "stalled")
    assert r.info["stop"] == "stalled" and r.info["generations_run"] == 2 and math.isinf(r.eps)
    # min_rate
    kw = dict(eps=[4.0, 2.0, 1.0], min_rate=0.9, seed=1)
    r = k.abc_pmc(prior, cost, 64, **kw)
    _same_run(r, po.oracle_pmc(orc, prior, cost, 64, **kw), "min_rate")
    assert r.info["stop"] == "min_rate" and r.info["generations_run"] == 1
    # degenerate: a coordinate whose spread underflows, c_11 == 0.0 exactly -- the factor fails, generation 0 stays
    p2, c2 = k.Factored(k.Normal(0, 1), k.Normal(0, 1e-200)), k.costs.GaussDist([0.0, 0.0])
    kw = dict(eps=[math.inf, 1.0], seed=1)
    r = k.abc_pmc(p2, c2, 32, **kw)
    _same_run(r, po.oracle_pmc(orc, p2, c2, 32, **kw), "degenerate")
    assert r.info["stop"] == "degenerate" and r.info["generations_run"] == 1 and r.cov[1, 1] == 0.0


# ---- 6. cancel ----------------------------------------------------------------------------------------
def test_cancel(k, gpu_ctx):
    prior = k.Factored(k.Uniform(1, 3), k.Uniform(0, 0.1))           # the README problem
    sim = k.costs.NormalMeanStdSim(1000, 2.0, 0.04)
    ctx = k.Context(0)
    try:
        ctx.cancel()                                     # on an idle context: cancels the next call, nothing is launched
        with pytest.raises(k.Cancelled) as ei:
            k.abc_pmc(prior, sim, 100, eps=[0.5, 0.3], seed=2, ctx=ctx)
        res = ei.value.result
        assert res.info["generations_run"] == 0 and res.info["stop"] == "cancelled" and res.C.size == 0
        want = k.abc_pmc(prior, sim, 100, eps=[0.5, 0.3], seed=2)                      # (the default context)
        got = k.abc_pmc(prior, sim, 100, eps=[0.5, 0.3], seed=2, ctx=ctx)
        _same(got.theta, want.theta, "the call after a cancelled one")
        _same(got.w, want.w, "the call after a cancelled one")
        # a long call: generation 1 asks for 20 000 rows at eps = 0.02, about one proposal in a few thousand even
        # from the mixture around generation 0 (eps = 0.5) -- seconds of work; the request comes after 0.3 s.
        # One call, bounded by its budget.
        timer = threading.Timer(0.3, ctx.cancel)
        timer.start()
        try:
            with pytest.raises(k.Cancelled) as ei:
                k.abc_pmc(prior, sim, 20_000, eps=[0.5, 0.001], max_draws=1 << 31, seed=5, ctx=ctx)
        finally:
            timer.cancel()
        r = ei.value.result
        assert r.info["stop"] == "cancelled" and r.info["generations_run"] in (0, 1)
        if r.info["generations_run"] == 1:               # the last complete generation: generation 0, intact
            a = k.abc_reject(prior, sim, 0.5, 20_000, seed=5, return_array=True)
            _same(r.theta, a.P, "the result of a cancelled call")
            _same(r.C, a.C, "the result of a cancelled call")
            assert np.all(r.w == 1.0 / 20_000) and r.eps == 0.5 and len(r.info["log"]) == 1
        # the context is usable afterwards
        got = k.abc_pmc(prior, sim, 100, eps=[0.5, 0.3], seed=2, ctx=ctx)
        _same(got.C, want.C, "the call after a call cancelled under way")
    finally:
        ctx.close()


# ---- 7. the known answer on the device ----------------------------------------------------------------------
def test_known_answer_on_the_device(k, orc, gpu_ctx):
    prior, cost = known_answer_case(k)
    r = k.abc_pmc(prior, cost, KA_N, eps=KA_EPS, seed=KA_SEED)
    assert r.info["stop"] == "done" and r.info["generations_run"] == len(KA_EPS)
    check_known_answer(r.theta, r.w, r.C, r.info["log"])
    _same_run(r, po.oracle_pmc(orc, prior, cost, KA_N, eps=KA_EPS, seed=KA_SEED), "known answer")
