"""CPU: ABC population Monte Carlo on a problem with a known answer, on the oracle restatement alone
(tests/abc_pmc_oracle.py; tests/test_gpu_abc_pmc.py runs the same case on the device).  Uniform(-10, 10) prior,
cost |x - 1.5|, eps = [4, 2, 1, 0.5]: the last generation targets U(1, 2), mean 1.5, standard deviation 0.5 / sqrt(3).
The bounds are conditions, not measurements: ess / N >= 0.5 and draws_g <= 16 N in every generation (a plain numpy
PMC gave ess / N >= 0.99 and draws <= 3 N); |mean - 1.5| <= 5 (0.5 / sqrt 3) / sqrt(256) = 0.090, five standard errors
at the ess floor; |std - 0.2887| <= 5 * 0.2887 * sqrt(0.8 / (4 * 256)) = 0.040 (the uniform's kurtosis is 1.8)."""
import math

import numpy as np

from abc_pmc_oracle import oracle_pmc

N, EPS, SEED = 512, [4.0, 2.0, 1.0, 0.5], 3


def known_answer_case(k):
    return k.Uniform(-10, 10), k.costs.AbsDiff(1.5)


def check_known_answer(theta, w, C, log):
    """the conditions above on a final population and its per-generation log (eps, draws, ess)"""
    assert len(log) == len(EPS) and [rec["eps"] for rec in log] == EPS
    for rec in log:
        assert rec["ess"] / N >= 0.5, rec
        assert rec["draws"] <= 16 * N, rec
    x = np.asarray(theta).reshape(N)
    assert abs(float(np.sum(w)) - 1.0) <= N * 2.0 ** -52
    assert np.all(C <= EPS[-1]) and np.all((x >= 1.0) & (x <= 2.0))
    mean = float(np.sum(w * x))
    std = math.sqrt(float(np.sum(w * (x - mean) ** 2)))
    assert abs(mean - 1.5) <= 5 * (0.5 / math.sqrt(3)) / math.sqrt(256), mean
    assert abs(std - 0.5 / math.sqrt(3)) <= 5 * (0.5 / math.sqrt(3)) * math.sqrt(0.8 / (4 * 256)), std


def test_known_answer_on_the_oracle(orc, k):
    prior, cost = known_answer_case(k)
    r = oracle_pmc(orc, prior, cost, N, eps=EPS, seed=SEED)
    assert r["stop"] == "done" and r["generations_run"] == len(EPS)
    check_known_answer(r["theta"], r["w"], r["C"], r["log"])
    # every particle's cost is replicate g of its row of the proposal stream
    from kissabc_jl_amd import _cdefs as cd
    g = len(EPS) - 1
    for i in (0, 1, N // 2, N - 1):
        assert r["C"][i] == orc.cost_eval(cost, r["theta"][i], seed=SEED, walker=int(r["index"][i]), t=g,
                                          domain=cd.DOM_EVAL_COST)
    assert np.all(np.diff(r["index"]) > 0) and r["log"][-1]["draws"] == r["index"][-1] + 1


def test_schedules_and_stops_on_the_oracle(orc, k):
    prior, cost = known_answer_case(k)
    # adaptive: the thresholds fall, the target ends the run
    r = oracle_pmc(orc, prior, cost, 64, q=0.5, eps_target=0.5, generations=12, seed=1)
    eps = [rec["eps"] for rec in r["log"]]
    assert eps[0] == math.inf and all(a > b for a, b in zip(eps, eps[1:])) and eps[-1] == 0.5 and r["stop"] == "target"
    # the generation bound
    r = oracle_pmc(orc, prior, cost, 64, q=0.5, generations=3, seed=1)
    assert r["stop"] == "done" and r["generations_run"] == 3
    # exhausted in generation 0 and later: the generation before is the result
    r = oracle_pmc(orc, prior, cost, 64, eps=[1e-9], max_draws=64, seed=1)
    assert r["stop"] == "exhausted" and r["generations_run"] == 0 and r["theta"].shape == (0, 1)
    r = oracle_pmc(orc, prior, cost, 64, eps=[4.0, 1e-9], max_draws=400, seed=1)
    assert r["stop"] == "exhausted" and r["generations_run"] == 1 and r["eps"] == 4.0 and np.all(r["w"] == 1.0 / 64)
    # min_rate
    r = oracle_pmc(orc, prior, cost, 64, eps=[4.0, 2.0, 1.0], min_rate=0.9, seed=1)
    assert r["stop"] == "min_rate" and r["generations_run"] == 1
    # degenerate: a coordinate whose spread underflows (c_11 == 0.0 exactly)
    r = oracle_pmc(orc, k.Factored(k.Normal(0, 1), k.Normal(0, 1e-200)), k.costs.GaussDist([0.0, 0.0]), 32,
                   eps=[math.inf, 1.0], seed=1)
    assert r["stop"] == "degenerate" and r["generations_run"] == 1
