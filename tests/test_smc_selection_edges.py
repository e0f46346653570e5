"""CPU: smc's ε-selection (src/smc.jl:131-153) on adversarial cost laws (tests/smc_scenarios.py).
quantile7 (tests/helpers.py, from Statistics.quantile's documented definition) against the oracle's
quantile bit for bit at the edges; the oracle's logged (ε, ESS, flag, resampled) of every iteration against
select_step applied to the oracle's own state one iteration earlier; and, on those states, the coverage
witnesses of the device courses reaching every branch the scenarios were written for."""
import math

import numpy as np
import pytest

import smc_scenarios as S
from helpers import (NO_ALIVE, key_of, quantile7, select_step, witness_dsel2, witness_loop,
                     witness_select)

TINY = 5e-324
QUANTILE_EDGES = [
    ([3.5], [0.0, 0.3, 1.0]),
    ([1.0, 2.0], [0.0, 0.25, 0.5, 1.0]),
    ([7.0] * 5, [0.0, 0.5, 0.95]),
    ([-0.0, 0.0, -0.0, 0.0], [0.1, 0.5, 0.9]),
    ([-1.0, -0.0, 0.0, 1.0], [1 / 3, 0.5, 2 / 3]),
    ([1.0, 2.0, math.inf, math.inf], [0.2, 1 / 3, 0.5, 0.9]),          # +Inf above: γ = 0 -> NaN, γ > 0 -> Inf
    ([-math.inf, -math.inf, 1.0, 2.0], [0.2, 1 / 3, 0.5, 0.9]),        # -Inf below
    ([-math.inf, math.inf], [0.0, 0.5, 1.0]),                         # -Inf + Inf
    ([-math.inf, -math.inf, math.inf], [0.25, 0.5, 0.75]),
    ([math.inf] * 3, [0.5]),
    ([-math.inf] * 3, [0.5]),
    ([0.0, TINY, 2 * TINY, 3 * TINY, 1e-310], [0.1, 0.3, 0.45, 0.7, 0.99]),   # subnormals
    ([-3 * TINY, -TINY, -0.0, TINY], [0.2, 0.5, 0.8]),
]


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or (a == b and math.copysign(1, a) == math.copysign(1, b))


def test_quantile7_equals_oracle_at_the_edges(orc):
    rng = np.random.default_rng(3)
    n_nan = n_gamma0 = 0
    for v, ps in QUANTILE_EDGES:
        for p in ps:
            for perm in (v, list(rng.permutation(np.array(v)))):
                got, ref = quantile7(perm, p), orc.quantile(np.array(perm), p)
                assert _same(got, ref), (v, p, got, ref)
                n_nan += math.isnan(got)
                aleph = len(v) * p + (1 - p)
                n_gamma0 += aleph == int(aleph)
    assert n_nan >= 4 and n_gamma0 >= 10
    # random draws from the scenario tables: mixed signs, ties, zeros, infinities
    for name in ("signed_zero", "inf_tail", "subnormal", "neg_inf_head", "cluster_outliers"):
        t = S.build(name, 300 if name != "cluster_outliers" else 70000, orc).table
        for n in (1, 2, 3, 17, 300):
            v = rng.choice(t, n)
            for p in (0.0, 0.05, 0.5, 0.7, 1.0, rng.random()):
                assert _same(quantile7(v, p), orc.quantile(v, p)), (name, n, p)


def _oracle_states(orc, k, sc):
    """the oracle's (C, alive) after k = 0 .. K-1 iterations and its full-length run"""
    cost = sc.cost(k)
    orc.register_user_cost(cost)
    prior = sc.prior(k)
    th0, C0 = sc.initial(orc)
    states = [(C0, np.ones(sc.N, dtype=bool))]
    full = orc.smc(prior, cost, **sc.kw())
    for it in range(1, full["iterations"]):
        r = orc.smc(prior, cost, **sc.kw(max_iterations=it))
        assert np.array_equal(r["C"], sc.costs_of(r["theta_all"]))
        states.append((r["C"], r["alive"]))
    return full, states


SIZES = [(n, N) for n in S.NAMES if n not in S.ERRORS and n != "cluster_outliers" for N in (200, 3000)] + \
    [("cluster_outliers", 1 << 17)]


@pytest.mark.parametrize("name,N", SIZES)
def test_oracle_iterations_equal_select_step(orc, k, name, N):
    sc = S.build(name, N, orc)
    full, states = _oracle_states(orc, k, sc)
    assert full["iterations"] == (1 if name == "neg_inf_head" else sc.K)
    for it, (C, alive) in enumerate(states):
        eps, flag, new, ess, res, err = select_step(C, alive, sc.alpha, sc.min_r_ess, sc.N)
        L = full["log"][it]
        assert err is None
        assert _same(L["eps"], eps) and (L["ess"], L["flag"], L["resampled"]) == (ess, flag, res), (it, L)
    eps = [L["eps"] for L in full["log"]]
    if name == "neg_mixed":
        assert max(eps) > 0 > min(eps)
    if name == "signed_zero":
        assert 0.0 in eps and full["log"][eps.index(0.0)]["flag"] == 0
        C0 = states[0][0]
        assert (np.signbit(C0) & (C0 == 0)).any() and (~np.signbit(C0) & (C0 == 0)).any() and (C0 < 0).any()
    if name == "signed_zero_floor":   # the minimum is -0.0 and ε is +0.0: flag 1 by value, not by key
        C, alive = states[1]
        Xa = C[alive]
        assert Xa.min() == 0 and np.signbit(Xa).any() and (~np.signbit(Xa) & (Xa == 0)).any()
        assert full["log"][1]["eps"] == 0 and not math.copysign(1, full["log"][1]["eps"]) < 0
        assert full["log"][1]["flag"] == 1 and key_of(full["log"][1]["eps"])[0] > key_of(-0.0)[0]
    if name == "inf_tail":
        assert eps[0] == math.inf and full["log"][0]["flag"] == 0 and np.isinf(states[0][0]).any()
        assert np.isfinite(states[1][0][states[1][1]]).all()
    if name == "neg_inf_head":
        assert eps == [-math.inf]
    if name == "subnormal":
        assert any(0 < e < 2.2250738585072014e-308 for e in eps) and 0.0 in eps
    if name == "plateau_ties":
        assert len(set(eps)) == 1
    if name == "cliff":
        assert any(a / b > 1e30 for a, b in zip(eps, eps[1:]) if b > 0)


@pytest.mark.parametrize("name", sorted(S.ERRORS))
@pytest.mark.parametrize("N", [200, 3000])
def test_nan_eps_is_the_no_alive_error(orc, k, name, N):
    """ε = NaN (γ = 0 with b = +Inf, or -Inf + Inf): no particle alive, a resample due: the oracle's error"""
    sc = S.build(name, N, orc)
    cost = sc.cost(k)
    orc.register_user_cost(cost)
    C0 = sc.initial(orc)[1]
    eps, flag, new, ess, res, err = select_step(C0, np.ones(N, dtype=bool), sc.alpha, sc.min_r_ess, N)
    assert math.isnan(eps) and ess == 0 and res == 1 and err == NO_ALIVE
    aleph = N * sc.alpha + (1 - sc.alpha)
    assert (aleph == int(aleph)) == (name == "inf_nan_eps")
    with pytest.raises(orc.OracleError) as e:
        orc.smc(sc.prior(k), cost, **sc.kw())
    assert str(e.value) == NO_ALIVE


def coverage(orc, k, name, N):
    """the branches the witnesses see on the oracle's states of one scenario (the device's, by parity):
    "select:..." the select kernel (and the phase-by-phase course), "loop:..." the loop kernel (257 <= N
    <= 65 536), "dsel2:<stall>" the one-exchange course from iteration 3 on (N > 4096)"""
    seen = set()
    sc = S.build(name, N, orc)
    full, states = _oracle_states(orc, k, sc)
    eps = [L["eps"] for L in full["log"]]
    for it, (C, alive) in enumerate(states):
        w = witness_select(C[alive], sc.alpha)
        seen |= {f"select:{b}" for b in ("state2", "needmin", "above_scan") if w[b]}
        if w["global_rounds"] > 1:
            seen.add("select:global_rounds>1")
        if w["list_rounds"] > 1:
            seen.add("select:list_rounds>1")
        if 257 <= N <= 65536:
            wl = witness_loop(C, alive, sc.alpha, eps[it - 1] if it >= 1 else None,
                              eps[it - 2] if it >= 2 else None)
            if wl["pred"]:
                seen.add("loop:hit" if wl["hit"] else "loop:miss")
            seen |= {f"loop:{b}" for b in ("over512", "state2") if wl[b]}
            if wl["ncand"] > 1024:
                seen.add("loop:error4")
        if N > 4096 and it >= 2:
            seen.add(f"dsel2:{witness_dsel2(C[alive], sc.alpha, eps[it - 1], eps[it - 2], eps[it], N)}")
    return seen


# the branches each scenario reaches at the sizes the GPU suite runs it (loop kernel 4 000 particles,
# the other courses 6 000; cluster_outliers 2^16 and 2^17)
EXPECTED = {
    "cliff": {"dsel2:3", "loop:hit", "loop:over512", "loop:state2", "select:list_rounds>1", "select:state2"},
    "cluster_outliers": {"dsel2:2", "loop:hit", "loop:over512", "select:global_rounds>1", "select:needmin"},
    "dead_pile": {"dsel2:3", "loop:error4", "loop:hit", "loop:over512", "loop:state2", "select:list_rounds>1", "select:needmin", "select:state2"},
    "gap_needmin": {"dsel2:3", "loop:hit", "loop:over512", "select:above_scan", "select:global_rounds>1", "select:list_rounds>1", "select:needmin"},
    "inf_tail": {"dsel2:1", "loop:hit", "loop:over512", "select:above_scan", "select:global_rounds>1", "select:list_rounds>1", "select:needmin"},
    "neg_inf_head": {"loop:over512", "loop:state2", "select:list_rounds>1", "select:state2"},
    "neg_mixed": {"dsel2:3", "loop:hit", "loop:miss", "loop:over512", "select:global_rounds>1", "select:list_rounds>1", "select:needmin"},
    "plateau_ties": {"dsel2:1", "loop:hit", "loop:over512", "loop:state2", "select:global_rounds>1", "select:list_rounds>1", "select:state2"},
    "signed_zero": {"dsel2:3", "dsel2:7", "loop:hit", "loop:miss", "loop:over512", "loop:state2", "select:list_rounds>1", "select:needmin", "select:state2"},
    "signed_zero_floor": {"dsel2:1", "loop:hit", "loop:over512", "loop:state2", "select:global_rounds>1", "select:list_rounds>1", "select:state2"},
    "subnormal": {"dsel2:2", "dsel2:3", "loop:hit", "loop:over512", "loop:state2", "select:global_rounds>1", "select:list_rounds>1", "select:needmin", "select:state2"},
}
GPU_SIZES = {n: ((1 << 16, 1 << 17) if n == "cluster_outliers" else (4000, 6000)) for n in S.NAMES if n not in S.ERRORS}


@pytest.mark.parametrize("name", sorted(GPU_SIZES))
def test_witnesses_reach_the_designed_branches(orc, k, name):
    seen = set().union(*(coverage(orc, k, name, N) for N in GPU_SIZES[name]))
    assert EXPECTED[name] <= seen, (name, sorted(seen))


def test_witnesses_reach_every_branch():
    """every branch of the device courses that the witnesses model is reached by some scenario"""
    union = set().union(*EXPECTED.values())
    assert {"select:global_rounds>1", "select:list_rounds>1", "select:state2", "select:needmin",
            "select:above_scan", "loop:hit", "loop:miss", "loop:over512", "loop:state2", "loop:error4",
            "dsel2:1", "dsel2:2", "dsel2:3", "dsel2:7"} <= union, sorted(union)
