"""CPU: the oracle's population runs from a state and into one (orc.smc / orc.abcde / orc.pfilter with resume= and
return_state=, orc_*_run_from): the run in two segments IS the whole run, bit for bit, wherever it is split -- the
result, the counts, the log and the end state.  With that the oracle is a reference for a continued device run
(the -m gpu resume files and tests/test_gpu_stream_counter.py), from states no short run reaches."""
import math

import numpy as np
import pytest


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _base(k):
    return k.Factored(k.Uniform(-5, 5), k.Uniform(-5, 5)), k.costs.GaussDist([0.5, -0.3])


def _same_arrays(a, b, names, what):
    for name in names:
        assert np.array_equal(_bits(a[name]), _bits(b[name])), (what, name)


def _same_state(a, b, arrays, scalars, floats, what):
    for name in arrays:
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, name)
    for name in scalars:
        assert getattr(a, name) == getattr(b, name), (what, name)
    for name in floats:
        assert _bits(getattr(a, name)) == _bits(getattr(b, name)), (what, name)


SMC_M = 9
SMC_KW = dict(alpha=0.75, min_r_ess=0.3, seed=5, r_epstol=0.0, mcmc_tol=0.0, epstol=-1e308)


@pytest.mark.parametrize("variant", ["base", "retrys", "discrete"])
def test_smc_split_equals_whole_at_every_boundary(k, orc, variant):
    prior, cost = _base(k)
    kw, N = dict(SMC_KW), 100
    if variant == "retrys":      # the pass counter is not the iteration
        kw.update(mcmc_retrys=3, mcmc_tol=0.45)
        N = 200                  # (100 particles end at iteration 3: fewer than mcmc_tol N acceptances)
    if variant == "discrete":    # the state holds the walkers between the integers the result rounds them to
        prior, cost = k.Factored(k.DiscreteUniform(-20, 20), k.Uniform(-5, 5)), k.costs.GaussDist([3.0, -0.3])
    whole = orc.smc(prior, cost, nparticles=N, max_iterations=SMC_M, return_state=True, **kw)
    assert whole["iterations"] == SMC_M and len(whole["log"]) == SMC_M
    passes = [rec["passes"] for rec in whole["log"]]
    assert any(rec["resampled"] for rec in whole["log"]) and any(rec["ess"] < N for rec in whole["log"])
    if variant == "retrys":
        assert max(passes) > 1 and whole["state"].pass_count == sum(passes) > SMC_M
    if variant == "discrete":
        assert np.any(whole["state"].theta != np.rint(whole["state"].theta))
    plain = orc.smc(prior, cost, nparticles=N, max_iterations=SMC_M, **kw)     # (without a state: the same run)
    _same_arrays(plain, whole, ("theta_all", "C"), variant)
    assert plain["log"] == whole["log"] and "state" not in plain
    for split in range(1, SMC_M):
        first = orc.smc(prior, cost, nparticles=N, max_iterations=split, return_state=True, **kw)
        st = first["state"]
        assert st.iteration == split == first["iterations"] and st.pass_count == sum(passes[:split])
        assert first["log"] == whole["log"][:split] == st.log
        kw2 = {key: v for key, v in kw.items() if key != "seed"}                 # (the seed is the state's)
        got = orc.smc(prior, cost, resume=st, max_iterations=SMC_M, return_state=True, **kw2)
        what = (variant, split)
        _same_arrays(got, whole, ("theta_all", "C"), what)
        assert np.array_equal(got["alive"], whole["alive"]), what
        assert _bits(got["eps"]) == _bits(whole["eps"]), what
        for name in ("iterations", "n_alive", "cost_evals", "proposals"):
            assert got[name] == whole[name], (what, name)
        assert got["log"] == whole["log"][split:], what                          # (this call's records)
        _same_state(got["state"], whole["state"], ("theta", "cost", "logprior", "alive"),
                    ("seed", "iteration", "pass_count", "accepted", "cost_evals", "proposals", "n_alive", "log"),
                    ("eps", "eps_prev"), what)


def test_smc_stop_tests_are_applied_to_the_state_first(k, orc):
    prior, cost = _base(k)
    kw = dict(SMC_KW, epstol=3.5)
    first = orc.smc(prior, cost, nparticles=100, max_iterations=SMC_M, return_state=True, **kw)
    assert first["iterations"] < SMC_M and first["eps"] <= 3.5                  # stopped by the rule
    st = first["state"]
    same = orc.smc(prior, cost, resume=st, max_iterations=SMC_M, return_state=True, **kw)
    assert same["iterations"] == first["iterations"] and same["log"] == []
    _same_arrays(same, first, ("theta_all", "C"), "same options")
    _same_state(same["state"], st, ("theta", "cost", "logprior", "alive"),
                ("iteration", "pass_count", "accepted", "cost_evals", "proposals", "n_alive"), ("eps", "eps_prev"), "")
    # max_iterations reached at the state: nothing more either
    capped = orc.smc(prior, cost, resume=st, max_iterations=st.iteration, **dict(kw, epstol=-1e308))
    assert capped["iterations"] == st.iteration and capped["log"] == []
    # a smaller epstol: the run goes on, to where a fresh run with that epstol stops
    kw2 = dict(kw, epstol=2.0)
    fresh = orc.smc(prior, cost, nparticles=100, max_iterations=SMC_M, **kw2)
    assert fresh["iterations"] > first["iterations"]
    more = orc.smc(prior, cost, resume=st, max_iterations=SMC_M, **kw2)
    _same_arrays(more, fresh, ("theta_all", "C"), "smaller epstol")
    assert more["iterations"] == fresh["iterations"] and more["log"] == fresh["log"][st.iteration:]


@pytest.mark.parametrize("earlystop", [False, True])
def test_abcde_split_equals_whole_at_every_boundary(k, orc, earlystop):
    prior, cost = _base(k)
    kw = dict(nparticles=60, alpha=0.3, earlystop=earlystop, seed=4)
    eps_target, ABCDE_G = (4.5, 20) if earlystop else (0.2, 8)
    whole = orc.abcde(prior, cost, eps_target, generations=ABCDE_G, return_state=True, **kw)
    if earlystop:   # the run ends in the break, which counts its iteration and draws nothing (:373 before :379)
        assert whole["reached_eps"] and 2 < whole["generations_run"] < ABCDE_G
        assert whole["state"].generation == whole["generations_run"] - 1
    else:
        assert whole["generations_run"] == ABCDE_G == whole["state"].generation and whole["nsims"] > 0
    plain = orc.abcde(prior, cost, eps_target, generations=ABCDE_G, **kw)
    _same_arrays(plain, whole, ("P", "C"), earlystop)
    for split in range(0, whole["state"].generation + 1):
        first = orc.abcde(prior, cost, eps_target, generations=split, return_state=True, **kw)
        st = first["state"]
        assert st.generation == split and st.nparticles == 60
        kw2 = {key: v for key, v in kw.items() if key not in ("seed", "nparticles")}
        got = orc.abcde(prior, cost, eps_target, resume=st, generations=ABCDE_G, return_state=True, **kw2)
        what = (earlystop, split)
        _same_arrays(got, whole, ("P", "C"), what)
        for name in ("reached_eps", "generations_run", "nsims"):
            assert got[name] == whole[name], (what, name)
        _same_state(got["state"], whole["state"], ("theta", "cost", "logprior"), ("seed", "generation", "nsims"), (),
                    what)
    # a state that already holds `generations` generations comes back unchanged
    st = whole["state"]
    again = orc.abcde(prior, cost, eps_target, resume=st, generations=st.generation, return_state=True,
                      alpha=0.3, earlystop=False)
    assert again["generations_run"] == st.generation and again["nsims"] == st.nsims
    assert np.array_equal(_bits(again["state"].theta), _bits(st.theta))


PF_KW = dict(q=0.9, eff_tol=0.0, epstol=-math.inf, seed=3)
PF_M = 7


@pytest.mark.parametrize("N", [100, 5])       # (5 is raised to the effective N of src/smc.jl:276-279)
def test_pfilter_split_equals_whole_at_every_boundary(k, orc, N):
    prior, cost = _base(k)
    whole = orc.pfilter(prior, cost, N, max_iters=PF_M, return_state=True, **PF_KW)
    assert whole["iterations"] == PF_M + 1 == whole["state"].iteration          # (:332 tests iters > max_iters)
    n_eff = whole["state"].nparticles
    assert n_eff == whole["P"].shape[0] >= N
    plain = orc.pfilter(prior, cost, N, max_iters=PF_M, **PF_KW)
    _same_arrays(plain, whole, ("P", "C"), N)
    for split in range(1, PF_M + 1):
        first = orc.pfilter(prior, cost, N, max_iters=split - 1, return_state=True, **PF_KW)
        st = first["state"]
        assert st.iteration == split == first["iterations"] and st.nparticles == n_eff
        assert (st.nreps, st.cost_evals) == (first["nreps"], first["cost_evals"])
        kw2 = {key: v for key, v in PF_KW.items() if key != "seed"}
        got = orc.pfilter(prior, cost, resume=st, max_iters=PF_M, return_state=True, **kw2)
        what = (N, split)
        _same_arrays(got, whole, ("P", "C"), what)
        for name in ("iterations", "nreps", "cost_evals"):
            assert got[name] == whole[name], (what, name)
        assert _bits(got["eps"]) == _bits(whole["eps"]) and _bits(got["eff"]) == _bits(whole["eff"]), what
        _same_state(got["state"], whole["state"], ("theta", "cost", "logprior"),
                    ("seed", "iteration", "nreps", "cost_evals"), ("eps", "eff"), what)
        # the stop tests on the state, with the call's options: max_iters used up -> unchanged
        same = orc.pfilter(prior, cost, resume=st, max_iters=split - 1, return_state=True, **kw2)
        assert same["iterations"] == split and same["nreps"] == st.nreps
        assert np.array_equal(_bits(same["state"].theta), _bits(st.theta))


def test_pfilter_stop_rules_at_the_state(k, orc):
    prior, cost = _base(k)
    kw = dict(q=0.9, seed=3, epstol=-math.inf)
    first = orc.pfilter(prior, cost, 100, eff_tol=0.5, max_iters=50, return_state=True, **kw)
    assert first["iterations"] < 50 and first["eff"] < 0.5                       # stopped by eff_tol
    st = first["state"]
    same = orc.pfilter(prior, cost, resume=st, eff_tol=0.5, max_iters=50, q=0.9, epstol=-math.inf)
    assert same["iterations"] == first["iterations"] and same["nreps"] == first["nreps"]
    _same_arrays(same, first, ("P", "C"), "same options")
    # a smaller eff_tol: it goes on, to where a fresh run with that eff_tol stops
    fresh = orc.pfilter(prior, cost, 100, eff_tol=0.3, max_iters=50, **kw)
    assert fresh["iterations"] > first["iterations"]
    more = orc.pfilter(prior, cost, resume=st, eff_tol=0.3, max_iters=50, q=0.9, epstol=-math.inf)
    _same_arrays(more, fresh, ("P", "C"), "smaller eff_tol")
    assert (more["iterations"], more["nreps"], more["cost_evals"]) == (fresh["iterations"], fresh["nreps"],
                                                                       fresh["cost_evals"])
