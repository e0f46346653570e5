"""-m gpu: ABCDE (src/smc.jl:347-430) and pfilter (:275-340) on adversarial cost laws
(tests/population_scenarios.py) on every device course.  ABCDE answers s = rand((1:N)[Δs .<= Δs[i]]) in the
one-workgroup kernel, by the generation kernel's own scans, the sixteen-lane teams, the sorted blocks (one and
two keys per lane) and the radix sort + wavelet matrix; pfilter takes ϵ = quantile(C, q) and idxok from the
select kernel with the rejection loop inside one launch or a launch per attempt; ABCDE_batch and pfilter_batch
run three seeds as the workgroups of one launch (pfilter_batch: ϵ and idxok by pf_select_workgroup).

Each run equals the oracle bit for bit, and on the single-run courses generation / iteration k + 1 of the
device equals abcde_step / pfilter_step (tests/helpers.py) of the device's own state after k, which does not go
through the oracle.  Every case is replayed on the CPU first (population_scenarios.replay_*: the gate that
test_population_cost_edges.py asserts for the same cases), so nothing runs here that does not end.

pf_small_kernel, the default course of pfilter up to 256 particles, takes the built-in costs only: a run-time
compiled cost at 130 particles goes phase by phase ("default-130").  It meets the finite tables through a state
handed to resume=, whose costs are table entries under a built-in cost (the last test)."""
import math

import numpy as np
import pytest

import population_scenarios as S
from helpers import abcde_step, bits_equal, pfilter_step

pytestmark = pytest.mark.gpu


def _env(monkeypatch, names, env):
    for v in names:
        monkeypatch.delenv(v, raising=False)
    for a, b in env.items():
        monkeypatch.setenv(a, b)


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def _problem(k, orc, name, N):
    sc = S.build(name, N)
    cost = sc.cost(k)
    orc.register_user_cost(cost)
    return sc, sc.prior(k), cost


# ---- ABCDE
def _abcde_equals_oracle(got, ref, what):
    assert bits_equal(got.P, ref["P"]) and bits_equal(got.C, ref["C"]), what
    assert got.reached_ϵ == ref["reached_eps"], what
    assert got.info["generations_run"] == ref["generations_run"] and got.info["nsims"] == ref["nsims"], what


def _abcde_state(s):
    return dict(theta=s.theta[:, 0].copy(), C=s.cost.copy(), logpi=s.logprior.copy(), generation=s.generation, nsims=s.nsims)


ABCDE_CASES = [(name, course, leg) for course, (_, _, only) in S.ABCDE_COURSES.items() for name in (only or S.NAMES)
               for leg in S.ABCDE_LEGS]


@pytest.mark.parametrize("name,course,leg", ABCDE_CASES)
def test_abcde_cost_edges_on_every_course(k, orc, gpu_ctx, monkeypatch, name, course, leg):
    env, N, _ = S.ABCDE_COURSES[course]
    _env(monkeypatch, S.ABCDE_ENV, env)
    S.replay_abcde(k, orc, name, N, leg)      # the gate
    sc, prior, cost = _problem(k, orc, name, N)
    pb = sc.problem(k, orc)
    got = k.ABCDE(prior, cost, sc.eps_target, return_array=True, return_state=True, **sc.abcde_kw(N, leg))
    _abcde_equals_oracle(got, orc.abcde(prior, cost, sc.eps_target, **sc.abcde_kw(N, leg)), (name, course, leg))
    assert got.info["generations_run"] == S.GENERATIONS
    # generation g + 1 from the device's own state after g (a generations = g run), without the oracle
    st = None
    for g in range(S.GENERATIONS + 1):
        r = got if g == S.GENERATIONS else k.ABCDE(prior, cost, sc.eps_target, return_array=True, return_state=True,
                                                   **sc.abcde_kw(N, leg, generations=g))
        dev = _abcde_state(r.info["state"])
        if st is not None:
            nxt = abcde_step(pb, st, eps_target=sc.eps_target, **S.ABCDE_LEGS[leg])
            for f in ("theta", "C", "logpi"):
                assert bits_equal(dev[f], nxt[f]), (name, course, leg, g, f)
            assert (dev["generation"], dev["nsims"]) == (nxt["generation"], nxt["nsims"]), (name, course, leg, g)
        st = dev


@pytest.mark.parametrize("leg", list(S.ABCDE_LEGS))
@pytest.mark.parametrize("name", S.NAMES)
def test_abcde_batch_cost_edges(k, orc, gpu_ctx, monkeypatch, name, leg):
    """three seeds as the workgroups of one launch; every run against the single-run oracle"""
    _env(monkeypatch, S.ABCDE_ENV, {})
    N = S.ABCDE_BATCH_N
    sc, prior, cost = _problem(k, orc, name, N)
    for seed in sc.batch_seeds:
        S.replay_abcde(k, orc, name, N, leg, seed)      # the gate
    kw = sc.abcde_kw(N, leg)
    del kw["seed"]
    got = k.ABCDE_batch(prior, cost, sc.eps_target, len(sc.batch_seeds), seeds=list(sc.batch_seeds), return_array=True, **kw)
    assert got.info["course"] == "grid" and got.info["launches"] == 1
    for r, seed in enumerate(sc.batch_seeds):
        _abcde_equals_oracle(got[r], orc.abcde(prior, cost, sc.eps_target, **sc.abcde_kw(N, leg, seed=seed)), (name, leg, seed))


# ---- pfilter
def _pfilter_equals_oracle(got, ref, what):
    assert bits_equal(got.P, ref["P"]) and bits_equal(got.C, ref["C"]), what
    for f in ("iterations", "nreps", "cost_evals"):
        assert got.info[f] == ref[f], (what, f, got.info[f], ref[f])
    assert _same(got.info["eps"], ref["eps"]) and _same(got.info["eff"], ref["eff"]), what


def _neg_mixed_runs_correctly(k, orc, N, run):
    """the same context after an error: a normal case, bit for bit"""
    sc, prior, cost = _problem(k, orc, "neg_mixed", N)
    _pfilter_equals_oracle(run(prior, cost, sc), orc.pfilter(prior, cost, N, **sc.pf_kw()), "after the error")


@pytest.mark.parametrize("name,course", [(name, course) for course in S.PF_COURSES for name in S.NAMES])
def test_pfilter_cost_edges_on_every_course(k, orc, gpu_ctx, monkeypatch, name, course):
    from kissabc_jl_amd import _cdefs as cd
    env, N = S.PF_COURSES[course]
    _env(monkeypatch, S.PF_ENV, env)
    states, nan = S.replay_pfilter(k, orc, name, N)      # the gate
    sc, prior, cost = _problem(k, orc, name, N)
    pb = sc.problem(k, orc)
    run = lambda prior, cost, sc, **kw: k.pfilter(prior, cost, N, return_array=True, **sc.pf_kw(**kw))  # noqa: E731
    if nan:
        # a NaN accepted by `Cp > ϵ` being false (:320): the next quantile(C, q) throws in the reference
        with pytest.raises(orc.OracleError) as eo:
            orc.pfilter(prior, cost, N, **sc.pf_kw())
        with pytest.raises(k.KabcError) as e:
            run(prior, cost, sc)
        assert str(e.value) == str(eo.value) == S.PF_NAN_ERROR
        assert e.value.status == eo.value.status == cd.KABC_ERR_NAN_COST
        _neg_mixed_runs_correctly(k, orc, N, run)
        niter = len(states) - 1        # (the iterations before the error are checked below)
    else:
        got = run(prior, cost, sc)
        _pfilter_equals_oracle(got, orc.pfilter(prior, cost, N, **sc.pf_kw()), (name, course))
        niter = got.info["iterations"]
    # iteration it + 1 from the device's own state after it (a max_iters = it - 1 run; the state after the
    # initial draw is the restated one), without the oracle
    st = states[0]
    for it in range(1, niter + 1):
        r = k.pfilter(prior, cost, N, return_array=True, return_state=True, **sc.pf_kw(max_iters=it - 1))
        s = r.info["state"]
        nxt = pfilter_step(pb, st, q=S.PF_KW["q"])
        what = (name, course, it)
        assert bits_equal(s.theta[:, 0], nxt["theta"]) and bits_equal(s.cost, nxt["C"]), what
        assert bits_equal(s.logprior, nxt["logpi"]), what
        assert (s.iteration, s.nreps, s.cost_evals) == (nxt["iteration"], nxt["nreps"], nxt["cost_evals"]), what
        assert _same(s.eps, nxt["eps"]) and _same(s.eff, nxt["eff"]), what
        st = dict(theta=s.theta[:, 0].copy(), C=s.cost.copy(), logpi=s.logprior.copy(), iteration=s.iteration,
                  nreps=s.nreps, cost_evals=s.cost_evals)


@pytest.mark.parametrize("name", S.NAMES)
def test_pfilter_batch_cost_edges(k, orc, gpu_ctx, monkeypatch, name):
    """three seeds as the workgroups of one launch (ϵ, idxok: pf_select_workgroup); every run against the
    single-run oracle, an error of the oracle being that run's status"""
    from kissabc_jl_amd import _cdefs as cd
    _env(monkeypatch, S.PF_ENV, {})
    N = S.PF_BATCH_N
    sc, prior, cost = _problem(k, orc, name, N)
    refs = []
    for seed in sc.batch_seeds:
        S.replay_pfilter(k, orc, name, N, seed)      # the gate
        try:
            refs.append(orc.pfilter(prior, cost, N, **sc.pf_kw(seed=seed)))
        except orc.OracleError as e:
            assert str(e) == S.PF_NAN_ERROR and e.status == cd.KABC_ERR_NAN_COST
            refs.append(None)
    assert any(r is None for r in refs) == (name == "nan_holes")
    kw = sc.pf_kw()
    del kw["seed"]
    batch = lambda prior, cost: k.pfilter_batch(prior, cost, N, len(sc.batch_seeds), seeds=list(sc.batch_seeds),  # noqa: E731
                                                return_array=True, **kw)
    if name == "nan_holes":
        with pytest.raises(k.KabcError) as e:
            batch(prior, cost)
        first = [r is None for r in refs].index(True)
        assert str(e.value) == f"run {first}: {S.PF_NAN_ERROR}" and e.value.status == cd.KABC_ERR_NAN_COST
        got = e.value.results
    else:
        got = batch(prior, cost)
    assert got.info["course"] == "grid" and got.info["launches"] == 1
    for r, ref in enumerate(refs):
        if ref is None:
            assert got[r] is None and got.info["status"][r] == cd.KABC_ERR_NAN_COST
        else:
            assert got.info["status"][r] == 0
            _pfilter_equals_oracle(got[r], ref, (name, sc.batch_seeds[r]))
    if name == "nan_holes":   # the same context goes on with a normal case
        sc2, prior2, cost2 = _problem(k, orc, "neg_mixed", N)
        for r, seed in enumerate(sc.batch_seeds):
            _pfilter_equals_oracle(batch(prior2, cost2)[r], orc.pfilter(prior2, cost2, N, **sc2.pf_kw(seed=seed)), seed)


@pytest.mark.parametrize("scheme", ["one-workgroup", "launch-per-phase"])
@pytest.mark.parametrize("name", S.CRAFTED_NAMES)
def test_pf_small_kernel_selects_on_a_state_of_table_costs(k, orc, gpu_ctx, monkeypatch, name, scheme):
    """pf_small_kernel (built-in costs only) continues a state whose costs are table entries
    (population_scenarios.crafted_pfilter_case): its ϵ by rank counting and idxok from ballots, and the
    iteration they feed, equal pfilter_step of that state -- without the oracle -- and the oracle's continuation;
    so do the launches per phase.  kabc_ctx_last_kernel names the course that ran."""
    from kissabc_jl_amd import _lib
    from prebuilt_matrix import FAMILY_ID
    _env(monkeypatch, S.PF_ENV, {} if scheme == "one-workgroup" else {"KABC_PF_SMALL": "0"})
    prior, cost, state, nxt = S.crafted_pfilter_case(k, orc, name)      # the gate
    got = k.pfilter(prior, cost, resume=state, return_array=True, return_state=True, ctx=gpu_ctx, **S.CRAFTED_KW)
    assert _lib.last_kernel(gpu_ctx)[0] == FAMILY_ID["PF_SMALL" if scheme == "one-workgroup" else "PF_PHASES"]
    s = got.info["state"]
    assert bits_equal(s.theta[:, 0], nxt["theta"]) and bits_equal(s.cost, nxt["C"]) and bits_equal(s.logprior, nxt["logpi"])
    assert (s.iteration, s.nreps, s.cost_evals) == (nxt["iteration"], nxt["nreps"], nxt["cost_evals"])
    assert _same(s.eps, nxt["eps"]) and _same(s.eff, nxt["eff"])
    prior, cost, state, _ = S.crafted_pfilter_case(k, orc, name)
    _pfilter_equals_oracle(got, orc.pfilter(prior, cost, resume=state, **S.CRAFTED_KW), (name, scheme))
