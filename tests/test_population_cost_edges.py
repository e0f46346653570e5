"""CPU: ABCDE (src/smc.jl:347-430) and pfilter (:275-340) on adversarial cost laws (tests/population_scenarios.py).

The oracle, generation by generation and iteration by iteration, against abcde_step and pfilter_step
(tests/helpers.py): restatements in numpy of src/smc.jl:371-420 and :297-333 with a Python Philox, which share
no code with the oracle or the kernels -- each next state of the oracle equals the step of its previous one bit
for bit, counts included.  And the gate: every (scenario, shape, options, seed) that
test_gpu_population_cost_edges.py runs is replayed here (population_scenarios.replay_*), and must end, move at
least 15 % of its rows, draw a donor and meet what the scenario was written for."""
import math

import numpy as np
import pytest

import population_scenarios as S
from helpers import bits_equal, kth_smallest_of_prefix, philox_py, stream_blocks


def test_stream_blocks_equal_the_scalar_philox(orc):
    """the vectorised Philox of the restatements against philox_py (pinned by the Random123 vectors in
    test_math_contract.py) and the oracle's stream, where the counter leaves 32 bits too"""
    R = orc.philox_rounds()
    seed, walkers = 0x0123456789ABCDEF, [0, 1, 5, 2 ** 31, 2 ** 32 - 1]
    for t in (0, 7, 2 ** 32 - 1, (3 << 24) | 17, 2 ** 32 + 3, 0xABCDEF00000003, 2 ** 56 - 1):
        for slot, dom in ((0, 11), (2, 15)):
            lo, hi = stream_blocks(seed, walkers, t, slot, dom, R)
            for j, w in enumerate(walkers):
                ref = philox_py([w, t & 0xffffffff, slot, dom | ((t >> 32) << 8)], [seed & 0xffffffff, seed >> 32], R)
                assert ref == orc.stream_block(seed, w, t, slot, dom)
                assert (int(lo[j]), int(hi[j])) == ((ref[1] << 32) | ref[0], (ref[3] << 32) | ref[2]), (hex(t), w)


def test_kth_smallest_of_prefix_is_the_definition():
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 64, 65, 1000):
        seq = rng.permutation(n)
        r = rng.integers(1, n + 1, 200)
        kk = (rng.random(200) * r).astype(np.int64)
        got = kth_smallest_of_prefix(seq, r, kk)
        assert [int(v) for v in got] == [int(np.sort(seq[:a])[b]) for a, b in zip(r, kk)]


def _same_abcde_state(s, st):
    return (bits_equal(s.theta[:, 0], st["theta"]) and bits_equal(s.cost, st["C"]) and bits_equal(s.logprior, st["logpi"])
            and s.generation == st["generation"] and s.nsims == st["nsims"])


ABCDE_RUNS = [(name, N, leg, S.SEED) for name, N in S.abcde_cases() for leg in S.ABCDE_LEGS] + \
    [(name, S.ABCDE_BATCH_N, leg, seed) for name in S.NAMES for leg in S.ABCDE_LEGS
     for seed in S.build(name, S.ABCDE_BATCH_N).batch_seeds[1:]]


@pytest.mark.parametrize("name,N,leg,seed", ABCDE_RUNS)
def test_abcde_oracle_generations_equal_abcde_step(orc, k, name, N, leg, seed):
    """(the gate of this case is asserted by replay_abcde)"""
    sc = S.build(name, N)
    cost, prior = sc.cost(k), sc.prior(k)
    orc.register_user_cost(cost)
    states = S.replay_abcde(k, orc, name, N, leg, seed)
    prev = None
    for g, st in enumerate(states):
        # the oracle continues its own state; one that holds a cost of -Inf cannot be handed back (resume= takes
        # finite costs only), so those generations are reached from the initial draw
        if prev is not None and np.isfinite(prev.cost).all():
            r = orc.abcde(prior, cost, sc.eps_target, return_state=True, resume=prev,
                          **sc.abcde_kw(N, leg, generations=g, seed=seed))
        else:
            r = orc.abcde(prior, cost, sc.eps_target, return_state=True, **sc.abcde_kw(N, leg, generations=g, seed=seed))
        prev = r["state"]
        assert _same_abcde_state(prev, st), (g, name, N, leg)
        assert bits_equal(prev.cost, sc.table[np.clip(np.trunc(prev.theta[:, 0]), 0, sc.table.size - 1).astype(int)])
    assert r["generations_run"] == S.GENERATIONS and r["nsims"] == states[-1]["nsims"]
    assert bits_equal(r["P"][:, 0], np.rint(states[-1]["theta"])) and bits_equal(r["C"], states[-1]["C"])
    assert r["reached_eps"] == bool(states[-1]["C"].max() <= sc.eps_target)


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def _same_pfilter_state(s, st):
    return (bits_equal(s.theta[:, 0], st["theta"]) and bits_equal(s.cost, st["C"]) and bits_equal(s.logprior, st["logpi"])
            and s.iteration == st["iteration"] and s.nreps == st["nreps"] and s.cost_evals == st["cost_evals"]
            and _same(s.eps, st["eps"]) and _same(s.eff, st["eff"]))


PF_RUNS = [(name, N, S.SEED) for name, N in S.pfilter_cases()] + \
    [(name, S.PF_BATCH_N, seed) for name in S.NAMES for seed in S.build(name, S.PF_BATCH_N).batch_seeds[1:]]


@pytest.mark.parametrize("name,N,seed", PF_RUNS)
def test_pfilter_oracle_iterations_equal_pfilter_step(orc, k, name, N, seed):
    """(the gate of this case is asserted by replay_pfilter).  A NaN cost accepted by `Cp > ϵ` being false (:320)
    makes the next quantile(C, q) throw in the reference: the oracle raises the library's error there."""
    from kissabc_jl_amd import _cdefs as cd
    sc = S.build(name, N)
    cost, prior = sc.cost(k), sc.prior(k)
    orc.register_user_cost(cost)
    states, nan = S.replay_pfilter(k, orc, name, N, seed)
    assert len(states) >= 2
    for st in states[1:]:
        r = orc.pfilter(prior, cost, N, return_state=True, **sc.pf_kw(max_iters=st["iteration"] - 1, seed=seed))
        assert _same_pfilter_state(r["state"], st), (st["iteration"], name, N)
    if nan:
        with pytest.raises(orc.OracleError) as e:
            orc.pfilter(prior, cost, N, **sc.pf_kw(seed=seed))
        assert str(e.value) == S.PF_NAN_ERROR and e.value.status == cd.KABC_ERR_NAN_COST
        return
    r = orc.pfilter(prior, cost, N, **sc.pf_kw(seed=seed))
    last = states[-1]
    assert r["iterations"] == last["iteration"] and _same(r["eps"], last["eps"]) and _same(r["eff"], last["eff"])
    assert r["nreps"] == last["nreps"] and r["cost_evals"] == last["cost_evals"]
    assert bits_equal(r["P"][:, 0], np.rint(last["theta"])) and bits_equal(r["C"], last["C"])


@pytest.mark.parametrize("name", S.CRAFTED_NAMES)
def test_pfilter_oracle_continues_a_state_of_table_costs_as_pfilter_step(orc, k, name):
    """the case that puts the tables in front of pf_small_kernel (population_scenarios.crafted_pfilter_case):
    the oracle's next iteration from that state is pfilter_step's"""
    prior, cost, state, nxt = S.crafted_pfilter_case(k, orc, name)
    r = orc.pfilter(prior, cost, resume=state, return_state=True, **S.CRAFTED_KW)
    assert _same_pfilter_state(r["state"], nxt), name
    assert r["iterations"] == 2 and bits_equal(r["P"][:, 0], np.rint(nxt["theta"]))
