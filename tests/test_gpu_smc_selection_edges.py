"""-m gpu: smc's ε-selection (src/smc.jl:131-153) on adversarial cost laws (tests/smc_scenarios.py) on every
device course: the one-workgroup kernel, the persistent loop kernel, the select kernel on 1, the default and
128 workgroups and launched cooperatively, the one-exchange course, sharded particles (P2P emulated ranks,
world 3, phase by phase and one exchange) and a sharded cost loop (world 2).

Each run equals the oracle bit for bit; on the single-GPU courses every logged iteration k + 1 also equals
select_step (tests/helpers.py) on the device's own state after k iterations (a max_iterations = k run), which
does not go through the oracle.  ε = NaN (ESS = 0 with a resample due) is the oracle's error on every course
and rank, and the context runs a normal case correctly afterwards."""
import math
import threading

import numpy as np
import pytest

import smc_scenarios as S
from helpers import NO_ALIVE, select_step, witness_dsel2, witness_loop

pytestmark = pytest.mark.gpu

_ENV = ("KABC_SMC_LOOP", "KABC_SMC_SPEC_SELECT", "KABC_SMC_SELECT_BLOCKS", "KABC_SMC_COOPERATIVE",
        "KABC_SMC_DIST_LOOKS")
# course: (environment, N, N of cluster_outliers or None)
COURSES = {
    "small": ({}, 200, None),
    "loop": ({"KABC_SMC_LOOP": "1"}, 4000, 1 << 16),
    "select-1": ({"KABC_SMC_LOOP": "0", "KABC_SMC_SPEC_SELECT": "0", "KABC_SMC_SELECT_BLOCKS": "1"}, 6000, 1 << 17),
    "select": ({"KABC_SMC_LOOP": "0", "KABC_SMC_SPEC_SELECT": "0"}, 6000, 1 << 17),
    "select-128": ({"KABC_SMC_LOOP": "0", "KABC_SMC_SPEC_SELECT": "0", "KABC_SMC_SELECT_BLOCKS": "128"},
                   20000, 1 << 17),
    "select-coop": ({"KABC_SMC_LOOP": "0", "KABC_SMC_SPEC_SELECT": "0", "KABC_SMC_COOPERATIVE": "1"},
                    6000, 1 << 17),
    "one-exchange": ({"KABC_SMC_LOOP": "0", "KABC_SMC_SPEC_SELECT": "1"}, 6000, 1 << 17),
}


def _env(monkeypatch, env):
    for v in _ENV:
        monkeypatch.delenv(v, raising=False)
    for a, b in env.items():
        monkeypatch.setenv(a, b)


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def _assert_equal(got, ref, what=""):
    assert got.info["iterations"] == ref["iterations"], what
    assert got.info["log"] == ref["log"], what
    assert _same(got.eps, ref["eps"]), what
    assert np.array_equal(got.info["alive"], ref["alive"]), what
    assert np.array_equal(got.info["theta_all"], ref["theta_all"]), what
    assert np.array_equal(got.C, ref["C"]), what
    assert got.info["cost_evals"] == ref["cost_evals"] and got.info["proposals"] == ref["proposals"], what


def _cases():
    out = []
    for course, (_, n, n_cl) in COURSES.items():
        for name in S.NAMES:
            if name == "dead_pile" and course == "small":
                continue
            if name == "cluster_outliers":
                if n_cl:
                    out.append((name, course, n_cl))
            else:
                out.append((name, course, n))
    return out


@pytest.mark.parametrize("name,course,N", _cases())
def test_selection_edges_on_every_course(k, orc, gpu_ctx, monkeypatch, name, course, N):
    _env(monkeypatch, COURSES[course][0])
    sc = S.build(name, N, orc)
    cost, prior = sc.cost(k), sc.prior(k)
    orc.register_user_cost(cost)
    if name in S.ERRORS:
        with pytest.raises(orc.OracleError) as eo:
            orc.smc(prior, cost, **sc.kw())
        with pytest.raises(k.KabcError) as e:
            k.smc(prior, cost, return_array=True, **sc.kw())
        assert str(e.value) == str(eo.value) == NO_ALIVE
        from kissabc_jl_amd import _cdefs as cd
        assert e.value.status == cd.KABC_ERR_INVALID_STATE
        # the same context goes on with a normal case
        ok = S.build("neg_mixed", N, orc)
        c2 = ok.cost(k)
        orc.register_user_cost(c2)
        _assert_equal(k.smc(ok.prior(k), c2, return_array=True, **ok.kw()), orc.smc(ok.prior(k), c2, **ok.kw()))
        return
    got = k.smc(prior, cost, return_array=True, **sc.kw())
    ref = orc.smc(prior, cost, **sc.kw())
    _assert_equal(got, ref, course)
    # iteration k + 1 of the device's log from the device's own state after k iterations; on those states
    # the witnesses tell whether the loop kernel gives up (error 4) and where the one-exchange course stalls
    e = [x["eps"] for x in got.info["log"]]
    C, alive = sc.initial(orc)[1], np.ones(N, dtype=bool)
    error4, stalls = False, 0
    for it in range(got.info["iterations"]):
        if it:
            r = k.smc(prior, cost, return_array=True, **sc.kw(max_iterations=it))
            assert r.info["iterations"] == it
            C, alive = r.C, r.info["alive"]
            assert np.array_equal(C, sc.costs_of(r.info["theta_all"]))
        eps, flag, _, ess, res, err = select_step(C, alive, sc.alpha, sc.min_r_ess, N)
        L = got.info["log"][it]
        assert err is None and _same(L["eps"], eps), (it, L, eps)
        assert (L["ess"], L["flag"], L["resampled"]) == (ess, flag, res), (it, L)
        if course == "loop":
            wl = witness_loop(C, alive, sc.alpha, e[it - 1] if it >= 1 else None, e[it - 2] if it >= 2 else None)
            error4 |= wl["ncand"] > 1024
        if course == "one-exchange" and it >= 2:
            stalls += witness_dsel2(C[alive], sc.alpha, e[it - 1], e[it - 2], e[it], N) != 0
    d = got.info["dist"]
    if course == "loop":
        # error 4: the loop kernel gave up and the call was repeated on the kernel-per-phase path, which
        # looks at the control block from the host; the persistent kernel makes no host look
        assert (d["host_looks"] > 0) == error4 == (name == "dead_pile"), d
    if course == "one-exchange":
        # the first two selections go phase by phase, then every stalled one
        assert d["phase_by_phase_selections"] == min(2, got.info["iterations"]) + stalls, (d, stalls)


def _ranks(k, comms, fn, timeout=300):
    """one host thread per rank; every rank's result or exception"""
    out = [None] * len(comms)

    def run(r):
        try:
            out[r] = ("ok", fn(comms[r]))
        except Exception as e:
            out[r] = ("err", e)

    th = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(len(comms))]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=timeout)
    assert all(o is not None for o in out), "a rank did not return"
    return out


@pytest.mark.parametrize("name", S.NAMES)
def test_selection_edges_sharded(k, orc, gpu_ctx, monkeypatch, name):
    """sharded particles on 3 emulated ranks (uneven shards; KABC_SMC_DIST_LOOKS 1: phase by phase, 0: one
    exchange) and a sharded cost loop on 2: the oracle's result, or its error, on every rank"""
    _env(monkeypatch, {})
    sc = S.build(name, 1 << 17 if name == "cluster_outliers" else 6000, orc)
    cost, prior = sc.cost(k), sc.prior(k)
    orc.register_user_cost(cost)
    try:
        ref, ref_err = orc.smc(prior, cost, **sc.kw()), None
    except orc.OracleError as e:
        ref, ref_err = None, str(e)
    assert (ref_err is not None) == (name in S.ERRORS)
    for shard, world, looks in (("particles", 3, "1"), ("particles", 3, "0"), ("cost_loop", 2, None)):
        if looks is None:
            monkeypatch.delenv("KABC_SMC_DIST_LOOKS", raising=False)
        else:
            monkeypatch.setenv("KABC_SMC_DIST_LOOKS", looks)
        comms = k.comm.init_all([0] * world, "p2p")
        try:
            out = _ranks(k, comms, lambda c: k.smc(prior, cost, return_array=True, comm=c, shard=shard, **sc.kw()))
        finally:
            for c in comms:
                c.close()
        what = (shard, world, looks)
        for r, (kind, v) in enumerate(out):
            if ref_err is not None:
                assert kind == "err" and isinstance(v, k.KabcError) and str(v) == ref_err, (what, r, v)
            else:
                assert kind == "ok", (what, r, v)
                _assert_equal(v, ref, (what, r))
    if ref_err is not None:   # the context goes on with a normal case
        ok = S.build("neg_mixed", 6000, orc)
        c2 = ok.cost(k)
        orc.register_user_cost(c2)
        _assert_equal(k.smc(ok.prior(k), c2, return_array=True, **ok.kw()), orc.smc(ok.prior(k), c2, **ok.kw()))
