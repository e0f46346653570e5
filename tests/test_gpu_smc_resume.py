"""-m gpu: a stopped smc run continued from its state (kabc_smc_run_from; smc(return_state=, resume=)) IS the
uninterrupted run -- theta_all, C, alive, eps, iterations, log, cost_evals and proposals, bit for bit -- on every
device course (the environments and sizes of tests/test_gpu_smc_selection_edges.py), wherever the run was split:
at every iteration boundary, in three segments, through save / load, with retry passes (the pass counter is not
the iteration), with a discrete prior (the walkers sit between integers), with a prepared cost's ring of passes,
by a stop rule, across the repetitions on another course, and by a cancel.  Every comparison is between device
runs; the uninterrupted runs are pinned to the oracle elsewhere (and once per course at the end of this file)."""
import ctypes as C
import math
import threading
import time

import numpy as np
import pytest

import smc_scenarios as S
from test_gpu_smc_selection_edges import _ENV, COURSES

pytestmark = pytest.mark.gpu

HOOKS = ("KABC_SMC_LOOP_GIVE_UP", "KABC_SMC_SELECT_TIME_OUT", "KABC_SMC_SMALL")
FOUR = ["small", "loop", "select", "one-exchange"]
M = 9
BASE_KW = dict(alpha=0.75, min_r_ess=0.3, seed=5, r_epstol=0.0, mcmc_tol=0.0, epstol=-1e308)
_REF = {}   # (course, variant) -> the uninterrupted run, computed once and never changed


def _env(monkeypatch, course, **extra):
    for v in _ENV + HOOKS:
        monkeypatch.delenv(v, raising=False)
    for a, b in dict(COURSES[course][0], **extra).items():
        monkeypatch.setenv(a, b)
    return COURSES[course][1]


def _base(k):
    return k.Factored(k.Uniform(-5, 5), k.Uniform(-5, 5)), k.costs.GaussDist([0.5, -0.3])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _assert_same(got, ref, what=""):
    assert got.info["iterations"] == ref.info["iterations"], what
    assert got.info["log"] == ref.info["log"], what
    assert _bits(got.eps) == _bits(ref.eps), what
    assert np.array_equal(got.info["alive"], ref.info["alive"]), what
    assert np.array_equal(_bits(got.info["theta_all"]), _bits(ref.info["theta_all"])), what
    assert np.array_equal(_bits(got.C), _bits(ref.C)), what
    assert got.info["cost_evals"] == ref.info["cost_evals"], what
    assert got.info["proposals"] == ref.info["proposals"], what
    assert got.info["n_alive"] == ref.info["n_alive"], what


def _assert_same_state(a, b, what=""):
    for name in ("theta", "cost", "logprior"):
        assert np.array_equal(_bits(getattr(a, name)), _bits(getattr(b, name))), (what, name)
    assert np.array_equal(a.alive, b.alive), what
    for name in ("nparticles", "D", "seed", "iteration", "pass_count", "accepted", "cost_evals", "proposals", "n_alive"):
        assert getattr(a, name) == getattr(b, name), (what, name)
    assert _bits(a.eps) == _bits(b.eps) and _bits(a.eps_prev) == _bits(b.eps_prev), what
    assert a.log == b.log, what


def _reference(k, course, variant, N, kw):
    """the uninterrupted run of the base problem (call with the course's environment set)"""
    key = (course, variant)
    if key not in _REF:
        prior, cost = _base(k)
        _REF[key] = k.smc(prior, cost, nparticles=N, return_array=True, **kw)
    return _REF[key]


def _base_reference(k, course, N):
    ref = _reference(k, course, "base", N, dict(BASE_KW, max_iterations=M))
    log = ref.info["log"]
    # what the splits rely on, on the device's own log: nine iterations, resamples at 4 and 8, dead particles at
    # every other boundary
    assert ref.info["iterations"] == M, log
    assert [i + 1 for i, rec in enumerate(log) if rec["resampled"]] == [4, 8], log
    assert all(rec["ess"] < N for rec in log), log
    return ref


def _segments(k, prior, cost, N, kw, bounds, via=None, **smc_kw):
    """the run in segments ending at `bounds`; `via`: a function every state passes through"""
    state, out = None, None
    for m in bounds:
        more = dict(resume=state) if state is not None else dict(nparticles=N)
        out = k.smc(prior, cost, return_array=True, return_state=True, **more, **dict(kw, max_iterations=m), **smc_kw)
        state = out.info["state"]
        assert state.iteration == out.info["iterations"] and state.nparticles == N
        assert out.info.get("first_iteration", 0) == (0 if "nparticles" in more else more["resume"].iteration)
        if via:
            state = via(state)
    return out


@pytest.mark.parametrize("split", list(range(1, M)))
@pytest.mark.parametrize("course", FOUR)
def test_split_at_every_boundary(k, gpu_ctx, monkeypatch, course, split):
    N = _env(monkeypatch, course)
    ref = _base_reference(k, course, N)
    prior, cost = _base(k)
    got = _segments(k, prior, cost, N, BASE_KW, [split, M])
    assert got.info["first_iteration"] == split
    _assert_same(got, ref, (course, split))
    st = got.info["state"]
    assert (st.iteration, st.cost_evals, st.proposals) == (M, ref.info["cost_evals"], ref.info["proposals"])
    assert st.pass_count == ref.info["mcmc_launches"] == got.info["mcmc_launches"]


@pytest.mark.parametrize("course", FOUR)
def test_three_segments_and_a_checkpoint_on_disk(k, gpu_ctx, monkeypatch, tmp_path, course):
    N = _env(monkeypatch, course)
    ref = _base_reference(k, course, N)
    prior, cost = _base(k)
    _assert_same(_segments(k, prior, cost, N, BASE_KW, [3, 7, M]), ref, course)

    def disk(state):
        path = str(tmp_path / f"{course}_{state.iteration}.npz")
        state.save(path)
        return k.SmcState.load(path)
    _assert_same(_segments(k, prior, cost, N, BASE_KW, [5, M], via=disk), ref, course)


def test_split_beyond_16_parameters(k, gpu_ctx, monkeypatch):
    """the run-time-dimension kernels (the smallest smc shape of tests/test_gpu_dyn_dim.py)"""
    for v in _ENV + HOOKS:
        monkeypatch.delenv(v, raising=False)
    rng = np.random.default_rng(8)
    prior, cost = k.Factored(*[k.Normal(0, 2)] * 20), k.costs.GaussDist(rng.normal(size=20))
    kw = dict(alpha=0.9, epstol=3.0, seed=4)
    ref = k.smc(prior, cost, nparticles=3000, return_array=True, **kw)
    n = ref.info["iterations"]
    assert n >= 4, n
    for split in (1, n // 2, n - 1):
        got = _segments(k, prior, cost, 3000, kw, [split, None])
        _assert_same(got, ref, split)
    # a finished run continued with the same options: nothing more happens
    again = k.smc(prior, cost, resume=got.info["state"], return_array=True, **kw)
    _assert_same(again, ref)


@pytest.mark.parametrize("split", list(range(1, M)))
@pytest.mark.parametrize("course", ["loop", "select"])
def test_split_with_retry_passes(k, gpu_ctx, monkeypatch, course, split):
    _env(monkeypatch, course)
    N = 4000
    kw = dict(BASE_KW, mcmc_retrys=2, mcmc_tol=0.45)
    ref = _reference(k, course, "retrys", N, dict(kw, max_iterations=M))
    passes = [rec["passes"] for rec in ref.info["log"]]
    assert ref.info["iterations"] == M and max(passes) > 1 and min(passes) < max(passes), passes
    prior, cost = _base(k)
    got = _segments(k, prior, cost, N, kw, [split, M])
    assert got.info["state"].pass_count == sum(passes) > M
    _assert_same(got, ref, (course, split))


@pytest.mark.parametrize("N", [200, 4000])
def test_split_with_a_discrete_prior(k, orc, gpu_ctx, monkeypatch, N):
    for v in _ENV + HOOKS:
        monkeypatch.delenv(v, raising=False)
    sc = S.build("neg_mixed", N, orc)
    prior, cost = sc.prior(k), sc.cost(k)
    kw = sc.kw()
    kw.pop("nparticles")
    total = kw.pop("max_iterations")
    ref = k.smc(prior, cost, nparticles=N, return_array=True, max_iterations=total, **kw)
    assert ref.info["iterations"] == total == 5
    first = k.smc(prior, cost, nparticles=N, return_array=True, return_state=True, max_iterations=2, **kw)
    st = first.info["state"]
    # the state holds the walkers themselves, between the integers the result rounds them to
    assert np.any(st.theta != np.rint(st.theta))
    assert np.array_equal(np.rint(st.theta), first.info["theta_all"])
    got = k.smc(prior, cost, resume=st, return_array=True, max_iterations=total, **kw)
    _assert_same(got, ref, N)


@pytest.mark.parametrize("split", [5, 21])
@pytest.mark.parametrize("N", [100, 300])
def test_split_with_a_prepared_cost(k, gpu_ctx, monkeypatch, N, split):
    """the README simulator on the one-workgroup course (100 particles) and on the kernel-per-phase course (300):
    its prepared passes live in a ring of 16 slots addressed by the pass counter"""
    for v in _ENV + HOOKS:
        monkeypatch.delenv(v, raising=False)
    prior = k.Factored(k.Uniform(1, 3), k.Truncated(k.Normal(0, 0.1), 0, 100))
    cost = k.costs.NormalMeanStdSim(1000, 2.0, 0.04)
    kw = dict(seed=2, r_epstol=0.0, mcmc_tol=0.0, epstol=-1e308)
    ref = _REF.get(("readme", N))
    if ref is None:
        ref = _REF[("readme", N)] = k.smc(prior, cost, nparticles=N, return_array=True, max_iterations=40, **kw)
    # (the one-workgroup kernel makes no host look; the kernel-per-phase course looks after each batch)
    assert ref.info["iterations"] == 40 and (ref.info["dist"]["host_looks"] > 0) == (N > 256)
    got = _segments(k, prior, cost, N, kw, [split, 40])
    _assert_same(got, ref, (N, split))


def test_a_long_segment_keeps_its_whole_log(k, gpu_ctx, monkeypatch):
    """more than 4096 iterations in one continued segment: the state's log has a record for every iteration"""
    N = _env(monkeypatch, "small")
    prior, cost = _base(k)
    kw = dict(BASE_KW, alpha=0.95, min_r_ess=None)
    total = 4300
    ref = k.smc(prior, cost, nparticles=N, return_array=True, return_state=True, max_iterations=total, **kw)
    assert ref.info["iterations"] == total and len(ref.info["log"]) == total
    got = _segments(k, prior, cost, N, kw, [100, total])
    assert len(got.info["state"].log) == total
    _assert_same(got, ref)


@pytest.mark.parametrize("course", ["small", "loop", "select"])
def test_stop_rules_at_the_state(k, gpu_ctx, monkeypatch, course):
    N = _env(monkeypatch, course)
    prior, cost = _base(k)
    kw = dict(BASE_KW, epstol=3.5, max_iterations=M)
    first = k.smc(prior, cost, nparticles=N, return_array=True, return_state=True, **kw)
    assert first.info["iterations"] == 4 and first.eps <= 3.5, first.info["log"]   # stopped by the rule
    st = first.info["state"]
    # the same options: no new iteration, the identical result and state
    same = k.smc(prior, cost, resume=st, return_array=True, return_state=True, **kw)
    assert same.info["first_iteration"] == 4
    _assert_same(same, first, course)
    _assert_same_state(same.info["state"], st, course)
    # a smaller epstol: the run goes on, to where a fresh run with that epstol stops
    kw2 = dict(kw, epstol=2.0)
    fresh = k.smc(prior, cost, nparticles=N, return_array=True, **kw2)
    assert fresh.info["iterations"] == 8, fresh.info["log"]
    _assert_same(k.smc(prior, cost, resume=st, return_array=True, **kw2), fresh, course)


@pytest.mark.parametrize("course,hook", [("small", "KABC_SMC_LOOP_GIVE_UP"), ("loop", "KABC_SMC_LOOP_GIVE_UP"),
                                         ("select", "KABC_SMC_SELECT_TIME_OUT")])
def test_repetitions_restart_from_the_state(k, gpu_ctx, monkeypatch, course, hook):
    N = _env(monkeypatch, course)
    ref = _base_reference(k, course, N)          # (without the hook)
    monkeypatch.setenv(hook, "1")
    prior, cost = _base(k)
    _assert_same(_segments(k, prior, cost, N, BASE_KW, [5, M]), ref, (course, hook))


def _cancel_problem(k):
    # a noisy cost (C4's model): epsilon levels off, with these options only max_iterations ends the run
    rng = np.random.default_rng(1)
    zstar = rng.normal(size=14)
    ybar = 1.0 + 0.5 * zstar + rng.normal(size=14) / np.sqrt(8)
    prior = k.Factored(k.Normal(0, 5), k.Uniform(0, 5), *[k.Normal(0, 1)] * 14)
    return prior, k.costs.HierGaussSim(ybar), dict(alpha=0.95, epstol=-1.0, r_epstol=0.0, mcmc_tol=0.0, seed=3)


@pytest.mark.parametrize("course", ["loop", "select"])
def test_cancelled_run_continues(k, monkeypatch, course):
    """tests/test_gpu_cancel.py's pattern at a length that keeps the whole log (4000 iterations at most, a few
    tenths of a second): the cancel comes from a thread a third of the way in; wherever it lands, the state on
    Cancelled.result is the state of the max_iterations = k run, and continuing it gives the uninterrupted run"""
    _env(monkeypatch, course)
    prior, cost, kw = _cancel_problem(k)
    N, total = 16384, 4000
    ctx = k.Context(0)
    try:
        k.smc(prior, cost, nparticles=N, ctx=ctx, max_iterations=50, **kw)     # (kernels loaded)
        t0 = time.perf_counter()
        k.smc(prior, cost, nparticles=N, ctx=ctx, max_iterations=400, **kw)
        est = (time.perf_counter() - t0) * total / 400
        timer = threading.Timer(max(est / 3, 0.005), ctx.cancel)
        timer.start()
        err = None
        try:
            k.smc(prior, cost, nparticles=N, ctx=ctx, max_iterations=total, return_array=True, return_state=True, **kw)
        except k.Cancelled as e:
            err = e
        timer.join()
        ctx.clear_cancel()
        assert err is not None, "the run finished before the cancel"
        part = err.result
        it = part.info["iterations"]
        assert 0 < it < total, it
        st = part.info["state"]
        upto = k.smc(prior, cost, nparticles=N, ctx=ctx, max_iterations=it, return_array=True, return_state=True, **kw)
        _assert_same(part, upto, (course, it))
        _assert_same_state(st, upto.info["state"], (course, it))
        more = min(it + 40, total)
        ref = k.smc(prior, cost, nparticles=N, ctx=ctx, max_iterations=more, return_array=True, **kw)
        got = k.smc(prior, cost, resume=st, ctx=ctx, max_iterations=more, return_array=True, **kw)
        assert got.info["first_iteration"] == it
        _assert_same(got, ref, (course, it))
    finally:
        ctx.close()


def _run_from_null(k, prior, cost, N, kw):
    """kabc_smc_run_from(from = NULL, to = NULL) through ctypes, as api.smc fills the arguments of kabc_smc_run"""
    from kissabc_jl_amd import _cdefs as cd, _lib
    lib, ctx = _lib.load(), _lib.default_context()
    fac = k.api.as_factored(prior)
    D = len(fac)
    o = cd.SmcOpts()
    lib.kabc_smc_default_opts(C.byref(o))
    o.nparticles, o.alpha, o.min_r_ess, o.seed = N, kw["alpha"], kw["min_r_ess"], kw["seed"]
    o.r_epstol, o.mcmc_tol, o.epstol, o.max_iterations = kw["r_epstol"], kw["mcmc_tol"], kw["epstol"], kw["max_iterations"]
    theta, Cst, alive = np.empty((N, D)), np.empty(N), np.zeros(N, np.uint8)
    log = (cd.SmcIter * 4096)()
    r = cd.SmcResult()
    r.theta, r.cost = theta.ctypes.data_as(cd.c_double_p), Cst.ctypes.data_as(cd.c_double_p)
    r.alive, r.iter_log, r.iter_log_cap = alive.ctypes.data_as(C.POINTER(C.c_uint8)), log, 4096
    cc = cost.to_c()
    _lib.check(lib.kabc_smc_run_from(ctx.handle, fac.to_c(), D, C.byref(cc), C.byref(o), None, None, C.byref(r)))
    return dict(theta_all=theta, C=Cst, alive=alive.view(np.bool_), eps=r.eps, iterations=r.iterations,
                cost_evals=r.cost_evals, proposals=r.proposals, launches=r.mcmc_launches,
                log=[dict(eps=log[i].eps, ess=log[i].ess, accepted=log[i].accepted, resampled=log[i].resampled,
                          flag=log[i].flag, passes=log[i].mcmc_passes) for i in range(r.iterations)])


@pytest.mark.parametrize("course", FOUR)
def test_default_path_unchanged(k, orc, gpu_ctx, monkeypatch, course):
    """smc() without the new keywords, and kabc_smc_run_from without states, are kabc_smc_run: the oracle's run"""
    N = _env(monkeypatch, course)
    prior, cost = _base(k)
    kw = dict(BASE_KW, max_iterations=M)
    got = _base_reference(k, course, N)
    assert "state" not in got.info and "first_iteration" not in got.info
    ref = orc.smc(prior, cost, nparticles=N, **kw)
    raw = _run_from_null(k, prior, cost, N, kw)
    for name, out in (("smc", dict(got.info, C=got.C, eps=got.eps)), ("run_from", raw)):
        assert out["iterations"] == ref["iterations"] and out["log"] == ref["log"], name
        assert _bits(out["eps"]) == _bits(ref["eps"]), name
        assert np.array_equal(out["alive"], ref["alive"]), name
        assert np.array_equal(_bits(out["theta_all"]), _bits(ref["theta_all"])), name
        assert np.array_equal(_bits(out["C"]), _bits(ref["C"])), name
        assert (out["cost_evals"], out["proposals"]) == (ref["cost_evals"], ref["proposals"]), name
    assert raw["launches"] == got.info["mcmc_launches"]


@pytest.mark.parametrize("course", FOUR)
def test_continued_run_equals_the_oracle_continued_from_the_same_state(k, orc, gpu_ctx, monkeypatch, course):
    """an independent reference for a continued run: the device's state after 4 iterations (the first resample),
    continued to 9 by the device and by the oracle (orc.smc(resume=), tests/test_oracle_resume.py)"""
    N = _env(monkeypatch, course)
    prior, cost = _base(k)
    first = k.smc(prior, cost, nparticles=N, return_array=True, return_state=True, **dict(BASE_KW, max_iterations=4))
    st = first.info["state"]
    assert st.iteration == 4 and st.n_alive == N and first.info["log"][3]["resampled"]
    rest = {a: b for a, b in BASE_KW.items() if a != "seed"}
    got = k.smc(prior, cost, resume=st, return_array=True, return_state=True, max_iterations=M, **rest)
    ref = orc.smc(prior, cost, resume=st, return_state=True, max_iterations=M, **rest)
    assert got.info["iterations"] == ref["iterations"] == M
    assert got.info["log"][4:] == ref["log"] and len(ref["log"]) == M - 4
    assert _bits(got.eps) == _bits(ref["eps"])
    assert np.array_equal(got.info["alive"], ref["alive"])
    assert np.array_equal(_bits(got.info["theta_all"]), _bits(ref["theta_all"]))
    assert np.array_equal(_bits(got.C), _bits(ref["C"]))
    assert (got.info["cost_evals"], got.info["proposals"]) == (ref["cost_evals"], ref["proposals"])
    _assert_same_state(got.info["state"], ref["state"], course)
