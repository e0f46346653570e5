"""-m gpu: a stopped pfilter run continued from its state (kabc_pfilter_run_from; pfilter(return_state=, resume=)) IS
the uninterrupted run, bit for bit, on every course of the driver (the one-workgroup kernel, the default loop of
four iterations per host look, a launch per attempt, verbose, a run-time dimension, a discrete prior, a raised N);
the stop rules are applied to the state first; and kabc_ctx_cancel stops a running call at an iteration boundary
with the result of `max_iters = k - 1`.

The yardstick is the uninterrupted device run, itself held against the oracle in the same test.  max_iters = m
runs m + 1 iterations: "split after k iterations" is a first call with max_iters = k - 1."""
import ctypes as C
import threading
import time

import numpy as np
import pytest

from test_gpu_abcde_resume import ctrl_c_child

pytestmark = pytest.mark.gpu

CANCEL_AFTER = 0.3
TARGET_S = 2.0          # what a cancelled call would take if the cancel were ignored
INFO = ("eps", "eff", "iterations", "nreps", "cost_evals", "nparticles")


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_result(a, b, what=""):
    assert np.array_equal(_u64(a.P), _u64(b.P)), what
    assert np.array_equal(_u64(a.C), _u64(b.C)), what
    for key in INFO:
        assert _u64(a.info[key]) == _u64(b.info[key]), (what, key, a.info[key], b.info[key])


def _same_state(a, b, what=""):
    for name in ("theta", "cost", "logprior", "eps", "eff"):
        assert np.array_equal(_u64(getattr(a, name)), _u64(getattr(b, name))), (what, name)
    for name in ("nparticles", "D", "seed", "iteration", "nreps", "cost_evals"):
        assert getattr(a, name) == getattr(b, name), (what, name)


def _against_oracle(orc, got, pri, cost, N, seed, kw):
    ref = orc.pfilter(pri, cost, N, seed=seed, **{a: b for a, b in kw.items() if a != "verbose"})
    assert got.P.shape == ref["P"].shape
    assert np.array_equal(got.P, ref["P"]) and np.array_equal(got.C, ref["C"])
    assert got.info["eps"] == ref["eps"] and got.info["eff"] == ref["eff"]
    assert got.info["iterations"] == ref["iterations"] and got.info["nreps"] == ref["nreps"]
    return ref


def _run(k, pri, cost, N, seed, **kw):
    return k.pfilter(pri, cost, N, seed=seed, return_array=True, return_state=True, **kw)


def _split(k, pri, cost, N, seed, kw, ks):
    """the uninterrupted run (with its state), and for every k in ks the run split after k iterations"""
    full = _run(k, pri, cost, N, seed, **kw)
    for kk in ks:
        first = _run(k, pri, cost, N, seed, **dict(kw, max_iters=kk - 1))
        st = first.info["state"]
        assert st.iteration == first.info["iterations"] == kk and st.seed == seed
        assert st.nparticles == first.info["nparticles"] == first.P.shape[0]
        assert (st.nreps, st.cost_evals) == (first.info["nreps"], first.info["cost_evals"])
        assert (st.eps, st.eff) == (first.info["eps"], first.info["eff"])
        # N and seed come from the state
        cont = k.pfilter(pri, cost, resume=st, return_array=True, return_state=True, **kw)
        _same_result(cont, full, f"split after {kk}")
        _same_state(cont.info["state"], full.info["state"], f"split after {kk}")
    return full


def _gauss(k):
    return k.Factored(k.Normal(0, 5), k.Normal(0, 5)), k.costs.GaussDist([1.0, -0.5])


@pytest.mark.parametrize("case", ["one_workgroup_100", "small_off_100", "default_loop_300", "passes_300"])
def test_split_after_every_iteration(k, orc, gpu_ctx, monkeypatch, case):
    """Gauss problem, seed 4, eff_tol = 0, max_iters = 5 (6 iterations), split after k = 1..5: the middle and the
    edge of a batch of four iterations"""
    for name in ("KABC_PF_SMALL", "KABC_PF_PASSES"):
        monkeypatch.delenv(name, raising=False)
    if case == "small_off_100":
        monkeypatch.setenv("KABC_PF_SMALL", "0")
    if case == "passes_300":
        monkeypatch.setenv("KABC_PF_PASSES", "1")
    N = int(case.rsplit("_", 1)[1])
    pri, cost = _gauss(k)
    kw = dict(eff_tol=0.0, max_iters=5)
    full = _split(k, pri, cost, N, 4, kw, range(1, 6))
    ref = _against_oracle(orc, full, pri, cost, N, 4, kw)
    assert ref["iterations"] == 6


@pytest.mark.parametrize("case", ["one_workgroup_100", "default_loop_300"])
def test_continued_run_equals_the_oracle_continued_from_the_same_state(k, orc, gpu_ctx, monkeypatch, case):
    """an independent reference for a continued run: the device's state after 3 iterations, continued to 6 by the
    device and by the oracle (orc.pfilter(resume=), tests/test_oracle_resume.py)"""
    for name in ("KABC_PF_SMALL", "KABC_PF_PASSES"):
        monkeypatch.delenv(name, raising=False)
    N = int(case.rsplit("_", 1)[1])
    pri, cost = _gauss(k)
    st = _run(k, pri, cost, N, 4, eff_tol=0.0, max_iters=2).info["state"]
    assert st.iteration == 3
    got = k.pfilter(pri, cost, resume=st, return_array=True, return_state=True, eff_tol=0.0, max_iters=5)
    ref = orc.pfilter(pri, cost, resume=st, return_state=True, eff_tol=0.0, max_iters=5)
    assert np.array_equal(_u64(got.P), _u64(ref["P"])) and np.array_equal(_u64(got.C), _u64(ref["C"]))
    for key in ("eps", "eff", "iterations", "nreps", "cost_evals"):
        assert _u64(got.info[key]) == _u64(ref[key]), key
    assert ref["iterations"] == 6 and ref["nreps"] > st.nreps
    _same_state(got.info["state"], ref["state"], case)


@pytest.mark.parametrize("case", ["verbose", "d17", "discrete", "raised_13"])
def test_split_other_shapes(k, orc, gpu_ctx, capfd, case):
    pri, cost = _gauss(k)
    N, kw, ks = 100, dict(eff_tol=0.0, max_iters=5), (2, 3)
    if case == "verbose":
        kw["verbose"] = True
    elif case == "d17":
        comps = [k.Normal(0, 2), k.Uniform(-3, 3), k.LogNormal(0.1, 0.4), k.DiscreteUniform(-4, 4)]
        pri = k.Factored(*[comps[j % 4] for j in range(17)])
        cost = k.costs.NormShell(2.0 * np.sqrt(17))
        kw["proposal_width"] = 0.6
    elif case == "discrete":
        pri = k.Factored(k.Normal(1, 0.5), k.DiscreteUniform(1, 10))
        cost = k.costs.NoisyQuadDU(5.5)
        N = 256
    elif case == "raised_13":
        N = 5
    full = _split(k, pri, cost, N, 4, kw, ks)
    _against_oracle(orc, full, pri, cost, N, 4, kw)
    if case == "raised_13":      # (N = 5 is raised to 13; for a state, N means the effective count)
        assert full.info["nparticles"] == full.info["state"].nparticles == 13
        again = k.pfilter(pri, cost, 13, resume=full.info["state"], return_array=True, **kw)
        _same_result(again, full)
    if case == "discrete":
        th = full.info["state"].theta[:, 1]
        assert np.array_equal(full.P[:, 1], np.rint(full.P[:, 1])) and not np.array_equal(th, np.rint(th))
    if case == "verbose":        # every iteration is printed once, with its number in the whole run
        lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("(iters, ")]
        assert [int(ln.split("(")[2].split(",")[0]) for ln in lines] == \
            [1, 2, 3, 4, 5, 6] + [1, 2] + [3, 4, 5, 6] + [1, 2, 3] + [4, 5, 6]


@pytest.mark.parametrize("N", [100, 400])
def test_stop_rules_are_applied_to_the_state(k, orc, gpu_ctx, N):
    """the uninterrupted epstol = 0.05 run takes 25 iterations; continued unchanged it stays put, with
    epstol = 0.02 it goes on (a run of its own from there, equal to the run that had 0.02 from the start: the
    tolerance enters nothing but the stop test)"""
    pri, cost = _gauss(k)
    done = _run(k, pri, cost, N, 4, epstol=0.05)
    ref = _against_oracle(orc, done, pri, cost, N, 4, dict(epstol=0.05))
    assert ref["iterations"] == 25
    st = done.info["state"]
    same = k.pfilter(pri, cost, resume=st, epstol=0.05, return_array=True, return_state=True)
    _same_result(same, done)
    _same_state(same.info["state"], st)
    on = k.pfilter(pri, cost, resume=st, epstol=0.02, return_array=True, return_state=True)
    assert on.info["iterations"] > 25
    _same_result(on, _run(k, pri, cost, N, 4, epstol=0.02))
    # a run that ended on max_iters goes on under a larger one, and stays put under the same
    a = _run(k, pri, cost, N, 4, eff_tol=0.0, max_iters=2)
    b = k.pfilter(pri, cost, resume=a.info["state"], eff_tol=0.0, max_iters=2, return_array=True)
    _same_result(b, a)
    c = k.pfilter(pri, cost, resume=a.info["state"], eff_tol=0.0, max_iters=4, return_array=True)
    assert c.info["iterations"] == 5


def test_run_from_without_states_is_kabc_pfilter_run(k, orc, gpu_ctx):
    from kissabc_jl_amd import _cdefs as cd, _lib
    lib = _lib.load()
    pri, cost = _gauss(k)
    N, D = 300, 2
    plain = k.pfilter(pri, cost, N, seed=4, eff_tol=0.0, max_iters=5, return_array=True)
    _against_oracle(orc, plain, pri, cost, N, 4, dict(eff_tol=0.0, max_iters=5))
    o = cd.PfilterOpts()
    lib.kabc_pfilter_default_opts(C.byref(o))
    o.nparticles, o.eff_tol, o.max_iters, o.seed = N, 0.0, 5, 4
    theta, Cst = np.empty((N, D)), np.empty(N)
    r = cd.PfilterResult()
    r.theta = theta.ctypes.data_as(cd.c_double_p)
    r.cost = Cst.ctypes.data_as(cd.c_double_p)
    cc = cost.to_c()
    _lib.check(lib.kabc_pfilter_run_from(gpu_ctx.handle, pri.to_c(), D, C.byref(cc), C.byref(o), None, None,
                                         C.byref(r)))
    assert np.array_equal(_u64(theta), _u64(plain.P)) and np.array_equal(_u64(Cst), _u64(plain.C))
    assert (r.eps, r.eff, r.iterations, r.nreps, r.cost_evals) == tuple(plain.info[key] for key in INFO[:5])


def test_retry_after_a_select_time_out_with_states(k, orc, gpu_ctx, monkeypatch):
    """KABC_SMC_SELECT_TIME_OUT=1 makes every ordinary-launch attempt of the loop course count as timed out, so each
    call is made twice, the second time with cooperative select launches.  The repeated attempt starts from the
    state again and is the one that fills `to`: 3 + 3 iterations under the hook are the 6 of the plain run"""
    for name in ("KABC_PF_SMALL", "KABC_PF_PASSES", "KABC_SMC_SELECT_TIME_OUT", "KABC_SMC_COOPERATIVE"):
        monkeypatch.delenv(name, raising=False)
    pri, cost = _gauss(k)
    N, kw = 300, dict(eff_tol=0.0, max_iters=5)
    full = _run(k, pri, cost, N, 4, **kw)
    ref = orc.pfilter(pri, cost, N, seed=4, return_state=True, **kw)
    assert ref["iterations"] == 6
    monkeypatch.setenv("KABC_SMC_SELECT_TIME_OUT", "1")
    first = _run(k, pri, cost, N, 4, **dict(kw, max_iters=2))
    st = first.info["state"]
    assert st.iteration == first.info["iterations"] == 3 and st.seed == 4
    cont = k.pfilter(pri, cost, resume=st, return_array=True, return_state=True, **kw)
    monkeypatch.delenv("KABC_SMC_SELECT_TIME_OUT")
    _same_result(cont, full)
    _same_state(cont.info["state"], full.info["state"])
    assert np.array_equal(_u64(cont.P), _u64(ref["P"])) and np.array_equal(_u64(cont.C), _u64(ref["C"]))
    for key in ("eps", "eff", "iterations", "nreps", "cost_evals"):
        assert _u64(cont.info[key]) == _u64(ref[key]), key
    _same_state(cont.info["state"], ref["state"])


def test_a_run_that_fails_on_the_device_leaves_no_state(k, gpu_ctx):
    """a user cost that is never finite: the initial draw gives up, the call fails with KABC_ERR_RETRY_EXHAUSTED and
    its own message, and the `to` state it was given keeps the -1 a failed run leaves (through ctypes: the Python
    error carries no result)"""
    from kissabc_jl_amd import _cdefs as cd, _lib
    from test_gpu_pfilter_batch import INF_SRC
    lib = _lib.load()
    pri = k.Factored(k.Normal(0, 5), k.Normal(0, 5))
    cost = k.costs.UserCost(INF_SRC, dims=[2], params=[-1.0], name="inf_in_run")
    N, D = 64, 2
    o = cd.PfilterOpts()
    lib.kabc_pfilter_default_opts(C.byref(o))
    o.nparticles, o.max_iters, o.seed = N, 12, 4
    assert lib.kabc_pfilter_nparticles(N, o.q, D) == N
    theta, Cst = np.empty((N, D)), np.empty(N)
    r = cd.PfilterResult()
    r.theta = theta.ctypes.data_as(cd.c_double_p)
    r.cost = Cst.ctypes.data_as(cd.c_double_p)
    to = k.PfilterState._empty(N, D)
    st_to = to._to_c()
    st_to.iteration = 7
    cc = cost.to_c()
    status = lib.kabc_pfilter_run_from(gpu_ctx.handle, pri.to_c(), D, C.byref(cc), C.byref(o), None, C.byref(st_to),
                                       C.byref(r))
    assert status == cd.KABC_ERR_RETRY_EXHAUSTED
    assert lib.kabc_last_error().decode() == \
        "pfilter: the prior never produced a finite (cost, logpdf) pair for some particle"
    assert st_to.iteration == -1


# ---- kabc_ctx_cancel ------------------------------------------------------------------------------------------

def test_cancel_pending_at_entry_launches_nothing(k):
    pri, cost = _gauss(k)
    ctx = k.Context(0)
    try:
        ref = k.pfilter(pri, cost, 100, seed=4, epstol=0.05, ctx=ctx, return_array=True)
        ctx.cancel()
        with pytest.raises(k.Cancelled) as e:
            k.pfilter(pri, cost, 100, seed=4, epstol=0.05, ctx=ctx, return_state=True)
        assert e.value.result.info["state"].iteration == -1 and e.value.result.info["iterations"] == 0
        # the request is consumed and the context usable
        _same_result(k.pfilter(pri, cost, 100, seed=4, epstol=0.05, ctx=ctx, return_array=True), ref)
    finally:
        ctx.close()


@pytest.mark.parametrize("N", [100, 300], ids=["one_workgroup_100", "default_loop_300"])
def test_cancel_a_running_call(k, N):
    """iterations made long by a simulator cost (NormalMeanStdSim), n_draws sized from a calibration run so that
    the call would last ~2 s; a timer cancels it at 0.3 s.  The stop is at an iteration boundary and an iteration
    is not a bounded amount of work: the latency is printed, not asserted."""
    pri = k.Factored(k.Uniform(-5, 10), k.Uniform(0.1, 6))
    # ten iterations, whatever they cost: ϵ ends at the 0.7^10 = 2.8 % quantile of the prior's costs, well above
    # the simulator's noise at the n_draws used here, so that every rejection loop ends
    kw = dict(eff_tol=0.0, max_iters=9)
    ctx = k.Context(0)
    try:
        def run(n_draws, **more):
            return k.pfilter(pri, k.costs.NormalMeanStdSim(n_draws, 2.0, 1.5), N, seed=4, ctx=ctx, return_array=True,
                             return_state=True, **dict(kw, **more))

        run(100)                                        # (first use: kernels loaded)
        t0 = time.perf_counter()
        run(1000)
        t1 = time.perf_counter()
        run(3000)
        per_draw = max((time.perf_counter() - t1) - (t1 - t0), 1e-4) / 2000
        n_draws = max(int(TARGET_S / per_draw), 3000)
        box = {}

        def fire():
            box["t"] = time.perf_counter()
            ctx.cancel()

        tm = threading.Timer(CANCEL_AFTER, fire)
        tm.start()
        err = None
        try:
            run(n_draws)
        except k.Cancelled as e:
            err = e
        t_ret = time.perf_counter()
        tm.join()
        assert err is not None, "the call finished before the cancel (calibration off?)"
        print(f"[cancel latency] pfilter N = {N}: {(t_ret - box['t']) * 1e3:.2f} ms, n_draws = {n_draws}")
        got = err.result
        kk = got.info["iterations"]
        assert 0 < kk < 10, kk
        assert got.info["state"].iteration == kk
        ref = run(n_draws, max_iters=kk - 1)
        _same_result(got, ref)
        _same_state(got.info["state"], ref.info["state"])
        # the state goes on as if nothing had happened: to the call's own total, against the call never cancelled
        full = run(n_draws)
        assert full.info["iterations"] == 10
        cost = k.costs.NormalMeanStdSim(n_draws, 2.0, 1.5)
        cont = k.pfilter(pri, cost, resume=got.info["state"], ctx=ctx, return_array=True, return_state=True, **kw)
        _same_result(cont, full)
        _same_state(cont.info["state"], full.info["state"])
    finally:
        ctx.close()


CTRL_C_CHILD = r"""
import sys, time
sys.path.insert(0, {root!r})
import kissabc_jl_amd as k
pri = k.Factored(k.Uniform(-5, 10), k.Uniform(0.1, 6))
ctx = k.Context(0)
def run(n_draws, max_iters=9):
    return k.pfilter(pri, k.costs.NormalMeanStdSim(n_draws, 2.0, 1.5), 100, seed=4, eff_tol=0.0, max_iters=max_iters,
                     ctx=ctx, return_array=True)
run(100)
t0 = time.perf_counter()
run(1000)
t1 = time.perf_counter()
run(3000)
per_draw = max((time.perf_counter() - t1) - (t1 - t0), 1e-4) / 2000
print("READY", flush=True)
try:
    run(max(int(3.0 / per_draw), 3000))
    print("NOT INTERRUPTED", flush=True)
    sys.exit(3)
except KeyboardInterrupt:
    print("INTERRUPTED", flush=True)
assert run(100, max_iters=2).info["iterations"] == 3
print("OK", flush=True)
"""


def test_ctrl_c_interrupts_pfilter(k, tmp_path):
    """pfilter() arms Ctrl-C: a SIGINT during a ~3 s call ends it at an iteration boundary with KeyboardInterrupt,
    and the context goes on working (the latency is one iteration: printed, not asserted)"""
    lat = ctrl_c_child(CTRL_C_CHILD, tmp_path)
    print(f"[cancel latency] ctrl-c pfilter: {lat * 1e3:.2f} ms")
