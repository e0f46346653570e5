"""-m gpu: a stopped ABCDE run continued from its state (kabc_abcde_run_from; ABCDE(return_state=, resume=)) IS the
uninterrupted run, bit for bit, on every course of the driver (the generation kernel's own scans, donor teams,
sorted blocks, the wavelet matrix, a run-time dimension, user costs, a specialised model); and kabc_ctx_cancel
stops a running call at a generation boundary with the result of `generations = k`.

The yardstick is the uninterrupted device run, itself held against the oracle in the same test.  "Split at k":
run with generations = k and return_state=True, then resume= to G.  The buffer set a generation reads is a matter
of THIS call's generation count while the streams count from the state: an odd and an even k per course."""
import ctypes as C
import os
import signal
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

from test_user_cost import ROSEN_SRC

pytestmark = pytest.mark.gpu

LATENCY_BOUND = 0.25    # seconds from cancel() to the raise (tests/test_gpu_cancel.py)
CANCEL_AFTER = 0.3
TARGET_S = 2.0          # what a cancelled call would take if the cancel were ignored


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_result(a, b, what=""):
    assert np.array_equal(_u64(a.P), _u64(b.P)), what
    assert np.array_equal(_u64(a.C), _u64(b.C)), what
    assert a.reached_eps == b.reached_eps, what
    assert a.info["generations_run"] == b.info["generations_run"], what
    assert a.info["nsims"] == b.info["nsims"], what


def _same_state(a, b, what=""):
    for name in ("theta", "cost", "logprior"):
        assert np.array_equal(_u64(getattr(a, name)), _u64(getattr(b, name))), (what, name)
    assert (a.nparticles, a.D, a.seed, a.generation, a.nsims) == (b.nparticles, b.D, b.seed, b.generation, b.nsims), what


def _against_oracle(orc, got, pri, cost, eps, seed, kw):
    ref = orc.abcde(pri, cost, eps, seed=seed, **kw)
    assert np.array_equal(got.P, ref["P"]) and np.array_equal(got.C, ref["C"])
    assert got.reached_eps == ref["reached_eps"]
    assert got.info["generations_run"] == ref["generations_run"] and got.info["nsims"] == ref["nsims"]


def _split(k, pri, cost, eps, seed, kw, ks, full=None):
    """the uninterrupted run of kw["generations"] (with its state), and for every k in ks the run split at k"""
    G = kw["generations"]
    if full is None:
        full = k.ABCDE(pri, cost, eps, seed=seed, return_array=True, return_state=True, **kw)
    for kk in ks:
        first = k.ABCDE(pri, cost, eps, seed=seed, return_array=True, return_state=True, **dict(kw, generations=kk))
        st = first.info["state"]
        assert st.generation == first.info["generations_run"] == kk and st.seed == seed
        assert st.nsims == first.info["nsims"]
        # `nparticles` and `seed` come from the state
        rest = dict(kw, generations=G)
        rest.pop("nparticles")
        cont = k.ABCDE(pri, cost, eps, resume=st, return_array=True, return_state=True, **rest)
        _same_result(cont, full, f"split at {kk}")
        _same_state(cont.info["state"], full.info["state"], f"split at {kk}")
    return full


def _gauss(k):
    return k.Factored(k.Normal(0, 5), k.Normal(0, 5)), k.costs.GaussDist([1.0, -0.5])


def test_every_boundary_and_a_checkpoint_on_disk(k, orc, gpu_ctx, tmp_path):
    """N = 100: two workgroups of the scan course, the second ragged; G = 6, split at every k in 0..6"""
    pri, cost = _gauss(k)
    kw = dict(nparticles=100, generations=6)
    full = _split(k, pri, cost, 0.05, 9, kw, range(0, 7))
    _against_oracle(orc, full, pri, cost, 0.05, 9, kw)
    assert full.info["state"].generation == 6
    # three segments, the state going through a file between them
    path = str(tmp_path / "abcde.npz")
    a = k.ABCDE(pri, cost, 0.05, seed=9, nparticles=100, generations=1, return_state=True)
    a.info["state"].save(path)
    b = k.ABCDE(pri, cost, 0.05, generations=4, resume=k.AbcdeState.load(path), return_state=True)
    assert b.info["generations_run"] == 4
    b.info["state"].save(path)
    c = k.ABCDE(pri, cost, 0.05, generations=6, resume=k.AbcdeState.load(path), return_array=True, return_state=True)
    _same_result(c, full)
    _same_state(c.info["state"], full.info["state"])


@pytest.mark.parametrize("case", ["donor_teams_257", "sorted_blocks_1537", "wavelet_4100", "scan_donor_off_257",
                                  "scan_blocks_from_1537", "d17_100"])
def test_split_on_every_course(k, orc, gpu_ctx, monkeypatch, case):
    """one odd and one even k on every course the donor draw has (1537 particles: 7 sorted blocks, the last one a
    single particle), and on the run-time-dimension kernels"""
    for name in ("KABC_ABCDE_RANK", "KABC_ABCDE_DONOR", "KABC_ABCDE_BLOCKS_FROM"):
        monkeypatch.delenv(name, raising=False)
    pri = k.Factored(k.DiscreteUniform(-10, 10), k.Normal(0, 3))
    cost = k.costs.GaussDist([3.0, -2.0])
    eps, N = 0.5, int(case.rsplit("_", 1)[1])
    if case == "wavelet_4100":
        monkeypatch.setenv("KABC_ABCDE_RANK", "wavelet")
    elif case == "scan_donor_off_257":
        monkeypatch.setenv("KABC_ABCDE_DONOR", "0")
    elif case == "scan_blocks_from_1537":    # (no sorted blocks, no donor teams: the generation kernel's own scans)
        monkeypatch.setenv("KABC_ABCDE_BLOCKS_FROM", "1000000000")
        monkeypatch.setenv("KABC_ABCDE_DONOR", "0")
    elif case == "d17_100":
        comps = [k.Normal(0, 2), k.Uniform(-3, 3), k.Gamma(2.5, 0.7), k.DiscreteUniform(-4, 4)]
        pri = k.Factored(*[comps[j % 4] for j in range(17)])
        cost = k.costs.GaussDist(np.linspace(-0.5, 1.5, 17))
        eps = 3.0
    kw = dict(nparticles=N, generations=5, proposal_width=0.9)
    full = _split(k, pri, cost, eps, 11, kw, (2, 3))
    _against_oracle(orc, full, pri, cost, eps, 11, kw)


@pytest.mark.parametrize("case", ["scan_100", "sorted_blocks_1537"])
def test_continued_run_equals_the_oracle_continued_from_the_same_state(k, orc, gpu_ctx, monkeypatch, case):
    """an independent reference for a continued run: the device's state after 2 generations, continued to 5 by the
    device and by the oracle (orc.abcde(resume=), tests/test_oracle_resume.py)"""
    for name in ("KABC_ABCDE_RANK", "KABC_ABCDE_DONOR", "KABC_ABCDE_BLOCKS_FROM"):
        monkeypatch.delenv(name, raising=False)
    pri = k.Factored(k.DiscreteUniform(-10, 10), k.Normal(0, 3))
    cost = k.costs.GaussDist([3.0, -2.0])
    N = int(case.rsplit("_", 1)[1])
    first = k.ABCDE(pri, cost, 0.5, seed=11, nparticles=N, generations=2, proposal_width=0.9, return_state=True)
    st = first.info["state"]
    assert st.generation == 2
    got = k.ABCDE(pri, cost, 0.5, resume=st, generations=5, proposal_width=0.9, return_array=True, return_state=True)
    ref = orc.abcde(pri, cost, 0.5, resume=st, generations=5, proposal_width=0.9, return_state=True)
    assert np.array_equal(_u64(got.P), _u64(ref["P"])) and np.array_equal(_u64(got.C), _u64(ref["C"]))
    assert got.reached_eps == ref["reached_eps"]
    assert got.info["generations_run"] == ref["generations_run"] == 5 and got.info["nsims"] == ref["nsims"] > st.nsims
    _same_state(got.info["state"], ref["state"], case)


def test_split_discrete_prior_state_is_not_rounded(k, orc, gpu_ctx):
    """DiscreteUniform + NoisyQuadDU: P is push_p'ed (integral), the state's theta is what the loop holds"""
    pri = k.Factored(k.Normal(1, 0.5), k.DiscreteUniform(1, 10))
    cost = k.costs.NoisyQuadDU(5.5)
    kw = dict(nparticles=128, generations=6)
    full = _split(k, pri, cost, 0.05, 9, kw, (2, 3))
    _against_oracle(orc, full, pri, cost, 0.05, 9, kw)
    th = full.info["state"].theta[:, 1]
    assert np.array_equal(full.P[:, 1], np.rint(full.P[:, 1]))
    assert not np.array_equal(th, np.rint(th))
    assert np.array_equal(np.rint(th), full.P[:, 1])


@pytest.mark.parametrize("form", ["hiprtc", "hipcc"])
def test_split_user_cost(k, gpu_ctx, monkeypatch, form):
    """a user cost compiled at run time (hipRTC) or built as a plugin by hipcc: its kernels take AbcdeArgs and
    AbcdeCtrl as they were; same formula as the built-in Rosenbrock, so that one is the yardstick's yardstick"""
    if form == "hipcc":
        monkeypatch.setenv("KABC_USER_PLUGIN", "hipcc")
    user = k.costs.UserCost(ROSEN_SRC + f"// abcde resume {form}\n", dims=[2], posteriors=["kernelized"])
    pri = k.Factored(k.Normal(0, 5), k.Normal(0, 5))
    kw = dict(nparticles=64, generations=5)
    full = _split(k, pri, user, 0.05, 3, kw, (2, 3))
    builtin = k.ABCDE(pri, k.costs.Rosenbrock(), 0.05, seed=3, return_array=True, **kw)
    _same_result(full, builtin)


def test_split_specialised_model(k, orc, gpu_ctx, monkeypatch):
    """KABC_SPECIALIZE=1: the model's own init / generation kernels (compiled at first sight)"""
    monkeypatch.setenv("KABC_SPECIALIZE", "1")
    pri = k.Factored(k.Normal(0.25, 5), k.Uniform(-4, 6))
    cost = k.costs.GaussDist([1.0, -0.5])
    kw = dict(nparticles=100, generations=5)
    full = _split(k, pri, cost, 0.05, 9, kw, (2, 3))
    monkeypatch.delenv("KABC_SPECIALIZE")
    _against_oracle(orc, full, pri, cost, 0.05, 9, kw)


def test_earlystop_break_is_taken_again(k, orc, gpu_ctx):
    """N = 200, α = 0.3, ϵ_target = 0.3, G = 60, seed 9: the break comes at generations_run = 43 (the breaking
    iteration is counted but draws nothing: the state's stream counter is 42)"""
    pri, cost = _gauss(k)
    kw = dict(nparticles=200, generations=60, alpha=0.3, earlystop=True)
    ref = orc.abcde(pri, cost, 0.3, seed=9, **kw)
    assert ref["generations_run"] == 43
    full = k.ABCDE(pri, cost, 0.3, seed=9, return_array=True, return_state=True, **kw)
    _against_oracle(orc, full, pri, cost, 0.3, 9, kw)
    assert full.info["state"].generation == 42
    states = {}
    for kk in (10, 42, 43, 50):
        first = k.ABCDE(pri, cost, 0.3, seed=9, return_array=True, return_state=True, **dict(kw, generations=kk))
        states[kk] = first.info["state"]
        cont = k.ABCDE(pri, cost, 0.3, resume=states[kk], return_array=True, return_state=True, generations=60,
                       alpha=0.3, earlystop=True)
        assert cont.info["generations_run"] == 43
        _same_result(cont, full, f"split at {kk}")
        _same_state(cont.info["state"], full.info["state"], f"split at {kk}")
    assert states[10].generation == 10 and states[42].generation == 42
    assert states[43].generation == 42 and states[50].generation == 42
    # a smaller target: the run goes on (a run of its own, not a piece of another one)
    on = k.ABCDE(pri, cost, 0.1, resume=states[50], return_array=True, generations=60, alpha=0.3, earlystop=True)
    assert on.info["generations_run"] > 43
    assert on.C.max() < full.C.max()


def test_state_at_or_past_generations_comes_back_unchanged(k, gpu_ctx):
    pri = k.Factored(k.Normal(1, 0.5), k.DiscreteUniform(1, 10))
    cost = k.costs.NoisyQuadDU(5.5)
    a = k.ABCDE(pri, cost, 0.05, seed=9, nparticles=128, generations=4, return_array=True, return_state=True)
    for G in (4, 2):
        b = k.ABCDE(pri, cost, 0.05, resume=a.info["state"], generations=G, return_array=True, return_state=True)
        _same_result(b, a, f"generations = {G}")      # (P push_p'ed again from the state's theta)
        _same_state(b.info["state"], a.info["state"], f"generations = {G}")


def test_run_from_without_states_is_kabc_abcde_run(k, orc, gpu_ctx):
    """kabc_abcde_run_from(from = NULL, to = NULL) through ctypes, as api.ABCDE fills the arguments of kabc_abcde_run"""
    from kissabc_jl_amd import _cdefs as cd, _lib
    lib = _lib.load()
    pri, cost = _gauss(k)
    N, D = 100, 2
    kw = dict(nparticles=N, generations=7)
    plain = k.ABCDE(pri, cost, 0.05, seed=9, return_array=True, **kw)
    _against_oracle(orc, plain, pri, cost, 0.05, 9, kw)
    o = cd.AbcdeOpts()
    lib.kabc_abcde_default_opts(C.byref(o))
    o.nparticles, o.generations, o.eps_target, o.seed = N, 7, 0.05, 9
    theta, Cst = np.empty((N, D)), np.empty(N)
    r = cd.AbcdeResult()
    r.theta = theta.ctypes.data_as(cd.c_double_p)
    r.cost = Cst.ctypes.data_as(cd.c_double_p)
    cc = cost.to_c()
    _lib.check(lib.kabc_abcde_run_from(gpu_ctx.handle, pri.to_c(), D, C.byref(cc), C.byref(o), None, None, C.byref(r)))
    assert np.array_equal(_u64(theta), _u64(plain.P)) and np.array_equal(_u64(Cst), _u64(plain.C))
    assert (r.generations_run, r.nsims, bool(r.reached_eps)) == (7, plain.info["nsims"], plain.reached_eps)


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
    o = cd.AbcdeOpts()
    lib.kabc_abcde_default_opts(C.byref(o))
    o.nparticles, o.generations, o.eps_target, o.seed = N, 20, 0.05, 9
    theta, Cst = np.empty((N, D)), np.empty(N)
    r = cd.AbcdeResult()
    r.theta = theta.ctypes.data_as(cd.c_double_p)
    r.cost = Cst.ctypes.data_as(cd.c_double_p)
    to = k.AbcdeState._empty(N, D)
    st_to = to._to_c()
    st_to.generation = 7
    cc = cost.to_c()
    status = lib.kabc_abcde_run_from(gpu_ctx.handle, pri.to_c(), D, C.byref(cc), C.byref(o), None, C.byref(st_to),
                                     C.byref(r))
    assert status == cd.KABC_ERR_RETRY_EXHAUSTED
    assert lib.kabc_last_error().decode() == \
        "ABCDE: the prior never produced a finite (cost, logpdf) pair for some particle"
    assert st_to.generation == -1


# ---- kabc_ctx_cancel ------------------------------------------------------------------------------------------

def test_cancel_pending_at_entry_launches_nothing(k):
    pri, cost = _gauss(k)
    ctx = k.Context(0)
    try:
        ref = k.ABCDE(pri, cost, 0.05, seed=9, nparticles=100, generations=5, ctx=ctx, return_array=True)
        ctx.cancel()
        t0 = time.perf_counter()
        with pytest.raises(k.Cancelled) as e:
            k.ABCDE(pri, cost, 0.05, seed=9, nparticles=100, generations=10**6, ctx=ctx, return_state=True)
        assert time.perf_counter() - t0 < 1.0          # (10^6 generations were not enqueued)
        assert e.value.result.info["state"].generation == -1 and e.value.result.info["generations_run"] == 0
        # the request is consumed and the context usable
        again = k.ABCDE(pri, cost, 0.05, seed=9, nparticles=100, generations=5, ctx=ctx, return_array=True)
        _same_result(again, ref)
    finally:
        ctx.close()


@pytest.mark.parametrize("N", [50, 1537], ids=["scan_50", "blocks_1537"])
def test_cancel_a_running_call(k, N):
    """generations made long by a simulator cost (NormalMeanStdSim), their number sized from a calibration run so
    that the call would last ~2 s; a timer cancels it at 0.3 s"""
    pri = k.Factored(k.Uniform(-5, 10), k.Uniform(0.1, 6))
    cost = k.costs.NormalMeanStdSim(2000 if N == 50 else 200, 2.0, 1.5)
    ctx = k.Context(0)
    try:
        def run(G, **kw):
            return k.ABCDE(pri, cost, 0.01, seed=5, nparticles=N, generations=G, ctx=ctx, return_array=True, **kw)

        run(64)                                         # (first use: kernels loaded)
        t0 = time.perf_counter()
        run(640)
        t1 = time.perf_counter()
        run(1920)
        per_gen = max((time.perf_counter() - t1) - (t1 - t0), 1e-4) / 1280
        G = max(int(TARGET_S / per_gen), 1000)
        box = {}

        def fire():
            box["t"] = time.perf_counter()
            ctx.cancel()

        tm = threading.Timer(CANCEL_AFTER, fire)
        tm.start()
        err = None
        try:
            run(G, return_state=True)
        except k.Cancelled as e:
            err = e
        t_ret = time.perf_counter()
        tm.join()
        assert err is not None, "the call finished before the cancel (calibration off?)"
        lat = t_ret - box["t"]
        print(f"[cancel latency] ABCDE N = {N}: {lat * 1e3:.2f} ms, G = {G}")
        assert lat < LATENCY_BOUND, lat
        got = err.result
        kg = got.info["generations_run"]
        assert 0 < kg < G, (kg, G)
        assert got.info["state"].generation == kg
        ref = run(kg, return_state=True)
        _same_result(got, ref)
        _same_state(got.info["state"], ref.info["state"])
        # the state goes on as if nothing had happened
        cont = k.ABCDE(pri, cost, 0.01, resume=got.info["state"], generations=kg + 5, ctx=ctx, return_array=True)
        _same_result(cont, run(kg + 5))
    finally:
        ctx.close()


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ctrl_c_child(source, tmp_path, after=0.3):
    """runs `source` (prints READY before its long call, INTERRUPTED on KeyboardInterrupt, OK at its end) as a child
    process, sends it SIGINT `after` seconds after READY; returns the seconds from the signal to INTERRUPTED"""
    script = tmp_path / "child.py"
    script.write_text(source.format(root=ROOT))
    p = subprocess.Popen(["timeout", "-k", "10", "60", sys.executable, str(script)],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
    lines = []

    def reader():
        for line in p.stdout:
            lines.append((time.perf_counter(), line.strip()))

    th = threading.Thread(target=reader)
    th.start()
    try:
        t_end = time.perf_counter() + 50
        while not any(l == "READY" for _, l in lines) and p.poll() is None and time.perf_counter() < t_end:
            time.sleep(0.01)
        assert any(l == "READY" for _, l in lines), (lines, p.poll())
        time.sleep(after)
        t_sig = time.perf_counter()
        os.kill(p.pid, signal.SIGINT)   # (timeout forwards it to the child)
        rc = p.wait(timeout=60)
    finally:
        if p.poll() is None:
            p.kill()
            p.wait()
        th.join()
    err = p.stderr.read()
    names = [l for _, l in lines]
    assert rc == 0, (rc, names, err[-2000:])
    assert names[-2:] == ["INTERRUPTED", "OK"], names
    return next(t for t, l in lines if l == "INTERRUPTED") - t_sig


CTRL_C_CHILD = r"""
import sys, time
sys.path.insert(0, {root!r})
import kissabc_jl_amd as k
pri = k.Factored(k.Uniform(-5, 10), k.Uniform(0.1, 6))
cost = k.costs.NormalMeanStdSim(2000, 2.0, 1.5)
ctx = k.Context(0)
def run(G):
    return k.ABCDE(pri, cost, 0.01, seed=5, nparticles=50, generations=G, ctx=ctx, return_array=True)
run(64)
t0 = time.perf_counter()
run(640)
t1 = time.perf_counter()
run(1920)
per_gen = max((time.perf_counter() - t1) - (t1 - t0), 1e-4) / 1280
print("READY", flush=True)
try:
    run(max(int(3.0 / per_gen), 1000))
    print("NOT INTERRUPTED", flush=True)
    sys.exit(3)
except KeyboardInterrupt:
    print("INTERRUPTED", flush=True)
assert run(5).info["generations_run"] == 5
print("OK", flush=True)
"""


def test_ctrl_c_interrupts_abcde(k, tmp_path):
    """ABCDE() arms Ctrl-C: a SIGINT during a ~3 s call ends it at a generation boundary with KeyboardInterrupt,
    and the context goes on working"""
    lat = ctrl_c_child(CTRL_C_CHILD, tmp_path)
    print(f"[cancel latency] ctrl-c ABCDE: {lat * 1e3:.2f} ms")
    assert lat < LATENCY_BOUND
