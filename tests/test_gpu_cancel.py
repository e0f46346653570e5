"""GPU: kabc_ctx_cancel on every path that polls (include/kabc.h).

Each cancelled call is sized from a short calibration run to take ~5 s if it were not cancelled, a
threading.Timer cancels it after ~0.3 s, and the test checks that the call raised Cancelled within
0.25 s of the cancel, that it completed some but not all of its generations / iterations, and that
what it left is bit-identical to an uncancelled call of exactly that length."""
import os
import signal
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGET_S = 5.0      # what a cancelled call would take if the cancel were ignored
CANCEL_AFTER = 0.3
LATENCY_BOUND = 0.25
LATENCIES = {}      # case -> seconds from cancel() to the raise (printed with -s)


def _cancel_later(ctx, delay=CANCEL_AFTER):
    box = {}

    def fire():
        box["t"] = time.perf_counter()
        ctx.cancel()

    tm = threading.Timer(delay, fire)
    tm.start()
    return tm, box


def _run_cancelled(k, ctx, fn, case):
    """fn() under a timer-driven cancel: returns the Cancelled exception"""
    tm, box = _cancel_later(ctx)
    err = None
    try:
        fn()
    except k.Cancelled as e:
        err = e
    t_ret = time.perf_counter()
    tm.join()
    assert err is not None, f"{case}: the call finished before the cancel (calibration off?)"
    lat = t_ret - box["t"]
    LATENCIES[case] = lat
    print(f"[cancel latency] {case}: {lat * 1e3:.2f} ms")
    assert lat < LATENCY_BOUND, (case, lat)
    return err


def _calibrate(fn, n):
    t0 = time.perf_counter()
    fn(n)
    return (time.perf_counter() - t0) / n


def _calibrate_marginal(fn, n):
    """seconds per unit beyond a call's fixed cost (an smc run's set-up and its first, phase-by-phase
    selections are worth many later iterations)"""
    t0 = time.perf_counter()
    fn(n)
    t1 = time.perf_counter()
    fn(3 * n)
    t2 = time.perf_counter()
    return max((t2 - t1) - (t1 - t0), 1e-6) / (2 * n)


def _box_model(k, D, cost=None):
    prior = k.Factored(*[k.Uniform(-5, 5)] * D)
    return k.ApproxKernelizedPosterior(prior, cost or k.costs.Rosenbrock(), 1.0)


def _ais_case(k, case, model, N, nt, cal, collect=False, seeds=None, max_gens=None):
    ctx = k.Context(0)
    try:
        kw = dict(ctx=ctx, seeds=seeds) if seeds is not None else dict(ctx=ctx, seed=11)
        ens = k.AisEnsemble(model, N, **kw).init()
        dt = _calibrate(lambda n: ens.advance(n, nt), cal)
        G = max(int(TARGET_S / dt), 2)
        if max_gens is not None:
            G = min(G, max_gens)
        x0, lp0, ll0, t0 = ens.state()
        lead = (ens.nchains,) if ens.batched else ()
        out = k._lib.pinned_empty((G,) + lead + (N, len(model))) if collect else None
        _run_cancelled(k, ctx, lambda: ens.advance(G, nt, out=out), case)
        x1, lp1, ll1, t1 = ens.state()
        assert (t1 - t0) % nt == 0
        kg = (t1 - t0) // nt
        assert 0 < kg < G, (case, kg, G)
        stats = dict(ens.last_stats)
        # the same start, advanced by exactly kg generations, never cancelled
        ref = k.AisEnsemble(model, N, **kw)
        ref.set_state(x0, lp0, ll0, t0)
        tr = ref.advance(kg, nt, collect=collect)
        assert ref.last_stats == stats
        x2, lp2, ll2, t2 = ref.state()
        assert t2 == t1
        for a, b in ((x1, x2), (lp1, lp2), (ll1, ll2)):
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), case
        if collect:
            assert np.array_equal(out[:kg].view(np.uint64), tr.view(np.uint64)), case
        # the handle stays usable: both go on with the same bits
        ens.advance(100, nt)
        ref.advance(100, nt)
        for a, b in zip(ens.state(), ref.state()):
            assert np.array_equal(np.asarray(a), np.asarray(b)), case
        ref.close()
        ens.close()
        return kg, G
    finally:
        ctx.close()


def test_cancel_small_driver_single_chain(k):
    model = _box_model(k, 2, k.costs.GaussDist([1.0, -0.5]))
    _ais_case(k, "ais small, 1 chain", model, 50, 1, 20000)


def test_cancel_small_driver_single_chain_trace(k):
    model = _box_model(k, 2, k.costs.GaussDist([1.0, -0.5]))
    # a trace of <= 80 000 generations (50 x 2 doubles each): one launch block
    _ais_case(k, "ais small, 1 chain, trace", model, 50, 64, 500, collect=True, max_gens=80000)


def test_cancel_small_driver_batch(k):
    model = _box_model(k, 2, k.costs.GaussDist([1.0, -0.5]))
    _ais_case(k, "ais small, batch of 4", model, 50, 1, 20000, seeds=[5, 6, 7, 8])


def test_cancel_half_generation_path(k):
    _ais_case(k, "ais half-generation, N 65536", _box_model(k, 8), 65536, 100, 20)


def test_cancel_half_generation_path_streamed_trace(k):
    # 4 MiB of trace per generation (one chunk each): long generations (~70 ms) keep the trace at 96 MiB
    _ais_case(k, "ais half-generation, N 65536, streamed trace", _box_model(k, 8), 65536, 32000, 1,
              collect=True, max_gens=24)


def test_cancel_runtime_dimension_path(k):
    _ais_case(k, "ais run-time dimension, D 20", _box_model(k, 20), 4096, 10, 20)


def _smc_problem(k):
    # C4's model (hierarchical Gaussian simulator): a noisy cost, so epsilon levels off; with these
    # options only max_iterations ends the run
    rng = np.random.default_rng(1)
    zstar = rng.normal(size=14)
    ybar = 1.0 + 0.5 * zstar + rng.normal(size=14) / np.sqrt(8)
    prior = k.Factored(k.Normal(0, 5), k.Uniform(0, 5), *[k.Normal(0, 1)] * 14)
    return prior, k.costs.HierGaussSim(ybar), dict(alpha=0.95, epstol=-1.0, r_epstol=0.0,
                                                      mcmc_tol=0.0, seed=3)


def _smc_case(k, case, N, cal, batched=None, looks=False):
    """`batched` / `looks`: the course the run must take (kabc_smc_dist_stats): the persistent kernels
    make no host look; the multi-kernel courses look at the control block, the one-exchange course in
    batches of iterations"""
    prior, cost, kw = _smc_problem(k)
    ctx = k.Context(0)
    try:
        dt = _calibrate_marginal(lambda n: k.smc(prior, cost, nparticles=N, ctx=ctx, max_iterations=n, **kw), cal)
        M = max(int(TARGET_S / dt), 2)
        err = _run_cancelled(k, ctx, lambda: k.smc(prior, cost, nparticles=N, ctx=ctx, max_iterations=M,
                                                   **kw), case)
        got = err.result
        d = got.info["dist"]
        assert (d["host_looks"] > 0) == looks, (case, d)
        if batched is not None:
            assert d["batched"] == batched, (case, d)
        it = got.info["iterations"]
        assert 0 < it < M, (case, it, M)
        ref = k.smc(prior, cost, nparticles=N, ctx=ctx, max_iterations=it, **kw)
        assert ref.info["iterations"] == it  # nothing but max_iterations ended it
        assert np.array_equal(got.info["theta_all"].view(np.uint64), ref.info["theta_all"].view(np.uint64))
        assert np.array_equal(np.asarray(got.C).view(np.uint64), np.asarray(ref.C).view(np.uint64))
        assert np.array_equal(got.info["alive"], ref.info["alive"])
        assert np.float64(got.eps).view(np.uint64) == np.float64(ref.eps).view(np.uint64)
        assert got.info["log"] == ref.info["log"]
        for key in ("n_alive", "cost_evals", "proposals"):
            assert got.info[key] == ref.info[key], key
    finally:
        ctx.close()


def test_cancel_smc_loop_kernel(k):
    _smc_case(k, "smc loop kernel, N 16384", 16384, 50, batched=False)


def test_cancel_smc_one_workgroup(k):
    _smc_case(k, "smc one workgroup, N 100", 100, 200, batched=False)


def test_cancel_smc_multi_kernel_course(k, monkeypatch):
    # the kernel-per-phase course with the select kernel: the host looks after each batch of iterations
    monkeypatch.setenv("KABC_SMC_LOOP", "0")
    monkeypatch.setenv("KABC_SMC_SPEC_SELECT", "0")
    _smc_case(k, "smc multi-kernel course, N 16384", 16384, 50, batched=False, looks=True)


def test_cancel_smc_one_exchange_course(k, monkeypatch):
    # the course of 2^20 particles and more (one-exchange selection, batches of up to eight iterations
    # between looks), forced at a smaller size
    monkeypatch.setenv("KABC_SMC_LOOP", "0")
    monkeypatch.setenv("KABC_SMC_SPEC_SELECT", "1")
    _smc_case(k, "smc one-exchange course, N 16384", 16384, 50, batched=True, looks=True)


def test_idle_request_cancels_the_next_call(k):
    model = _box_model(k, 2, k.costs.GaussDist([1.0, -0.5]))
    ctx = k.Context(0)
    try:
        ens = k.AisEnsemble(model, 50, ctx=ctx, seed=2).init()
        s0 = ens.state()
        ctx.cancel()
        t0 = time.perf_counter()
        with pytest.raises(k.Cancelled):
            ens.advance(10 ** 7, 1)   # (~10 s if it launched)
        assert time.perf_counter() - t0 < 0.05
        s1 = ens.state()
        for a, b in zip(s0, s1):
            assert np.array_equal(np.asarray(a), np.asarray(b))
        # the request was consumed: the next call runs, with the bits of a fresh context
        tr = ens.advance(20, 3, collect=True)
        fresh_ctx = k.Context(0)
        fresh = k.AisEnsemble(model, 50, ctx=fresh_ctx, seed=2).init()
        assert np.array_equal(tr, fresh.advance(20, 3, collect=True))
        fresh.close()
        fresh_ctx.close()
        # clear_cancel drops a pending request
        ctx.cancel()
        ctx.clear_cancel()
        ens.advance(5, 1)
        # smc: refused before it launches, then runs
        prior, cost, kw = _smc_problem(k)
        ctx.cancel()
        with pytest.raises(k.Cancelled):
            k.smc(prior, cost, nparticles=100, ctx=ctx, max_iterations=10 ** 6, **kw)
        r = k.smc(prior, cost, nparticles=100, ctx=ctx, max_iterations=5, **kw)
        assert r.info["iterations"] == 5
        ens.close()
    finally:
        ctx.close()


CHILD = r"""
import sys, time
sys.path.insert(0, {root!r})
import kissabc_jl_amd as k
prior = k.Factored(k.Uniform(-5, 5), k.Uniform(-5, 5))
model = k.ApproxKernelizedPosterior(prior, k.costs.GaussDist([1.0, -0.5]), 1.0)
ctx = k.Context(0)
t0 = time.perf_counter()
k.sample(model, k.AIS(50), 50 * 20000, ctx=ctx, return_array=True)
per_gen = (time.perf_counter() - t0) / 20000
gens = int(5.0 / per_gen)
print("READY", flush=True)
try:
    k.sample(model, k.AIS(50), 100, discard_initial=50 * gens, ctx=ctx, return_array=True)
    print("NOT INTERRUPTED", flush=True)
    sys.exit(3)
except KeyboardInterrupt:
    print("INTERRUPTED", flush=True)
out = k.sample(model, k.AIS(50), 1000, ctx=ctx, return_array=True, seed=4)
assert out.shape == (1000, 2)
print("OK", flush=True)
"""


def test_ctrl_c_interrupts_sample(k, tmp_path):
    script = tmp_path / "child.py"
    script.write_text(CHILD.format(root=ROOT))
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
        time.sleep(1.0)
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
    t_int = next(t for t, l in lines if l == "INTERRUPTED")
    LATENCIES["ctrl-c"] = t_int - t_sig
    print(f"[cancel latency] ctrl-c: {(t_int - t_sig) * 1e3:.2f} ms")
    assert t_int - t_sig < LATENCY_BOUND
