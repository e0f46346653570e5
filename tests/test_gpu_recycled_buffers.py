"""-m gpu: results on buffers recycled from a context's pool (csrc/host_common.hpp DevBufs).

The run-to-completion entry points take their working buffers from the pool of their context, and
DevBufs::alloc hands out any cached buffer up to twice too large: a smaller call after a larger one runs on
the larger call's buffers, full of its bytes.  On one k.Context a larger call is followed by a smaller one whose
buffers fall between one half and the full size of the first (4096 -> 2500 particles); the second result must
equal the oracle and the same call on a fresh context.  For smc a cancelled larger call in between (the request
is pending at entry: Cancelled) changes nothing; kabc_pfilter_run does not look at the request.

Drivers covered -- every entry point that allocates through DevBufs with a context: kabc_smc_run (loop kernel
and the kernel-per-phase path), kabc_smc_run_batch, kabc_pfilter_run, kabc_pfilter_run_batch, kabc_abcde_run_batch,
kabc_abc_reject, kabc_abc_reject_batch, kabc_cost_eval (cost.evaluate) and kabc_prior_predictive.  For smc a
larger call is also cancelled from a host thread while it runs, so that its buffers go back to the pool in the
middle of an iteration; the next call must still equal the oracle.  The same smc sequence with KABC_POOL_MB=0
(read once per process) rides in a child of tests/test_gpu_poisoned_memory.py."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _d4(k):
    return k.Factored(*[k.Normal(0, 3)] * 4), k.costs.GaussDist([1.0, -0.5, 0.25, 2.0])


def _u(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _smc_equal(got, ref):
    assert got.info["log"] == ref["log"] and got.info["iterations"] == ref["iterations"] >= 2
    assert np.array_equal(_u(got.info["theta_all"]), _u(ref["theta_all"])) and np.array_equal(_u(got.C), _u(ref["C"]))
    assert np.array_equal(got.info["alive"], ref["alive"]) and _u(got.eps) == _u(ref["eps"])
    assert got.info["cost_evals"] == ref["cost_evals"] and got.info["proposals"] == ref["proposals"]


@pytest.mark.parametrize("loop", ["1", "0"])
def test_smc_smaller_call_after_a_larger_one(k, orc, gpu_ctx, monkeypatch, loop):
    monkeypatch.setenv("KABC_SMC_LOOP", loop)
    monkeypatch.setenv("KABC_SMC_SPEC_SELECT", "0")
    prior, cost = _d4(k)
    kw = dict(alpha=0.9, epstol=1.0, seed=5)
    ref = orc.smc(prior, cost, nparticles=2500, **kw)
    ctx, fresh = k.Context(0), k.Context(0)
    try:
        k.smc(prior, cost, nparticles=4096, ctx=ctx, return_array=True, **kw)
        a = k.smc(prior, cost, nparticles=2500, ctx=ctx, return_array=True, **kw)
        _smc_equal(a, ref)
        ctx.cancel()
        with pytest.raises(k.Cancelled):
            k.smc(prior, cost, nparticles=4096, ctx=ctx, return_array=True, **kw)
        b = k.smc(prior, cost, nparticles=2500, ctx=ctx, return_array=True, **kw)
        _smc_equal(b, ref)
        _smc_equal(k.smc(prior, cost, nparticles=2500, ctx=fresh, return_array=True, **kw), ref)
    finally:
        ctx.close()
        fresh.close()


def test_pfilter_smaller_call_after_a_larger_one(k, orc, gpu_ctx):
    prior, cost = _d4(k)
    kw = dict(max_iters=6, seed=5)
    ref = orc.pfilter(prior, cost, 2500, **kw)
    ctx, fresh = k.Context(0), k.Context(0)

    def same(got):
        assert got.P.shape == ref["P"].shape
        assert np.array_equal(_u(got.P), _u(ref["P"])) and np.array_equal(_u(got.C), _u(ref["C"]))
        assert [got.info[f] for f in ("eps", "iterations", "nreps", "cost_evals")] == \
            [ref[f] for f in ("eps", "iterations", "nreps", "cost_evals")]
    try:
        k.pfilter(prior, cost, 4096, ctx=ctx, return_array=True, **kw)
        same(k.pfilter(prior, cost, 2500, ctx=ctx, return_array=True, **kw))
        same(k.pfilter(prior, cost, 2500, ctx=fresh, return_array=True, **kw))
    finally:
        ctx.close()
        fresh.close()


def test_smc_after_a_call_cancelled_while_it_ran(k, orc, gpu_ctx, monkeypatch):
    """a cancel from a host thread during the larger run (kernel-per-phase path: the host looks at the request
    between iterations): the run stops with its buffers in use and hands them to the pool as they are"""
    monkeypatch.setenv("KABC_SMC_LOOP", "0")
    monkeypatch.setenv("KABC_SMC_SPEC_SELECT", "0")
    prior, cost = _d4(k)
    kw = dict(alpha=0.9, seed=5)
    ref = orc.smc(prior, cost, nparticles=2500, epstol=1.0, **kw)
    ctx = k.Context(0)
    try:
        t = threading.Timer(0.05, ctx.cancel)
        t.start()
        try:
            # (epstol = 0 with a bounded loop: thousands of iterations, far longer than the timer)
            k.smc(prior, cost, nparticles=4096, ctx=ctx, return_array=True, epstol=0.0, max_iterations=20000, **kw)
            cancelled = False
        except k.Cancelled:
            cancelled = True
        t.join()
        ctx.clear_cancel()
        assert cancelled, "the larger run ended before the cancel request: nothing was left half-used"
        _smc_equal(k.smc(prior, cost, nparticles=2500, ctx=ctx, return_array=True, epstol=1.0, **kw), ref)
    finally:
        ctx.close()


def _assert_same(got, want, what):
    assert set(want) <= set(got), what
    for key, w in want.items():
        g, w = np.asarray(got[key]), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, key, g.shape, w.shape, g.dtype, w.dtype)
        same = np.array_equal(_u(g), _u(w)) if g.dtype == np.float64 else np.array_equal(g, w)
        assert same, (what, key)


def _batch_drivers(k):
    """name -> (run(ctx, size) -> {key: array}, oracle(o, size) -> the same keys, larger size, smaller size)"""
    import poison_child as pc
    n2 = pc.n2_prior(k)
    g = k.costs.GaussDist([1.0, -0.5])
    seeds = pc.SEEDS3
    targets = lambda kk: [kk.costs.GaussDist([1.0 + 0.3 * r, -0.5 + 0.1 * r]) for r in range(3)]   # noqa: E731

    def packed(res, pack):
        out = {}
        for r in range(len(seeds)):
            out.update({f"{key}_{r}": v for key, v in pack(res[r]).items()})
        return out

    smc_kw = dict(alpha=0.9, epstol=0.05)
    pf_kw = dict(epstol=0.05, max_iters=12)
    de_kw = dict(generations=15)
    return {
        "smc_batch": (
            lambda ctx, n: packed(k.smc_batch(n2, g, 3, seeds=seeds, nparticles=n, ctx=ctx, return_array=True, **smc_kw), pc._smc_dev),
            lambda o, n: packed([o.smc(n2, g, seed=s, nparticles=n, **smc_kw) for s in seeds], pc._smc_orc), 256, 160),
        "pfilter_batch": (
            lambda ctx, n: packed(k.pfilter_batch(n2, g, n, 3, seeds=seeds, ctx=ctx, return_array=True, **pf_kw), pc._pf_dev),
            lambda o, n: packed([o.pfilter(n2, g, n, seed=s, **pf_kw) for s in seeds], pc._pf_orc), 256, 160),
        "abcde_batch": (
            lambda ctx, n: packed(k.ABCDE_batch(n2, g, 0.05, 3, seeds=seeds, nparticles=n, ctx=ctx, return_array=True, **de_kw), pc._de_dev),
            lambda o, n: packed([o.abcde(n2, g, 0.05, seed=s, nparticles=n, **de_kw) for s in seeds], pc._de_orc), 256, 160),
        "abc_reject": (
            lambda ctx, n: pc._rej_dev(k.abc_reject(n2, g, draws=n, keep=n // 3, seed=3, first_row=7, ctx=ctx, return_array=True)),
            lambda o, n: pc.reject_case("x", pc.n2_prior, lambda kk: kk.costs.GaussDist([1.0, -0.5]), {}, draws=n,
                                        keep=n // 3).orc(k, o), 4096, 2500),
        "abc_reject_batch": (
            lambda ctx, n: {key: v for key, v in pc.reject_batch_case("x", pc.n2_prior, targets, seeds, {}, draws=n,
                                                                      keep=n // 3).dev(k, ctx).items() if key != "course"},
            lambda o, n: pc.reject_batch_case("x", pc.n2_prior, targets, seeds, {}, draws=n, keep=n // 3).orc(k, o),
            4096, 2500),
        "cost_evaluate": (
            lambda ctx, n: pc.evaluate_case("x", lambda kk: kk.costs.NoisyQuadDU(5.5), 2, n, 2, {}).dev(k, ctx),
            lambda o, n: pc.evaluate_case("x", lambda kk: kk.costs.NoisyQuadDU(5.5), 2, n, 2, {}).orc(k, o), 4096, 2500),
        "prior_predictive": (
            lambda ctx, n: {key: v for key, v in pc.predictive_case("x", pc.n2_prior, lambda kk: kk.costs.GaussDist([1.0, -0.5]),
                                                                    n, {}).dev(k, ctx).items() if key != "launches"},
            lambda o, n: pc.predictive_case("x", pc.n2_prior, lambda kk: kk.costs.GaussDist([1.0, -0.5]), n, {}).orc(k, o),
            4096, 2500),
    }


@pytest.mark.parametrize("name", ["smc_batch", "pfilter_batch", "abcde_batch", "abc_reject", "abc_reject_batch",
                                  "cost_evaluate", "prior_predictive"])
def test_other_pooled_drivers_smaller_call_after_a_larger_one(k, orc, gpu_ctx, name):
    run, oracle, big, small = _batch_drivers(k)[name]
    ref = oracle(orc, small)
    ctx, fresh = k.Context(0), k.Context(0)
    try:
        run(ctx, big)
        _assert_same(run(ctx, small), ref, (name, "recycled"))
        _assert_same(run(fresh, small), ref, (name, "fresh context"))
    finally:
        ctx.close()
        fresh.close()
