"""GPU: pfilter_batch / kabc_pfilter_run_batch -- many independent pfilter runs in one call.

Run r of a batch must be bit-identical to pfilter(prior, cost_r, N, seed=seeds[r], <same keywords>) in every
field pfilter returns: the population, the costs, eps, eff, iterations, nreps and cost_evals.  With at most
256 particles and length(prior) <= 16 the runs are the workgroups of one launch, each from its initial draw
to its output, the rejection loops parallel over attempts (KABC_PF_BATCH_SPREAD=0: one lane per particle);
other shapes run one after another, with the same bits."""
import threading
import time

import numpy as np
import pytest

from helpers import REDRAW_SEED, assert_redraws_happen, redraw_case

pytestmark = pytest.mark.gpu

SEEDS5 = [1, 977, 2 ** 40 + 3, 123456789, 0x9E3779B97F4A7C15 % (1 << 63)]


def _eff_same(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def _same(got, ref, what):
    assert np.asarray(got.P).shape == np.asarray(ref.P).shape, what
    assert np.array_equal(np.asarray(got.P).view(np.uint64), np.asarray(ref.P).view(np.uint64)), what
    assert np.array_equal(np.asarray(got.C).view(np.uint64), np.asarray(ref.C).view(np.uint64)), what
    for f in ("eps", "iterations", "nreps", "cost_evals", "nparticles"):
        assert got.info[f] == ref.info[f], (what, f, got.info, ref.info)
    assert _eff_same(got.info["eff"], ref.info["eff"]), (what, got.info, ref.info)


def _same_as_oracle(got, ref, what):
    assert got.P.shape == ref["P"].shape, what
    assert np.array_equal(got.P.view(np.uint64), ref["P"].view(np.uint64)), what
    assert np.array_equal(got.C.view(np.uint64), ref["C"].view(np.uint64)), what
    for f in ("eps", "iterations", "nreps", "cost_evals"):
        assert got.info[f] == ref[f], (what, f, got.info, ref[f])
    assert _eff_same(got.info["eff"], ref["eff"]), what


def _user_cost(k):
    # (the noisy L1 user cost of tests/test_gpu_abcde_batch.py)
    return k.costs.UserCost("""
KABC_HD double kabc_user_cost(const double* x, int D, const double* params, const double* data,
                              int64_t ndata, kabc_cost_rng_t* rng) {
    double z0, z1;
    kabc_cost_rng_normal2(rng, &z0, &z1);
    return kabc_fabs(x[0] - params[0]) + kabc_fabs(x[1] - params[1]) + 0.01 * kabc_fabs(z0);
}
""", dims=[2], params=[1.0, -0.5], name="abcde_batch_l1_noisy")


README_PRIOR = lambda k: k.Factored(k.Uniform(1, 3), k.Truncated(k.Normal(0, 0.1), 0, 100))  # noqa: E731

CASES = ["defaults_100", "defaults_plain", "q9_255", "discrete_256", "raised_13", "dirac_d1", "d16_mixed",
         "nothing_bad", "max_iters0", "per_dataset", "readme_sim", "user_rtc"]


def _case(k, orc, name):
    N2 = k.Factored(k.Normal(0, 5), k.Normal(0, 5))
    g = k.costs.GaussDist([1.0, -0.5])
    if name == "defaults_100":
        return N2, g, 100, dict(epstol=0.05)
    if name == "defaults_plain":   # ends by eff = NaN once nothing is above ϵ
        return N2, g, 100, dict()
    if name == "q9_255":
        return N2, k.costs.NoisyBanana(0.0), 255, dict(q=0.9, max_iters=20, proposal_width=0.5)
    if name == "discrete_256":     # the low-acceptance case: final eff 0.07-0.10
        return (k.Factored(k.Normal(1, 0.5), k.DiscreteUniform(1, 10)), k.costs.NoisyQuadDU(5.5), 256,
                dict(max_iters=15))
    if name == "raised_13":        # N = 5 is raised to ceil(9 / 0.7) = 13
        return N2, g, 5, dict(max_iters=10)
    if name == "dirac_d1":         # a scalar prior
        return k.Normal(1, 0.2), k.costs.DiracSq(1.5), 64, dict(max_iters=12)
    if name == "d16_mixed":
        comps = [k.Normal(0, 2), k.Uniform(-3, 3), k.Gamma(2.5, 0.7), k.DiscreteUniform(-4, 4)]
        return (k.Factored(*[comps[j % 4] for j in range(16)]), k.costs.GaussDist(np.linspace(-0.5, 1.5, 16)), 100,
                dict(max_iters=8, proposal_width=0.6, eff_tol=0.0))
    if name == "nothing_bad":      # every cost equal: nothing is above ϵ, eff = 0/0 = NaN after one iteration
        return (k.Factored(k.DiscreteUniform(3, 3), k.DiscreteUniform(4, 4)), k.costs.GaussDist([3.0, 4.0]), 50,
                dict())
    if name == "max_iters0":
        return N2, g, 100, dict(max_iters=0)
    if name == "per_dataset":
        return N2, [k.costs.GaussDist([1.0 + 0.3 * r, -0.5 + 0.1 * r]) for r in range(5)], 100, dict(epstol=0.05)
    if name == "readme_sim":       # final eff 0.07-0.09
        return README_PRIOR(k), k.costs.NormalMeanStdSim(1000, 2.0, 0.04), 100, dict(max_iters=30)
    if name == "user_rtc":
        noisy = _user_cost(k)
        orc.register_user_cost(noisy)
        return N2, noisy, 80, dict(max_iters=15)
    raise KeyError(name)


@pytest.mark.parametrize("spread", ["spread", "one-lane-per-particle"])
@pytest.mark.parametrize("name", CASES)
def test_batch_equals_single_runs(k, orc, gpu_ctx, monkeypatch, name, spread):
    """R = 5 unrelated seeds, one launch; every run equals its own pfilter() call, the first and last also
    the oracle"""
    monkeypatch.delenv("KABC_PF_BATCH", raising=False)
    if spread == "spread":
        monkeypatch.delenv("KABC_PF_BATCH_SPREAD", raising=False)
    else:
        monkeypatch.setenv("KABC_PF_BATCH_SPREAD", "0")
    prior, cost, N, kw = _case(k, orc, name)
    costs = cost if isinstance(cost, list) else [cost] * 5
    out = k.pfilter_batch(prior, cost, N, 5, seeds=SEEDS5, return_array=True, **kw)
    assert out.info["course"] == "grid" and out.info["launches"] == 1, out.info
    assert out.info["runs_per_launch"] == 5 and len(out) == 5
    assert out.info["status"] == [0] * 5
    for r in range(5):
        _same(out[r], k.pfilter(prior, costs[r], N, seed=SEEDS5[r], return_array=True, **kw), (name, r))
    for r in (0, 4):
        _same_as_oracle(out[r], orc.pfilter(prior, costs[r], N, seed=SEEDS5[r], **kw), (name, r))
    # the entries are views into one [R][N_eff][D] / [R][N_eff] block
    assert out.info["nparticles"] == out[0].P.shape[0]
    base, cbase = out[0].P.__array_interface__["data"][0], out[0].C.__array_interface__["data"][0]
    for r in range(5):
        assert out[r].P.__array_interface__["data"][0] == base + r * out[0].P.nbytes
        assert out[r].C.__array_interface__["data"][0] == cbase + r * out[0].C.nbytes


@pytest.mark.parametrize("spread", ["spread", "one-lane-per-particle"])
def test_batch_initial_redraws_bit_exact(k, orc, gpu_ctx, monkeypatch, spread):
    """every run's initial draw goes past attempt 0 (a cost that is +Inf half of the time, src/smc.jl:280-294):
    5 seeds at 50 particles in one launch, each run the oracle's"""
    monkeypatch.delenv("KABC_PF_BATCH", raising=False)
    if spread == "spread":
        monkeypatch.delenv("KABC_PF_BATCH_SPREAD", raising=False)
    else:
        monkeypatch.setenv("KABC_PF_BATCH_SPREAD", "0")
    seeds = [REDRAW_SEED] + SEEDS5[1:]
    for s in seeds:
        run0 = lambda pri, cost: orc.pfilter(pri, cost, 50, max_iters=0, seed=s)  # noqa: E731
        assert_redraws_happen(run0, redraw_case(k), redraw_case(k, 0.0))
    prior, cost = redraw_case(k)
    out = k.pfilter_batch(prior, cost, 50, 5, seeds=seeds, max_iters=8, return_array=True)
    assert out.info["course"] == "grid" and out.info["launches"] == 1, out.info
    assert out.info["status"] == [0] * 5
    for r in range(5):
        _same_as_oracle(out[r], orc.pfilter(prior, cost, 50, seed=seeds[r], max_iters=8), (spread, r))


def test_thousand_runs_one_grid(k, gpu_ctx, monkeypatch):
    monkeypatch.delenv("KABC_PF_BATCH", raising=False)
    monkeypatch.delenv("KABC_PF_BATCH_SPREAD", raising=False)
    N2 = k.Factored(k.Normal(0, 5), k.Normal(0, 5))
    cost = k.costs.GaussDist([1.0, -0.5])
    out = k.pfilter_batch(N2, cost, 100, 1000, seed=17, epstol=0.05, return_array=True)
    assert out.info["course"] == "grid" and out.info["runs_per_launch"] == 1000 and out.info["launches"] == 1
    seeds = k.api.chain_seeds(17, 1000)
    for r in (0, 1, 499, 999):
        _same(out[r], k.pfilter(N2, cost, 100, seed=seeds[r], epstol=0.05, return_array=True), r)
    base = out[0].P.__array_interface__["data"][0]
    assert out[999].P.__array_interface__["data"][0] == base + 999 * out[0].P.nbytes
    assert out[999].C.__array_interface__["data"][0] == out[0].C.__array_interface__["data"][0] + 999 * 100 * 8
    # the default seeds are chain_seeds(seed, nruns), and the runs differ from each other
    assert not np.array_equal(out[0].P, out[1].P)


@pytest.mark.parametrize("shape", ["batch_off", "n257", "d17"])
def test_sequential_course_same_bits(k, gpu_ctx, monkeypatch, shape):
    monkeypatch.delenv("KABC_PF_BATCH", raising=False)
    N2 = k.Factored(k.Normal(0, 5), k.Normal(0, 5))
    prior, cost, N, kw = N2, k.costs.GaussDist([1.0, -0.5]), 100, dict(max_iters=12)
    if shape == "batch_off":
        monkeypatch.setenv("KABC_PF_BATCH", "0")
    elif shape == "n257":
        N = 257
    else:
        prior = k.Factored(*[k.Normal(0, 2)] * 17)
        cost = k.costs.GaussDist(np.linspace(-1, 1, 17))
        kw = dict(max_iters=6, eff_tol=0.0)
    out = k.pfilter_batch(prior, cost, N, 3, seeds=SEEDS5[:3], return_array=True, **kw)
    assert out.info["course"] == "sequential" and out.info["runs_per_launch"] == 1, out.info
    assert out.info["launches"] == 3
    for r in range(3):
        _same(out[r], k.pfilter(prior, cost, N, seed=SEEDS5[r], return_array=True, **kw), (shape, r))


INF_SRC = """
KABC_HD double kabc_user_cost(const double* x, int D, const double* params, const double* data,
                              int64_t ndata, kabc_cost_rng_t* rng) {
    // params[0] < 0: a simulator that never produces a finite distance
    return params[0] < 0.0 ? KABC_INF : kabc_fabs(x[0] - params[0]) + kabc_fabs(x[1] + 0.5);
}
"""


def test_failing_run_leaves_the_others_alone(k, gpu_ctx, monkeypatch):
    monkeypatch.delenv("KABC_PF_BATCH", raising=False)
    N2 = k.Factored(k.Normal(0, 5), k.Normal(0, 5))
    costs = [k.costs.UserCost(INF_SRC, dims=[2], params=[-1.0 if r == 3 else 1.0 + 0.1 * r], name="inf_in_run")
             for r in range(5)]
    kw = dict(max_iters=12, return_array=True)
    with pytest.raises(k.KabcError) as e1:
        k.pfilter(N2, costs[3], 64, seed=SEEDS5[3], **kw)
    msg = str(e1.value)   # kabc_pfilter_run's own message
    assert "never produced a finite" in msg
    with pytest.raises(k.KabcError) as ei:
        k.pfilter_batch(N2, costs, 64, seeds=SEEDS5, **kw)
    e = ei.value
    assert str(e) == "run 3: " + msg, str(e)
    assert e.results.info["course"] == "grid"
    assert e.results.info["status"] == [0, 0, 0, k._cdefs.KABC_ERR_RETRY_EXHAUSTED, 0]
    assert [r is None for r in e.results] == [False, False, False, True, False]
    for r in (0, 1, 2, 4):
        _same(e.results[r], k.pfilter(N2, costs[r], 64, seed=SEEDS5[r], **kw), r)


def test_cancel_batch(k, monkeypatch):
    """pfilter's iterations are not a fixed amount of work (they grow as eff falls), so the call is made
    long by the NUMBER of runs.  n_draws of the simulator is the knob: large enough that the R which
    makes the call last about 5 s fits 65535, small enough that the longest iteration of a run stays
    well inside the bound.  Measured on an MI355X with N_DRAWS = 20000: see CANCEL_NOTES below."""
    monkeypatch.delenv("KABC_PF_BATCH", raising=False)
    monkeypatch.delenv("KABC_PF_BATCH_SPREAD", raising=False)
    prior = README_PRIOR(k)
    cost = k.costs.NormalMeanStdSim(N_DRAWS, 2.0, 0.04)
    kw = dict(return_array=True)
    OK, CANCELLED = 0, k._cdefs.KABC_ERR_CANCELLED
    ctx = k.Context(0)
    try:
        def timed(n):
            t0 = time.perf_counter()
            k.pfilter_batch(prior, cost, 100, n, seed=5, ctx=ctx, **kw)
            return time.perf_counter() - t0
        R0 = 1024
        a, b = timed(R0), timed(2 * R0)
        dt = max(b - a, 1e-6) / R0
        R = min(max(int(5.0 / dt), 2), 65535)
        print(f"cancel_batch: n_draws={N_DRAWS} t({R0})={a:.3f} s t({2 * R0})={b:.3f} s -> R={R}, "
              f"expected {R * dt:.2f} s")
        seeds = k.api.chain_seeds(5, R)
        box = {}

        def fire():
            box["t"] = time.perf_counter()
            ctx.cancel()

        tm = threading.Timer(0.3, fire)
        tm.start()
        err = None
        try:
            k.pfilter_batch(prior, cost, 100, R, seed=5, ctx=ctx, **kw)
        except k.Cancelled as ex:
            err = ex
        t_ret = time.perf_counter()
        tm.join()
        assert err is not None, "the batch finished before the cancel"
        print(f"cancel_batch: returned {t_ret - box['t']:.3f} s after the request")
        assert t_ret - box["t"] < 0.25, t_ret - box["t"]
        got, status = err.result, err.result.info["status"]
        assert len(got) == R
        finished, stopped, unstarted = [], [], []
        for r in range(R):
            assert status[r] in (OK, CANCELLED), (r, status[r])
            if status[r] == OK:
                assert got[r] is not None
                finished.append(r)
            elif got[r] is not None:
                assert got[r].info["iterations"] >= 1, (r, got[r].info)
                stopped.append(r)
            else:
                unstarted.append(r)
        print(f"cancel_batch: finished {len(finished)}, stopped {len(stopped)}, never started {len(unstarted)}")
        assert stopped, "no run was stopped at an iteration boundary"
        assert len(finished) < R, "the call finished"
        for r in (stopped[0], stopped[-1]):
            n = got[r].info["iterations"]
            _same(got[r], k.pfilter(prior, cost, 100, seed=seeds[r], ctx=ctx, max_iters=n - 1, **kw), (r, n))
        if finished:
            r = finished[0]
            _same(got[r], k.pfilter(prior, cost, 100, seed=seeds[r], ctx=ctx, **kw), r)
        # the request was consumed: the next call on the context runs normally
        out = k.pfilter_batch(prior, cost, 100, 2, seeds=seeds[:2], ctx=ctx, max_iters=2, **kw)
        assert [x.info["iterations"] for x in out] == [3, 3] and out.info["status"] == [0, 0]
    finally:
        ctx.close()


N_DRAWS = 20000
CANCEL_NOTES = """MI355X, n_draws = 20000: 1024 runs 0.478 s, 2048 runs 0.960 s -> R = 10604 for 5 s; the
call returned 0.021 s after the request; 513 runs had finished, 511 were stopped at an iteration boundary,
9580 were never started."""


@pytest.mark.parametrize("name", ["discrete_256", "readme_sim"])
def test_counters_are_the_sequential_loops(k, orc, gpu_ctx, monkeypatch, name):
    """nreps and cost_evals of the attempt-parallel phase are what the sequential loop books: attempts
    evaluated beyond a particle's first success are discarded and never counted"""
    monkeypatch.delenv("KABC_PF_BATCH", raising=False)
    monkeypatch.delenv("KABC_PF_BATCH_SPREAD", raising=False)
    prior, cost, N, kw = _case(k, orc, name)
    out = k.pfilter_batch(prior, cost, N, 5, seeds=SEEDS5, return_array=True, **kw)
    assert out.info["course"] == "grid"
    for r in range(5):
        ref = orc.pfilter(prior, cost, N, seed=SEEDS5[r], **kw)
        assert out[r].info["nreps"] == ref["nreps"], (name, r, out[r].info, ref["nreps"])
        assert out[r].info["cost_evals"] == ref["cost_evals"], (name, r, out[r].info, ref["cost_evals"])
        assert out[r].info["iterations"] == ref["iterations"], (name, r)
