"""GPU: ABCDE_batch / kabc_abcde_run_batch -- many independent ABCDE runs in one call.

Run r of a batch must be bit-identical to ABCDE(prior, cost_r, eps, seed=seeds[r], <same keywords>) in
every field ABCDE returns: the population, the costs, reached_ϵ, generations_run and nsims.  With
nparticles <= 256 and length(prior) <= 16 the runs are the workgroups of one launch, each from its initial
draw to its last generation; other shapes run one after another, with the same bits."""
import threading
import time

import numpy as np
import pytest

from helpers import REDRAW_SEED, assert_redraws_happen, redraw_case

pytestmark = pytest.mark.gpu

SEEDS5 = [1, 977, 2 ** 40 + 3, 123456789, 0x9E3779B97F4A7C15 % (1 << 63)]


def _same(got, ref, what):
    assert np.array_equal(np.asarray(got.P).view(np.uint64), np.asarray(ref.P).view(np.uint64)), what
    assert np.array_equal(np.asarray(got.C).view(np.uint64), np.asarray(ref.C).view(np.uint64)), what
    assert got.reached_ϵ == ref.reached_ϵ, what
    assert got.info["generations_run"] == ref.info["generations_run"], what
    assert got.info["nsims"] == ref.info["nsims"], what


def _same_as_oracle(got, ref, what):
    assert np.array_equal(got.P, ref["P"]) and np.array_equal(got.C, ref["C"]), what
    assert got.reached_ϵ == ref["reached_eps"], what
    assert got.info["generations_run"] == ref["generations_run"] and got.info["nsims"] == ref["nsims"], what


def _user_cost(k):
    return k.costs.UserCost("""
KABC_HD double kabc_user_cost(const double* x, int D, const double* params, const double* data,
                              int64_t ndata, kabc_cost_rng_t* rng) {
    double z0, z1;
    kabc_cost_rng_normal2(rng, &z0, &z1);
    return kabc_fabs(x[0] - params[0]) + kabc_fabs(x[1] - params[1]) + 0.01 * kabc_fabs(z0);
}
""", dims=[2], params=[1.0, -0.5], name="abcde_batch_l1_noisy")


def _cases(k, orc):
    N2 = k.Factored(k.Normal(0, 5), k.Normal(0, 5))
    g = k.costs.GaussDist([1.0, -0.5])
    comps = [k.Normal(0, 2), k.Uniform(-3, 3), k.Gamma(2.5, 0.7), k.DiscreteUniform(-4, 4)]
    mixed16 = k.Factored(*[comps[j % 4] for j in range(16)])
    noisy = _user_cost(k)
    orc.register_user_cost(noisy)
    targets = [k.costs.GaussDist([1.0 + 0.3 * r, -0.5 + 0.1 * r]) for r in range(5)]
    return {
        # tests/test_abcde.py's cases, at most 256 particles
        "gauss": (N2, g, 0.05, dict(nparticles=256, generations=100)),
        "gauss_alpha_early": (N2, g, 0.3, dict(nparticles=200, generations=60, alpha=0.3, earlystop=True)),
        "banana_noisy": (N2, k.costs.NoisyBanana(0.0), 0.05, dict(nparticles=256, generations=50, proposal_width=0.8)),
        "dirac_d1": (k.Normal(1, 0.2), k.costs.DiracSq(1.5), 0.01, dict(nparticles=64)),
        "discrete": (k.Factored(k.Normal(1, 0.5), k.DiscreteUniform(1, 10)), k.costs.NoisyQuadDU(5.5), 0.05,
                     dict(nparticles=128, generations=30)),
        # the edges of the one-workgroup shape
        "n3": (N2, g, 0.05, dict(nparticles=3, generations=40)),
        "gen0": (N2, g, 0.05, dict(nparticles=100, generations=0)),
        "d16_mixed": (mixed16, k.costs.GaussDist(np.linspace(-0.5, 1.5, 16)), 3.0,
                      dict(nparticles=100, generations=25, proposal_width=0.9)),
        "per_dataset": (N2, targets, 0.1, dict(nparticles=50, generations=20, alpha=0.2)),
        "user_rtc": (N2, noisy, 0.05, dict(nparticles=80, generations=30)),
    }


@pytest.mark.parametrize("name", ["gauss", "gauss_alpha_early", "banana_noisy", "dirac_d1", "discrete", "n3", "gen0",
                                  "d16_mixed", "per_dataset", "user_rtc"])
def test_batch_equals_single_runs(k, orc, gpu_ctx, monkeypatch, name):
    """R = 5 unrelated seeds, one launch; every run equals its own ABCDE() call, the first and last
    also the oracle"""
    monkeypatch.delenv("KABC_ABCDE_SMALL", raising=False)
    prior, cost, eps, kw = _cases(k, orc)[name]
    costs = cost if isinstance(cost, list) else [cost] * 5
    out = k.ABCDE_batch(prior, cost, eps, 5, seeds=SEEDS5, return_array=True, **kw)
    assert out.info["course"] == "grid" and out.info["launches"] == 1, out.info
    assert out.info["runs_per_launch"] == 5 and len(out) == 5
    for r in range(5):
        _same(out[r], k.ABCDE(prior, costs[r], eps, seed=SEEDS5[r], return_array=True, **kw), (name, r))
    for r in (0, 4):
        _same_as_oracle(out[r], orc.abcde(prior, costs[r], eps, seed=SEEDS5[r], **kw), (name, r))
    # the entries are views into one [R][N][D] block
    base = out[0].P.__array_interface__["data"][0]
    for r in range(5):
        assert out[r].P.__array_interface__["data"][0] == base + r * out[0].P.nbytes


def test_batch_initial_redraws_bit_exact(k, orc, gpu_ctx, monkeypatch):
    """every run's initial draw goes past attempt 0 (a cost that is +Inf half of the time, src/smc.jl:351-366):
    5 seeds at 50 particles in one launch, each run the oracle's"""
    monkeypatch.delenv("KABC_ABCDE_SMALL", raising=False)
    kw = dict(nparticles=50, generations=15)
    seeds = [REDRAW_SEED] + SEEDS5[1:]
    for s in seeds:
        run0 = lambda pri, cost: orc.abcde(pri, cost, 0.5, nparticles=50, generations=0, seed=s)  # noqa: E731
        assert_redraws_happen(run0, redraw_case(k), redraw_case(k, 0.0))
    prior, cost = redraw_case(k)
    out = k.ABCDE_batch(prior, cost, 0.5, 5, seeds=seeds, return_array=True, **kw)
    assert out.info["course"] == "grid" and out.info["launches"] == 1, out.info
    for r in range(5):
        ref = orc.abcde(prior, cost, 0.5, seed=seeds[r], **kw)
        assert np.array_equal(out[r].P.view(np.uint64), ref["P"].view(np.uint64)), r
        assert np.array_equal(out[r].C.view(np.uint64), ref["C"].view(np.uint64)), r
        _same_as_oracle(out[r], ref, r)


def test_thousand_runs_one_grid(k, gpu_ctx):
    N2 = k.Factored(k.Normal(0, 5), k.Normal(0, 5))
    cost = k.costs.GaussDist([1.0, -0.5])
    out = k.ABCDE_batch(N2, cost, 0.05, 1000, seed=17, return_array=True)
    assert out.info["course"] == "grid" and out.info["runs_per_launch"] == 1000 and out.info["launches"] == 1
    seeds = k.api.chain_seeds(17, 1000)
    for r in (0, 1, 499, 999):
        _same(out[r], k.ABCDE(N2, cost, 0.05, seed=seeds[r], return_array=True), r)
    base = out[0].P.__array_interface__["data"][0]
    assert out[999].P.__array_interface__["data"][0] == base + 999 * out[0].P.nbytes
    assert out[999].C.__array_interface__["data"][0] == out[0].C.__array_interface__["data"][0] + 999 * 50 * 8
    # the default seeds are chain_seeds(seed, nruns), and the runs differ from each other
    assert not np.array_equal(out[0].P, out[1].P)


@pytest.mark.parametrize("shape", ["small_off", "n257", "d17"])
def test_sequential_course_same_bits(k, gpu_ctx, monkeypatch, shape):
    monkeypatch.delenv("KABC_ABCDE_SMALL", raising=False)
    N2 = k.Factored(k.Normal(0, 5), k.Normal(0, 5))
    prior, cost, kw = N2, k.costs.GaussDist([1.0, -0.5]), dict(nparticles=100, generations=15)
    if shape == "small_off":
        monkeypatch.setenv("KABC_ABCDE_SMALL", "0")
    elif shape == "n257":
        kw["nparticles"] = 257
    else:
        prior = k.Factored(*[k.Normal(0, 2)] * 17)
        cost = k.costs.GaussDist(np.linspace(-1, 1, 17))
    out = k.ABCDE_batch(prior, cost, 0.1, 3, seeds=SEEDS5[:3], return_array=True, **kw)
    assert out.info["course"] == "sequential" and out.info["runs_per_launch"] == 1, out.info
    for r in range(3):
        _same(out[r], k.ABCDE(prior, cost, 0.1, seed=SEEDS5[r], return_array=True, **kw), (shape, r))


INF_SRC = """
KABC_HD double kabc_user_cost(const double* x, int D, const double* params, const double* data,
                              int64_t ndata, kabc_cost_rng_t* rng) {
    // params[0] < 0: a simulator that never produces a finite distance
    return params[0] < 0.0 ? KABC_INF : kabc_fabs(x[0] - params[0]) + kabc_fabs(x[1] + 0.5);
}
"""


def test_failing_run_leaves_the_others_alone(k, gpu_ctx):
    N2 = k.Factored(k.Normal(0, 5), k.Normal(0, 5))
    costs = [k.costs.UserCost(INF_SRC, dims=[2], params=[-1.0 if r == 3 else 1.0 + 0.1 * r], name="inf_in_run")
             for r in range(5)]
    kw = dict(nparticles=64, generations=20, return_array=True)
    msg = "ABCDE: the prior never produced a finite (cost, logpdf) pair for some particle"
    with pytest.raises(k.KabcError) as ei:
        k.ABCDE_batch(N2, costs, 0.05, seeds=SEEDS5, **kw)
    e = ei.value
    assert str(e) == "run 3: " + msg, str(e)
    assert e.results.info["course"] == "grid"
    assert e.results.info["status"] == [0, 0, 0, k._cdefs.KABC_ERR_RETRY_EXHAUSTED, 0]
    assert [r is None for r in e.results] == [False, False, False, True, False]
    for r in (0, 1, 2, 4):
        _same(e.results[r], k.ABCDE(N2, costs[r], 0.05, seed=SEEDS5[r], **kw), r)
    with pytest.raises(k.KabcError, match="never produced a finite"):
        k.ABCDE(N2, costs[3], 0.05, seed=SEEDS5[3], **kw)


def test_cancel_batch(k):
    # an expensive simulator (the README cost with 20 000 draws per evaluation) keeps the generations
    # long, so that the cancelled runs end after a few hundred of them
    prior = k.Factored(k.Uniform(1, 3), k.Truncated(k.Normal(0, 0.1), 0, 100))
    cost = k.costs.NormalMeanStdSim(20000, 2.0, 0.04)
    kw = dict(nparticles=50, return_array=True)
    seeds = [3, 4, 5, 6]
    ctx = k.Context(0)
    try:
        def timed(n):
            t0 = time.perf_counter()
            k.ABCDE_batch(prior, cost, 0.0, 4, seeds=seeds, ctx=ctx, generations=n, **kw)
            return time.perf_counter() - t0
        a, b = timed(20), timed(100)
        dt = max(b - a, 1e-6) / 80
        M = max(int(5.0 / dt), 2)
        box = {}

        def fire():
            box["t"] = time.perf_counter()
            ctx.cancel()

        tm = threading.Timer(0.3, fire)
        tm.start()
        err = None
        try:
            k.ABCDE_batch(prior, cost, 0.0, 4, seeds=seeds, ctx=ctx, generations=M, **kw)
        except k.Cancelled as ex:
            err = ex
        t_ret = time.perf_counter()
        tm.join()
        assert err is not None, "the batch finished before the cancel"
        assert t_ret - box["t"] < 0.25, t_ret - box["t"]
        got = err.result
        assert len(got) == 4 and all(g is not None for g in got)
        assert err.result.info["status"] == [k._cdefs.KABC_ERR_CANCELLED] * 4
        for r in (0, 3):
            n = got[r].info["generations_run"]
            assert 0 < n < M, (r, n, M)
            _same(got[r], k.ABCDE(prior, cost, 0.0, seed=seeds[r], ctx=ctx, generations=n, **kw), r)
        # the request was consumed: the next call on the context runs normally
        out = k.ABCDE_batch(prior, cost, 0.0, 2, seeds=seeds[:2], ctx=ctx, generations=3, **kw)
        assert [x.info["generations_run"] for x in out] == [3, 3]
    finally:
        ctx.close()
