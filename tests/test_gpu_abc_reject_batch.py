"""-m gpu: abc_reject_batch (kabc_abc_reject_batch; the kernel of csrc/abc_reject_batch_kernel.hpp).

The contract under test (include/kabc.h): run r of a batch IS abc_reject(prior, costs[r], eps[r], ..., seed=seeds[r]),
bit for bit, on every course.  Every comparison is on bit patterns and EVERY run of every batch is compared; a subset
is also compared with the CPU oracle's own tables (tests/abc_reject_batch_oracle.py), so the check is not only GPU
against GPU."""
import math

import numpy as np
import pytest

from abc_reject_batch_oracle import assert_run_equals, batch_tables, expected_batch
from test_gpu_abc_reject import D20_SRC, DIMS, FIRST_ROWS, SEEDS, _prior

pytestmark = pytest.mark.gpu


def _variants(k):
    """every built-in cost: (name, (D, r) -> the cost of run r, [D...]) with the dimensions
    tests/test_gpu_abc_reject.py uses for it; the runs' params / data differ (Rosenbrock and NoisyBanana have nothing
    to vary: their runs differ by seed or eps)"""
    rng = np.random.default_rng(5)
    centers = {D: rng.normal(size=D) for D in DIMS}
    ybars = {D: rng.normal(size=D - 2) for D in DIMS if D >= 3}
    wiener = np.sqrt(0.25 * np.arange(31.0) ** 2 + 4.0 * np.arange(31.0))
    return [
        ("GaussDist", lambda D, r: k.costs.GaussDist(centers[D] + 0.1 * r), list(DIMS)),
        ("Rosenbrock", lambda D, r: k.costs.Rosenbrock(), [D for D in DIMS if D >= 2]),
        ("HierGaussSim", lambda D, r: k.costs.HierGaussSim(ybars[D] - 0.2 * r), [D for D in DIMS if D >= 3]),
        ("NormalMeanStdSim", lambda D, r: k.costs.NormalMeanStdSim(1000, 2.0 + 0.05 * r, 0.04 + 0.005 * r), [2]),
        ("DiracSq", lambda D, r: k.costs.DiracSq(1.5 + 0.25 * r), [1]),
        ("AbsDiff", lambda D, r: k.costs.AbsDiff(1.5 - 0.25 * r), [1]),
        ("NormShell", lambda D, r: k.costs.NormShell(1.5 + 0.5 * r), list(DIMS)),
        ("NoisyQuadDU", lambda D, r: k.costs.NoisyQuadDU(5.5 + r), [2]),
        ("Mixture", lambda D, r: k.costs.Mixture(0.1 * r), [1]),
        ("NoisyBanana", lambda D, r: k.costs.NoisyBanana(0.5), [2]),
        ("WienerRms", lambda D, r: k.costs.WienerRms(wiener * (1.0 + 0.05 * r)), [2]),
    ]


def _singles(k, prior, costs, eps, n, seeds, **kw):
    return [k.abc_reject(prior, c, None if eps is None else eps[r], n, seed=seeds[r], return_array=True, **kw)
            for r, c in enumerate(costs)]


def _compare(batch, singles, what):
    assert len(batch) == len(singles)
    for r, (b, s) in enumerate(zip(batch, singles)):               # every run, no sampling
        assert_run_equals(b, s, what + (r,))


# ---- 1. each run equals its own abc_reject ----------------------------------------------------------
def test_each_run_equals_its_single_call(k, gpu_ctx):
    R, N = 4, 6000
    ran_ids, courses = set(), set()
    shift = 0
    for name, make, dims in _variants(k):
        for D in dims:
            costs = [make(D, r) for r in range(R)]
            prior = _prior(k, D, shift)
            shift += 1
            for shared in (True, False):
                for first_row in FIRST_ROWS:
                    seeds = [SEEDS[0]] * R if shared else [SEEDS[1] + 7 * r for r in range(R)]
                    what = (name, D, "shared seed" if shared else "seeds", first_row)
                    kw = dict(draws=N, first_row=first_row)
                    # keep mode; its eps (the 60th smallest cost of each run) feeds the threshold cases
                    sk = _singles(k, prior, costs, None, None, seeds, keep=60, **kw)
                    bk = k.abc_reject_batch(prior, costs, seeds=seeds, keep=60, return_array=True, **kw)
                    _compare(bk, sk, what + ("keep",))
                    courses.add(bk.info["course"])
                    want = "sequential" if D == 128 else ("table" if shared else "grid")
                    assert bk.info["course"] == want, (what, bk.info)
                    eps = [s.eps * (1.0 if r % 2 else 0.5) for r, s in enumerate(sk)]   # runs of different pace
                    assert all(math.isfinite(e) for e in eps), (what, eps)
                    for n in (20, 65):                                # 65 > 60: at least the odd runs are exhausted
                        st = _singles(k, prior, costs, eps, n, seeds, **kw)
                        bt = k.abc_reject_batch(prior, costs, eps, n, seeds=seeds, return_array=True, **kw)
                        _compare(bt, st, what + ("eps", n))
                        assert bt.info["status"] == [0] * R
                    assert any(s.info["exhausted"] for s in st), what
            ran_ids.add(costs[0].id)
    assert sorted(ran_ids) == list(range(1, 12)), ran_ids
    assert courses == {"table", "grid", "sequential"}, courses


# ---- 2. against the CPU oracle's tables --------------------------------------------------------------
def test_against_the_oracle(k, orc, gpu_ctx):
    rng = np.random.default_rng(12)
    cases = [
        ("GaussDist", _prior(k, 8, 1), [k.costs.GaussDist(rng.normal(size=8)) for _ in range(3)], 1500),
        ("NormalMeanStdSim", k.Factored(k.Uniform(1, 3), k.Uniform(0, 0.1)),
         [k.costs.NormalMeanStdSim(1000, 2.0 + 0.1 * r, 0.04) for r in range(3)], 300),
        ("Mixture", k.Gamma(2.0, 0.7), [k.costs.Mixture(0.2 * r) for r in range(3)], 1500),
        ("NoisyQuadDU, a discrete prior", k.Factored(k.Normal(1, 0.5), k.DiscreteUniform(1, 10)),
         [k.costs.NoisyQuadDU(3.5 + 2 * r) for r in range(3)], 1500),
    ]
    for name, prior, costs, N in cases:
        for seeds, first_row in (([SEEDS[0]] * 3, FIRST_ROWS[1]), ([3, 4, 3], FIRST_ROWS[0])):
            tabs = batch_tables(orc, prior, costs, N, seeds, first_row)
            eps = [float(np.nanquantile(t[2], q, method="lower")) for t, q in zip(tabs, (0.2, 0.05, 0.01))]
            for n in (5, N):
                want = expected_batch(tabs, eps=eps, n=n)
                got = k.abc_reject_batch(prior, costs, eps, n, seeds=seeds, draws=N, first_row=first_row,
                                         return_array=True)
                for r in range(3):
                    assert_run_equals(got[r], want[r], (name, seeds, "eps", n, r))
            want = expected_batch(tabs, keep=40)
            got = k.abc_reject_batch(prior, costs, seeds=seeds, draws=N, keep=40, first_row=first_row, return_array=True)
            for r in range(3):
                assert_run_equals(got[r], want[r], (name, seeds, "keep", r))
            assert got.info["course"] == "table"                      # ([3, 4, 3]: runs 0 and 2 share a table)


# ---- 3. the courses give the same bits ----------------------------------------------------------------
def test_courses_agree(k, gpu_ctx, monkeypatch):
    rng = np.random.default_rng(8)
    R, N = 6, 20000
    prior = _prior(k, 8, 3)
    costs = [k.costs.GaussDist(rng.normal(size=8)) for _ in range(R)]
    seeds = [11] * R
    base = _singles(k, prior, costs, None, None, seeds, draws=N, keep=200)
    eps = [s.eps for s in base]
    ref_t = _singles(k, prior, costs, eps, 150, seeds, draws=N)
    for env, course in (({}, "table"), ({"KABC_REJECT_BATCH_COURSE": "grid"}, "grid"),
                        ({"KABC_REJECT_BATCH": "0"}, "sequential"), ({"KABC_REJECT_BATCH_COMPACT": "wg"}, "table"),
                        ({"KABC_REJECT_BATCH_COURSE": "grid", "KABC_REJECT_BATCH_COMPACT": "wg"}, "grid")):
        with monkeypatch.context() as m:
            for name, v in env.items():
                m.setenv(name, v)
            bt = k.abc_reject_batch(prior, costs, eps, 150, seeds=seeds, draws=N, return_array=True)
            bk = k.abc_reject_batch(prior, costs, seeds=seeds, draws=N, keep=200, return_array=True)
        assert bt.info["course"] == course and bk.info["course"] == course, (env, bt.info, bk.info)
        _compare(bt, ref_t, (str(env), "eps"))
        _compare(bk, base, (str(env), "keep"))
        if course == "table":      # the table is drawn once: fewer theta rows than the grid's R per row
            assert 0 < bk.info["rows_drawn"] < R * N, bk.info
        if course == "grid":
            assert bk.info["rows_drawn"] >= R * N, bk.info
    # shapes the batch kernel does not take go one after another and still match
    A = rng.normal(size=(4, 4))
    mv = k.MvNormal(rng.normal(size=4), A @ A.T + 0.4 * np.eye(4))
    ros = [k.costs.Rosenbrock()] * 3
    s3 = [5, 6, 7]
    want = _singles(k, mv, ros, [30.0, 40.0, 50.0], 50, s3, draws=N)
    got = k.abc_reject_batch(mv, ros, [30.0, 40.0, 50.0], 50, seeds=s3, draws=N, return_array=True)
    assert got.info["course"] == "sequential" and [g.info["course"] for g in got] == ["phases"] * 3
    _compare(got, want, ("MvNormal",))
    monkeypatch.setenv("KABC_USER_PLUGIN", "hiprtc")
    users = [k.costs.UserCost(D20_SRC, dims=[20], params=[0.25 + 0.1 * r], name="dyn_user_reject") for r in range(3)]
    p20 = k.Factored(*[k.Normal(0, 1)] * 19, k.Beta(2.0, 2.0))
    want = _singles(k, p20, users, None, None, [9] * 3, draws=N, keep=100)
    got = k.abc_reject_batch(p20, users, seeds=[9] * 3, draws=N, keep=100, return_array=True)
    assert got.info["course"] == "sequential"
    _compare(got, want, ("UserCost",))


# ---- 4. runs that finish at different times -----------------------------------------------------------
def test_runs_finish_at_different_times(k, orc, gpu_ctx, monkeypatch):
    prior = k.Factored(k.Normal(1, 0.5), k.DiscreteUniform(1, 10))
    costs = [k.costs.NoisyQuadDU(t) for t in (3.5, 5.5, 7.5, 4.5)]
    N, n, seeds = 3000, 12, [3] * 4
    tabs = batch_tables(orc, prior, costs, N, seeds)
    # eps from the oracle table's cost quantiles: every row; one row in a hundred; fewer rows than n; none
    eps = [float(np.nanmax(tabs[0][2])), float(np.nanquantile(tabs[1][2], 0.01)),
           float(np.sort(tabs[2][2])[8]), float(np.nanmin(tabs[3][2])) - 1.0]
    assert not np.isnan(tabs[0][2][:n]).any()
    want = expected_batch(tabs, eps=eps, n=n)
    # a record buffer of 64: no look has fewer rows than the piece that cannot overflow, capacity / runs = 16
    # (include/kabc.h), so run 0, whose first 12 rows all accept, completes in the first look whatever its size
    monkeypatch.setenv("KABC_REJECT_CAPACITY", "64")
    got = k.abc_reject_batch(prior, costs, eps, n, seeds=seeds, draws=N, return_array=True)
    # the spread really occurred
    assert got.info["course"] == "table" and got.info["launches"] >= 3, got.info     # several looks
    assert got[0].info["draws"] == n <= 64 // 4 and got[0].C.size == n and not got[0].info["exhausted"]
    assert got[0].info["draws"] < got[1].info["draws"] < N and got[1].C.size == n and not got[1].info["exhausted"]
    assert got[1].info["draws"] > 10 * (64 // 4)                  # far beyond a first look that the buffer could hold
    assert got[2].info["exhausted"] and got[2].C.size == 9 and got[2].info["draws"] == N
    assert got[3].info["exhausted"] and got[3].C.size == 0 and got[3].info["draws"] == N
    for r in range(4):
        assert_run_equals(got[r], want[r], ("oracle", r))
    monkeypatch.delenv("KABC_REJECT_CAPACITY")
    _compare(got, _singles(k, prior, costs, eps, n, seeds, draws=N), ("singles",))


# ---- 5. overflow ----------------------------------------------------------------------------------------
def test_overflow_drops_nothing(k, gpu_ctx, monkeypatch):
    rng = np.random.default_rng(2)
    prior = k.Factored(k.Normal(0, 1), k.Uniform(-2, 2))
    costs = [k.costs.GaussDist(rng.normal(size=2)) for _ in range(5)]
    N, seeds = 20000, [4] * 5
    # eps from each run's own cost column (keep = N returns every row): all rows beside 1 %, 10 %, 0.1 % and 50 %
    full = _singles(k, prior, costs, None, None, seeds, draws=N, keep=N)
    eps = [math.inf] + [float(np.quantile(full[r].C, q)) for r, q in ((1, 0.01), (2, 0.1), (3, 0.001), (4, 0.5))]
    want = _singles(k, prior, costs, eps, N, seeds, draws=N)
    assert want[0].C.size == N and 0 < want[3].C.size < want[1].C.size < want[2].C.size < want[4].C.size < N
    for compact in ("wave", "wg"):
        monkeypatch.setenv("KABC_REJECT_BATCH_COMPACT", compact)
        monkeypatch.setenv("KABC_REJECT_CAPACITY", "256")
        got = k.abc_reject_batch(prior, costs, eps, N, seeds=seeds, draws=N, return_array=True)
        monkeypatch.delenv("KABC_REJECT_CAPACITY")
        _compare(got, want, ("overflow", compact))
        assert np.array_equal(got[0].info["index"], np.arange(N))      # the order is restored
        assert got.info["launches"] >= sum(w.C.size for w in want) // 256   # no look held more than the buffer
        gk = k.abc_reject_batch(prior, costs, seeds=seeds, draws=N, keep=N // 2, return_array=True)
        _compare(gk, _singles(k, prior, costs, None, None, seeds, draws=N, keep=N // 2), ("keep half", compact))


# ---- 6. edges -------------------------------------------------------------------------------------------
def test_edges(k, gpu_ctx):
    prior = k.Factored(k.Normal(0, 1), k.Uniform(-2, 2))
    g = k.costs.GaussDist([0.3, -0.2])
    # one run
    one = k.abc_reject_batch(prior, [g], 0.1, 50, seeds=[8], draws=50000, return_array=True)
    assert len(one) == 1 and one.info["nruns"] == 1
    assert_run_equals(one[0], k.abc_reject(prior, g, 0.1, 50, draws=50000, seed=8, return_array=True), "nruns = 1")
    # one DeviceCost, runs that differ by eps / by seed
    by_eps = k.abc_reject_batch(prior, g, [0.05, 0.1, 0.2], 30, nruns=3, seed=8, draws=50000, return_array=True)
    _compare(by_eps, _singles(k, prior, [g] * 3, [0.05, 0.1, 0.2], 30, [8] * 3, draws=50000), ("by eps",))
    by_seed = k.abc_reject_batch(prior, g, 0.1, 30, seeds=[1, 2, 3], draws=50000, return_array=True)
    assert by_seed.info["course"] == "grid"
    _compare(by_seed, _singles(k, prior, [g] * 3, [0.1] * 3, 30, [1, 2, 3], draws=50000), ("by seed",))
    # n = 0: nothing asked for, nothing launched
    none = k.abc_reject_batch(prior, [g, g], 0.1, 0, return_array=True)
    assert none.info["launches"] == 0 and all(r.C.size == 0 and r.info["draws"] == 0 for r in none)
    # more runs than one launch's grid holds rows for: a few thousand runs x a few thousand draws
    rng = np.random.default_rng(21)
    R, N = 3000, 4000
    costs = [k.costs.GaussDist(c) for c in rng.normal(size=(R, 2))]
    eps = list(rng.uniform(0.02, 0.3, size=R))
    big = k.abc_reject_batch(prior, costs, eps, 5, seed=6, draws=N, return_array=True)
    assert big.info["course"] == "table" and big.info["runs_per_launch"] == R
    _compare(big, _singles(k, prior, costs, eps, 5, [6] * R, draws=N), ("3000 runs, table",))
    assert any(r.info["exhausted"] for r in big) and any(not r.info["exhausted"] for r in big)
    R2 = 1500
    seeds = [1000 + r for r in range(R2)]
    big = k.abc_reject_batch(prior, costs[:R2], eps[:R2], 5, seeds=seeds, draws=N, return_array=True)
    assert big.info["course"] == "grid"
    _compare(big, _singles(k, prior, costs[:R2], eps[:R2], 5, seeds, draws=N), ("1500 runs, grid",))
    # keep mode with +Inf costs (NoisyBanana p_inf = 0.5: half of the rows cost +Inf) -- more rows kept than are
    # finite, so +Inf ties are broken by the lower index; runs 0 and 1 share a seed, run 2 does not
    pb = k.Factored(k.Normal(0, 2), k.Normal(0, 2))
    nb = [k.costs.NoisyBanana(0.5)] * 3
    Nb = 8000
    want = _singles(k, pb, nb, None, None, [5, 5, 6], draws=Nb, keep=3 * Nb // 4)
    got = k.abc_reject_batch(pb, nb, seeds=[5, 5, 6], draws=Nb, keep=3 * Nb // 4, return_array=True)
    _compare(got, want, ("NoisyBanana keep",))
    assert got[0].eps == math.inf and np.isinf(got[0].C).sum() > Nb // 8
    assert_run_equals(got[1], got[0], "two runs of one seed and one dataset")


# ---- 7. cancel --------------------------------------------------------------------------------------------
def test_cancel_pending_at_entry(k, gpu_ctx):
    import ctypes as C
    from kissabc_jl_amd import _lib
    prior = k.Factored(k.Normal(0, 1), k.Uniform(-2, 2))
    costs = [k.costs.GaussDist([0.1 * r, 0.0]) for r in range(4)]
    ctx = k.Context(0)
    try:
        ctx.cancel()                                   # on an idle context: cancels the next call
        with pytest.raises(k.Cancelled) as ei:
            k.abc_reject_batch(prior, costs, 0.1, 20, draws=10000, ctx=ctx, return_array=True)
        res = ei.value.result
        assert res.info["launches"] == 0 and res.info["status"] == [7] * 4
        assert all(r.C.size == 0 and r.info["draws"] == 0 for r in res)
        st = (C.c_int64 * 4)()
        _lib.load().kabc_reject_batch_stats(st)
        assert st[1] == 0 and st[3] == 0               # no launch, no row drawn
        ctx.clear_cancel()
        got = k.abc_reject_batch(prior, costs, 0.1, 20, draws=10000, ctx=ctx, return_array=True)
        _compare(got, _singles(k, prior, costs, [0.1] * 4, 20, [0] * 4, draws=10000), ("after a cancelled call",))
    finally:
        ctx.close()


def test_cancel_pending_at_entry_one_after_another(k, gpu_ctx, monkeypatch):
    """the same on the course that hands the runs to abc_reject in turn: run 0 takes the request, no run launches"""
    monkeypatch.setenv("KABC_REJECT_BATCH", "0")
    prior = k.Factored(k.Normal(0, 1), k.Uniform(-2, 2))
    costs = [k.costs.GaussDist([0.1 * r, 0.0]) for r in range(3)]
    ctx = k.Context(0)
    try:
        ctx.cancel()
        with pytest.raises(k.Cancelled) as ei:
            k.abc_reject_batch(prior, costs, 0.1, 20, draws=10000, ctx=ctx, return_array=True)
        res = ei.value.result
        assert res.info["course"] == "sequential" and res.info["launches"] == 0 and res.info["status"] == [7] * 3
        assert all(r.C.size == 0 and r.info["draws"] == 0 for r in res)
        got = k.abc_reject_batch(prior, costs, 0.1, 20, draws=10000, ctx=ctx, return_array=True)
        assert got.info["course"] == "sequential" and got.info["launches"] >= 3
        _compare(got, _singles(k, prior, costs, [0.1] * 3, 20, [0] * 3, draws=10000), ("after a cancelled call",))
    finally:
        ctx.close()
