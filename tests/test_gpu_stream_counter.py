"""-m gpu: the random streams where the transition counter leaves 32 bits.

Every draw is a function of (seed, walker, t, slot, domain); word 1 of the Philox counter holds the low half of t,
word 3 the domain byte and the upper 24 bits (include/kabc_philox.h).  A short run never moves that upper word, so
a kernel that narrowed `t0 + s` or `g * nt`, or took word 3 out of a sub-step loop, would pass every other test.
Here every driver starts from a counter next to 2^32, with all 24 upper bits in use, or at the end of the range:

  AIS      set_state(x, lp, ll, t0) on the handle's own init() state, device against OracleAIS from the same
           state: the trace, the debug records (move id, accept and evaluated flags, partner rows), the final
           x / lp / ll / t and stats(), bit for bit, on every advance course, with the costs that draw
  pfilter  t = (iteration << 24) | attempt: runs of 263 iterations (the upper word moves at iteration 256), whole
           and split at 255 and 256, against the oracle and against the oracle continued from the same state
  smc      a state after three iterations whose pass counter is set next to 2^32 ... 2^56, continued on the four
           courses, against the oracle continued from the same state
  ABCDE    the same with the generation counter; opts->generations is then a 64-bit total
  limits   counters at or beyond 2^56 (pfilter: iterations at or beyond 2^32) are refused before anything is
           launched, with the message the oracle gives

The word-3 composition itself is pinned against a third statement of Philox in tests/test_math_contract.py (the
device and the oracle's costs compile the same header, so parity alone would not see it wrong)."""
import math

import numpy as np
import pytest

from test_gpu_smc_resume import BASE_KW, FOUR, _env as _smc_env
from test_user_cost import BANANA_LPI, SIM_SRC

pytestmark = pytest.mark.gpu

T = 2 ** 32
LIMIT = 2 ** 56
NT = 8
COUNTERS = {"T-3": T - 3, "T-8": T - 8, "ABCDEF*T-3": 0xABCDEF * T - 3, "2^56-16": LIMIT - 16}
AIS_ENV = ("KABC_AIS_SMALL", "KABC_AIS_WIDE", "KABC_SPECIALIZE", "KABC_AUX_KIB")


def _box(k, D, cost=None, eps=1.0):
    return k.ApproxKernelizedPosterior(k.Factored(*[k.Uniform(-5, 5)] * D), cost or k.costs.Rosenbrock(), eps)


def _course(monkeypatch, course):
    """the environment of an advance course and the driver it must report"""
    for name in AIS_ENV:
        monkeypatch.delenv(name, raising=False)
    if course == "small":
        return "small"
    monkeypatch.setenv("KABC_AIS_SMALL", "0")
    if course == "existing":
        monkeypatch.setenv("KABC_AIS_WIDE", "0")
    elif course == "wide":          # (=2: a launch that cannot take the wide kernel is an error)
        monkeypatch.setenv("KABC_AIS_WIDE", "2")
        monkeypatch.setenv("KABC_SPECIALIZE", "0")
    return "halves"


def _records_equal(dbg, tr, N):
    """the device's debug records against the oracle's trace records of one generation: move id, accept and
    evaluated flags as they are, partner ROWS of the complementary half against walker ids"""
    for col in (0, 1, 5):
        assert np.array_equal(dbg[:, :, col], tr[:, :, col]), col
    n0 = (N + 1) // 2
    base = np.where(np.arange(N) < n0, n0, 0)[:, None]
    for col in (2, 3, 4):
        d = dbg[:, :, col].astype(np.int64)
        assert np.array_equal(np.where(d >= 0, d + base, -1), tr[:, :, col].astype(np.int64)), col


def _both_refuse(k, orc, device, oracle, word):
    """the library and the oracle refuse with KABC_ERR_INVALID_ARG and the same message"""
    from kissabc_jl_amd import _cdefs as cd
    with pytest.raises(k.KabcError) as e:
        device()
    with pytest.raises(orc.OracleError) as eo:
        oracle()
    assert str(e.value) == str(eo.value) and word in str(e.value), (str(e.value), str(eo.value))
    assert e.value.status == eo.value.status == cd.KABC_ERR_INVALID_ARG


def _start(k, orc, model, N, seed, t0, init_model=None):
    """a handle and an oracle at (the handle's init() state, t0).  init_model: the model whose init() state is
    taken where the model's own cannot be drawn"""
    if init_model is None:
        ens = k.AisEnsemble(model, N, seed=seed).init()
        x, lp, ll, t = ens.state()
        assert t == 0
    else:
        first = k.AisEnsemble(init_model, N, seed=seed).init()
        x, lp, ll, _ = first.state()
        first.close()
        ens = k.AisEnsemble(model, N, seed=seed)
    o = orc.OracleAIS(model, N, seed=seed)
    ens.set_state(x, lp, ll, t0)
    o.set_state(x, lp, ll, t0)
    return ens, o


def _ais_case(k, orc, model, N, t0, driver, nt=NT, seed=3, calls=(1, 2), init_model=None, moves=True):
    """device against oracle from (init() state, t0) over the advance calls `calls` (generations of each): the
    trace of every call, the debug records of the calls of one generation, the final state and the counters"""
    ens, o = _start(k, orc, model, N, seed, t0, init_model)
    try:
        assert ens.driver == driver
        done = 0
        seen = set()
        for g in calls:
            if g == 1:
                ens.set_debug(nt)
            got = ens.advance(g, nt, collect=True)
            ref, tr = o.generations_sync(g, nt, trace=True)
            assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), (done, g)
            if g == 1:
                dbg = ens.get_debug(nt)
                ens.set_debug(0)
                _records_equal(dbg, tr[0], N)
                seen |= set(np.unique(dbg[:, :, 0]).tolist())
            done += g
        xs, lps, lls, t = ens.state()
        xo, lpo, llo, to = o.state()
        assert t == to == t0 + done * nt
        for a, b in ((xs, xo), (lps, lpo), (lls, llo)):
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
        assert ens.stats() == o.stats()
        if moves:
            assert seen == {1, 2, 3}      # the records cover stretch, DE and walk
        return ens.stats()
    finally:
        ens.close()
        o.close()


# ---- AIS: the first start counter on every course -------------------------------------------------------------
SHAPES = [("small", 12, 2), ("small", 100, 2), ("small", 512, 8), ("existing", 130, 3), ("existing", 641, 3)]


@pytest.mark.parametrize("course,N,D", SHAPES)
def test_ais_first_counter_on_every_shape(k, orc, gpu_ctx, monkeypatch, course, N, D):
    """t0 = 2^32 - 3, nt = 8: the upper word changes at sub-step 3 of the first launch"""
    driver = _course(monkeypatch, course)
    _ais_case(k, orc, _box(k, D), N, T - 3, driver)


@pytest.mark.parametrize("name", list(COUNTERS))
def test_ais_wide_geometry(k, orc, gpu_ctx, monkeypatch, name):
    """193 rows per half, nt = 9 = 2 K + 1: the last chunk of sub-steps holds one"""
    driver = _course(monkeypatch, "wide")
    t0 = COUNTERS[name] if name != "2^56-16" else LIMIT - 18      # (two generations of nine sub-steps)
    _ais_case(k, orc, _box(k, 8), 386, t0, driver, nt=9, calls=(1, 1) if name == "2^56-16" else (1, 2))


@pytest.mark.parametrize("name", ["T-8", "ABCDEF*T-3", "2^56-16"])
@pytest.mark.parametrize("course,N,D", SHAPES)
def test_ais_other_counters(k, orc, gpu_ctx, monkeypatch, course, N, D, name):
    """T - 8: the change falls on a generation boundary, two generations in one call and as two calls;
    0xABCDEF T - 3: all 24 upper bits in use, the carry runs through them; 2^56 - 16: the last two admissible
    generations (one more is refused: test_ais_counter_range_is_enforced)"""
    driver = _course(monkeypatch, course)
    t0 = COUNTERS[name]
    if name == "T-8":
        one = _ais_case(k, orc, _box(k, D), N, t0, driver, calls=(2,), moves=False)     # (no records: one call)
        two = _ais_case(k, orc, _box(k, D), N, t0, driver, calls=(1, 1))
        assert one == two
    elif name == "2^56-16":
        _ais_case(k, orc, _box(k, D), N, t0, driver, calls=(1, 1))
    else:
        _ais_case(k, orc, _box(k, D), N, t0, driver)


def test_ais_model_specialised_kernels(k, orc, gpu_ctx, monkeypatch):
    """the model's own kernels (tests/test_gpu_user_priors.py::test_specialised_ais_kernels_bit_exact waits for
    them the same way): four prior families, NormShell"""
    for name in AIS_ENV:
        monkeypatch.delenv(name, raising=False)
    four = k.Factored(k.Gamma(2.5, 0.7), k.LogNormal(0.3, 0.6), k.Beta(2.0, 3.0), k.Exponential(2.0))
    model = k.ApproxKernelizedPosterior(four, k.costs.NormShell(2.0), 0.5)
    h = k.compile_model(model, families=1)
    assert h > 0
    try:
        probe = k.AisEnsemble(model, 333, seed=3).init()
        assert probe.spec_state() == ("active", 0)
        driver = probe.driver
        probe.close()
        _ais_case(k, orc, model, 333, T - 3, driver)
    finally:
        k._lib.check(k._lib.load().kabc_model_release(h))


@pytest.mark.parametrize("N,driver", [(130, "halves"), (40, "small")])
def test_ais_run_time_dimension(k, orc, gpu_ctx, monkeypatch, N, driver):
    """20 parameters: the launch per half-generation (130 walkers) and the one-workgroup kernel (40)"""
    for name in AIS_ENV:
        monkeypatch.delenv(name, raising=False)
    if driver == "halves":
        monkeypatch.setenv("KABC_AIS_SMALL", "0")
    _ais_case(k, orc, _box(k, 20, eps=2.0), N, T - 3, driver)


def test_ais_batch_handle(k, orc, gpu_ctx, monkeypatch):
    """three chains in one handle (no debug records there): each against a single-chain oracle"""
    for name in AIS_ENV:
        monkeypatch.delenv(name, raising=False)
    model, N, seeds, t0 = _box(k, 2), 20, [3, 977, 2 ** 40 + 3], T - 3
    ens = k.AisEnsemble(model, N, seeds=seeds).init()
    x, lp, ll, _ = ens.state()
    ens.set_state(x, lp, ll, t0)
    got = ens.advance(3, NT, collect=True)                  # [generation][chain][N][D]
    xs, lps, lls, t = ens.state()
    assert t == t0 + 3 * NT
    total = {"proposals": 0, "cost_evals": 0, "accepted": 0}
    for c, seed in enumerate(seeds):
        o = orc.OracleAIS(model, N, seed=seed)
        o.set_state(x[c], lp[c], ll[c], t0)
        assert np.array_equal(got[:, c], o.generations_sync(3, NT)), c
        xo, lpo, llo, to = o.state()
        assert to == t and np.array_equal(xs[c], xo) and np.array_equal(lps[c], lpo) and np.array_equal(lls[c], llo), c
        for key, v in o.stats().items():
            total[key] += v
        o.close()
    assert ens.stats() == total
    ens.close()


# ---- AIS: the costs that draw, and the other posterior kinds --------------------------------------------------
README_PRIOR = lambda k: k.Factored(k.Uniform(1, 3), k.Truncated(k.Normal(0, 0.1), 0, 100))    # noqa: E731


def _stochastic(k, orc, name):
    """(model, model whose init() state the case starts from or None)"""
    if name == "hier":          # normals prefetched by the producers
        prior = k.Factored(k.Normal(0, 5), k.Uniform(0, 5), k.Normal(0, 1), k.Normal(0, 1))
        return k.ApproxKernelizedPosterior(prior, k.costs.HierGaussSim(np.array([0.9, 1.3])), 0.5), None
    if name == "banana":        # uniforms, Inf costs
        return _box(k, 2, k.costs.NoisyBanana(0.5), 2.0), None
    if name.startswith("meanstd"):      # the prepared-cost pre-pass, keyed by t0
        n = int(name[7:])
        model = k.ApproxKernelizedPosterior(README_PRIOR(k), k.costs.NormalMeanStdSim(n, 2.0, 0.05), 0.05)
        if n > 1:
            return model, None
        # one draw: the simulator's standard deviation is 0 / 0, every cost is NaN and no walker can be initialised
        # (on the oracle either) -- the case starts from the init() state of the 300-draw model: every proposal
        # inside the prior is evaluated and refused
        return model, k.ApproxKernelizedPosterior(README_PRIOR(k), k.costs.NormalMeanStdSim(300, 2.0, 0.05), 0.05)
    if name == "user":          # a hipRTC cost drawing from `rng`
        data = np.cumsum(np.random.default_rng(5).normal(size=24)) * 0.3
        cost = k.costs.UserCost(SIM_SRC, dims=[3], params=[0.5], data=data, name="ar1", posteriors=["kernelized"])
        orc.register_user_cost(cost)
        return k.ApproxKernelizedPosterior(k.Factored(k.Uniform(-1, 1), k.Uniform(0, 2), k.Normal(0, 1)), cost, 0.2), None
    raise KeyError(name)


@pytest.mark.parametrize("course,N", [("small", 100), ("existing", 130)])
@pytest.mark.parametrize("name", ["hier", "banana", "meanstd1", "meanstd3", "meanstd300", "user"])
def test_ais_costs_that_draw(k, orc, gpu_ctx, monkeypatch, name, course, N):
    """the *_COST domains see the upper word too: t0 = 2^32 - 3"""
    driver = _course(monkeypatch, course)
    model, init_model = _stochastic(k, orc, name)
    stats = _ais_case(k, orc, model, N, T - 3, driver, init_model=init_model)
    assert stats["cost_evals"] > 0
    if name == "meanstd1":
        assert stats["accepted"] == 0
    else:
        assert stats["accepted"] > 0


def test_ais_prepared_cost_in_blocks_of_sub_steps(k, orc, gpu_ctx, monkeypatch):
    """the pre-pass buffer bounded to one KiB: a launch of 8 sub-steps is cut into blocks, each keyed by
    t0 + its first sub-step -- the block that starts beyond 2^32 included"""
    driver = _course(monkeypatch, "existing")
    monkeypatch.setenv("KABC_AUX_KIB", "1")
    model, _ = _stochastic(k, orc, "meanstd300")
    _ais_case(k, orc, model, 130, T - 3, driver)


@pytest.mark.parametrize("course,N", [("small", 100), ("existing", 130)])
@pytest.mark.parametrize("kind", ["threshold", "common"])
def test_ais_other_posterior_kinds(k, orc, gpu_ctx, monkeypatch, kind, course, N):
    driver = _course(monkeypatch, course)
    if kind == "threshold":
        model = k.ApproxPosterior(k.Factored(*[k.Uniform(-5, 5)] * 2), k.costs.Rosenbrock(), 30.0)
    else:
        banana = k.costs.UserCost(BANANA_LPI, dims=[2], name="banana", posteriors=["common"])
        orc.register_user_cost(banana)
        model = k.CommonLogDensity(2, k.Factored(k.Normal(0, 1), k.Normal(0, 1)), banana)
    _ais_case(k, orc, model, N, T - 3, driver)


# ---- AIS: the end of the range --------------------------------------------------------------------------------
@pytest.mark.parametrize("course,N", [("small", 100), ("existing", 130)])
def test_ais_counter_range_is_enforced(k, orc, gpu_ctx, monkeypatch, course, N):
    """kabc_ais_set_state with t >= 2^56, and an advance that would count past 2^56, are KABC_ERR_INVALID_ARG
    with the oracle's message, before anything is launched: the handle stays where it was"""
    _course(monkeypatch, course)
    model = _box(k, 2)
    ens, o = _start(k, orc, model, N, 3, LIMIT - 16)
    x, lp, ll, _ = ens.state()
    for bad in (LIMIT, LIMIT + 5, 2 ** 64 - 1):
        _both_refuse(k, orc, lambda: ens.set_state(x, lp, ll, bad), lambda: o.set_state(x, lp, ll, bad),
                     "must be below 2^56")
    assert ens.state()[3] == LIMIT - 16
    for gens, nt in ((3, NT), (1, 17), (2 ** 62, 2 ** 31 - 1)):
        _both_refuse(k, orc, lambda: ens.advance(gens, nt), lambda: o.generations_sync(gens, nt, collect=False),
                     "would pass 2^56")
    before = ens.stats()
    assert ens.state()[3] == LIMIT - 16 and np.array_equal(ens.state()[0], x) and before == o.stats()
    assert np.array_equal(ens.advance(2, NT, collect=True), o.generations_sync(2, NT))     # the last two fit
    assert ens.state()[3] == LIMIT == o.state()[3]
    with pytest.raises(k.KabcError, match="would pass"):
        ens.advance(1, 1)
    ens.advance(0, NT)                                       # (nothing to count)
    ens.close()
    o.close()


# ---- pfilter across iteration 256 -----------------------------------------------------------------------------
PF_KW = dict(eff_tol=0.0, epstol=-math.inf, max_iters=262)
PF_NREPS = {(100, 1): 1873, (100, 2): 1875, (300, 1): 3479, (300, 2): 3433}     # on the CPU oracle
PF_COURSES = {"one_workgroup_100": (100, 0.95, {}), "small_off_100": (100, 0.95, {"KABC_PF_SMALL": "0"}),
              "default_loop_300": (300, 0.97, {}), "passes_300": (300, 0.97, {"KABC_PF_PASSES": "1"})}
_PF_REF = {}


def _pf_problem(k):
    return k.Factored(k.Uniform(-5, 5), k.Uniform(-5, 5)), k.costs.GaussDist([0.5, -0.3])


def _pf_oracle(k, orc, N, q, seed):
    key = (N, q, seed)
    if key not in _PF_REF:
        pri, cost = _pf_problem(k)
        ref = _PF_REF[key] = orc.pfilter(pri, cost, N, q=q, seed=seed, **PF_KW)
        assert ref["iterations"] == 263, ref["iterations"]          # (the case does not quietly stop early)
        assert ref["nreps"] == PF_NREPS[(N, seed)] and 1e-3 < ref["eps"] < 1e-1
    return _PF_REF[key]


def _pf_equal(got, ref, what):
    assert np.array_equal(got.P.view(np.uint64), ref["P"].view(np.uint64)), what
    assert np.array_equal(got.C.view(np.uint64), ref["C"].view(np.uint64)), what
    for key in ("eps", "eff"):
        assert np.float64(got.info[key]).view(np.uint64) == np.float64(ref[key]).view(np.uint64), (what, key)
    for key in ("iterations", "nreps", "cost_evals"):
        assert got.info[key] == ref[key], (what, key, got.info[key], ref[key])


def _pf_env(monkeypatch, env):
    for name in ("KABC_PF_SMALL", "KABC_PF_PASSES"):
        monkeypatch.delenv(name, raising=False)
    for a, b in env.items():
        monkeypatch.setenv(a, b)


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("case", list(PF_COURSES))
def test_pfilter_across_iteration_256(k, orc, gpu_ctx, monkeypatch, case, seed):
    N, q, env = PF_COURSES[case]
    _pf_env(monkeypatch, env)
    pri, cost = _pf_problem(k)
    ref = _pf_oracle(k, orc, N, q, seed)
    got = k.pfilter(pri, cost, N, q=q, seed=seed, return_array=True, **PF_KW)
    _pf_equal(got, ref, (case, seed))


@pytest.mark.parametrize("split", [255, 256])
@pytest.mark.parametrize("case", list(PF_COURSES))
def test_pfilter_split_at_the_upper_word(k, orc, gpu_ctx, monkeypatch, case, split):
    """the device segments equal the whole run, and the oracle continued from the device's state"""
    N, q, env = PF_COURSES[case]
    _pf_env(monkeypatch, env)
    pri, cost = _pf_problem(k)
    ref = _pf_oracle(k, orc, N, q, 1)
    first = k.pfilter(pri, cost, N, q=q, seed=1, return_array=True, return_state=True, **dict(PF_KW, max_iters=split - 1))
    st = first.info["state"]
    assert st.iteration == split == first.info["iterations"]
    kw = dict(PF_KW, q=q)
    cont = k.pfilter(pri, cost, resume=st, return_array=True, return_state=True, **kw)
    _pf_equal(cont, ref, (case, split, "whole"))
    oc = orc.pfilter(pri, cost, resume=st, return_state=True, **kw)
    _pf_equal(cont, oc, (case, split, "oracle from the state"))
    a, b = cont.info["state"], oc["state"]
    for name in ("theta", "cost", "logprior"):
        assert np.array_equal(getattr(a, name).view(np.uint64), getattr(b, name).view(np.uint64)), name
    assert (a.iteration, a.nreps, a.cost_evals, a.seed) == (b.iteration, b.nreps, b.cost_evals, b.seed) and a.iteration == 263


def test_pfilter_run_time_dimension_across_iteration_256(k, orc, gpu_ctx, monkeypatch):
    """17 Uniform(-5, 5) components, N = 50 raised to 73 (src/smc.jl:276-279); q = 0.95 reaches 263 iterations on
    the oracle (checked here)"""
    _pf_env(monkeypatch, {})
    pri = k.Factored(*[k.Uniform(-5, 5)] * 17)
    cost = k.costs.GaussDist(np.random.default_rng(17).uniform(-1, 1, 17))
    kw = dict(PF_KW, q=0.95)
    ref = orc.pfilter(pri, cost, 50, seed=1, **kw)
    assert ref["iterations"] == 263 and ref["P"].shape == (73, 17)
    got = k.pfilter(pri, cost, 50, seed=1, return_array=True, **kw)
    assert got.info["nparticles"] == 73
    _pf_equal(got, ref, "d17")
    first = k.pfilter(pri, cost, 50, seed=1, return_array=True, return_state=True, **dict(kw, max_iters=254))
    st = first.info["state"]
    assert st.iteration == 255
    _pf_equal(k.pfilter(pri, cost, resume=st, return_array=True, **kw), ref, "d17 split")
    _pf_equal(k.pfilter(pri, cost, resume=st, return_array=True, **kw), orc.pfilter(pri, cost, resume=st, **kw),
              "d17 oracle from the state")


def test_pfilter_iteration_range_is_enforced(k, orc, gpu_ctx):
    pri, cost = _pf_problem(k)
    first = k.pfilter(pri, cost, 100, q=0.95, seed=1, return_state=True, eff_tol=0.0, max_iters=2)
    st = first.info["state"]
    st.iteration = 2 ** 32
    kw = dict(q=0.95, eff_tol=0.0, max_iters=2 ** 32 + 4)
    _both_refuse(k, orc, lambda: k.pfilter(pri, cost, resume=st, **kw), lambda: orc.pfilter(pri, cost, resume=st, **kw),
                 "below 2^32")
    # the last admissible iterations: t = (iteration << 24) | attempt next to 2^56
    st.iteration = 2 ** 32 - 3
    kw = dict(q=0.95, eff_tol=0.0, max_iters=2 ** 32 - 2)
    got = k.pfilter(pri, cost, resume=st, return_array=True, **kw)
    assert got.info["iterations"] == 2 ** 32 - 1
    _pf_equal(got, orc.pfilter(pri, cost, resume=st, **kw), "2^32 - 3")


# ---- smc from a state with a high pass counter ----------------------------------------------------------------
SMC_PASS = {"T-2": T - 2, "ABCDEF*T-2": 0xABCDEF * T - 2, "2^56-64": LIMIT - 64}
_SMC_STATE = {}


def _smc_equal(got, ref, first, what):
    assert got.info["iterations"] == ref["iterations"], what
    assert got.info["log"][first:] == ref["log"], what
    assert np.float64(got.eps).view(np.uint64) == np.float64(ref["eps"]).view(np.uint64), what
    assert np.array_equal(got.info["alive"], ref["alive"]), what
    assert np.array_equal(got.info["theta_all"].view(np.uint64), ref["theta_all"].view(np.uint64)), what
    assert np.array_equal(np.asarray(got.C).view(np.uint64), ref["C"].view(np.uint64)), what
    assert (got.info["cost_evals"], got.info["proposals"]) == (ref["cost_evals"], ref["proposals"]), what


def _smc_from_high_pass(k, orc, prior, cost, N, kw, key, pass_count, total=9, at=3):
    """the state after `at` iterations (computed once per problem and course, and copied), its pass counter set to
    `pass_count`, continued to `total` iterations: the device against the oracle from the same state"""
    if key not in _SMC_STATE:
        out = k.smc(prior, cost, nparticles=N, return_array=True, return_state=True, **dict(kw, max_iterations=at))
        assert out.info["iterations"] == at, out.info["log"]
        _SMC_STATE[key] = out.info["state"]
    s = _SMC_STATE[key]
    st = k.SmcState(s.theta.copy(), s.cost.copy(), s.logprior.copy(), s.alive.copy(), seed=s.seed, iteration=s.iteration,
                    pass_count=pass_count, eps=s.eps, eps_prev=s.eps_prev, accepted=s.accepted,
                    cost_evals=s.cost_evals, proposals=s.proposals, n_alive=s.n_alive, log=s.log)
    rest = {a: b for a, b in kw.items() if a != "seed"}
    got = k.smc(prior, cost, resume=st, return_array=True, return_state=True, **dict(rest, max_iterations=total))
    ref = orc.smc(prior, cost, resume=st, return_state=True, **dict(rest, max_iterations=total))
    _smc_equal(got, ref, at, key)
    a, b = got.info["state"], ref["state"]
    assert a.pass_count == b.pass_count == pass_count + sum(rec["passes"] for rec in ref["log"])
    for name in ("theta", "cost", "logprior"):
        assert np.array_equal(getattr(a, name).view(np.uint64), getattr(b, name).view(np.uint64)), (key, name)
    assert np.array_equal(a.alive, b.alive) and a.log == b.log
    return ref


def _smc_base(k):
    return k.Factored(k.Uniform(-5, 5), k.Uniform(-5, 5)), k.costs.GaussDist([0.5, -0.3])


def _smc_n(monkeypatch, course):
    N = _smc_env(monkeypatch, course)
    return 100 if course == "small" else N


@pytest.mark.parametrize("name", list(SMC_PASS))
@pytest.mark.parametrize("course", FOUR)
def test_smc_from_a_high_pass_counter(k, orc, gpu_ctx, monkeypatch, course, name):
    N = _smc_n(monkeypatch, course)
    prior, cost = _smc_base(k)
    ref = _smc_from_high_pass(k, orc, prior, cost, N, BASE_KW, (course, "base"), SMC_PASS[name])
    assert ref["iterations"] == 9 and len(ref["log"]) == 6


@pytest.mark.parametrize("course", ["small", "loop", "select"])
def test_smc_retry_passes_across_the_upper_word(k, orc, gpu_ctx, monkeypatch, course):
    """mcmc_retrys = 3: the pass counter is not the iteration, and it crosses 2^32 inside one.  From 2^32 - 3 the
    iterations after the state run 1, 2, 2, 3, 1, 2 passes (the oracle's log, asserted): passes 2^32 - 1 and 2^32
    are the two of iteration 5.  (From 2^32 - 2 the crossing would fall between iterations 4 and 5.)  The
    one-workgroup course takes the 200 particles of tests/test_gpu_smc_selection_edges.py: with 100 the run ends
    at iteration 3, where fewer than mcmc_tol N proposals were accepted."""
    N = _smc_env(monkeypatch, course)
    prior, cost = _smc_base(k)
    kw = dict(BASE_KW, mcmc_retrys=3, mcmc_tol=0.45)
    start = T - 3
    ref = _smc_from_high_pass(k, orc, prior, cost, N, kw, (course, "retrys"), start)
    passes = [rec["passes"] for rec in ref["log"]]
    assert ref["iterations"] == 9 and max(passes) > 1, passes
    before = [start + sum(passes[:i]) for i in range(len(passes))]
    assert any(c + 1 <= T - 1 and c + n >= T for c, n in zip(before, passes)), passes


@pytest.mark.parametrize("course", ["small", "loop", "select"])
def test_smc_run_time_dimension_from_a_high_pass_counter(k, orc, gpu_ctx, monkeypatch, course):
    """the 20-parameter problem of tests/test_gpu_smc_resume.py::test_split_beyond_16_parameters (3000 particles,
    with the environment of each course)"""
    _smc_env(monkeypatch, course)
    rng = np.random.default_rng(8)
    prior, cost = k.Factored(*[k.Normal(0, 2)] * 20), k.costs.GaussDist(rng.normal(size=20))
    kw = dict(alpha=0.9, epstol=3.0, seed=4)
    ref = _smc_from_high_pass(k, orc, prior, cost, 3000, kw, (course, "d20"), T - 2)
    assert ref["iterations"] > 3


@pytest.mark.parametrize("course,N", [("small", 100), ("loop", 300), ("select", 300)])
def test_smc_prepared_cost_from_a_high_pass_counter(k, orc, gpu_ctx, monkeypatch, course, N):
    """the README simulator: its prepared passes live in a ring addressed by the pass counter (pass % aux_ring);
    100 particles: the one-workgroup course, 300: beyond it, with the environment of the loop and of the
    kernel-per-phase course"""
    _smc_env(monkeypatch, course)
    prior = k.Factored(k.Uniform(1, 3), k.Truncated(k.Normal(0, 0.1), 0, 100))
    cost = k.costs.NormalMeanStdSim(1000, 2.0, 0.04)
    kw = dict(seed=2, r_epstol=0.0, mcmc_tol=0.0, epstol=-1e308)
    ref = _smc_from_high_pass(k, orc, prior, cost, N, kw, ("readme", course), T - 2, total=24)
    assert ref["iterations"] == 24


def test_smc_pass_range_is_enforced(k, orc, gpu_ctx, monkeypatch):
    N = _smc_n(monkeypatch, "small")
    prior, cost = _smc_base(k)
    out = k.smc(prior, cost, nparticles=N, return_state=True, **dict(BASE_KW, max_iterations=3))
    st = out.info["state"]
    rest = {a: b for a, b in BASE_KW.items() if a != "seed"}
    for pass_count, total, word in ((LIMIT, 9, "must be below 2^56"), (LIMIT - 5, 9, "could pass 2^56"),
                                    (LIMIT - 64, None, "could pass 2^56")):
        st.pass_count = pass_count
        _both_refuse(k, orc, lambda: k.smc(prior, cost, resume=st, max_iterations=total, **rest),
                     lambda: orc.smc(prior, cost, resume=st, max_iterations=total, **rest), word)


# ---- ABCDE from a state with a high generation counter --------------------------------------------------------
ABCDE_COURSES = {"donor_teams_257": {}, "sorted_blocks_1537": {}, "wavelet_4100": {"KABC_ABCDE_RANK": "wavelet"},
                 "scan_donor_off_257": {"KABC_ABCDE_DONOR": "0"},
                 "scan_blocks_from_1537": {"KABC_ABCDE_BLOCKS_FROM": "1000000000", "KABC_ABCDE_DONOR": "0"},
                 "d17_100": {}}
_ABCDE_STATE = {}


@pytest.mark.parametrize("name", ["T-3", "ABCDEF*T-3"])
@pytest.mark.parametrize("case", list(ABCDE_COURSES))
def test_abcde_from_a_high_generation_counter(k, orc, gpu_ctx, monkeypatch, case, name):
    """the courses of tests/test_gpu_abcde_resume.py::test_split_on_every_course: the state after 3 generations,
    its generation set next to 2^32, continued for 8 more -- opts->generations is a 64-bit total"""
    for env in ("KABC_ABCDE_RANK", "KABC_ABCDE_DONOR", "KABC_ABCDE_BLOCKS_FROM"):
        monkeypatch.delenv(env, raising=False)
    for a, b in ABCDE_COURSES[case].items():
        monkeypatch.setenv(a, b)
    pri = k.Factored(k.DiscreteUniform(-10, 10), k.Normal(0, 3))
    cost = k.costs.GaussDist([3.0, -2.0])
    eps, N = 0.5, int(case.rsplit("_", 1)[1])
    if case == "d17_100":
        comps = [k.Normal(0, 2), k.Uniform(-3, 3), k.Gamma(2.5, 0.7), k.DiscreteUniform(-4, 4)]
        pri = k.Factored(*[comps[j % 4] for j in range(17)])
        cost = k.costs.GaussDist(np.linspace(-0.5, 1.5, 17))
        eps = 3.0
    if case not in _ABCDE_STATE:
        out = k.ABCDE(pri, cost, eps, seed=11, nparticles=N, generations=3, proposal_width=0.9, return_state=True)
        assert out.info["state"].generation == 3
        _ABCDE_STATE[case] = out.info["state"]
    s = _ABCDE_STATE[case]
    g0 = {"T-3": T - 3, "ABCDEF*T-3": 0xABCDEF * T - 3}[name]
    st = k.AbcdeState(s.theta.copy(), s.cost.copy(), s.logprior.copy(), seed=s.seed, generation=g0, nsims=s.nsims)
    kw = dict(generations=g0 + 8, proposal_width=0.9)
    got = k.ABCDE(pri, cost, eps, resume=st, return_array=True, return_state=True, **kw)
    ref = orc.abcde(pri, cost, eps, resume=st, return_state=True, **kw)
    assert np.array_equal(got.P.view(np.uint64), ref["P"].view(np.uint64))
    assert np.array_equal(got.C.view(np.uint64), ref["C"].view(np.uint64))
    assert got.reached_eps == ref["reached_eps"]
    assert got.info["generations_run"] == ref["generations_run"] == g0 + 8
    assert got.info["nsims"] == ref["nsims"] > s.nsims
    a, b = got.info["state"], ref["state"]
    assert a.generation == b.generation == g0 + 8
    for field in ("theta", "cost", "logprior"):
        assert np.array_equal(getattr(a, field).view(np.uint64), getattr(b, field).view(np.uint64)), field


def test_abcde_generation_range_is_enforced(k, orc, gpu_ctx):
    pri, cost = k.Factored(k.Normal(0, 5), k.Normal(0, 5)), k.costs.GaussDist([1.0, -0.5])
    out = k.ABCDE(pri, cost, 0.05, seed=9, nparticles=100, generations=2, return_state=True)
    st = out.info["state"]
    for generation, total, word in ((LIMIT, LIMIT + 8, "must be below 2^56"), (LIMIT - 3, LIMIT + 1, "at most 2^56")):
        st.generation = generation
        _both_refuse(k, orc, lambda: k.ABCDE(pri, cost, 0.05, resume=st, generations=total),
                     lambda: orc.abcde(pri, cost, 0.05, resume=st, generations=total), word)
    # the last three admissible generations
    st.generation = LIMIT - 3
    got = k.ABCDE(pri, cost, 0.05, resume=st, generations=LIMIT, return_array=True)
    ref = orc.abcde(pri, cost, 0.05, resume=st, generations=LIMIT)
    assert np.array_equal(got.P, ref["P"]) and np.array_equal(got.C, ref["C"])
    assert got.info["generations_run"] == ref["generations_run"] == LIMIT and got.info["nsims"] == ref["nsims"]
