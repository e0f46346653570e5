"""CPU: the state of a stopped smc run (kabc_smc_state_t, kabc_smc_run_from; SmcState, smc(resume=, return_state=)):
the declaration, the ctypes mirror and the library agree, SmcState.save / load keep every bit, and the
arguments the Python layer refuses are refused before any library call -- none of it needs a device."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "kabc.h")).read(), flags=re.S)


def test_prototypes_in_sync(k):
    from kissabc_jl_amd import _cdefs as cd, _lib
    hdr = _header()
    lib = _lib.load()
    for sym in ("kabc_smc_state_sizeof", "kabc_smc_run_from"):
        assert re.search(r"\b%s\s*\(" % sym, hdr), f"{sym} is not declared in include/kabc.h"
        assert hasattr(lib, sym), f"{sym} is not exported"
        assert sym in cd.PROTOTYPES
    assert cd.PROTOTYPES["kabc_smc_state_sizeof"] == (C.c_int64, [])
    res, args = cd.PROTOTYPES["kabc_smc_run_from"]
    assert res is C.c_int
    assert args == [C.c_void_p, C.POINTER(cd.Prior), C.c_int32, C.POINTER(cd.Cost), C.POINTER(cd.SmcOpts),
                    C.POINTER(cd.SmcState), C.POINTER(cd.SmcState), C.POINTER(cd.SmcResult)]
    m = re.search(r"kabc_smc_run_from\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
    want = ["kabc_ctx_t*", "const kabc_prior_t*", "int32_t", "const kabc_cost_t*", "const kabc_smc_opts_t*",
            "const kabc_smc_state_t*", "kabc_smc_state_t*", "kabc_smc_result_t*"]
    got = [re.sub(r"\s*\w+$", "", re.sub(r"\s+", " ", a.strip())) for a in m.group(1).split(",")]
    assert got == want
    # the existing table is untouched: the new struct is checked through its own function
    assert lib.kabc_version() == cd.KABC_VERSION == 321
    assert lib.kabc_abi_sizeof(11) == -1


def test_mirror_matches_the_declaration_and_the_library(k):
    from kissabc_jl_amd import _cdefs as cd, _lib
    lib = _lib.load()
    assert C.sizeof(cd.SmcState) == lib.kabc_smc_state_sizeof() == 120
    body = re.search(r"typedef struct kabc_smc_state \{(.*?)\} kabc_smc_state_t;", _header(), flags=re.S).group(1)
    ctype = {"int64_t": C.c_int64, "int32_t": C.c_int32, "uint64_t": C.c_uint64, "double": C.c_double,
             "double*": cd.c_double_p, "uint8_t*": C.POINTER(C.c_uint8)}
    decl = []
    for line in body.split(";"):
        line = re.sub(r"\s+", " ", line.strip())
        if line:
            ty, name = re.match(r"(.+?)\s*(\w+)$", line).groups()
            decl.append((name, ctype[ty.replace(" ", "")]))
    mirror = [("pass" if n == "pass_" else n, t) for n, t in cd.SmcState._fields_]
    assert mirror == decl


def _state(k, N=7, D=3, log=None):
    rng = np.random.default_rng(3)
    theta = rng.normal(size=(N, D))
    theta[0, 0], theta[1, 1] = -0.0, 2.5            # (a walker between integers, a signed zero)
    cost = rng.normal(size=N)
    cost[:5] = [math.nan, -0.0, 0.0, math.inf, -math.inf]
    cost[5] = np.uint64(0x7ff8dead0000beef).view(np.float64)  # (a NaN with a payload)
    lp = rng.normal(size=N)
    lp[2] = -math.inf
    alive = (np.arange(N) % 2).astype(np.uint8)
    if log is None:
        log = [dict(eps=math.inf, ess=N, accepted=3, resampled=0, flag=0, passes=1),
               dict(eps=-0.0, ess=4, accepted=0, resampled=1, flag=1, passes=3)]
    return k.SmcState(theta, cost, lp, alive, seed=2**64 - 1, iteration=len(log), pass_count=2**40 + 5, eps=-0.0,
                      eps_prev=math.inf, accepted=2, cost_evals=2**33, proposals=2**34 + 1, n_alive=int(alive.sum()),
                      log=log)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _assert_same_state(a, b):
    for name in ("theta", "cost", "logprior"):
        assert getattr(a, name).shape == getattr(b, name).shape
        assert np.array_equal(_bits(getattr(a, name)), _bits(getattr(b, name))), name
    assert a.alive.dtype == b.alive.dtype == np.uint8 and np.array_equal(a.alive, b.alive)
    for name in ("nparticles", "D", "seed", "iteration", "pass_count", "accepted", "cost_evals", "proposals", "n_alive"):
        assert getattr(a, name) == getattr(b, name) and type(getattr(b, name)) is int, name
    for name in ("eps", "eps_prev"):
        assert _bits(getattr(a, name)) == _bits(getattr(b, name)), name
    assert len(a.log) == len(b.log)
    for ra, rb in zip(a.log, b.log):
        assert list(ra) == list(rb)
        for key in ra:
            assert type(ra[key]) is type(rb[key]), key
            assert _bits(ra[key]) == _bits(rb[key]) if key == "eps" else ra[key] == rb[key], key


@pytest.mark.parametrize("empty_log", [False, True])
def test_save_load_round_trip(k, tmp_path, empty_log):
    st = _state(k, log=[] if empty_log else None)
    path = str(tmp_path / "state.npz")
    st.save(path)
    assert os.path.exists(path)
    with np.load(path, allow_pickle=False) as z:    # arrays and scalars only: loads with pickle refused
        assert all(z[name].dtype != object for name in z.files)
    back = k.SmcState.load(path)
    _assert_same_state(st, back)
    assert back.log == [] if empty_log else len(back.log) == 2
    # and again: a loaded state saves to the same values
    back.save(str(tmp_path / "again.npz"))
    _assert_same_state(st, k.SmcState.load(str(tmp_path / "again.npz")))


def test_state_to_c_carries_every_field(k):
    st = _state(k)
    c = st._to_c()
    assert (c.nparticles, c.D, c.seed, c.iteration, c.pass_) == (7, 3, 2**64 - 1, 2, 2**40 + 5)
    assert (c.accepted, c.cost_evals, c.proposals, c.n_alive) == (2, 2**33, 2**34 + 1, 3)
    assert _bits(c.eps) == _bits(-0.0) and c.eps_prev == math.inf
    assert c.theta[4] == st.theta[1, 1] and c.alive[1] == 1 and c.logprior[2] == -math.inf


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name})")


@pytest.fixture
def no_library(k, monkeypatch):
    """any attempt to load the library or to make a context fails the test"""
    def boom(*a, **kw):
        raise AssertionError("a library call was made")
    monkeypatch.setattr(k._lib, "load", boom)
    monkeypatch.setattr(k._lib, "default_context", boom)


def test_python_side_refusals_need_no_device(k, no_library):
    st = _state(k)                                   # 7 particles, 3 parameters
    prior3 = k.Factored(*[k.Uniform(-5, 5)] * 3)
    prior2 = k.Factored(*[k.Uniform(-5, 5)] * 2)
    cost = k.costs.GaussDist([0.5, -0.3, 0.1])
    with pytest.raises(ValueError, match="nparticles"):
        k.smc(prior3, cost, resume=st, nparticles=8)
    with pytest.raises(ValueError, match="prior"):
        k.smc(prior2, k.costs.GaussDist([0.5, -0.3]), resume=st)
    comm = object()                                  # (never touched: the refusal comes first)
    with pytest.raises(ValueError, match="comm"):
        k.smc(prior3, cost, resume=st, comm=comm)
    with pytest.raises(ValueError, match="comm"):
        k.smc(prior3, cost, return_state=True, comm=comm)
    with pytest.raises(TypeError, match="SmcState"):
        k.smc(prior3, cost, resume={"theta": st.theta})
    with pytest.raises(ValueError, match="entries"):
        k.SmcState(st.theta, st.cost[:-1], st.logprior, st.alive, seed=0, iteration=0, pass_count=0, eps=math.inf,
                   eps_prev=math.inf, accepted=0, cost_evals=0, proposals=0, n_alive=0)


def test_library_refuses_bad_states_before_it_launches(k):
    """kabc_smc_run_from validates the states before it touches the context: KABC_ERR_INVALID_ARG with a
    message, on a machine without a device too (the context argument is never used)"""
    from kissabc_jl_amd import _cdefs as cd, _lib
    lib = _lib.load()
    D, N = 2, 50
    prior = k.Factored(*[k.Uniform(-5, 5)] * D)
    cc = k.costs.GaussDist([0.5, -0.3]).to_c()
    o = cd.SmcOpts()
    lib.kabc_smc_default_opts(C.byref(o))
    o.nparticles = N
    fake_ctx = C.c_void_p(8)

    def call(st, to=None):
        r = cd.SmcResult()
        status = lib.kabc_smc_run_from(fake_ctx, prior.to_c(), D, C.byref(cc), C.byref(o), C.byref(st),
                                       C.byref(to) if to is not None else None, C.byref(r))
        return status, lib.kabc_last_error().decode()

    def good():
        rng = np.random.default_rng(0)
        s = k.SmcState(rng.normal(size=(N, D)), rng.normal(size=N), rng.normal(size=N), np.ones(N, np.uint8), seed=1,
                       iteration=2, pass_count=2, eps=1.0, eps_prev=2.0, accepted=5, cost_evals=100, proposals=100,
                       n_alive=N)
        return s, s._to_c()

    s, c = good()
    c.logprior = None
    assert call(c) == (cd.KABC_ERR_INVALID_ARG, "kabc_smc_run_from: an array of `from` is NULL")
    s, c = good()
    c.nparticles = N + 1
    status, msg = call(c)
    assert status == cd.KABC_ERR_INVALID_ARG and "nparticles" in msg
    s, c = good()
    c.D = D + 1
    status, msg = call(c)
    assert status == cd.KABC_ERR_INVALID_ARG and "D differs" in msg
    s, c = good()
    c.iteration = -1
    status, msg = call(c)
    assert status == cd.KABC_ERR_INVALID_ARG and "iteration" in msg
    s, c = good()
    s.alive[3] = 0                                   # (n_alive still says N)
    status, msg = call(c)
    assert status == cd.KABC_ERR_INVALID_ARG and "n_alive" in msg
    s, c = good()
    s2, to = good()
    to.cost = None
    to.iteration = 7
    status, msg = call(c, to)
    assert status == cd.KABC_ERR_INVALID_ARG and "`to`" in msg
    assert to.iteration == -1                        # a call that fails leaves no state
    # `to` is a state of its own: the struct `from` points to, or one of its arrays, is refused -- and the
    # caller's state is left as it was
    s, c = good()
    status, msg = call(c, c)
    assert status == cd.KABC_ERR_INVALID_ARG and "shares" in msg
    assert c.iteration == 2
    s2, to = good()
    to.alive = c.alive
    status, msg = call(c, to)
    assert status == cd.KABC_ERR_INVALID_ARG and "shares" in msg and c.iteration == 2


def test_library_and_oracle_refuse_a_pass_counter_beyond_the_streams(k, orc):
    """the stream address holds 56 bits of the pass counter (include/kabc_philox.h): a state at or beyond 2^56,
    or one from which max_iterations x (1 + mcmc_retrys) passes could count past it, is KABC_ERR_INVALID_ARG
    before anything is launched -- in the library and, with the same message, in the oracle"""
    from kissabc_jl_amd import _cdefs as cd, _lib
    lib = _lib.load()
    D, N = 2, 50
    prior = k.Factored(*[k.Uniform(-5, 5)] * D)
    cost = k.costs.GaussDist([0.5, -0.3])
    cc = cost.to_c()

    def state(pass_count, iteration=3):
        rng = np.random.default_rng(0)
        return k.SmcState(rng.normal(size=(N, D)), rng.normal(size=N), rng.normal(size=N), np.ones(N, np.uint8), seed=1,
                          iteration=iteration, pass_count=pass_count, eps=1.0, eps_prev=2.0, accepted=5,
                          cost_evals=100, proposals=100, n_alive=N)

    def library(st, max_iterations, mcmc_retrys=0):
        o = cd.SmcOpts()
        lib.kabc_smc_default_opts(C.byref(o))
        o.nparticles, o.max_iterations, o.mcmc_retrys = N, max_iterations, mcmc_retrys
        c, r = st._to_c(), cd.SmcResult()
        status = lib.kabc_smc_run_from(C.c_void_p(8), prior.to_c(), D, C.byref(cc), C.byref(o), C.byref(c), None,
                                       C.byref(r))      # (the context is never used: every call here is refused)
        return status, lib.kabc_last_error().decode()

    def oracle(st, max_iterations, mcmc_retrys=0):
        try:
            orc.smc(prior, cost, resume=st, max_iterations=max_iterations, mcmc_retrys=mcmc_retrys)
        except orc.OracleError as e:
            return e.status, str(e)
        return 0, ""

    for p in (2 ** 56, 2 ** 56 + 5, 2 ** 63, 2 ** 64 - 1):
        status, msg = library(state(p), 9)
        assert status == cd.KABC_ERR_INVALID_ARG and "pass counter must be below 2^56" in msg, p
        assert oracle(state(p), 9) == (status, msg)
    # a call that could run past the limit: 6 iterations left, of one pass each, from 2^56 - 5
    status, msg = library(state(2 ** 56 - 5), 9)
    assert status == cd.KABC_ERR_INVALID_ARG and "could pass 2^56" in msg
    assert oracle(state(2 ** 56 - 5), 9) == (status, msg)
    # ... and of up to four passes each from 2^56 - 23; from 2^56 - 24 they fit
    status, msg = library(state(2 ** 56 - 23), 9, mcmc_retrys=3)
    assert status == cd.KABC_ERR_INVALID_ARG and "could pass 2^56" in msg
    assert oracle(state(2 ** 56 - 23), 9, mcmc_retrys=3) == (status, msg)
    # the default max_iterations (100 000) from the last admissible counters
    status, msg = library(state(2 ** 56 - 64), 0)
    assert status == cd.KABC_ERR_INVALID_ARG and "could pass 2^56" in msg
    # what fits is not refused (the oracle; the library from such states: tests/test_gpu_stream_counter.py)
    out = orc.smc(prior, cost, resume=state(2 ** 56 - 6), max_iterations=9, r_epstol=0.0, mcmc_tol=0.0, epstol=-1e308,
                  return_state=True)
    assert out["iterations"] == 9 and out["state"].pass_count == 2 ** 56
