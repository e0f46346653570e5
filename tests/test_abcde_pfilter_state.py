"""CPU: the states of a stopped ABCDE or pfilter run (kabc_abcde_state_t / kabc_pfilter_state_t, kabc_*_run_from;
AbcdeState / PfilterState, ABCDE(...) and pfilter(...) with resume= and return_state=): the declarations, the
ctypes mirrors and the library agree, save / load keep every bit, and the arguments the Python layer or the
library refuses are refused before anything is launched -- none of it needs a device."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVERS = ("abcde", "pfilter")


def _header():
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "kabc.h")).read(), flags=re.S)


def _types(cd, drv):
    return {"abcde": (cd.AbcdeOpts, cd.AbcdeState, cd.AbcdeResult),
            "pfilter": (cd.PfilterOpts, cd.PfilterState, cd.PfilterResult)}[drv]


@pytest.mark.parametrize("drv", DRIVERS)
def test_prototypes_in_sync(k, drv):
    from kissabc_jl_amd import _cdefs as cd, _lib
    hdr = _header()
    lib = _lib.load()
    opts, state, result = _types(cd, drv)
    for sym in (f"kabc_{drv}_state_sizeof", f"kabc_{drv}_run_from"):
        assert re.search(r"\b%s\s*\(" % sym, hdr), f"{sym} is not declared in include/kabc.h"
        assert hasattr(lib, sym), f"{sym} is not exported"
        assert sym in cd.PROTOTYPES
    assert cd.PROTOTYPES[f"kabc_{drv}_state_sizeof"] == (C.c_int64, [])
    res, args = cd.PROTOTYPES[f"kabc_{drv}_run_from"]
    assert res is C.c_int
    assert args == [C.c_void_p, C.POINTER(cd.Prior), C.c_int32, C.POINTER(cd.Cost), C.POINTER(opts),
                    C.POINTER(state), C.POINTER(state), C.POINTER(result)]
    m = re.search(r"kabc_%s_run_from\s*\(([^;]*?)\)\s*;" % drv, hdr, flags=re.S)
    want = ["kabc_ctx_t*", "const kabc_prior_t*", "int32_t", "const kabc_cost_t*", f"const kabc_{drv}_opts_t*",
            f"const kabc_{drv}_state_t*", f"kabc_{drv}_state_t*", f"kabc_{drv}_result_t*"]
    got = [re.sub(r"\s*\w+$", "", re.sub(r"\s+", " ", a.strip())) for a in m.group(1).split(",")]
    assert got == want
    # the existing table is untouched: the new structs are checked through their own functions
    assert lib.kabc_version() == cd.KABC_VERSION
    assert lib.kabc_abi_sizeof(11) == -1


@pytest.mark.parametrize("drv,size", [("abcde", 64), ("pfilter", 88)])
def test_mirror_matches_the_declaration_and_the_library(k, drv, size):
    from kissabc_jl_amd import _cdefs as cd, _lib
    lib = _lib.load()
    state = _types(cd, drv)[1]
    assert C.sizeof(state) == getattr(lib, f"kabc_{drv}_state_sizeof")() == size
    body = re.search(r"typedef struct kabc_%s_state \{(.*?)\} kabc_%s_state_t;" % (drv, drv), _header(),
                     flags=re.S).group(1)
    ctype = {"int64_t": C.c_int64, "int32_t": C.c_int32, "uint64_t": C.c_uint64, "double": C.c_double,
             "double*": cd.c_double_p}
    decl = []
    for line in body.split(";"):
        line = re.sub(r"\s+", " ", line.strip())
        if not line:
            continue
        ty, names = re.match(r"(\w+)\s*(.+)$", line).groups()    # ("double", "eps, eff") / ("double", "* theta")
        for name in names.split(","):
            name = name.strip()
            decl.append((name.lstrip("* "), ctype[ty + ("*" if name.startswith("*") else "")]))
    assert list(state._fields_) == decl


def _arrays(N=7, D=3):
    rng = np.random.default_rng(3)
    theta = rng.normal(size=(N, D))
    theta[0, 0], theta[1, 1] = -0.0, 2.5            # (a signed zero, a particle between integers)
    cost = rng.normal(size=N)
    cost[:3] = [-0.0, 0.0, 5e-324]
    lp = rng.normal(size=N)
    lp[2] = -1e300
    return theta, cost, lp


def _state(k, drv, N=7, D=3):
    theta, cost, lp = _arrays(N, D)
    if drv == "abcde":
        return k.AbcdeState(theta, cost, lp, seed=2**64 - 1, generation=2**40 + 5, nsims=2**63 + 9)
    return k.PfilterState(theta, cost, lp, seed=2**64 - 1, iteration=2**40 + 5, eps=-0.0, eff=math.nan,
                          nreps=2**63 + 9, cost_evals=2**33)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _assert_same_state(a, b):
    assert type(a) is type(b)
    for name in ("theta", "cost", "logprior"):
        assert getattr(a, name).shape == getattr(b, name).shape
        assert np.array_equal(_bits(getattr(a, name)), _bits(getattr(b, name))), name
    for name in ("nparticles", "D") + type(a)._INTS:
        assert getattr(a, name) == getattr(b, name) and type(getattr(b, name)) is int, name
    for name in type(a)._FLOATS:
        assert _bits(getattr(a, name)) == _bits(getattr(b, name)) and type(getattr(b, name)) is float, name


@pytest.mark.parametrize("drv", DRIVERS)
def test_save_load_round_trip(k, tmp_path, drv):
    st = _state(k, drv)
    cls = type(st)
    path = str(tmp_path / "state.npz")
    st.save(path)
    assert os.path.exists(path)
    with np.load(path, allow_pickle=False) as z:    # arrays and scalars only: loads with pickle refused
        assert all(z[name].dtype != object for name in z.files)
    back = cls.load(path)
    _assert_same_state(st, back)
    # and again: a loaded state saves to the same values
    back.save(str(tmp_path / "again.npz"))
    _assert_same_state(st, cls.load(str(tmp_path / "again.npz")))


@pytest.mark.parametrize("drv", DRIVERS)
def test_state_to_c_carries_every_field(k, drv):
    st = _state(k, drv)
    c = st._to_c()
    assert (c.nparticles, c.D, c.reserved, c.seed) == (7, 3, 0, 2**64 - 1)
    if drv == "abcde":
        assert (c.generation, c.nsims) == (2**40 + 5, 2**63 + 9)
    else:
        assert (c.iteration, c.nreps, c.cost_evals) == (2**40 + 5, 2**63 + 9, 2**33)
        assert _bits(c.eps) == _bits(-0.0) and math.isnan(c.eff)
    assert c.theta[4] == st.theta[1, 1] and _bits(c.cost[0]) == _bits(-0.0) and c.logprior[2] == -1e300
    assert {name for name, _ in type(c)._fields_} == \
        {"nparticles", "D", "reserved", "theta", "cost", "logprior"} | set(type(st)._INTS) | set(type(st)._FLOATS)


@pytest.fixture
def no_library(k, monkeypatch):
    """any attempt to load the library or to make a context fails the test"""
    def boom(*a, **kw):
        raise AssertionError("a library call was made")
    monkeypatch.setattr(k._lib, "load", boom)
    monkeypatch.setattr(k._lib, "default_context", boom)


def test_python_side_refusals_need_no_device(k, no_library):
    prior3 = k.Factored(*[k.Uniform(-5, 5)] * 3)
    prior2 = k.Factored(*[k.Uniform(-5, 5)] * 2)
    cost = k.costs.GaussDist([0.5, -0.3, 0.1])
    a, p = _state(k, "abcde"), _state(k, "pfilter")      # 7 particles, 3 parameters
    with pytest.raises(ValueError, match="nparticles"):
        k.ABCDE(prior3, cost, 0.1, resume=a, nparticles=8)
    with pytest.raises(ValueError, match="N = 8"):
        k.pfilter(prior3, cost, 8, resume=p)
    with pytest.raises(ValueError, match="prior"):
        k.ABCDE(prior2, k.costs.GaussDist([0.5, -0.3]), 0.1, resume=a)
    with pytest.raises(ValueError, match="prior"):
        k.pfilter(prior2, k.costs.GaussDist([0.5, -0.3]), resume=p)
    # each driver takes its own state, not the other's, not a dict
    with pytest.raises(TypeError, match="AbcdeState"):
        k.ABCDE(prior3, cost, 0.1, resume=p)
    with pytest.raises(TypeError, match="PfilterState"):
        k.pfilter(prior3, cost, resume=a)
    with pytest.raises(TypeError, match="AbcdeState"):
        k.ABCDE(prior3, cost, 0.1, resume={"theta": a.theta})
    with pytest.raises(TypeError, match="N is required"):
        k.pfilter(prior3, cost)
    with pytest.raises(ValueError, match="entries"):
        k.AbcdeState(a.theta, a.cost[:-1], a.logprior, seed=0, generation=0, nsims=0)
    with pytest.raises(ValueError, match="entries"):
        k.PfilterState(p.theta, p.cost, p.logprior[:-1], seed=0, iteration=0, eps=math.inf, eff=math.nan, nreps=0,
                       cost_evals=0)
    with pytest.raises(TypeError, match="scalars"):
        k.AbcdeState(a.theta, a.cost, a.logprior, seed=0, generation=0)


@pytest.mark.parametrize("drv", DRIVERS)
def test_library_refuses_bad_states_before_it_launches(k, drv):
    """kabc_*_run_from validates the states before it touches the context: KABC_ERR_INVALID_ARG with a message,
    on a machine without a device too (the context argument is never used)"""
    from kissabc_jl_amd import _cdefs as cd, _lib
    lib = _lib.load()
    D, N = 2, 50
    prior = k.Factored(*[k.Uniform(-5, 5)] * D)
    cc = k.costs.GaussDist([0.5, -0.3]).to_c()
    opts, state, result = _types(cd, drv)
    o = opts()
    getattr(lib, f"kabc_{drv}_default_opts")(C.byref(o))
    o.nparticles = N
    counter = "generation" if drv == "abcde" else "iteration"
    fake_ctx = C.c_void_p(8)

    def call(st, to=None):
        r = result()
        status = getattr(lib, f"kabc_{drv}_run_from")(fake_ctx, prior.to_c(), D, C.byref(cc), C.byref(o), C.byref(st),
                                                      C.byref(to) if to is not None else None, C.byref(r))
        return status, lib.kabc_last_error().decode()

    def good(n=N):
        rng = np.random.default_rng(0)
        arrays = rng.normal(size=(n, D)), rng.normal(size=n), rng.normal(size=n)
        if drv == "abcde":
            s = k.AbcdeState(*arrays, seed=1, generation=2, nsims=100)
        else:
            s = k.PfilterState(*arrays, seed=1, iteration=2, eps=1.0, eff=0.5, nreps=100, cost_evals=90)
        return s, s._to_c()

    for name in ("theta", "cost", "logprior"):
        s, c = good()
        setattr(c, name, None)
        assert call(c) == (cd.KABC_ERR_INVALID_ARG, f"kabc_{drv}_run_from: an array of `from` is NULL")
    s, c = good()
    c.nparticles = N + 1
    status, msg = call(c)
    assert status == cd.KABC_ERR_INVALID_ARG and "nparticles" in msg
    s, c = good()
    c.D = D + 1
    status, msg = call(c)
    assert status == cd.KABC_ERR_INVALID_ARG and "D differs" in msg
    s, c = good()
    setattr(c, counter, -1)
    status, msg = call(c)
    assert status == cd.KABC_ERR_INVALID_ARG and counter in msg
    for name, i, v in (("cost", 3, math.nan), ("cost", N - 1, math.inf), ("logprior", 0, -math.inf),
                       ("logprior", 7, math.nan)):
        s, c = good()
        getattr(s, name)[i] = v
        status, msg = call(c)
        assert status == cd.KABC_ERR_INVALID_ARG and "not finite" in msg, (name, i, v)
    s, c = good()
    s2, to = good()
    to.cost = None
    setattr(to, counter, 7)
    status, msg = call(c, to)
    assert status == cd.KABC_ERR_INVALID_ARG and "`to`" in msg
    assert getattr(to, counter) == -1                # a call that fails leaves no state
    # `to` is a state of its own: the struct `from` points to, or one of its arrays, is refused -- and the
    # caller's state is left as it was
    s, c = good()
    status, msg = call(c, c)
    assert status == cd.KABC_ERR_INVALID_ARG and "shares" in msg
    assert getattr(c, counter) == 2
    for name in ("theta", "cost", "logprior"):
        s2, to = good()
        setattr(to, name, getattr(c, name))
        status, msg = call(c, to)
        assert status == cd.KABC_ERR_INVALID_ARG and "shares" in msg and getattr(c, counter) == 2


def test_pfilter_state_is_checked_against_the_effective_n(k):
    """opts->nparticles = 5 at D = 2, q = 0.7 is raised to 13 (src/smc.jl:276-279): a state of 13 particles passes
    the check of the particle count (and is then refused for another reason), one of 5 does not"""
    from kissabc_jl_amd import _cdefs as cd, _lib
    lib = _lib.load()
    D = 2
    assert lib.kabc_pfilter_nparticles(5, 0.7, D) == 13
    prior = k.Factored(*[k.Uniform(-5, 5)] * D)
    cc = k.costs.GaussDist([0.5, -0.3]).to_c()
    o = cd.PfilterOpts()
    lib.kabc_pfilter_default_opts(C.byref(o))
    o.nparticles = 5

    def call(n):
        rng = np.random.default_rng(0)
        s = k.PfilterState(rng.normal(size=(n, D)), rng.normal(size=n), rng.normal(size=n), seed=1, iteration=-1,
                           eps=1.0, eff=0.5, nreps=0, cost_evals=0)
        c = s._to_c()
        r = cd.PfilterResult()
        status = lib.kabc_pfilter_run_from(C.c_void_p(8), prior.to_c(), D, C.byref(cc), C.byref(o), C.byref(c), None,
                                           C.byref(r))
        return status, lib.kabc_last_error().decode()

    status, msg = call(5)
    assert status == cd.KABC_ERR_INVALID_ARG and "effective N" in msg
    status, msg = call(13)
    assert status == cd.KABC_ERR_INVALID_ARG and "iteration is negative" in msg


@pytest.mark.parametrize("drv", DRIVERS)
def test_library_and_oracle_refuse_a_counter_beyond_the_streams(k, orc, drv):
    """the stream address holds 56 bits of the counter (include/kabc_philox.h): ABCDE's generation counter must
    stay below 2^56 (and opts->generations, the total, at or below it); pfilter's counter is
    (iteration << 24) | attempt, so its iteration must stay below 2^32.  KABC_ERR_INVALID_ARG before anything is
    launched, in the library and, with the same message, in the oracle"""
    from kissabc_jl_amd import _cdefs as cd, _lib
    lib = _lib.load()
    D, N = 2, 50
    prior = k.Factored(*[k.Uniform(-5, 5)] * D)
    cost = k.costs.GaussDist([0.5, -0.3])
    cc = cost.to_c()
    opts, _, result = _types(cd, drv)

    def state(counter):
        rng = np.random.default_rng(0)
        arrays = rng.normal(size=(N, D)), rng.normal(size=N), rng.normal(size=N)
        if drv == "abcde":
            return k.AbcdeState(*arrays, seed=1, generation=counter, nsims=100)
        return k.PfilterState(*arrays, seed=1, iteration=counter, eps=1.0, eff=0.5, nreps=100, cost_evals=90)

    def library(st, total):
        o = opts()
        getattr(lib, f"kabc_{drv}_default_opts")(C.byref(o))
        o.nparticles = N
        if drv == "abcde":
            o.generations = total
        else:
            o.max_iters, o.eff_tol = total, 0.0
        c, r = st._to_c(), result()
        # (the context is never used: every call here is refused)
        status = getattr(lib, f"kabc_{drv}_run_from")(C.c_void_p(8), prior.to_c(), D, C.byref(cc), C.byref(o),
                                                      C.byref(c), None, C.byref(r))
        return status, lib.kabc_last_error().decode()

    def oracle(st, total):
        try:
            if drv == "abcde":
                orc.abcde(prior, cost, 0.01, resume=st, generations=total)
            else:
                orc.pfilter(prior, cost, resume=st, max_iters=total, eff_tol=0.0)
        except orc.OracleError as e:
            return e.status, str(e)
        return 0, ""

    limit, word = (2 ** 56, "generation must be below 2^56") if drv == "abcde" else (2 ** 32, "iteration must be below 2^32")
    for c in (limit, limit + 5, 2 ** 62):
        status, msg = library(state(c), c + 8)
        assert status == cd.KABC_ERR_INVALID_ARG and word in msg, c
        assert oracle(state(c), c + 8) == (status, msg)
    if drv == "abcde":      # the total a call may be asked for
        status, msg = library(state(limit - 3), limit + 1)
        assert status == cd.KABC_ERR_INVALID_ARG and "generations must be at most 2^56" in msg
        assert oracle(state(limit - 3), limit + 1) == (status, msg)
    # the last admissible counters are not refused (the oracle; the library from such states:
    # tests/test_gpu_stream_counter.py)
    if drv == "abcde":
        out = orc.abcde(prior, cost, 0.01, resume=state(limit - 3), generations=limit, return_state=True)
        assert out["generations_run"] == limit and out["state"].generation == limit
    else:
        out = orc.pfilter(prior, cost, resume=state(limit - 3), max_iters=limit - 3, eff_tol=0.0, return_state=True)
        assert out["iterations"] == limit - 2 == out["state"].iteration
