"""CPU: abc_reject_batch / kabc_abc_reject_batch -- Python's refusals (made before the library is touched), the C
entry point's own (made with ctx = NULL, as tests/test_abc_reject_args.py makes them for the single call), the
agreement of header, ctypes table and Julia shim, and the selection logic of a batch restated on the CPU oracle
(tests/abc_reject_batch_oracle.py): the expectation the GPU tests compare against does not come from the GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from abc_reject_batch_oracle import batch_tables, expected_batch, same_bits
from abc_reject_oracle import oracle_reject

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- Python refusals ---------------------------------------------------------------------------
def test_python_refusals(k, monkeypatch):
    from kissabc_jl_amd import _lib

    def no_library(*a, **kw):
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(_lib, "default_context", no_library)
    prior = k.Factored(k.Normal(0, 1), k.Normal(0, 1))
    g = [k.costs.GaussDist([0.0, 1.0]), k.costs.GaussDist([0.5, 1.0]), k.costs.GaussDist([1.0, 1.0])]
    f = k.abc_reject_batch
    with pytest.raises(TypeError, match="DeviceCost or a sequence of DeviceCosts"):
        f(prior, [g[0], lambda x: 0.0], 0.1, 10)
    with pytest.raises(ValueError, match="nruns or seeds is required"):
        f(prior, g[0], 0.1, 10)
    with pytest.raises(ValueError, match="3 costs for nruns = 2"):
        f(prior, g, 0.1, 10, nruns=2)
    with pytest.raises(ValueError, match="outside 1..65535"):
        f(prior, [], 0.1, 10)
    with pytest.raises(ValueError, match="outside 1..65535"):
        f(prior, g[0], 0.1, 10, nruns=65536)
    with pytest.raises(ValueError, match="outside 1..65535"):
        f(prior, g[0], 0.1, 10, nruns=0)
    with pytest.raises(ValueError, match="cost 1 differs from cost 0"):
        f(prior, [g[0], k.costs.Rosenbrock()], 0.1, 10)
    with pytest.raises(ValueError, match="cost 2 differs from cost 0"):
        f(prior, [g[0], g[1], k.costs.GaussDist([0.0, 1.0, 2.0])], 0.1, 10)
    with pytest.raises(ValueError, match=r"len\(seeds\) = 2 != nruns = 3"):
        f(prior, g, 0.1, 10, seeds=[1, 2])
    with pytest.raises(ValueError, match=r"len\(eps\) = 2 != nruns = 3"):
        f(prior, g, [0.1, 0.2], 10)
    with pytest.raises(ValueError, match="eps of run 1 is NaN"):
        f(prior, g, [0.1, math.nan, 0.2], 10)
    with pytest.raises(ValueError, match="eps of run 0 is NaN"):
        f(prior, g, math.nan, 10)
    with pytest.raises(ValueError, match="takes rows of 1 parameters, got 2"):
        f(prior, [k.costs.Mixture(0.0), k.costs.Mixture(0.1)], 0.1, 10)
    # what abc_reject refuses, abc_reject_batch refuses in the same words
    with pytest.raises(ValueError, match=r"either \(eps, n\) or \(draws, keep\)"):
        f(prior, g)
    with pytest.raises(ValueError, match=r"either \(eps, n\) or \(draws, keep\)"):
        f(prior, g, 0.1)
    with pytest.raises(ValueError, match=r"either \(eps, n\) or \(draws, keep\)"):
        f(prior, g, n=10)
    with pytest.raises(ValueError, match="not both"):
        f(prior, g, 0.1, 10, draws=100, keep=5)
    with pytest.raises(ValueError, match="not both"):
        f(prior, g, [0.1, 0.2, 0.3], draws=100, keep=5)
    with pytest.raises(ValueError, match="keep needs draws"):
        f(prior, g, keep=5)
    with pytest.raises(ValueError, match="keep must be >= 1"):
        f(prior, g, draws=100, keep=0)
    with pytest.raises(ValueError, match="draws must be >= keep"):
        f(prior, g, draws=4, keep=5)
    with pytest.raises(ValueError, match="n must be >= 0"):
        f(prior, g, 0.1, -1)
    with pytest.raises(ValueError, match="draws must be >= 1"):
        f(prior, g, 0.1, 10, draws=0)
    with pytest.raises(ValueError, match="first_row must be >= 0"):
        f(prior, g, 0.1, 10, first_row=-1)
    with pytest.raises(ValueError, match=r"first_row \+ draws <= 2\^32"):
        f(prior, g, 0.1, 10, draws=100, first_row=(1 << 32) - 99)


def test_public_surface(k):
    assert "abc_reject_batch" in k.__all__ and callable(k.abc_reject_batch)
    from kissabc_jl_amd import api
    assert issubclass(api.RejectBatchResult, list)
    doc = k.abc_reject_batch.__doc__
    assert "NOT independent" in doc and "chain_seeds" in doc     # common random numbers are stated plainly


# ---- the C entry point's own refusals (ctx = NULL) ---------------------------------------------
def _abi_args(k, R=3, D=2, cap=8):
    from kissabc_jl_amd import _cdefs as cd, _lib
    lib = _lib.load()
    costs = [k.costs.GaussDist([0.25 * (r + 1)] * D) for r in range(R)]
    ccs = (cd.Cost * R)(*[c.to_c() for c in costs])
    o = cd.RejectOpts()
    lib.kabc_reject_default_opts(C.byref(o))
    o.eps, o.n_accept = 0.5, 4
    bufs = (np.zeros((R, cap, D)), np.zeros((R, cap)), np.zeros((R, cap)), np.zeros((R, cap), dtype=np.int64))
    res = (cd.RejectResult * R)()
    for r in range(R):
        res[r].theta = bufs[0][r].ctypes.data_as(cd.c_double_p)
        res[r].cost = bufs[1][r].ctypes.data_as(cd.c_double_p)
        res[r].logprior = bufs[2][r].ctypes.data_as(cd.c_double_p)
        res[r].index = bufs[3][r].ctypes.data_as(C.POINTER(C.c_int64))
        res[r].capacity = cap
    st = (C.c_int * R)(*([-7] * R))
    return lib, cd, costs, ccs, o, res, st, bufs


def test_abi_refusals(k):
    R = 3
    lib, cd, costs, ccs, o, res, st, bufs = _abi_args(k, R)
    prior = k.Factored(k.Normal(0, 1), k.Uniform(-1, 1)).to_c()
    f = lib.kabc_abc_reject_batch
    fake = C.c_void_p(8)      # never dereferenced: every case below is refused before the context is used

    def refused(msg, ctx=None, prior_=prior, D=2, costs_=ccs, nruns=R, seeds=None, eps=None, opts=o, res_=res, st_=st):
        got = f(ctx, prior_, D, costs_, nruns, seeds, eps, C.byref(opts) if opts is not None else None, res_, st_)
        assert got == cd.KABC_ERR_INVALID_ARG, (msg, got, lib.kabc_last_error())
        assert msg in lib.kabc_last_error(), (msg, lib.kabc_last_error())

    refused(b"ctx is NULL")                                      # everything else is in order
    refused(b"ctx is NULL", seeds=(C.c_uint64 * R)(1, 2, 3), eps=(C.c_double * R)(0.1, 0.2, math.inf))
    for kw in ({"prior_": None}, {"costs_": None}, {"opts": None}, {"res_": None}, {"st_": None}):
        refused(b"NULL argument", ctx=fake, **kw)
    refused(b"nruns = 0 is outside 1..65535", nruns=0)
    refused(b"nruns = -1 is outside 1..65535", nruns=-1)
    refused(b"nruns = 65536 is outside 1..65535", nruns=65536)
    refused(b"D = 0 outside 1..256", D=0)
    refused(b"D = 257 outside 1..256", D=257)

    def with_opts(**kw):
        o2 = cd.RejectOpts()
        C.memmove(C.byref(o2), C.byref(o), C.sizeof(o))
        for name, v in kw.items():
            setattr(o2, name, v)
        return o2
    refused(b"n_accept = -1", opts=with_opts(n_accept=-1))
    refused(b"max_draws = -5", opts=with_opts(max_draws=-5))
    refused(b"keep = -2", opts=with_opts(keep=-2))
    refused(b"run 0: result.capacity = 8 below n_accept = 9", opts=with_opts(n_accept=9))
    refused(b"run 0: result.capacity = 8 below keep = 9", opts=with_opts(keep=9, max_draws=100))
    refused(b"1 <= keep <= max_draws", opts=with_opts(keep=5, max_draws=4))
    refused(b"1 <= keep <= max_draws", opts=with_opts(keep=5, max_draws=0))
    refused(b"first_row + max_draws <= 2^32", opts=with_opts(max_draws=100, first_row=(1 << 32) - 99))
    refused(b"first_row + max_draws <= 2^32", opts=with_opts(first_row=-1))
    refused(b"run 0: eps is NaN", opts=with_opts(eps=math.nan))
    refused(b"run 2: eps is NaN", eps=(C.c_double * R)(0.1, 0.2, math.nan))
    # the per-run eps replace opts.eps; keep mode ignores both
    refused(b"ctx is NULL", opts=with_opts(eps=math.nan), eps=(C.c_double * R)(0.1, 0.2, 0.3))
    refused(b"ctx is NULL", opts=with_opts(eps=math.nan, keep=4, max_draws=100), eps=(C.c_double * R)(*[math.nan] * R))
    # one run's result too small / an array missing
    res[1].capacity = 3
    refused(b"run 1: result.capacity = 3 below n_accept = 4")
    res[1].capacity = 8
    res[2].index = None
    refused(b"run 2: NULL argument")
    res[2].index = bufs[3][2].ctypes.data_as(C.POINTER(C.c_int64))
    # unequal costs
    other = [costs[0], costs[1], k.costs.GaussDist([0.1, 0.2, 0.3])]
    refused(b"run 2: the costs of a batch share id, nparams and ndata", costs_=(cd.Cost * R)(*[c.to_c() for c in other]))
    other = [costs[0], k.costs.Rosenbrock(), costs[2]]
    refused(b"run 1: the costs of a batch share id, nparams and ndata", costs_=(cd.Cost * R)(*[c.to_c() for c in other]))
    bad = (cd.Cost * R)(*[c.to_c() for c in costs])
    bad[1].params = None
    refused(b"NULL params / data array", costs_=bad)
    # nothing was written: not a result row, not a status
    assert not any(b.any() for b in bufs) and list(st) == [-7] * R
    out = (C.c_int64 * 4)(9, 9, 9, 9)
    lib.kabc_reject_batch_stats(out)
    assert list(out) == [0, 0, 0, 0]                             # a refused call launched nothing
    lib.kabc_reject_batch_stats(None)                            # NULL is ignored


def test_header_ctypes_and_shim_agree(k):
    from kissabc_jl_amd import _cdefs as cd, _lib
    lib = _lib.load()
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "kabc.h")).read(), flags=re.S)
    m = re.search(r"kabc_status_t\s+kabc_abc_reject_batch\(([^;]*)\);", hdr)
    assert m, "kabc_abc_reject_batch is not declared in include/kabc.h"
    params = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
    assert params == ["kabc_ctx_t* ctx", "const kabc_prior_t* prior", "int32_t D", "const kabc_cost_t* costs",
                      "int64_t nruns", "const uint64_t* seeds", "const double* eps", "const kabc_reject_opts_t* opts",
                      "kabc_reject_result_t* results", "kabc_status_t* status"]
    assert re.search(r"void\s+kabc_reject_batch_stats\(int64_t out\[4\]\);", hdr)
    res, args = cd.PROTOTYPES["kabc_abc_reject_batch"]
    assert res is C.c_int and len(args) == len(params)
    assert args[4] is C.c_int64 and args[5] == C.POINTER(C.c_uint64) and args[6] == cd.c_double_p
    assert args[8] == C.POINTER(cd.RejectResult) and args[9] == C.POINTER(C.c_int)
    assert cd.PROTOTYPES["kabc_reject_batch_stats"] == (None, [C.POINTER(C.c_int64)])
    for sym in ("kabc_abc_reject_batch", "kabc_reject_batch_stats"):
        assert hasattr(lib, sym)
    assert lib.kabc_version() == 321                             # no new struct, no new version
    assert lib.kabc_abi_sizeof(34) == -1
    shim = open(os.path.join(ROOT, "kissabc.jl_amd", "julia", "KissABCHip.jl")).read()
    assert "ccall((:kabc_abc_reject_batch, libkabc)" in shim
    assert re.search(r"^export .*\babc_reject_batch\b", shim, flags=re.M)
    assert re.search(r"^function abc_reject_batch\(", shim, flags=re.M)


# ---- the selection logic of a batch, on the oracle alone ---------------------------------------
def test_batch_expectation_on_the_oracle(orc, k):
    prior = k.Factored(k.Normal(1, 0.5), k.DiscreteUniform(1, 10))
    costs = [k.costs.NoisyQuadDU(t) for t in (3.5, 5.5, 7.5)]
    N, first_row = 80, (1 << 31) + 5
    # a shared seed: the theta and log-prior columns of the runs' tables are the same bits -- the reference table
    tabs = batch_tables(orc, prior, costs, N, [3, 3, 3], first_row)
    for P, lp, _ in tabs[1:]:
        assert same_bits(P, tabs[0][0]) and same_bits(lp, tabs[0][1])
    assert not same_bits(tabs[0][2], tabs[1][2])                 # the costs differ: the datasets do
    # ... and distinct seeds give distinct draws
    tabs2 = batch_tables(orc, prior, costs, N, [3, 4, 5], first_row)
    assert same_bits(tabs2[0][0], tabs[0][0]) and not same_bits(tabs2[1][0], tabs[0][0])
    # per-run eps from each run's own cost quantiles: a run that finishes early, one that is exhausted, one that
    # accepts nothing
    eps = [float(np.sort(tabs[0][2])[40]), float(np.sort(tabs[1][2])[5]), float(np.min(tabs[2][2])) - 1.0]
    want = expected_batch(tabs, eps=eps, n=10)
    assert want[0]["index"].size == 10 and not want[0]["exhausted"] and want[0]["draws"] < N
    assert want[0]["draws"] == int(want[0]["index"][-1]) + 1
    assert want[1]["index"].size == 6 and want[1]["exhausted"] and want[1]["draws"] == N
    assert want[2]["index"].size == 0 and want[2]["exhausted"] and want[2]["draws"] == N
    # every run of the expectation IS the single call's oracle restatement
    for r in range(3):
        Pg, Cg, lpg, eg, idx, d, ex = oracle_reject(orc, prior, costs[r], eps=eps[r], n=10, draws=N, seed=3,
                                                    first_row=first_row)
        w = want[r]
        assert np.array_equal(idx, w["index"]) and d == w["draws"] and ex == w["exhausted"] and eg == w["eps"]
        assert same_bits(Pg, w["P"]) and same_bits(Cg, w["C"]) and same_bits(lpg, w["logprior"])
    # keep mode
    wk = expected_batch(tabs, keep=7)
    for r in range(3):
        Pg, Cg, lpg, eg, idx, d, ex = oracle_reject(orc, prior, costs[r], draws=N, keep=7, seed=3, first_row=first_row)
        assert np.array_equal(idx, wk[r]["index"]) and eg == wk[r]["eps"] and wk[r]["draws"] == N
        assert same_bits(Pg, wk[r]["P"]) and idx.size == 7 and np.all(np.diff(idx) > 0)
