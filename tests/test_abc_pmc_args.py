"""CPU: abc_pmc / kabc_abc_pmc -- the refusals that need no device (Python's, made before the library is touched, and
the C entry point's own, made with ctx = NULL), the three struct layouts, the exported symbols and the stream domain."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_python_refusals(k, monkeypatch):
    from kissabc_jl_amd import _lib

    def no_library(*a, **kw):
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(_lib, "default_context", no_library)
    prior = k.Factored(k.Normal(0, 1), k.Normal(0, 1))
    g = k.costs.GaussDist([0.0, 1.0])
    with pytest.raises(TypeError, match="must be a DeviceCost"):
        k.abc_pmc(prior, lambda x: 0.0, 100, eps=[1.0])
    with pytest.raises(ValueError, match="takes rows of 1 parameters, got 2"):
        k.abc_pmc(prior, k.costs.Mixture(0.0), 100, eps=[1.0])
    with pytest.raises(ValueError, match=r"outside 1\.\.16"):
        k.abc_pmc(k.Factored(*[k.Normal(0, 1)] * 17), k.costs.GaussDist([0.0] * 17), 100, eps=[1.0])
    with pytest.raises(ValueError, match="continuous prior"):
        k.abc_pmc(k.Factored(k.Normal(0, 1), k.DiscreteUniform(1, 10)), g, 100, eps=[1.0])
    with pytest.raises(ValueError, match="continuous prior"):
        k.abc_pmc(k.Factored(k.NegativeBinomial(3, 0.5), k.Normal(0, 1)), g, 100, eps=[1.0])
    with pytest.raises(ValueError, match="nparticles = 3 outside"):
        k.abc_pmc(prior, g, 3, eps=[1.0])                     # N < D + 2
    with pytest.raises(ValueError, match="nparticles = 1048577 outside"):
        k.abc_pmc(prior, g, (1 << 20) + 1, eps=[1.0])
    with pytest.raises(ValueError, match="q outside"):
        k.abc_pmc(prior, g, 100, q=0.0)
    with pytest.raises(ValueError, match="q outside"):
        k.abc_pmc(prior, g, 100, q=1.0)
    with pytest.raises(ValueError, match="not both"):
        k.abc_pmc(prior, g, 100, eps=[1.0], q=0.5)
    with pytest.raises(ValueError, match="scale must be > 0"):
        k.abc_pmc(prior, g, 100, eps=[1.0], scale=0.0)
    with pytest.raises(ValueError, match="scale must be > 0"):
        k.abc_pmc(prior, g, 100, eps=[1.0], scale=math.nan)
    with pytest.raises(ValueError, match="holds a NaN"):
        k.abc_pmc(prior, g, 100, eps=[1.0, math.nan])
    with pytest.raises(ValueError, match="empty"):
        k.abc_pmc(prior, g, 100, eps=[])
    with pytest.raises(ValueError, match="eps0 / eps_target is NaN"):
        k.abc_pmc(prior, g, 100, eps0=math.nan)
    with pytest.raises(ValueError, match="eps0 / eps_target is NaN"):
        k.abc_pmc(prior, g, 100, eps_target=math.nan)
    with pytest.raises(ValueError, match="max_draws outside"):
        k.abc_pmc(prior, g, 100, eps=[1.0], max_draws=99)
    with pytest.raises(ValueError, match="max_draws outside"):
        k.abc_pmc(prior, g, 100, eps=[1.0], max_draws=(1 << 32) + 1)
    with pytest.raises(ValueError, match="generations outside"):
        k.abc_pmc(prior, g, 100, generations=0)
    with pytest.raises(ValueError, match="generations outside"):
        k.abc_pmc(prior, g, 100, generations=1 << 24)
    with pytest.raises(ValueError, match=r"generations must be len\(eps\)"):
        k.abc_pmc(prior, g, 100, eps=[2.0, 1.0], generations=3)
    with pytest.raises(ValueError, match="kernel must be"):
        k.abc_pmc(prior, g, 100, eps=[1.0], kernel="banded")
    with pytest.raises(ValueError, match="min_rate is NaN"):
        k.abc_pmc(prior, g, 100, eps=[1.0], min_rate=math.nan)


def test_defaults_of_check_pmc_args(k):
    from kissabc_jl_amd import _cdefs as cd
    from kissabc_jl_amd.costs import check_pmc_args
    prior = k.Factored(k.Normal(0, 1), k.Normal(0, 1))
    g = k.costs.GaussDist([0.0, 1.0])
    N, eps, q, G, kid, M = check_pmc_args(g, prior, 4, None, None, math.inf, -math.inf, None, "full", 2.0, None, 0.0)
    assert (N, eps, q, G, kid, M) == (4, None, 0.5, 20, cd.PMC_KERNEL_FULL, 40_000)
    N, eps, q, G, kid, M = check_pmc_args(g, prior, 1 << 20, [3, 2, 1], None, math.inf, -math.inf, None, "diag", 2.0, None, 0.0)
    assert eps.tolist() == [3.0, 2.0, 1.0] and q is None and G == 3 and kid == cd.PMC_KERNEL_DIAG and M == 1 << 32


def test_public_surface(k):
    assert "abc_pmc" in k.__all__ and callable(k.abc_pmc) and "PmcResult" in k.__all__
    assert k.PmcResult._fields == ("theta", "w", "C", "logprior", "eps", "info")
    rng = np.random.default_rng(0)
    theta = rng.normal(size=(50, 2))
    w = rng.random(50)
    w /= w.sum()
    r = k.PmcResult(theta, w, np.zeros(50), np.zeros(50), 0.5,
                    {"mean": w @ theta, "cov": np.eye(2), "scalar": False})
    assert r.ϵ == 0.5 and np.array_equal(r.mean, w @ theta) and r.ess == pytest.approx(1.0 / np.sum(w * w))
    P = r.resample(2000, seed=1)
    assert len(P) == 2 and len(P[0]) == 2000
    assert abs(P[0].mean() - r.mean[0]) < 5 * theta[:, 0].std() / math.sqrt(r.ess)
    assert len(r.resample()[1]) == 50


def _abi_args(k, D=2, N=8, G=3):
    from kissabc_jl_amd import _cdefs as cd, _lib
    lib = _lib.load()
    cost = k.costs.GaussDist([0.25] * D)
    o = cd.PmcOpts()
    lib.kabc_pmc_default_opts(C.byref(o))
    o.nparticles, o.generations, o.max_draws = N, G, 100 * N
    bufs = [np.zeros((N, D)), np.zeros(N), np.zeros(N), np.zeros(N), np.zeros(N, dtype=np.int64), np.zeros(D), np.zeros((D, D))]
    log = (cd.PmcGen * G)()
    r = cd.PmcResult()
    for name, b in zip(("theta", "w", "cost", "logprior"), bufs[:4]):
        setattr(r, name, b.ctypes.data_as(cd.c_double_p))
    r.index = bufs[4].ctypes.data_as(C.POINTER(C.c_int64))
    r.mean, r.cov = bufs[5].ctypes.data_as(cd.c_double_p), bufs[6].ctypes.data_as(cd.c_double_p)
    r.log = log
    return lib, cd, cost, o, r, bufs, log


def test_default_opts(k):
    lib, cd, _, _, _, _, _ = _abi_args(k)
    o = cd.PmcOpts()
    C.memset(C.byref(o), 0x55, C.sizeof(o))
    lib.kabc_pmc_default_opts(C.byref(o))
    assert (o.nparticles, o.generations, o.max_draws, o.kernel, o.reserved, o.seed) == (0, 0, 0, 0, 0, 0)
    assert not o.eps and o.eps0 == math.inf and o.eps_target == -math.inf
    assert (o.q, o.scale, o.min_rate) == (0.5, 2.0, 0.0)
    lib.kabc_pmc_default_opts(None)


def test_abi_refusals(k):
    lib, cd, cost, o, r, bufs, log = _abi_args(k)
    cc = cost.to_c()
    prior = k.Factored(k.Normal(0, 1), k.Uniform(-1, 1)).to_c()
    f = lib.kabc_abc_pmc
    fake = C.c_void_p(8)      # never dereferenced: every case below is refused before the context is used

    def refused(msg, ctx=fake, prior_=prior, D=2, cost_=None, opts=o, res=r, status=cd.KABC_ERR_INVALID_ARG):
        got = f(ctx, prior_, D, C.byref(cc) if cost_ is None else cost_, C.byref(opts) if opts is not None else None,
                C.byref(res) if res is not None else None)
        assert got == status, (msg, got, lib.kabc_last_error())
        assert msg in lib.kabc_last_error(), (msg, lib.kabc_last_error())

    def with_opts(**kw):
        o2 = cd.PmcOpts()
        C.memmove(C.byref(o2), C.byref(o), C.sizeof(o))
        for name, v in kw.items():
            setattr(o2, name, v)
        return o2

    refused(b"ctx is NULL", ctx=None)                             # everything else is in order
    refused(b"NULL argument", prior_=None)
    refused(b"NULL argument", opts=None)
    refused(b"NULL argument", res=None)
    assert f(fake, prior, 2, None, C.byref(o), C.byref(r)) == cd.KABC_ERR_INVALID_ARG
    for name in ("theta", "w", "cost", "logprior", "index", "log", "mean", "cov"):
        r2 = cd.PmcResult()
        C.memmove(C.byref(r2), C.byref(r), C.sizeof(r))
        setattr(r2, name, None)
        refused(b"NULL argument", res=r2)
    refused(b"D outside 1..16", D=0)
    refused(b"D outside 1..16", D=17, opts=with_opts(nparticles=100, max_draws=1000))
    refused(b"nparticles outside", opts=with_opts(nparticles=3))
    refused(b"nparticles outside", opts=with_opts(nparticles=(1 << 20) + 1, max_draws=1 << 21))
    refused(b"generations outside", opts=with_opts(generations=0))
    refused(b"generations outside", opts=with_opts(generations=1 << 24))
    refused(b"max_draws outside", opts=with_opts(max_draws=7))
    refused(b"max_draws outside", opts=with_opts(max_draws=(1 << 32) + 1))
    refused(b"scale must be > 0", opts=with_opts(scale=0.0))
    refused(b"scale must be > 0", opts=with_opts(scale=math.nan))
    refused(b"min_rate is NaN", opts=with_opts(min_rate=math.nan))
    refused(b"kernel must be", opts=with_opts(kernel=2))
    refused(b"q outside (0, 1)", opts=with_opts(q=0.0))
    refused(b"q outside (0, 1)", opts=with_opts(q=1.0))
    refused(b"eps0 / eps_target is NaN", opts=with_opts(eps0=math.nan))
    refused(b"eps0 / eps_target is NaN", opts=with_opts(eps_target=math.nan))
    sched = np.array([2.0, math.nan, 1.0])
    refused(b"eps holds a NaN", opts=with_opts(eps=sched.ctypes.data_as(cd.c_double_p)))
    cc2 = cost.to_c()
    cc2.params = None
    refused(b"NULL params / data array", cost_=C.byref(cc2))
    # a discrete component: unsupported, before the context is used
    disc = k.Factored(k.Normal(0, 1), k.DiscreteUniform(1, 10)).to_c()
    refused(b"is discrete", prior_=disc, status=cd.KABC_ERR_UNSUPPORTED)
    assert not any(b.any() for b in bufs)
    # the verification entry
    y = np.zeros((4, 2))
    dp = lambda a: a.ctypes.data_as(cd.c_double_p)
    g = lib.kabc_pmc_kernel_sums
    assert g(None, 2, 4, dp(y), 4, dp(y), dp(y[:, 0].copy()), dp(np.zeros(4))) == cd.KABC_ERR_INVALID_ARG
    assert b"ctx is NULL" in lib.kabc_last_error()
    assert g(fake, 17, 4, dp(y), 4, dp(y), dp(y), dp(y)) == cd.KABC_ERR_INVALID_ARG
    assert g(fake, 2, 0, dp(y), 4, dp(y), dp(y), dp(y)) == cd.KABC_ERR_INVALID_ARG
    assert g(fake, 2, 4, dp(y), (1 << 20) + 1, dp(y), dp(y), dp(y)) == cd.KABC_ERR_INVALID_ARG
    assert g(fake, 2, 4, None, 4, dp(y), dp(y), dp(y)) == cd.KABC_ERR_INVALID_ARG


def test_struct_layouts_symbols_and_domain(k):
    from kissabc_jl_amd import _cdefs as cd, _lib
    lib = _lib.load()
    for which, T in ((cd.ABI_PMC_OPTS, cd.PmcOpts), (cd.ABI_PMC_GEN, cd.PmcGen), (cd.ABI_PMC_RESULT, cd.PmcResult)):
        assert C.sizeof(T) == lib.kabc_abi_sizeof(which), T
        for f, (name, _) in enumerate(T._fields_):
            assert getattr(T, name).offset == lib.kabc_abi_offsetof(which, f), (T, name)
        assert lib.kabc_abi_offsetof(which, len(T._fields_)) == -1
    assert (C.sizeof(cd.PmcOpts), C.sizeof(cd.PmcGen), C.sizeof(cd.PmcResult)) == (88, 32, 96)
    # the first block stays closed, 34 closes the pair of kabc_abc_reject, nothing follows the three
    assert lib.kabc_abi_sizeof(11) == -1 and lib.kabc_abi_sizeof(34) == -1 and lib.kabc_abi_sizeof(38) == -1
    for sym in ("kabc_abc_pmc", "kabc_pmc_default_opts", "kabc_pmc_kernel_sums", "kabc_pmc_stats"):
        assert hasattr(lib, sym) and sym in cd.PROTOTYPES
    hdr = open(os.path.join(ROOT, "include", "kabc_philox.h")).read()
    m = re.search(r"#define KABC_DOM_PMC_MOVE (\d+)u", hdr)
    assert m and int(m.group(1)) == cd.DOM_PMC_MOVE == 19
    doms = [int(v) for v in re.findall(r"#define KABC_DOM_\w+ (\d+)u", hdr)]
    assert len(doms) == len(set(doms))                            # no two streams share a domain
    khdr = open(os.path.join(ROOT, "include", "kabc.h")).read()
    assert int(re.search(r"#define KABC_PMC_CHUNK (\d+)", khdr).group(1)) == cd.KABC_PMC_CHUNK
    names = re.search(r"KABC_PMC_STOP_DONE = 0,(.*?)\};", khdr, re.S).group(0)
    assert [n.lower() for n in re.findall(r"KABC_PMC_STOP_(\w+) = \d", names)] == list(cd.PMC_STOP_NAMES)
