"""CPU: DeviceCost.evaluate / prior_predictive -- the refusals that need no device (Python's, and the C
entry points' own, made with ctx = NULL as tests/test_ais_batch_args.py makes them), the two new stream
domains, and the LAW of the new addressing on the oracle alone: replicates along the transition word t
are as independent as walkers are (the moment checks of tests/test_cost_formulas.py, same inputs, same
tolerances, draws taken over a grid of rows i and replicates j)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- Python refusals: before the library is touched --------------------------------------------
def test_python_refusals(k, monkeypatch):
    from kissabc_jl_amd import _lib

    def no_library(*a, **kw):
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(_lib, "default_context", no_library)
    sim = k.costs.NormalMeanStdSim(1000, 2.0, 0.04)              # dim = 2
    with pytest.raises(ValueError, match="takes rows of 2 parameters, got 3"):
        sim.evaluate(np.zeros((5, 3)))
    with pytest.raises(ValueError, match="takes rows of 1 parameters, got 2"):
        k.costs.DiracSq(1.5)([0.5, 0.5])
    with pytest.raises(ValueError, match="takes rows of 4 parameters"):
        k.DeviceCost(1, params=[0.0] * 4, dim=4).evaluate(np.zeros(3))
    g = k.costs.GaussDist([0.0, 1.0])
    for bad in (0, -3):
        with pytest.raises(ValueError, match="nrep must be >= 1"):
            g.evaluate(np.zeros((4, 2)), nrep=bad)
    with pytest.raises(ValueError, match="first_row must be >= 0"):
        g.evaluate(np.zeros((4, 2)), first_row=-1)
    with pytest.raises(ValueError, match=r"first_row \+ n <= 2\^32"):
        g.evaluate(np.zeros((4, 2)), first_row=(1 << 32) - 3)
    with pytest.raises(ValueError, match="one row"):
        g.evaluate(np.zeros((2, 2, 2)))
    prior = k.Factored(k.Normal(0, 1), k.Normal(0, 1))
    with pytest.raises(TypeError, match="must be a DeviceCost"):
        k.prior_predictive(prior, lambda x: 0.0, 10)
    with pytest.raises(ValueError, match="takes rows of 1 parameters, got 2"):
        k.prior_predictive(prior, k.costs.Mixture(0.0), 10)
    with pytest.raises(ValueError, match="nrep must be >= 1"):
        k.prior_predictive(prior, g, 10, nrep=0)
    with pytest.raises(ValueError, match="first_row must be >= 0"):
        k.prior_predictive(prior, g, 10, first_row=-1)
    with pytest.raises(ValueError, match="n must be >= 0"):
        k.prior_predictive(prior, g, -1)


def test_call_is_evaluate(k):
    assert k.DeviceCost.__call__ is k.DeviceCost.evaluate
    assert "prior_predictive" in k.__all__ and callable(k.prior_predictive)


# ---- the C entry points' own refusals (no device needed: ctx = NULL) ---------------------------
def _eval_args(k, D=2, n=4):
    from kissabc_jl_amd import _cdefs as cd
    cost = k.costs.GaussDist([0.25] * D)
    cc = cost.to_c()
    theta = np.zeros((max(n, 1), max(D, 1)))
    out = np.zeros((max(n, 1), 3))
    return cd, cost, cc, theta, out


def test_cost_eval_abi_refusals(k):
    from kissabc_jl_amd import _lib
    lib = _lib.load()
    cd, cost, cc, theta, out = _eval_args(k)
    dp = cd.c_double_p
    f = lib.kabc_cost_eval
    th, o = theta.ctypes.data_as(dp), out.ctypes.data_as(dp)
    fake = C.c_void_p(8)      # never dereferenced: every case below is refused before the context is used
    cases = [
        ((None, C.byref(cc), 2, 4, th, 3, 1, 0, o), b"ctx is NULL"),
        ((fake, None, 2, 4, th, 3, 1, 0, o), b"NULL argument"),
        ((fake, C.byref(cc), 2, 4, None, 3, 1, 0, o), b"NULL argument"),
        ((fake, C.byref(cc), 2, 4, th, 3, 1, 0, None), b"NULL argument"),
        ((None, C.byref(cc), 2, 4, th, 0, 1, 0, o), b"nrep = 0"),
        ((None, C.byref(cc), 2, 4, th, 3, 1, (1 << 32) - 3, o), b"first_row + n <= 2^32"),
        ((None, C.byref(cc), 2, 4, th, 3, 1, -1, o), b"first_row + n <= 2^32"),
        ((None, C.byref(cc), 0, 4, th, 3, 1, 0, o), b"D = 0 outside 1..256"),
        ((None, C.byref(cc), 257, 4, th, 3, 1, 0, o), b"D = 257 outside 1..256"),
    ]
    for args, msg in cases:
        assert f(*args) == cd.KABC_ERR_INVALID_ARG, msg
        assert msg in lib.kabc_last_error(), (msg, lib.kabc_last_error())
    # the last row that fits: first_row + n == 2^32 passes the range check (and stops at the NULL context)
    assert f(None, C.byref(cc), 2, 4, th, 3, 1, (1 << 32) - 4, o) == cd.KABC_ERR_INVALID_ARG
    assert b"ctx is NULL" in lib.kabc_last_error()
    # a NULL params array behind a non-zero length
    cc2 = cost.to_c()
    cc2.params = None
    assert f(None, C.byref(cc2), 2, 4, th, 3, 1, 0, o) == cd.KABC_ERR_INVALID_ARG
    assert b"NULL params / data array" in lib.kabc_last_error()
    assert not out.any()


def test_prior_predictive_abi_refusals(k):
    from kissabc_jl_amd import _lib
    lib = _lib.load()
    cd, cost, cc, theta, out = _eval_args(k)
    dp = cd.c_double_p
    prior = k.Factored(k.Normal(0, 1), k.Uniform(-1, 1)).to_c()
    f = lib.kabc_prior_predictive
    th, o = theta.ctypes.data_as(dp), out.ctypes.data_as(dp)
    fake = C.c_void_p(8)
    cases = [
        ((None, prior, 2, C.byref(cc), 4, 3, 1, 0, th, None, o), b"ctx is NULL"),
        ((fake, None, 2, C.byref(cc), 4, 3, 1, 0, th, None, o), b"NULL argument"),
        ((fake, prior, 2, None, 4, 3, 1, 0, th, None, o), b"NULL argument"),
        ((fake, prior, 2, C.byref(cc), 4, 3, 1, 0, None, None, o), b"NULL argument"),
        ((fake, prior, 2, C.byref(cc), 4, 3, 1, 0, th, None, None), b"NULL argument"),
        ((None, prior, 2, C.byref(cc), 4, 0, 1, 0, th, None, o), b"nrep = 0"),
        ((None, prior, 2, C.byref(cc), 4, 3, 1, (1 << 32) - 3, th, None, o), b"first_row + n <= 2^32"),
        ((None, prior, 0, C.byref(cc), 4, 3, 1, 0, th, None, o), b"D = 0 outside 1..256"),
        ((None, prior, 257, C.byref(cc), 4, 3, 1, 0, th, None, o), b"D = 257 outside 1..256"),
    ]
    for args, msg in cases:
        assert f(*args) == cd.KABC_ERR_INVALID_ARG, msg
        assert msg in lib.kabc_last_error(), (msg, lib.kabc_last_error())


# ---- the two new domains -----------------------------------------------------------------------
def test_domains_match_the_header_and_collide_with_nothing():
    from kissabc_jl_amd import _cdefs as cd
    text = open(os.path.join(ROOT, "include", "kabc_philox.h")).read()
    doms = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (KABC_DOM_\w+) (\d+)u", text)}
    assert doms["KABC_DOM_EVAL_COST"] == cd.DOM_EVAL_COST == 17
    assert doms["KABC_DOM_EVAL_DRAW"] == cd.DOM_EVAL_DRAW == 18
    assert len(doms) >= 18 and len(set(doms.values())) == len(doms), doms
    assert all(0 < v < 256 for v in doms.values())      # (counter word 3 keeps 8 bits for the domain)


# ---- the law of the (row, replicate) addressing, on the oracle ---------------------------------
def _grid(orc, cost, x, rows=200, reps=100, seed=11):
    from kissabc_jl_amd import _cdefs as cd
    return np.array([[orc.cost_eval(cost, x, seed=seed, walker=i, t=j, domain=cd.DOM_EVAL_COST)
                      for j in range(reps)] for i in range(rows)])


def test_grid_mixture(orc, k):
    g = _grid(orc, k.costs.Mixture(0.0), [10.0])
    v = g.ravel() - 10.0
    assert abs(v.mean()) < 5 * np.sqrt(0.505 / v.size)
    assert abs(v.var() / 0.505 - 1) < 0.06
    assert abs((np.abs(v) < 0.3).mean() - (0.9973002 + 0.2358228) / 2) < 0.015
    # no two cells of the grid share a stream
    assert np.unique(g.view(np.uint64)).size == g.size
    # replicates 0 and 1 of a row are uncorrelated: |r| within 4 standard errors over 2000 rows
    two = _grid(orc, k.costs.Mixture(0.0), [10.0], rows=2000, reps=2)
    r = np.corrcoef(two[:, 0], two[:, 1])[0, 1]
    assert abs(r) < 4 / np.sqrt(2000), r


def test_grid_noisy_quad_du(orc, k):
    n_, du, target = 1.3, 4.0, 5.5
    v = _grid(orc, k.costs.NoisyQuadDU(target), [n_, du]).ravel()
    base = (n_ * n_ + du) * n_ - target
    sd = 0.01 * (n_ * n_ + du)
    assert abs(v.mean() - base) < 5 * sd / np.sqrt(v.size)
    assert abs(v.std() / sd - 1) < 0.03
    assert abs(((v - base) / sd > 1.0).mean() - 0.158655) < 0.012


def test_grid_noisy_banana(orc, k):
    v = _grid(orc, k.costs.NoisyBanana(0.0), [1.0, 1.0]).ravel()
    assert np.all(np.isfinite(v)) and v.min() >= 0
    assert abs(v.mean() / (50e-4 + 1e-4) - 1) < 0.05
    x = np.array([0.3, -0.7])
    u = _grid(orc, k.costs.NoisyBanana(0.0), x).ravel()
    a0, b0 = x[0] - x[1] ** 2, x[1] - 1.0
    mean = 50 * (a0 * a0 + 1e-4) + (b0 * b0 + 1e-4)
    assert abs(u.mean() / mean - 1) < 0.01
    h = _grid(orc, k.costs.NoisyBanana(0.5), x).ravel()
    assert abs(np.isinf(h).mean() - 0.5) < 0.02
    assert abs(h[np.isfinite(h)].mean() / mean - 1) < 0.02


def test_grid_normal_meanstd_sim(orc, k):
    n, mu, sig = 1000, 2.0, 0.04
    v = _grid(orc, k.costs.NormalMeanStdSim(n, mu, sig), [mu, sig], rows=40, reps=100).ravel()
    want = sig * sig / n + 2500 * sig * sig / (2 * (n - 1))
    assert abs((v * v).mean() / want - 1) < 0.08
    off = _grid(orc, k.costs.NormalMeanStdSim(n, mu + 0.1, sig), [mu, sig], rows=20, reps=100).ravel()
    assert abs(off.mean() - 0.1) < 0.01
    wide = _grid(orc, k.costs.NormalMeanStdSim(n, mu, sig), [mu, 2 * sig], rows=20, reps=100).ravel()
    assert abs(wide.mean() - 50 * sig) < 0.1
