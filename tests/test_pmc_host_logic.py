"""The host rules of ABC population Monte Carlo (kissabc.jl_amd/csrc/pmc_rules.hpp: moments, proposal covariance and
its factor, the CDF, the whitened coordinates, the weights from the kernel sums, the schedule and the stop rules) need
no GPU: tests/pmc_host_check.cpp runs them stand-alone, built with AddressSanitizer and UBSan, and every number it
prints is compared bit for bit with the numpy restatement tests/abc_pmc_oracle.py makes from the header's words."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import abc_pmc_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(shutil.which("c++") is None, reason="no c++ on PATH")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pmc_host") / "pmc_host_check")
    cmd = ["c++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "kissabc.jl_amd", "csrc"), os.path.join(ROOT, "tests", "pmc_host_check.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def _hex(a):
    return " ".join(f"{int(b):016x}" for b in np.ascontiguousarray(a, dtype=np.float64).ravel().view(np.uint64))


def _run(exe, text):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    out = {}
    for line in r.stdout.splitlines():
        name, *vals = line.split()
        out.setdefault(name, []).append(vals)
    return out


def _doubles(vals):
    return np.array([int(v, 16) for v in vals], dtype=np.uint64).view(np.float64)


def _same(got, want, what):
    got, want = np.asarray(got, dtype=np.float64).ravel(), np.asarray(want, dtype=np.float64).ravel()
    assert got.shape == want.shape, what
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (what, got[:4], want[:4])


def _populations():
    rng = np.random.default_rng(11)
    N, D = 40, 3
    theta = rng.normal(size=(N, D)) * [1.0, 3.0, 0.2] + [0.5, -2.0, 10.0]
    theta[:, 2] += 0.7 * theta[:, 0]
    w = rng.random(N)
    w /= w.sum()
    ties = theta.copy()
    ties[5] = ties[4]
    ties[17] = ties[4]
    ties[:, 1] = np.round(ties[:, 1])                    # many equal coordinates
    zero_w = w.copy()
    zero_w[[0, 3, 4, 39]] = 0.0
    zero_w /= zero_w.sum()
    flat = theta.copy()
    flat[:, 1] = 0.0                                     # a coordinate without spread: c_11 == 0.0 exactly
    dup = theta.copy()
    dup[:, 2] = dup[:, 0]                                # a duplicated column: whatever the factor says, both agree
    one = rng.normal(size=(5, 1))
    return {"plain": (theta, w), "ties": (ties, np.full(N, 1.0 / N)), "zero_weights": (theta, zero_w),
            "flat_column": (flat, w), "duplicated_column": (dup, w), "d1": (one, np.full(5, 0.2))}


@pytest.mark.parametrize("kernel", ["full", "diag"])
@pytest.mark.parametrize("name", ["plain", "ties", "zero_weights", "flat_column", "duplicated_column", "d1"])
def test_moments_factor_cdf_whitening(exe, orc, name, kernel):
    theta, w = _populations()[name]
    N, D = theta.shape
    scale = 2.0 if kernel == "full" else 1.5
    got = _run(exe, f"moments {N} {D} {_hex([scale])} {int(kernel == 'diag')} {_hex(theta)} {_hex(w)}\n")
    mu, c = po.moments(theta, w)
    rc, L, W = po.mvn_prepare(orc, po.proposal_cov(c, scale, kernel))
    _same(_doubles(got["mu"][0]), mu, "mu")
    _same(_doubles(got["c"][0]), c, "c")
    assert int(got["rc"][0][0]) == rc
    if name == "flat_column":
        assert rc == 2                                   # the run stops as degenerate
    if name in ("plain", "ties", "zero_weights", "d1"):
        assert rc == 0
    if rc == 0:
        _same(_doubles(got["L"][0]), L, "L")
        _same(_doubles(got["W"][0]), W, "W")
        _same(_doubles(got["y"][0]), po.whiten(theta, mu, W), "y")
        if kernel == "diag":
            assert np.count_nonzero(L - np.diag(np.diag(L))) == 0
    _same(_doubles(got["cdf"][0]), po.cdf_of(w), "cdf")
    assert int(got["steps"][0][0]) == math.ceil(math.log2(N))


def test_weights_from_sums(exe, orc):
    rng = np.random.default_rng(5)
    N = 37
    lp = rng.normal(size=N) * 3 - 4
    S = rng.random(N) * 1e-3
    lp[7] = lp[8]
    S[7] = S[8]                                          # ties
    S[20] = 1e-250                                       # one particle far out in the proposal's tail
    got = _run(exe, f"weights {N} {_hex(lp)} {_hex(S)}\n")
    w, ess = po.weights_from_sums(orc, lp, S)
    assert got["ok"][0] == ["1"]
    _same(_doubles(got["w"][0]), w, "w")
    _same(_doubles(got["ess"][0]), [ess], "ess")
    assert w[7] == w[8] and 1.0 <= ess <= N
    for bad in (0.0, math.inf, math.nan, -1.0, 5e-324):  # a sum that is 0 or not finite (5e-324: v overflows): degenerate
        S2 = S.copy()
        S2[3] = bad
        assert _run(exe, f"weights {N} {_hex(lp)} {_hex(S2)}\n")["ok"][0] == ["0"]
        assert po.weights_from_sums(orc, lp, S2) is None


def _after(exe, orc, *, eps, N, G, g, eps_g, draws, q=0.5, target=-math.inf, min_rate=0.0, C):
    adaptive = eps is None
    text = f"after {int(adaptive)} {N} {G} {g} {_hex([eps_g])} {draws} {_hex([q])} {_hex([target])} {_hex([min_rate])} "
    if not adaptive:
        text += _hex(eps) + " "
    got = _run(exe, text + _hex(C) + "\n")
    stop, nxt = po.after_generation(orc, g, eps_g, draws, np.asarray(C, dtype=np.float64), N, eps, q, target, G, min_rate)
    code = int(got["stop"][0][0])
    assert (po.STOPS[code] if code >= 0 else None) == stop, (code, stop)
    if stop is None:
        _same(_doubles(got["eps_next"][0]), [nxt], "eps_next")
    return stop, nxt


def test_schedule_and_stop_rules(exe, orc):
    rng = np.random.default_rng(2)
    N = 50
    C = rng.random(N)
    # explicit schedule: the next entry, then done
    assert _after(exe, orc, eps=[4.0, 2.0, 1.0], N=N, G=3, g=0, eps_g=4.0, draws=90, C=C) == (None, 2.0)
    assert _after(exe, orc, eps=[4.0, 2.0, 1.0], N=N, G=3, g=2, eps_g=1.0, draws=90, C=C)[0] == "done"
    # min_rate: N / draws below it ends the run, but not on the schedule's last generation
    assert _after(exe, orc, eps=[4.0, 2.0, 1.0], N=N, G=3, g=1, eps_g=2.0, draws=501, min_rate=0.1, C=C)[0] == "min_rate"
    assert _after(exe, orc, eps=[4.0, 2.0, 1.0], N=N, G=3, g=1, eps_g=2.0, draws=500, min_rate=0.1, C=C) == (None, 1.0)
    assert _after(exe, orc, eps=[4.0, 2.0, 1.0], N=N, G=3, g=2, eps_g=1.0, draws=501, min_rate=0.1, C=C)[0] == "done"
    # adaptive: the quantile, floored at the target
    stop, nxt = _after(exe, orc, eps=None, N=N, G=9, g=0, eps_g=math.inf, draws=N, q=0.3, C=C)
    assert stop is None and nxt == orc.quantile(C, 0.3) == float(np.quantile(C, 0.3))
    stop, nxt = _after(exe, orc, eps=None, N=N, G=9, g=3, eps_g=0.9, draws=N, q=0.3, target=0.5, C=C)
    assert stop is None and nxt == 0.5
    assert _after(exe, orc, eps=None, N=N, G=9, g=4, eps_g=0.5, draws=N, q=0.3, target=0.5, C=C)[0] == "target"
    assert _after(exe, orc, eps=None, N=N, G=9, g=8, eps_g=0.9, draws=N, q=0.3, C=C)[0] == "done"
    # stalled: a cost with two values -- the quantile does not fall (from generation 2 on)
    two = np.where(np.arange(N) % 3 == 0, 0.0, 1.0)
    assert _after(exe, orc, eps=None, N=N, G=9, g=0, eps_g=math.inf, draws=N, q=0.5, C=two) == (None, 1.0)
    assert _after(exe, orc, eps=None, N=N, G=9, g=1, eps_g=1.0, draws=N, q=0.5, C=two)[0] == "stalled"
    assert _after(exe, orc, eps=None, N=N, G=9, g=1, eps_g=1.0, draws=N, q=0.2, C=two) == (None, 0.0)
    # +Inf costs under eps_0 = +Inf: the quantile's non-finite branch, a NaN threshold stalls
    inf = np.where(np.arange(N) < 30, math.inf, 1.0)
    assert _after(exe, orc, eps=None, N=N, G=9, g=0, eps_g=math.inf, draws=N, q=0.9, C=inf)[1] == math.inf


def test_refusals(exe):
    def check(D=2, N=10, G=3, M=100, scale=2.0, min_rate=0.0, kernel=0, adaptive=1, q=0.5, eps0=math.inf, target=-math.inf):
        out = _run(exe, f"check {D} {N} {G} {M} {_hex([scale])} {_hex([min_rate])} {kernel} {adaptive} {_hex([q])} "
                        f"{_hex([eps0])} {_hex([target])}\n")
        return " ".join(out["check"][0])
    assert check() == "ok" and check(adaptive=0) == "ok" and check(N=4) == "ok" and check(D=16, N=18, M=18) == "ok"
    assert "D outside" in check(D=0) and "D outside" in check(D=17, N=100)
    assert "nparticles" in check(N=3) and "nparticles" in check(N=(1 << 20) + 1, M=1 << 21)
    assert "generations" in check(G=0) and "generations" in check(G=1 << 24)
    assert "max_draws" in check(M=9) and "max_draws" in check(M=(1 << 32) + 1)
    assert "scale" in check(scale=0.0) and "scale" in check(scale=math.nan) and "scale" in check(scale=-1.0)
    assert "min_rate" in check(min_rate=math.nan)
    assert "kernel" in check(kernel=2)
    assert "q outside" in check(q=0.0) and "q outside" in check(q=1.0) and "q outside" in check(q=math.nan)
    assert check(adaptive=0, q=7.0) == "ok"              # (q belongs to the adaptive schedule)
    assert "NaN" in check(eps0=math.nan) and "NaN" in check(target=math.nan)
