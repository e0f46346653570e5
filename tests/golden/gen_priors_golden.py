#!/usr/bin/env python3
"""Generates tests/golden/priors_logpdf.json with scipy.stats.

The reference evaluates prior densities through Distributions.jl
(src/priors.jl:18-36), which is not in the reference tree and cannot run
here (no Julia).  These vectors pin our restatement of each family against an
independent implementation (scipy 1.15; the edge cases at the end: mpmath at 50
digits, with scipy checked against it).  Run: python tests/golden/gen_priors_golden.py
"""
import json
import os

import mpmath as mp
import numpy as np
from scipy import stats

rng = np.random.default_rng(20261002)
out = {"generator": "scipy.stats " + __import__("scipy").__version__ + ", mpmath " + mp.__version__,
       "cases": []}


def add(kind, params, xs, logpdf):
    out["cases"].append({"kind": kind, "params": [float(p) for p in params],
                         "x": [float(v) for v in xs],
                         "logpdf": [float(v) if np.isfinite(v) else ("-inf" if v < 0 else "inf")
                                    for v in logpdf]})


# Uniform(a,b)
for a, b in [(0, 1), (-5, 5), (100, 101), (1, 3), (0, 4)]:
    xs = np.concatenate([rng.uniform(a - 1, b + 1, 12), [a, b, a - 1e-9, b + 1e-9]])
    add("Uniform", (a, b), xs, stats.uniform(a, b - a).logpdf(xs))
# Normal(mu,sigma)
for mu, s in [(0, 1), (0, 5), (1, 0.2), (1, 0.5), (-3.5, 12.0)]:
    xs = rng.normal(mu, 3 * s, 16)
    add("Normal", (mu, s), xs, stats.norm(mu, s).logpdf(xs))
# Truncated(Normal(mu,sigma), lo, hi)
for mu, s, lo, hi in [(0, 0.1, 0, 100), (0, 0.05, 0, 100), (1, 2, -1, 4), (0, 1, 2, 5)]:
    xs = np.concatenate([rng.uniform(lo - 0.5, min(hi, lo + 6 * s) + 0.5, 14), [lo, hi]])
    add("TruncNormal", (mu, s, lo, hi), xs,
        stats.truncnorm((lo - mu) / s, (hi - mu) / s, loc=mu, scale=s).logpdf(xs))
# Beta(alpha,beta)
for a, b in [(15, 2), (2, 2), (0.5, 0.5), (1, 3), (4.5, 1)]:
    xs = np.concatenate([rng.uniform(0, 1, 14), [-0.1, 1.1, 1e-12, 1 - 1e-12]])
    add("Beta", (a, b), xs, stats.beta(a, b).logpdf(xs))
# DiscreteUniform(a,b)
for a, b in [(1, 2), (1, 10), (0, 0), (-3, 4)]:
    xs = np.concatenate([np.arange(a - 2, b + 3, dtype=float), [a + 0.5]])
    lp = stats.randint(a, b + 1).logpmf(xs)
    add("DiscreteUniform", (a, b), xs, lp)
# NegativeBinomial(r,p)  (socks prior: test/runtests.jl:46-50)
prior_mu, prior_sd = 30.0, 15.0
size = -prior_mu ** 2 / (prior_mu - prior_sd ** 2)
for r, p in [(size, size / (prior_mu + size)), (1, 0.5), (10, 0.9), (0.3, 0.01)]:
    xs = np.concatenate([rng.integers(0, 200, 14).astype(float), [0.0, 1.0, -1.0, 2.5]])
    add("NegativeBinomial", (r, p), xs, stats.nbinom(r, p).logpmf(xs))
# Exponential(theta), Gamma(alpha, theta), LogNormal(mu, sigma)
for th in [1.0, 0.2, 7.5]:
    xs = np.concatenate([rng.exponential(th, 12), [0.0, -1.0]])
    add("Exponential", (th,), xs, stats.expon(scale=th).logpdf(xs))
for a, th in [(1.0, 1.0), (2.5, 0.7), (0.4, 3.0), (30.0, 0.1)]:
    xs = np.concatenate([rng.gamma(a, th, 12), [-1.0]])
    add("Gamma", (a, th), xs, stats.gamma(a, scale=th).logpdf(xs))
for mu, s in [(0, 1), (1.5, 0.3)]:
    xs = np.concatenate([rng.lognormal(mu, s, 12), [0.0, -2.0]])
    add("LogNormal", (mu, s), xs, stats.lognorm(s, scale=np.exp(mu)).logpdf(xs))


# ---- edge cases: references from mpmath at 50 digits (scipy must agree to 1e-13 where it is finite) ----
mp.mp.dps = 50


def mp_add(kind, params, xs, f, scipy_logpdf, scipy_rtol=1e-13):
    """f(x) -> mpmath log-density; scipy_logpdf: the same through scipy, checked against it to
    scipy_rtol (looser only where scipy itself cancels: see the callers)"""
    ref = np.array([float(f(mp.mpf(float(x)))) for x in xs])
    with np.errstate(all="ignore"):
        sc = scipy_logpdf(np.asarray(xs, dtype=float))
    both = np.isfinite(ref) & np.isfinite(sc)
    assert np.array_equal(np.isfinite(ref), np.isfinite(sc)) or kind == "TruncNormal", (kind, params)
    assert np.allclose(sc[both], ref[both], rtol=scipy_rtol, atol=scipy_rtol), (kind, params, sc, ref)
    add(kind, params, xs, ref)


def tn_logmass(za, zb):
    """log(Phi(zb) - Phi(za)) in the tail where it has the most relative precision"""
    if za >= 0:
        return mp.log(mp.ncdf(-za) - mp.ncdf(-zb))
    return mp.log(mp.ncdf(zb) - mp.ncdf(za))


def tn_case(mu, s, lo, hi, scipy_rtol=1e-13):
    za, zb = (mp.mpf(lo) - mu) / s, (mp.mpf(hi) - mu) / s
    lm = tn_logmass(za, zb)
    f = lambda x: (-((x - mu) / s) ** 2 / 2 - mp.log(s * mp.sqrt(2 * mp.pi)) - lm   # noqa: E731
                   if lo <= x <= hi else mp.mpf("-inf"))
    ends = [v for v in (lo, hi) if np.isfinite(v)]
    span_lo = lo if np.isfinite(lo) else hi - 6 * s
    span_hi = hi if np.isfinite(hi) else lo + 6 * s
    if np.isfinite(lo) and not np.isfinite(hi):
        span_hi = lo + s * 5 / max(1.0, float(za))
    if np.isfinite(hi) and not np.isfinite(lo):
        span_lo = hi - s * 5 / max(1.0, -float(zb))
    xs = np.concatenate([rng.uniform(span_lo, span_hi, 6), ends,
                         [np.nextafter(e, -np.inf if e == lo else np.inf) for e in ends]])
    mp_add("TruncNormal", (mu, s, lo, hi), xs, f,
           lambda v: stats.truncnorm((lo - mu) / s, (hi - mu) / s, loc=mu, scale=s).logpdf(v), scipy_rtol)


# scipy's truncnorm (1.15) loses digits beyond |z| ~ 8 (to 5e-13) and in narrow windows (its log-mass
# is a difference of CDFs: 2e-8 at width 1e-9, 2e-6 at 2e-12): there it is only a sanity check
FAR, NARROW = 1e-12, 1e-5


inf = float("inf")
for z in (0.5, 1, 2, 3, 5, 8, 20, 37, 38.5, 40, 60):     # one-sided far tails, both signs
    tn_case(0.0, 1.0, z, inf, 1e-13 if z < 8 else FAR)
    tn_case(0.0, 1.0, -inf, -z, 1e-13 if z < 8 else FAR)
for z in (0.5, 3, 8, 37, 40, 60):                        # two-sided tail windows, both signs
    for w in (1e-3, 0.1, 1, 5):
        tn_case(0.0, 1.0, z, z + w, 1e-13 if z < 8 else FAR)
        tn_case(0.0, 1.0, -z - w, -z, 1e-13 if z < 8 else FAR)
tn_case(2.0, 0.5, 2.0 + 0.5 * 40, 2.0 + 0.5 * 41, FAR)         # beyond erfc's underflow, scaled
for w in (1e-9, 1e-6):                                   # narrow windows: centre, z = 0.5 and 3
    tn_case(0.0, 1.0, -w / 2, w / 2, NARROW)
    for z in (0.5, 3.0):
        tn_case(0.0, 1.0, z, z + w, NARROW)
        tn_case(0.0, 1.0, -z - w, -z, NARROW)
tn_case(0.0, 1.0, -1e-12, 1e-12, NARROW)
for w in (0.01, 0.5, 4.0):                               # windows across the mean
    tn_case(0.0, 1.0, -w / 3, 2 * w / 3)
    tn_case(1.5, 2.0, 1.5 - w, 1.5 + w / 4)

# Beta / Gamma / NegativeBinomial: tiny shapes, x near 0 and 1
xb = [1e-300, 1e-200, 1e-30, 1e-8, 0.3, 0.5, 1 - 1e-8, 1 - 2 ** -52, 1 - 2 ** -53, 0.0, 1.0]
for a, b in [(1e-3, 1e-3), (0.01, 0.01), (1e-3, 2.0), (2.0, 1e-3), (0.5, 0.25)]:
    xs = [x for x in xb if (x > 0 or a >= 1) and (x < 1 or b >= 1)]
    f = lambda x, a=a, b=b: ((a - 1) * mp.log(x) + (b - 1) * mp.log1p(-x) - mp.log(mp.beta(a, b))   # noqa: E731
                             if 0 < x < 1 else mp.mpf("-inf") if (x == 0 and a > 1) or (x == 1 and b > 1)
                             else mp.mpf("nan"))
    mp_add("Beta", (a, b), xs, f, stats.beta(a, b).logpdf)
for a, th in [(1e-3, 1.0), (0.05, 2.0), (0.999999, 1.0), (1.000001, 1.0), (1e-3, 1e-300), (2.0, 1e300)]:
    xs = [v * th for v in (1e-300, 1e-30, 1e-8, 0.5, 3.0) if 0 < v * th < inf] + [-1.0]
    f = lambda x, a=a, th=th: ((a - 1) * mp.log(x) - x / th - mp.loggamma(a) - a * mp.log(th)   # noqa: E731
                               if x > 0 else mp.mpf("-inf"))
    mp_add("Gamma", (a, th), xs, f, stats.gamma(a, scale=th).logpdf)
for r, p in [(0.01, 0.5), (0.01, 1e-9), (1e-3, 0.999999), (1e-3, 1e-9), (1e4, 0.5)]:
    xs = [0.0, 1.0, 2.0, 5.0, 17.0, 60.0]
    f = lambda x, r=r, p=p: (mp.loggamma(x + r) - mp.loggamma(x + 1) - mp.loggamma(r) + r * mp.log(p)   # noqa: E731
                             + x * mp.log1p(-p))
    mp_add("NegativeBinomial", (r, p), xs, f, stats.nbinom(r, p).logpmf)

path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "priors_logpdf.json")
with open(path, "w") as f:
    json.dump(out, f, indent=1)
print("wrote", path, len(out["cases"]), "cases")
