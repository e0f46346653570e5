"""Shared helpers for the test-suite (model builders, golden loaders)."""
import json
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_prior_golden(name="priors_logpdf.json"):
    with open(os.path.join(GOLDEN, name)) as f:
        data = json.load(f)
    for c in data["cases"]:
        c["logpdf"] = np.array([(-np.inf if v == "-inf" else np.inf if v == "inf" else v)
                                for v in c["logpdf"]], dtype=float)
        c["x"] = np.array(c["x"], dtype=float)
    return data["cases"]


def make_dist(k, kind, params):
    return {
        "Uniform": k.Uniform, "Normal": k.Normal, "TruncNormal": k.TruncatedNormal,
        "Beta": k.Beta, "DiscreteUniform": k.DiscreteUniform,
        "NegativeBinomial": k.NegativeBinomial, "Exponential": k.Exponential,
        "Gamma": k.Gamma, "LogNormal": k.LogNormal,
        # run-time compiled families (kabc_compile_prior_plugin)
        "Poisson": k.Poisson, "Laplace": k.Laplace, "TruncatedGamma": k.TruncatedGamma,
    }[kind](*params)


def ulp_diff(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    sp = np.abs(np.nextafter(b, np.inf) - b)
    sp = np.where(sp == 0, 5e-324, sp)
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b) / sp
    return np.where(same, 0.0, d)


# ---- the law of a prior's draws against an independent reference (test_prior_laws.py, test_gpu_prior_laws.py)
class Law:
    """The reference law of one prior component as check_law needs it.

    cdf(t): P(X <= t) for a real t given as an mpmath number (exact midpoints between doubles);
    ppf(q): approximate quantiles (numpy; only used to place the chi^2 bin edges, whose probabilities
    come from cdf); lo, hi: the support; mean, sd, kurt (excess): None where they do not exist or are
    not checked; discrete: integer support (cdf at integers, no rounding of draws)."""

    def __init__(self, cdf, ppf, lo, hi, mean=None, sd=None, kurt=None, discrete=False, sf=None):
        self.cdf, self.ppf, self.lo, self.hi = cdf, ppf, float(lo), float(hi)
        self.sf = sf or (lambda t: 1 - cdf(t))
        self.mean, self.sd, self.kurt, self.discrete = mean, sd, kurt, discrete


def _mid(a, b):
    import mpmath as mp
    return (mp.mpf(float(a)) + mp.mpf(float(b))) / 2


def _rounding_mass(law, v):
    """P(the real draw rounds to the double v) under round-to-nearest (integers for a discrete law)"""
    if law.discrete:
        return float(law.cdf(v) - law.cdf(v - 1))
    up, down = np.nextafter(v, np.inf), np.nextafter(v, -np.inf)
    hi_p = law.sf(_mid(v, up)) if v < law.hi else 0
    lo_p = law.cdf(_mid(down, v)) if v > law.lo else 0
    return float(1 - hi_p - lo_p)


def _count_ok(c, n, p, what):
    """a count of draws against its binomial expectation: 6 standard errors, and a slack of 3
    for the counts of a few that a vanishing p (a birthday collision of doubles) still allows"""
    sd = np.sqrt(n * p * (1 - p))
    assert abs(c - n * p) <= 6 * sd + 3, f"{what}: {c} of {n} draws, expected {n * p:.6g} (sd {sd:.3g})"


def check_law(x, law, label="", nbins=64, p_min=1e-6):
    """The protocol of tests/test_prior_laws.py, correct for doubles, not only for reals:
      * no NaN, nothing outside the support, no infinity (no family here has mass beyond the
        largest double at the parameters tested);
      * point masses: the most frequent value and each finite end of the support appear as often
        as the reference law puts mass on the reals that round to them (6 standard errors) -- a
        plain KS test fails faithful samplers at tiny shapes, where whole percents of the mass round
        to 0 or 1;
      * chi^2 over `nbins` bins with edges at the reference quantiles rounded to doubles, merged
        where they coincide (or hold less than 5 expected draws), probabilities from the reference
        cdf: p > p_min;
      * mean and variance within 6 standard errors where the law gives them."""
    from scipy import stats
    x = np.asarray(x, dtype=np.float64).ravel()
    n = x.size
    assert not np.isnan(x).any(), f"{label}: {np.isnan(x).sum()} NaN draws"
    assert np.isfinite(x).all(), f"{label}: infinite draws"
    assert x.min() >= law.lo and x.max() <= law.hi, f"{label}: draws outside [{law.lo}, {law.hi}]: {x.min()}, {x.max()}"
    if law.discrete:
        assert np.array_equal(x, np.rint(x)), f"{label}: non-integer draws"
    # point masses
    vals, cnt = np.unique(x, return_counts=True)
    i = int(np.argmax(cnt))
    if cnt[i] >= 2 or law.discrete:
        _count_ok(int(cnt[i]), n, _rounding_mass(law, vals[i]), f"{label}: most frequent value {vals[i]!r}")
    for end in (law.lo, law.hi):
        if np.isfinite(end):
            _count_ok(int(np.sum(x == end)), n, _rounding_mass(law, end), f"{label}: draws at the end {end!r}")
    # chi^2 on (merged) quantile bins; a draw equal to an edge counts in the bin above it
    with np.errstate(all="ignore"):
        e = np.asarray(law.ppf(np.arange(1, nbins) / nbins), dtype=np.float64)
    if law.discrete:
        e = np.floor(e) + 1.0                        # bins [e_i, e_{i+1}) of integers
    e = np.unique(e[np.isfinite(e) & (e > law.lo) & (e <= law.hi if law.discrete else e < law.hi)])
    if law.discrete:
        cdf_at = [law.cdf(v - 1) for v in e]
    else:
        cdf_at = [law.cdf(_mid(np.nextafter(v, -np.inf), v)) for v in e]
    probs = np.diff(np.array([0.0] + [float(c) for c in cdf_at] + [1.0]))
    obs = np.bincount(np.searchsorted(e, x, side="right"), minlength=len(probs)).astype(float)
    # merge bins with fewer than 5 expected draws into their neighbour
    P, O = [], []
    for p, o in zip(probs, obs):
        if P and (P[-1] * n < 5 or p * n < 5):
            P[-1] += p
            O[-1] += o
        else:
            P.append(p)
            O.append(o)
    if len(P) > 1 and P[-1] * n < 5:
        P[-2] += P.pop()
        O[-2] += O.pop()
    P, O = np.array(P), np.array(O)
    if len(P) > 1:
        chi2 = float(np.sum((O - n * P) ** 2 / (n * P)))
        pv = stats.chi2(len(P) - 1).sf(chi2)
        assert pv > p_min, f"{label}: chi^2 {chi2:.1f} on {len(P) - 1} dof, p = {pv:.3g}"
    # moments, standardised (scales such as 1e-300 would underflow the squares)
    if law.mean is not None and law.sd is not None and law.sd > 0:
        z = (x - law.mean) / law.sd
        assert abs(z.mean()) <= 6 / np.sqrt(n), f"{label}: mean off by {z.mean() * np.sqrt(n):.2f} SE"
        if law.kurt is not None and np.isfinite(law.kurt):
            se = np.sqrt((law.kurt + 2) / n)
            assert abs(np.mean(z * z) - 1) <= 6 * se, f"{label}: variance off by {(np.mean(z * z) - 1) / se:.2f} SE"


def prior_law(kind, params):
    """Law of make_dist(k, kind, params): mpmath cdfs (40 digits) where scipy's lose the rounding masses
    of tiny shapes and far tails, scipy's where mpmath's series do not converge (shapes >= 100)"""
    import mpmath as mp
    from scipy import special, stats
    mp.mp.dps = 40
    mpf, inf = mp.mpf, float("inf")
    reg = dict(regularized=True)
    if kind == "TruncNormal":
        mu, s, lo, hi = map(float, params)
        za, zb = (mpf(lo) - mu) / s, (mpf(hi) - mu) / s
        right = za >= 0           # in the right tail P(Z > z) keeps the digits, elsewhere P(Z < z)
        F = (lambda z: -mp.ncdf(-z)) if right else mp.ncdf
        Z = F(zb) - F(za)

        def cdf(t):
            z = min(max((mpf(t) - mu) / s, za), zb)
            return (F(z) - F(za)) / Z

        def sf(t):
            z = min(max((mpf(t) - mu) / s, za), zb)
            return (F(zb) - F(z)) / Z
        phi = lambda z: mp.npdf(z) / Z                                        # noqa: E731
        m1 = mp.quad(lambda z: z * phi(z), [za, zb])
        m2 = mp.quad(lambda z: (z - m1) ** 2 * phi(z), [za, zb])
        m4 = mp.quad(lambda z: (z - m1) ** 4 * phi(z), [za, zb])
        ref = stats.truncnorm((lo - mu) / s, (hi - mu) / s, loc=mu, scale=s)
        return Law(cdf, ref.ppf, lo, hi, mean=float(mu + s * m1), sd=float(s * mp.sqrt(m2)),
                   kurt=float(m4 / m2 ** 2 - 3), sf=sf)
    if kind == "Gamma":
        a, th = map(float, params)
        ref = stats.gamma(a, scale=th)
        if a < 100:
            cdf = lambda t: mp.gammainc(a, 0, max(mpf(t), 0) / th, **reg)            # noqa: E731
            sf = lambda t: mp.gammainc(a, max(mpf(t), 0) / th, mp.inf, **reg)        # noqa: E731
        else:
            cdf = lambda t: mpf(special.gammainc(a, max(float(t), 0) / th))          # noqa: E731
            sf = lambda t: mpf(special.gammaincc(a, max(float(t), 0) / th))          # noqa: E731
        return Law(cdf, ref.ppf, 0.0, inf, mean=a * th, sd=math.sqrt(a) * th, kurt=6 / a, sf=sf)
    if kind == "Beta":
        a, b = map(float, params)
        ref = stats.beta(a, b)
        m, v, _, kt = (float(u) for u in ref.stats(moments="mvsk"))
        clip = lambda t: min(max(mpf(t), 0), 1)                                      # noqa: E731
        if max(a, b) < 100:
            cdf = lambda t: mp.betainc(a, b, 0, clip(t), **reg)                      # noqa: E731
            sf = lambda t: mp.betainc(a, b, clip(t), 1, **reg)                       # noqa: E731
        else:
            cdf = lambda t: mpf(special.betainc(a, b, float(clip(t))))               # noqa: E731
            sf = lambda t: mpf(special.betaincc(a, b, float(clip(t))))               # noqa: E731
        return Law(cdf, ref.ppf, 0.0, 1.0, mean=m, sd=math.sqrt(v), kurt=kt, sf=sf)
    if kind == "Exponential":
        th = float(params[0])
        return Law(lambda t: -mp.expm1(-max(mpf(t), 0) / th), stats.expon(scale=th).ppf, 0.0, inf,
                   mean=th, sd=th, kurt=6.0, sf=lambda t: mp.exp(-max(mpf(t), 0) / th))
    if kind == "LogNormal":
        mu, s = map(float, params)
        ref = stats.lognorm(s, scale=np.exp(mu))
        m, v, _, kt = (float(u) for u in ref.stats(moments="mvsk"))
        z = lambda t: (mp.log(mpf(t)) - mu) / s if t > 0 else -mp.inf                # noqa: E731
        return Law(lambda t: mp.ncdf(z(t)), ref.ppf, 0.0, inf, mean=m, sd=math.sqrt(v),
                   kurt=kt if s < 0.5 else None, sf=lambda t: mp.ncdf(-z(t)))
    if kind == "Laplace":
        mu, th = map(float, params)
        cdf = lambda t: (mp.exp((mpf(t) - mu) / th) / 2 if t < mu else 1 - mp.exp(-(mpf(t) - mu) / th) / 2)  # noqa: E731
        return Law(cdf, stats.laplace(mu, th).ppf, -inf, inf, mean=mu, sd=math.sqrt(2) * th, kurt=3.0)
    if kind == "TruncatedGamma":
        a, th, lo, hi = map(float, params)
        G = lambda t: mp.gammainc(a, 0, min(max(mpf(t), lo, 0), hi) / th, **reg)  # noqa: E731
        Z = G(hi) - G(lo)
        g = stats.gamma(a, scale=th)
        ppf = lambda q: g.ppf(g.cdf(lo) + q * (g.cdf(hi) - g.cdf(lo)))              # noqa: E731
        return Law(lambda t: (G(t) - G(lo)) / Z, ppf, max(lo, 0.0), hi, sf=lambda t: (G(hi) - G(t)) / Z)
    # discrete families: cdf at integers (floats are fine: no rounding of the draws)
    if kind == "DiscreteUniform":
        a, b = map(float, params)
        nn = b - a + 1
        cdf = lambda t: mpf(min(max(np.floor(float(t)) - a + 1, 0), nn)) / nn       # noqa: E731
        ppf = lambda q: a + np.floor(q * nn)                                          # noqa: E731
        return Law(cdf, ppf, a, b, mean=(a + b) / 2, sd=math.sqrt((nn * nn - 1) / 12), kurt=-6 * (nn * nn + 1) / (5 * (nn * nn - 1)) if nn > 1 else None, discrete=True)
    if kind in ("Poisson", "NegativeBinomial"):
        ref = stats.poisson(float(params[0])) if kind == "Poisson" else stats.nbinom(*map(float, params))
        m, v, _, kt = (float(u) for u in ref.stats(moments="mvsk"))
        return Law(lambda t: mpf(ref.cdf(float(t))), ref.ppf, 0.0, inf, mean=m, sd=math.sqrt(v), kurt=kt, discrete=True,
                   sf=lambda t: mpf(ref.sf(float(t))))
    raise KeyError(kind)


# ---- one ε-selection of smc (src/smc.jl:131-153), independent of the oracle and the kernels
# (tests/smc_scenarios.py, test_smc_selection_edges.py, test_gpu_smc_selection_edges.py)
def quantile7(v, p):
    """Statistics.quantile(v, p) with its defaults (alpha = beta = 1, "type 7"), from the documented
    definition: aleph = n p + (1 - p), j = trunc(aleph) in [1, n - 1], γ = aleph - j in [0, 1], the
    order statistics a = v(j), b = v(j+1); a + γ(b - a) when both are finite, else (1 - γ)a + γb."""
    s = np.sort(np.asarray(v, dtype=np.float64))
    n = s.size
    if n == 0:
        raise ValueError("collection must be non-empty")
    if np.isnan(s).any():
        raise ValueError("quantiles are undefined in presence of NaNs")
    aleph = float(n) * p + (1.0 - p)
    j = 1 if n == 1 else min(max(int(aleph), 1), n - 1)
    g = min(max(aleph - float(j), 0.0), 1.0)
    a = float(s[j - 1])
    b = float(s[0] if n == 1 else s[j])
    with np.errstate(invalid="ignore"):
        if math.isfinite(a) and math.isfinite(b):
            return float(np.float64(a) + np.float64(g) * (np.float64(b) - np.float64(a)))
        return float((1.0 - np.float64(g)) * np.float64(a) + np.float64(g) * np.float64(b))


NO_ALIVE = "no alive particle to resample from"


def select_step(C, alive, alpha, min_r_ess, N):
    """Step 1 and the decision of step 2 of one smc iteration (src/smc.jl:134-147), by value
    comparisons only: returns (ε, flag, new alive mask, ESS, resample, error).  `error` is
    NO_ALIVE when ESS = 0 and a resample is due (the reference's ceil(Int, N/0) throws)."""
    C = np.asarray(C, dtype=np.float64)
    alive = np.asarray(alive, dtype=bool)
    Xa = C[alive]
    eps = quantile7(Xa, alpha)
    mn = float(Xa.min())
    with np.errstate(invalid="ignore"):
        flag = 0 if eps > mn else 1
        new = (C <= eps) if flag else (C < eps)
    ess = int(new.sum())
    resample = int(alpha * float(ess) <= float(N) * min_r_ess)
    err = NO_ALIVE if (resample and ess == 0) else None
    return eps, flag, new, ess, resample, err


def key_of(x):
    """the kernels' order-preserving key of a double (csrc/smc_kernels.hpp key_of): -0.0 < +0.0"""
    u = np.atleast_1d(np.asarray(x, dtype=np.float64)).view(np.uint64)
    top = np.uint64(1 << 63)
    return np.where(u & top, ~u, u | top)


def _bits(span):
    return int(span).bit_length()


def _narrow(keys, lo, hi, kt):
    """one 1024-bin histogram round of the kernels over the sorted key array `keys` restricted to
    [lo, hi]: the bin of rank kt.  Returns (lo, hi, kt, count, shift)."""
    shift = max(_bits(hi - lo) - 10, 0)
    sel = keys[(keys >= np.uint64(lo)) & (keys <= np.uint64(hi))]
    bins = ((sel - np.uint64(lo)) >> np.uint64(shift)).astype(np.int64)
    cnt = np.bincount(bins, minlength=1024)
    cum = np.cumsum(cnt)
    b = int(np.searchsorted(cum, kt, side="right"))
    before = int(cum[b - 1]) if b else 0
    nlo = lo + (b << shift)
    nhi = min(nlo + (1 << shift) - 1, hi)
    return nlo, nhi, kt - before, int(cnt[b]), shift


def _target(n, alpha):
    aleph = float(n) * alpha + (1.0 - alpha)
    return 1 if n == 1 else min(max(int(aleph), 1), n - 1)


def witness_select(Xa, alpha):
    """the select kernel's narrowing (csrc/smc_kernels.hpp, smc_select_kernel (c)) on the alive costs
    Xa: global 1024-bin rounds until the range holds <= kSelCand = 4096 keys, list rounds until
    <= 64, state 2 (every key of the range equal), needmin (rank j is above the final range) and
    above_scan (needmin, and no listed key lies above the range: X is scanned again).  The phase-by-phase
    course (csrc/smc_dsel_kernels.hpp dsel_*) narrows with the same states: its narrowing rounds are the
    global rounds here, and above_scan is its dsel_above pass."""
    keys = np.sort(key_of(Xa))
    n = keys.size
    j = _target(n, alpha)
    lo, hi, kt, cnt = int(keys[0]), int(keys[-1]), j - 1, n
    out = dict(global_rounds=0, list_rounds=0, state2=False, needmin=False)
    state = 2 if lo == hi else (1 if n <= 4096 else 0)
    while state == 0:
        lo, hi, kt, cnt, shift = _narrow(keys, lo, hi, kt)
        out["global_rounds"] += 1
        state = 2 if shift == 0 else (1 if cnt <= 4096 else 0)
    listed = None
    if state == 1:
        listed = (lo, hi)
        state = 3 if cnt <= 64 else 0
        while state == 0:
            if hi == lo:
                state = 2
                break
            lo, hi, kt, cnt, shift = _narrow(keys, lo, hi, kt)
            out["list_rounds"] += 1
            state = 2 if shift == 0 else (3 if cnt <= 64 else 0)
    out["state2"] = state == 2
    out["needmin"] = n > 1 and kt + 1 >= cnt
    # the key above the final range is looked up among the listed keys; without a list, or with none of
    # them above the range, the costs are scanned again (the phase-by-phase course's dsel_above pass)
    out["above_scan"] = out["needmin"] and (listed is None or not bool(
        ((keys > np.uint64(hi)) & (keys <= np.uint64(listed[1]))).any()))
    return out


def loop_key(x):
    """the loop and one-workgroup kernels' key: -0.0 folded onto +0.0 (key_of(x + 0.0))"""
    return key_of(np.asarray(x, dtype=np.float64) + 0.0)


def witness_loop(C, alive, alpha, eps_1, eps_2):
    """the persistent loop kernel's selection (csrc/smc_loop_kernel.hpp) of an iteration whose two
    previous ε are eps_1 (last) and eps_2 (None: fewer than two): whether the predicted window
    [key(ε) - max(8 d, 4096), key(ε)] held the target rank ("hit") or missed, the histogram rounds,
    whether a round's bin held more than kLoopCand = 512 alive keys, and the candidate count of the
    final bin (alive and dead particles: over kLoopCandCap = 1024 it is error 4)."""
    C = np.asarray(C, dtype=np.float64)
    alive = np.asarray(alive, dtype=bool)
    kall = loop_key(C)
    keys = np.sort(kall[alive])
    n = keys.size
    kt = _target(n, alpha) - 1
    out = dict(pred=False, hit=False, rounds=0, over512=False, ncand=0, state2=False)
    lo, hi = int(keys[0]), int(keys[-1])
    have = None
    if eps_2 is not None and math.isfinite(eps_1) and math.isfinite(eps_2):
        out["pred"] = True
        whi = int(loop_key(eps_1)[0])
        kp = int(loop_key(eps_2)[0])
        d = min(kp - whi if kp > whi else 1, 1 << 56)
        span = max(d * 8, 4096)
        wlo = whi - span if whi > span else 0
        below, above = int((keys < np.uint64(wlo)).sum()), int((keys > np.uint64(whi)).sum())
        if above == 0 and kt >= below:
            out["hit"] = True
            lo, hi, kt, have = wlo, whi, kt - below, True
    state = 0
    while state == 0:
        if lo == hi:
            state = 2
            break
        lo, hi, kt, cnt, shift = _narrow(keys, lo, hi, kt)
        out["rounds"] += 1
        if shift == 0:
            state = 2
        elif cnt <= 512:
            state = 1
        else:
            out["over512"] = True
    out["state2"] = state == 2
    if state == 1:
        out["ncand"] = int(((kall >= np.uint64(lo)) & (kall <= np.uint64(hi))).sum())
    return out


def witness_dsel2(Xa, alpha, eps_1, eps_2, eps_now, N):
    """the one-exchange course's stall reason (csrc/smc_dsel_kernels.hpp dsel2_*) for an iteration of a
    single-rank run of N > kDselStage = 4096 particles whose two previous ε are eps_1 (last) and eps_2:
    1 no window (d = eps_2 - eps_1 not > 0 or not finite), 2 the window holds more alive keys than the
    payload slot (max(4096, N / 8)), 3 the target rank outside the window [key(eps_1 - 1.4 d),
    key(eps_1 - 0.65 d)], 5 the target's bin holds more than kSelCand = 4096 keys, 7 the selected ε is 0.
    0: the course decided.  (7 is also raised when needmin finds no key above the final range: not
    modelled.)"""
    keys = np.sort(key_of(Xa))
    n = keys.size
    e1, e0 = float(eps_1), float(eps_2)
    with np.errstate(invalid="ignore", over="ignore"):
        d = e0 - e1
    if not (math.isfinite(e1) and math.isfinite(d) and d > 0.0):
        return 1
    wlo, whi = int(key_of(e1 - 1.4 * d)[0]), int(key_of(e1 - 0.65 * d)[0])
    if wlo > whi:
        return 1
    below = int((keys < np.uint64(wlo)).sum())
    inside = int(((keys >= np.uint64(wlo)) & (keys <= np.uint64(whi))).sum())
    if inside > max(4096, (N // 8 + 1) & ~1):      # the payload slot's capacity (capi_smc.hip spec_cap)
        return 2
    kt = _target(n, alpha) - 1 - below
    if kt < 0 or kt >= inside:
        return 3
    _, _, _, cnt, _ = _narrow(keys, wlo, whi, kt)
    if cnt > 4096:
        return 5
    if eps_now == 0.0:
        return 7
    return 0


# ---- the re-draw loop of the initial population (src/smc.jl:351-366 ABCDE, :280-294 pfilter):
# cases in which rows of the first draw are rejected and drawn again (test_abcde.py, test_pfilter.py,
# test_gpu_abcde_batch.py, test_gpu_pfilter_batch.py)
REDRAW_SEED = 7


def redraw_case(k, p_inf=0.5):
    """NoisyBanana(0.5) returns +Inf with probability 1/2 from the cost's own stream: about half of the
    rows of the initial population are drawn again, some of them several times.  p_inf = 0: the same
    problem without re-draws."""
    return k.Factored(k.Normal(0, 5), k.Normal(0, 5)), k.costs.NoisyBanana(p_inf)


REDRAW_USER_SRC = """
KABC_HD double kabc_user_cost(const double* x, int D, const double* params, const double* data,
                              int64_t ndata, kabc_cost_rng_t* rng) {
    // params[1] > 0: no finite distance on the half space x[0] < 0
    if (params[1] > 0.0 && x[0] < 0.0) return KABC_INF;
    double s = 0.0;
    for (int k = 0; k < D; ++k) s += kabc_fabs(x[k] - params[0]);
    return s;
}
"""


def redraw_user_case(k, orc, inf_branch=True, D=17):
    """the run-time-dimension kernels (length(prior) > 16) with a user cost that is +Inf on half of the
    prior's mass; inf_branch = False: the same cost without that branch"""
    cost = k.costs.UserCost(REDRAW_USER_SRC, dims=[D], params=[0.5, 1.0 if inf_branch else 0.0],
                            name="redraw_half_space")
    orc.register_user_cost(cost)
    return k.Factored(*[k.Normal(0, 2)] * D), cost


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def assert_redraws_happen(run0, case, case_plain):
    """run0(prior, cost) -> the oracle's initial population (generations = 0 / max_iters = 0): the case is
    informative when at least one of its rows differs from the row drawn without the Inf branch"""
    with_inf, plain = run0(*case)["P"], run0(*case_plain)["P"]
    assert with_inf.shape == plain.shape
    changed = int(np.any(with_inf.view(np.uint64) != plain.view(np.uint64), axis=1).sum())
    assert changed >= 1, "no row of the initial population was drawn again"
    return changed


# ---- one generation of ABCDE (src/smc.jl:371-414) and one iteration of pfilter (:297-333) on a table cost
# (tests/population_scenarios.py), written from the reference and the documented stream layout
# (include/kabc_philox.h, the comments of csrc/population_model.hpp), not from the oracle or the kernels
# (test_population_cost_edges.py, test_gpu_population_cost_edges.py)
def philox_py(ctr, key, rounds):
    """Philox4x32-R written a third time, from the published round function (Salmon et al. SC'11):
    multiply two counter words by the two constants, swap / xor with the round key, bump the key."""
    x, kk = list(ctr), list(key)
    M0, M1, W0, W1, mask = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xffffffff
    for r in range(rounds):
        if r:
            kk = [(kk[0] + W0) & mask, (kk[1] + W1) & mask]
        p0, p1 = M0 * x[0], M1 * x[2]
        x = [(p1 >> 32) ^ x[1] ^ kk[0], p1 & mask, (p0 >> 32) ^ x[3] ^ kk[1], p0 & mask]
    return x


DOM_ABCDE_INIT, DOM_ABCDE_MOVE, DOM_PF_INIT, DOM_PF_MOVE = 9, 11, 13, 15     # (include/kabc_philox.h)


def stream_blocks(seed, walkers, t, slot, domain, rounds):
    """philox_py over an array of walkers: the block (seed, walker, t, slot, domain) of each as its two 64-bit
    words (lo, hi).  counter = (walker, t lo32, slot, domain | t hi24 << 8), key = (seed lo32, seed hi32);
    uint64 arithmetic holds the product of two 32-bit words."""
    u, mask, s32 = np.uint64, np.uint64(0xffffffff), np.uint64(32)
    w = np.asarray(walkers, dtype=np.uint64)
    t = int(t)
    x = [w.copy(), np.full_like(w, t & 0xffffffff), np.full_like(w, slot), np.full_like(w, domain | ((t >> 32) << 8))]
    k0, k1 = seed & 0xffffffff, seed >> 32
    for r in range(rounds):
        if r:
            k0, k1 = (k0 + 0x9E3779B9) & 0xffffffff, (k1 + 0xBB67AE85) & 0xffffffff
        p0, p1 = u(0xD2511F53) * x[0], u(0xCD9E8D57) * x[2]
        x = [(p1 >> s32) ^ x[1] ^ u(k0), p1 & mask, (p0 >> s32) ^ x[3] ^ u(k1), p0 & mask]
    return (x[1] << s32) | x[0], (x[3] << s32) | x[2]


def stream_index(r, n):
    """kabc_index: floor(r n / 2^64) of each 64-bit word, in Python integers; n a count or one per word"""
    n = np.broadcast_to(np.asarray(n), np.shape(r))
    return np.array([(int(a) * int(b)) >> 64 for a, b in zip(r, n)], dtype=np.int64)


def jl_max(a, b):
    """Julia's max of two doubles: a NaN is kept, max(-0.0, 0.0) = 0.0"""
    if a != a or b != b:
        return math.nan
    if a == b:
        return b if math.copysign(1.0, a) < 0 else a
    return a if a > b else b


def jl_extrema(v):
    """Julia's extrema: (NaN, NaN) with a NaN among the values"""
    v = np.asarray(v, dtype=np.float64)
    if np.isnan(v).any():
        return math.nan, math.nan
    return float(v.min()), float(v.max())


def kth_smallest_of_prefix(seq, r, k):
    """the k[q]-th smallest (from 0) of seq[:r[q]] for every query q, seq a permutation of 0 .. n - 1: the
    queries walk the bits of the answer from the top, the sequence stably partitioned by each bit in turn
    (test_population_cost_edges.py checks it against np.sort(seq[:r])[k])"""
    cur = np.asarray(seq, dtype=np.int64)
    lo, hi, k = np.zeros(len(r), dtype=np.int64), np.array(r, dtype=np.int64), np.array(k, dtype=np.int64)
    ans = np.zeros(len(r), dtype=np.int64)
    for bit in range(max(1, int(cur.size - 1).bit_length()) - 1, -1, -1):
        one = ((cur >> bit) & 1).astype(bool)
        z = np.concatenate([[0], np.cumsum(~one)])        # zeros among cur[:p]
        zl, zh = z[lo], z[hi]
        up = k >= zh - zl                                 # the answer has this bit set
        k = np.where(up, k - (zh - zl), k)
        lo, hi = np.where(up, z[-1] + lo - zl, zl), np.where(up, z[-1] + hi - zh, zh)
        ans |= up.astype(np.int64) << bit
        cur = np.concatenate([cur[~one], cur[one]])
    return ans


class TableProblem:
    """cost(x) = table[x[0]] under x[0] ~ DiscreteUniform(0, M - 1), as population_scenarios.SOURCE computes it:
    the index is x[0] truncated towards zero and clamped; push_p rounds to nearest-even (src/types.jl:29-32)
    and the log-prior is `lp0` on the integers 0 .. M - 1 and -Inf elsewhere.  normal_pairs: the library's
    Box-Muller of two stream words (the oracle's orc.normal_pairs), used for pfilter's scale only."""

    def __init__(self, table, lp0, seed, rounds, normal_pairs):
        self.table = np.asarray(table, dtype=np.float64)
        self.M, self.lp0, self.seed, self.rounds, self.normal_pairs = self.table.size, float(lp0), int(seed), rounds, normal_pairs

    def cost(self, x):
        return self.table[np.clip(np.trunc(x), 0, self.M - 1).astype(np.int64)]

    def in_support(self, x):
        r = np.rint(x)
        return (r >= 0) & (r <= self.M - 1)


def abcde_step(pb, st, *, eps_target, alpha, earlystop, proposal_width=1.0):
    """One pass of the loop of src/smc.jl:371-420 on the state st = dict(theta [N], C, logpi, generation,
    nsims): the next state (a new dict; "broke": the earlystop break of :377-379, which moves nothing and
    draws nothing) with "w", the witnesses of what the generation met.

    The draws of particle i in generation g = st["generation"] + 1 are the blocks 0 and 1 of the stream
    (seed, i, g, DOM_ABCDE_MOVE): block 0 lo the donor's position among (1:N)[Δs .<= Δs[i]], block 0 hi the
    partner a among the N - 1 others of s, block 1 lo the partner b among the N - 2 others of s and a (an
    index at or above an excluded one moves up by one), block 1 hi the uniform of :403.  With this prior
    w_prior is 0 or -Inf (asserted), so log(rand) > min(0, w_prior) is false for 0 -- rand < 1 -- and true
    for -Inf: the uniform's bits decide nothing."""
    th, C, lp = (np.asarray(st[f], dtype=np.float64) for f in ("theta", "C", "logpi"))
    N, g = C.size, st["generation"] + 1
    assert np.all(lp == pb.lp0) and not np.isnan(C).any()
    el, eh = jl_extrema(C)                                                   # :376
    w = dict(n_donor=0, neg_donor=False, zero_needs_donor=False, tie_frac=0.0, inf_eval=False, nan_refused=0,
             neg_inf_state=bool(np.isneginf(C).any()), eps_pop_nan=False, span_overflow=False)
    if earlystop and eh <= eps_target:                                       # :377-379
        return dict(st, broke=True, w=w)
    with np.errstate(over="ignore", invalid="ignore"):
        span = np.float64(eh) - np.float64(el)
        pop = np.float64(el) + np.float64(alpha) * span
    eps_pop = jl_max(float(eps_target), float(pop))                          # :380
    w["eps_pop_nan"] = eps_pop != eps_pop
    w["span_overflow"] = bool(np.isfinite(el) and np.isfinite(eh) and np.isinf(span))
    w["tie_frac"] = float(np.unique(C, return_counts=True)[1].max()) / N
    active = ~(C <= eps_target) if earlystop else np.ones(N, dtype=bool)     # :382-384
    eps_i = np.where(C <= eps_target, float(eps_target), eps_pop)            # :388
    with np.errstate(invalid="ignore"):
        need = active & (C > eps_i)                                          # :389
    idx = np.arange(N)
    lo0, hi0 = stream_blocks(pb.seed, idx, g, 0, DOM_ABCDE_MOVE, pb.rounds)
    lo1, _ = stream_blocks(pb.seed, idx, g, 1, DOM_ABCDE_MOVE, pb.rounds)
    s = idx.copy()
    who = np.flatnonzero(need)                                               # :390
    if who.size:    # (1:N)[Δs .<= Δs[i]] is the first `count` entries of the stable order by cost, in index order
        order = np.argsort(C, kind="stable")
        count = np.searchsorted(C[order], C[who], side="right")
        s[who] = kth_smallest_of_prefix(order, count, stream_index(lo0[who], count))
    w["n_donor"] = int(need.sum())
    w["neg_donor"] = bool(need.any() and el < 0)         # (the donors' set holds the minimum)
    zeros = C == 0.0
    w["zero_needs_donor"] = bool((need & zeros).any() and np.signbit(C[zeros]).any() and not np.signbit(C[zeros]).all())
    a = stream_index(hi0, N - 1)                                             # :392-395
    a += a >= s
    b = stream_index(lo1, N - 2)                                             # :396-399
    first, second = np.minimum(a, s), np.maximum(a, s)
    b += b >= first
    b += b >= second
    gamma = proposal_width * 2.38 / math.sqrt(2.0 * 1)                       # :368, length(prior) = 1
    tp = th[s] + (th[a] - th[b]) * gamma                                     # :400
    ok = pb.in_support(tp)
    lpp = np.where(ok, pb.lp0, -np.inf)                                      # :401
    go = active & ok                                                         # :402-403
    dp = pb.cost(tp)                                                         # :405
    with np.errstate(invalid="ignore"):
        acc = go & (dp <= np.maximum(eps_i, C))                              # :406 (np.maximum keeps a NaN, as Julia's max)
    w["inf_eval"] = bool((go & np.isposinf(dp)).any())
    w["nan_refused"] = int((go & np.isnan(dp)).sum())
    assert not (acc & np.isnan(dp)).any()
    return dict(theta=np.where(acc, tp, th), C=np.where(acc, dp, C), logpi=np.where(acc, lpp, lp), generation=g,
                nsims=st["nsims"] + int(go.sum()), broke=False, w=w)


def pfilter_step(pb, st, *, q, proposal_width=0.75):
    """One pass of the loop of src/smc.jl:297-333 on the state st = dict(theta [N], C, logpi, iteration,
    nreps, cost_evals): the next state with this iteration's "eps", "eff", "nok", "nbad" and "max_attempts".
    quantile7 raises ValueError on a NaN cost, as Statistics.quantile does.

    Attempt k (from 0) of particle i in iteration it = st["iteration"] + 1 draws from the blocks 0..2 of the
    stream (seed, i, (it << 24) | k, DOM_PF_MOVE): block 0 lo the position of b in idxok, block 0 hi that of c
    among the others of b, block 1 lo that of d among the others of b and c, block 1 hi the uniform of :316
    (deciding nothing here, as in abcde_step), block 2 the normal pair whose first is randn.  The bad
    particles read ok particles only and write themselves only, so their order does not matter."""
    th, C, lp = (np.array(st[f], dtype=np.float64) for f in ("theta", "C", "logpi"))
    it = st["iteration"] + 1
    assert np.all(lp == pb.lp0)
    eps = quantile7(C, q)                                                    # :299
    with np.errstate(invalid="ignore"):
        bad = C > eps                                                        # :300
    idxok, pending = np.flatnonzero(~bad), np.flatnonzero(bad)               # :301-302
    nok, nbad = idxok.size, pending.size
    nreps = evals = attempt = 0
    while pending.size:
        assert nok >= 3, "b, c and d cannot be distinct: the reference never leaves :309-311"
        assert attempt < 1 << 24
        t = (it << 24) | attempt
        lo0, hi0 = stream_blocks(pb.seed, pending, t, 0, DOM_PF_MOVE, pb.rounds)
        lo1, _ = stream_blocks(pb.seed, pending, t, 1, DOM_PF_MOVE, pb.rounds)
        lo2, hi2 = stream_blocks(pb.seed, pending, t, 2, DOM_PF_MOVE, pb.rounds)
        jb = stream_index(lo0, nok)                                          # :309-311
        jc = stream_index(hi0, nok - 1)
        jc += jc >= jb
        first, second = np.minimum(jb, jc), np.maximum(jb, jc)
        jd = stream_index(lo1, nok - 2)
        jd += jd >= first
        jd += jd >= second
        b, c, d = idxok[jb], idxok[jc], idxok[jd]
        z = pb.normal_pairs(np.stack([lo2, hi2], axis=1).ravel())[:, 0]
        p = th[b] + (th[d] - th[c]) * (z * proposal_width)                   # :312
        nreps += pending.size                                                # :313
        ok = pb.in_support(p)                                                # :315-318
        Cp = pb.cost(p)                                                      # :319
        evals += int(ok.sum())
        with np.errstate(invalid="ignore"):
            done = ok & ~(Cp > eps)                                          # :320-322
        i = pending[done]
        th[i], C[i], lp[i] = p[done], Cp[done], pb.lp0                       # :323-325
        pending = pending[~done]
        attempt += 1
    eff = nbad / nreps if nreps else math.nan                                # :328 (0/0)
    return dict(theta=th, C=C, logpi=lp, iteration=it, nreps=st["nreps"] + nreps, cost_evals=st["cost_evals"] + evals,
                eps=eps, eff=eff, nok=nok, nbad=nbad, max_attempts=attempt)
