"""ABC population Monte Carlo restated on the CPU oracle alone (helper of tests/test_abc_pmc_*.py and
tests/test_gpu_abc_pmc.py), from the words of include/kabc.h ("ABC population Monte Carlo on the device"), step by
step and in its order of operations.  Only primitives oracle/oracle.py exposes are used: stream_block,
math_vec("u01" | "normal_pair" | "exp" | "sqrt"), push_p, factored_logpdf, cost_eval(..., t=g, walker=r,
domain=DOM_EVAL_COST), quantile, and tests/abc_reject_oracle.py for generation 0.  Every sum runs in the stated
order from 0.0; numpy is used elementwise only (one IEEE operation per element, no reductions)."""
import math

import numpy as np

from abc_reject_oracle import oracle_table

CHUNK = 256
STOPS = ("done", "exhausted", "degenerate", "target", "stalled", "min_rate", "cancelled")


# ---- step 1 -------------------------------------------------------------------------------------
def moments(theta, w):
    """mu [D], c [D][D]: sums over i ascending"""
    N, D = theta.shape
    mu = np.zeros(D)
    for i in range(N):
        mu = mu + w[i] * theta[i]
    c = np.zeros((D, D))
    for i in range(N):
        d = theta[i] - mu
        c = c + (w[i] * d)[:, None] * d[None, :]
    return mu, c


def proposal_cov(c, scale, kernel):
    s = scale * c
    if kernel == "diag":
        s = np.where(np.eye(c.shape[0], dtype=bool), s, 0.0)
    return s


# ---- step 2: kabc_mvn_prepare of include/kabc_mvnormal.h ------------------------------------------
def mvn_prepare(orc, cov):
    """(rc, L, W): rc 0 ok, 1 not symmetric, 2 not positive definite"""
    D = cov.shape[0]
    L, W = np.zeros((D, D)), np.zeros((D, D))
    for i in range(D):
        for j in range(D):
            a, b = float(cov[i, j]), float(cov[j, i])
            m = max(abs(a), abs(b))
            if not abs(a - b) <= 1e-12 * m:
                return 1, L, W
    for i in range(D):
        for j in range(i + 1):
            s = float(cov[i, j])
            for k in range(j):
                s = s - L[i, k] * L[j, k]
            if i == j:
                if not s > 0.0 or not math.isfinite(s):
                    return 2, L, W
                L[i, i] = orc.math_vec("sqrt", np.array([s]))[0]
            else:
                L[i, j] = s / L[j, j]
    for c in range(D):
        W[c, c] = 1.0 / L[c, c]
        for i in range(c + 1, D):
            s = 0.0
            for k in range(c, i):
                s = s + L[i, k] * W[k, c]
            W[i, c] = -s / L[i, i]
    return 0, L, W


# ---- step 3 -------------------------------------------------------------------------------------
def cdf_of(w):
    out, s = np.empty(len(w)), 0.0
    for j in range(len(w)):
        s = s + float(w[j])
        out[j] = s
    return out


# ---- step 4 -------------------------------------------------------------------------------------
def _words64(orc, seed, r, g, slot, cd):
    b = orc.stream_block(seed, r, g, slot, cd.DOM_PMC_MOVE)
    return (b[1] << 32) | b[0], (b[3] << 32) | b[2]


def proposals(orc, theta, cdf, L, seed, g, rows):
    """(x [n][D] before push_p, ancestors [n]) of the proposal rows `rows` of generation g"""
    from kissabc_jl_amd import _cdefs as cd
    N, D = theta.shape
    n, npair = len(rows), (D + 1) // 2
    lo0 = np.array([_words64(orc, seed, r, g, 0, cd)[0] for r in rows], dtype=np.uint64)
    u = orc.math_vec("u01", lo0.view(np.float64))
    target = u * cdf[N - 1]
    anc = np.minimum(np.searchsorted(cdf, target, side="right"), N - 1)   # #{j : cdf_j <= target}, at most N - 1
    words = np.array([_words64(orc, seed, r, g, 1 + m, cd) for r in rows for m in range(npair)], dtype=np.uint64)
    z = orc.math_vec("normal_pair", words.reshape(-1).view(np.float64)).reshape(n, 2 * npair)
    x = np.empty((n, D))
    for k in range(D):
        acc = np.zeros(n)
        for m in range(k + 1):
            acc = acc + L[k, m] * z[:, m]
        x[:, k] = theta[anc, k] + acc
    return x, anc


def generation(orc, prior, cost, theta, w, L, eps, seed, g, N, max_draws, batch=512):
    """steps 4-5: the first N accepted proposal rows of generation g in index order, or None (exhausted);
    returns (theta', C, lp, index, draws)"""
    from kissabc_jl_amd import _cdefs as cd
    cdf = cdf_of(w)
    P_, C_, lp_, idx_ = [], [], [], []
    r0 = 0
    while r0 < max_draws and len(idx_) < N:
        rows = range(r0, min(max_draws, r0 + batch))
        x, _ = proposals(orc, theta, cdf, L, seed, g, rows)
        P = orc.push_p(prior, x)
        lp = orc.factored_logpdf(prior, P)
        for j, r in enumerate(rows):
            if not math.isfinite(lp[j]):
                continue                                     # (counted as a draw, never simulated)
            c = orc.cost_eval(cost, P[j], seed=seed, walker=r, t=g, domain=cd.DOM_EVAL_COST)
            if c <= eps:                                     # (NaN <= eps is False)
                P_.append(P[j]); C_.append(c); lp_.append(lp[j]); idx_.append(r)
                if len(idx_) == N:
                    break
        r0 = rows[-1] + 1
    if len(idx_) < N:
        return None
    return np.array(P_), np.array(C_), np.array(lp_), np.array(idx_, dtype=np.int64), idx_[-1] + 1


# ---- step 6 -------------------------------------------------------------------------------------
def whiten(theta, mu, W):
    n, D = theta.shape
    y = np.empty((n, D))
    for k in range(D):
        z = np.zeros(n)
        for j in range(k + 1):
            z = z + W[k, j] * (theta[:, j] - mu[j])
        y[:, k] = z
    return y


def kernel_sums(orc, y_new, y_anc, w_anc):
    """S_i = sum over chunks c of 256 ancestors (ascending) of P_ic = sum_{j in c, ascending} w_j exp(-0.5 d2_ij)"""
    n, D = y_new.shape
    m = y_anc.shape[0]
    S = np.zeros(n)
    for c0 in range(0, m, CHUNK):
        ya = y_anc[c0:c0 + CHUNK]
        d2 = np.zeros((n, ya.shape[0]))
        for k in range(D):
            t = y_new[:, k][:, None] - ya[:, k][None, :]
            d2 = d2 + t * t
        E = orc.math_vec("exp", (-0.5 * d2).reshape(-1)).reshape(d2.shape)
        P = np.zeros(n)
        for j in range(ya.shape[0]):
            P = P + w_anc[c0 + j] * E[:, j]
        S = S + P
    return S


def weights_from_sums(orc, lp, S):
    """(w, ess) or None (degenerate)"""
    if not np.all(np.isfinite(S) & (S > 0.0)):
        return None
    with np.errstate(over="ignore"):
        v = orc.math_vec("exp", lp - np.max(lp)) / S
    tot = 0.0
    for x in v:
        tot = tot + float(x)
    if not (tot > 0.0 and math.isfinite(tot)):
        return None
    w = v / tot
    return w, ess_of(w)


def ess_of(w):
    s2 = 0.0
    for x in w:
        s2 = s2 + float(x) * float(x)
    return 1.0 / s2


# ---- the schedule and the stop rules ---------------------------------------------------------------
def after_generation(orc, g, eps_g, draws_g, C, N, eps, q, eps_target, generations, min_rate):
    """(stop name, None) when the run ends with generation g, else (None, eps of generation g + 1)"""
    adaptive = eps is None
    if adaptive and eps_g <= eps_target:
        return "target", None
    if g + 1 == generations:
        return "done", None
    if N / draws_g < min_rate:
        return "min_rate", None
    if not adaptive:
        return None, float(eps[g + 1])
    Q = orc.quantile(C, q)
    e = eps_target if Q < eps_target else Q
    if math.isnan(e) or (g + 1 >= 2 and e >= eps_g):
        return "stalled", None
    return None, e


# ---- the run -----------------------------------------------------------------------------------
def oracle_pmc(orc, prior, cost, N, *, eps=None, q=None, eps0=math.inf, eps_target=-math.inf, generations=None,
               kernel="full", scale=2.0, max_draws=None, min_rate=0.0, seed=0):
    """abc_pmc's result from the oracle: dict(theta, w, C, logprior, index, eps, log, stop, generations_run)"""
    from kissabc_jl_amd.distributions import as_factored
    prior = as_factored(prior)
    D = len(prior)
    if eps is not None:
        eps = [float(e) for e in eps]
        generations = len(eps)
    else:
        q = 0.5 if q is None else q
        generations = 20 if generations is None else generations
    max_draws = min(1 << 32, 10_000 * N) if max_draws is None else max_draws
    out = dict(theta=np.empty((0, D)), w=np.empty(0), C=np.empty(0), logprior=np.empty(0),
               index=np.empty(0, dtype=np.int64), eps=math.nan, log=[], stop="done", generations_run=0)
    # generation 0: abc_reject in threshold mode, the table grown batch by batch
    eps_g = eps[0] if eps is not None else float(eps0)
    P_, lp_, C_, r0 = [], [], [], 0
    idx = np.empty(0, dtype=np.int64)
    while r0 < max_draws and idx.size < N:
        n = min(1024, max_draws - r0)
        P, lp, C = oracle_table(orc, prior, cost, n, seed, r0)
        P_.append(P); lp_.append(lp); C_.append(C)
        r0 += n
        with np.errstate(invalid="ignore"):
            idx = np.flatnonzero(np.concatenate(C_) <= eps_g)[:N]
    if idx.size < N:
        out["stop"] = "exhausted"
        return out
    theta, lp, C = np.concatenate(P_)[idx], np.concatenate(lp_)[idx], np.concatenate(C_)[idx]
    w = np.full(N, 1.0 / N)
    index, draws = idx.astype(np.int64), int(idx[-1]) + 1
    g = 0
    while True:
        out.update(theta=theta, w=w, C=C, logprior=lp, index=index, eps=eps_g, generations_run=g + 1)
        out["log"].append(dict(eps=eps_g, draws=draws, ess=ess_of(w)))
        stop, eps_next = after_generation(orc, g, eps_g, draws, C, N, eps, q, eps_target, generations, min_rate)
        if stop is not None:
            out["stop"] = stop
            return out
        g, eps_g = g + 1, eps_next
        mu, c = moments(theta, w)
        rc, L, W = mvn_prepare(orc, proposal_cov(c, scale, kernel))
        if rc != 0:
            out["stop"] = "degenerate"
            return out
        new = generation(orc, prior, cost, theta, w, L, eps_g, seed, g, N, max_draws)
        if new is None:
            out["stop"] = "exhausted"
            return out
        theta_n, C_n, lp_n, index_n, draws_n = new
        S = kernel_sums(orc, whiten(theta_n, mu, W), whiten(theta, mu, W), w)
        ww = weights_from_sums(orc, lp_n, S)
        if ww is None:
            out["stop"] = "degenerate"
            return out
        theta, C, lp, index, draws, w = theta_n, C_n, lp_n, index_n, draws_n, ww[0]
