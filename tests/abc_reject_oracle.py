"""Rejection ABC restated on the CPU oracle alone (helper of tests/test_abc_reject_args.py and
tests/test_gpu_abc_reject.py).  The contract (include/kabc.h, kabc_abc_reject): row i is row i of the pilot
simulation -- theta_i = push_p(prior, rand(prior)) from (seed, walker = first_row + i, DOM_EVAL_DRAW), its
log-prior, its cost under (seed, walker = first_row + i, t = 0, DOM_EVAL_COST) -- and a result is a SELECTION of
rows of that table.  The table is built from oracle.factored_rand, push_p, factored_logpdf and cost_eval only;
the two selections are plain numpy on the table's cost column, so they also apply to a table that
prior_predictive made."""
import numpy as np


def oracle_table(orc, prior, cost, draws, seed=0, first_row=0):
    """(P [draws][D], logprior [draws], C [draws]) of the first `draws` rows"""
    from kissabc_jl_amd import _cdefs as cd
    P = orc.push_p(prior, orc.factored_rand(prior, draws, seed, domain=cd.DOM_EVAL_DRAW, first_walker=first_row))
    lp = orc.factored_logpdf(prior, P)
    C = np.array([orc.cost_eval(cost, P[i], seed=seed, walker=first_row + i, t=0, domain=cd.DOM_EVAL_COST)
                  for i in range(draws)], dtype=np.float64)
    return P, lp, C


def select_threshold(C, eps, n):
    """threshold mode on a table of len(C) = max_draws rows: (index, draws, exhausted)"""
    C = np.asarray(C, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        idx = np.flatnonzero(C <= eps)[:n]          # (NaN <= eps is False: a NaN cost never accepts)
    if idx.size == n:
        return idx, (int(idx[-1]) + 1 if n else 0), False
    return idx, C.size, True


def select_keep(C, k):
    """keep mode on a table of len(C) = N rows: (index in index order, eps = the largest kept cost)"""
    C = np.asarray(C, dtype=np.float64)
    cand = np.flatnonzero(~np.isnan(C))
    order = np.lexsort((cand, C[cand]))             # by (C, i): ties go to the lower index
    idx = np.sort(cand[order[:k]])
    return idx, (float(np.max(C[idx])) if idx.size else float("nan"))


def oracle_reject(orc, prior, cost, eps=None, n=None, draws=None, keep=None, seed=0, first_row=0):
    """abc_reject's (P, C, logprior, eps, index, draws, exhausted) from the oracle; threshold mode needs `draws`
    (the budget) too: the table has to end somewhere"""
    P, lp, C = oracle_table(orc, prior, cost, draws, seed, first_row)
    if keep is not None:
        idx, e = select_keep(C, keep)
        return P[idx], C[idx], lp[idx], e, idx, draws, False
    idx, d, exhausted = select_threshold(C, eps, n)
    return P[idx], C[idx], lp[idx], float(eps), idx, d, exhausted
