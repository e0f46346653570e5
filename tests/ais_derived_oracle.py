"""The test snippets of the derived quantities g(θ) (include/kabc.h, "user-defined derived quantities") next to
their numpy restatements -- one rounded numpy operation per C operation, nothing fused, so the device's
fp64 result (compiled with -ffp-contract=off) equals the restatement bit for bit -- and the composition with the
three summary oracles: the derived set is, by definition, their result on restatement(trace).

    SNIPPETS[name] = (source, D, G, params, restatement)     restatement(rows [...][D], params) -> [...][G]
    summarize(name, trace, L=0, hist=None)                   the composed oracle on a one-chain trace [gens][N][D]
"""
import numpy as np

import ais_autocorr_oracle as ao
import ais_hist_oracle as ho
import ais_summary_oracle as so

KABC_MAX_DIM = 16

HEAD = "KABC_HD void kabc_user_derived(const double* x, int D, const double* params, int nparams, double* g, int G) {\n"

SRC_A = HEAD + """    const double c = params[0];
    g[0] = x[0] * x[1];
    const double num = x[0] - c;
    const double sq = x[1] * x[1];
    const double den = 1.0 + sq;
    g[1] = num / den;
    g[2] = x[0] > x[1] ? 1.0 : 0.0;
}
"""

SRC_B = HEAD + """    for (int j = 0; j < G; ++j) g[j] = x[j];
}
"""

SRC_C = HEAD + """    double s = 0.0;
    for (int k = 0; k < D; ++k) {
        const double sq = x[k] * x[k];
        s = s + sq;
    }
    g[0] = s;
}
"""

SRC_D = HEAD + """    for (int j = 0; j < G; ++j) {
        const double t = (double)j * x[1];
        g[j] = x[0] + t;
    }
}
"""

SRC_E = HEAD + """    g[0] = x[0] > 0.0 ? x[1] : 0.0 / 0.0;
    g[1] = x[0] > 0.0 ? 1.0 / 0.0 : -1.0 / 0.0;
}
"""


def _rows(x):
    return np.asarray(x, dtype=np.float64)


def restate_a(x, params):
    x = _rows(x)
    c = np.float64(params[0])
    x0, x1 = x[..., 0], x[..., 1]
    g0 = x0 * x1
    num = x0 - c
    sq = x1 * x1
    den = np.float64(1.0) + sq
    g1 = num / den
    g2 = np.where(x0 > x1, 1.0, 0.0)
    return np.stack([g0, g1, g2], axis=-1)


def restate_b(x, params=()):
    return _rows(x).copy()


def restate_c(x, params=()):
    x = _rows(x)
    s = np.zeros(x.shape[:-1])
    for k in range(x.shape[-1]):                  # in index order, the square rounded before it is added
        sq = x[..., k] * x[..., k]
        s = s + sq
    return s[..., None]


def restate_d(x, params=(), G=17):
    x = _rows(x)
    cols = []
    for j in range(G):
        t = np.float64(j) * x[..., 1]
        cols.append(x[..., 0] + t)
    return np.stack(cols, axis=-1)


def restate_e(x, params=()):
    x = _rows(x)
    pos = x[..., 0] > 0.0
    g0 = np.where(pos, x[..., 1], np.nan)
    g1 = np.where(pos, np.inf, -np.inf)
    return np.stack([g0, g1], axis=-1)


# name -> (source, D, G, params, restatement); B is the identity at any D (G = D)
SNIPPETS = {
    "A": (SRC_A, 2, 3, (0.25,), restate_a),
    "B": (SRC_B, None, None, (), restate_b),
    "C": (SRC_C, 20, 1, (), restate_c),
    "D": (SRC_D, 2, 17, (), restate_d),
    "E": (SRC_E, 2, 2, (), restate_e),
}


def restate(name, x, params=None):
    src, D, G, p, fn = SNIPPETS[name]
    return fn(x, p if params is None else params)


def summarize(name, trace, L=0, hist=None, params=None):
    """the derived set of a one-chain trace [gens][N][D]: so / ao's dict over restatement(trace) ("full" up to
    KABC_MAX_DIM derived values, variances beyond), plus "counts" [G][B + 2] with hist = (lo, hi, B), plus
    "g", the mapped trace itself"""
    trace = np.asarray(trace, dtype=np.float64)
    assert trace.ndim == 3
    with np.errstate(invalid="ignore", over="ignore"):
        g = restate(name, trace, params)
        full = g.shape[-1] <= KABC_MAX_DIM
        out = ao.summarize(g, L, full) if L else so.summarize(g, full)
        if hist is not None:
            lo, hi, B = hist
            out["counts"] = ho.histogram(g, lo, hi, B)
    out["g"] = g
    return out


def mismatches(got, want, L=0, hist=None, equal_nan=False):
    """where a one-chain derived PosteriorSummary differs from summarize()'s dict: the moments (and, with L,
    the autocorrelation's fields) bit for bit -- with equal_nan a NaN equals any NaN -- and the counts"""
    if got is None:
        return ["derived: None"]
    if equal_nan:
        bad = []
        fields = list(so.FIELDS) + (list(ao.AC_FIELDS) if L else [])
        for f in fields:
            attr = ao.AC_FIELDS.get(f, f)
            g, w = np.asarray(getattr(got, attr), dtype=np.float64), np.asarray(want[f], dtype=np.float64)
            if g.shape != w.shape or not np.array_equal(g, w, equal_nan=True):
                bad.append(f"{f}: {g!r} != {w!r}")
    else:
        bad = ao.mismatches(got, want) if L else so.mismatches(got, want)
    if hist is not None:
        lo, hi, B = hist
        if got.hist is None:
            return bad + ["hist: None"]
        full = np.concatenate([got.underflow[:, None], got.hist, got.overflow[:, None]], axis=1)
        if full.shape != want["counts"].shape or not np.array_equal(full, want["counts"]):
            bad.append(f"counts: {full!r} != {want['counts']!r}")
        if not np.all(full.sum(axis=1) == np.uint64(got.n)):
            bad.append(f"sums {full.sum(axis=1)} != n = {got.n}")
    return bad
