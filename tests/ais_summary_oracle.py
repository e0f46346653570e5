"""numpy restatement of the AIS posterior summary (include/kabc.h, "posterior summaries on the device"):
the fixed order of fp64 operations the device accumulators and their row tree follow, applied to a trace
[G][N][D] of one chain.  numpy's elementwise fp64 add / subtract / multiply / divide are IEEE operations
and nothing here is fused or reordered, so the device's result equals this one bit for bit.

    st = begin(D, full)            accumulators at their start
    fold(st, trace)                one or several times: the generations in order
    out = finish(st)               n, pivot, sum1, sum2, min, max, mean, cov
    summarize(trace, full)         the three in one go
"""
import numpy as np


def begin(N, D, full=True):
    return {"N": int(N), "D": int(D), "full": bool(full), "G": 0, "pivot": None,
            "S1": np.zeros((N, D)), "S2": np.zeros((N, D, D) if full else (N, D)),
            "mn": np.full((N, D), np.inf), "mx": np.full((N, D), -np.inf)}


def fold(st, trace):
    """the generations of trace [G][N][D] into the per-row accumulators, sequentially in g"""
    trace = np.asarray(trace, dtype=np.float64)
    assert trace.ndim == 3 and trace.shape[1:] == (st["N"], st["D"])
    D = st["D"]
    for r in trace:
        if st["pivot"] is None:
            st["pivot"] = r[0].copy()                      # row 0 of the first summarised generation
        d = r - st["pivot"]
        st["S1"] += d
        if st["full"]:
            for k in range(D):
                for l in range(k + 1):
                    st["S2"][:, k, l] += d[:, k] * d[:, l]   # the product is rounded, then added
        else:
            st["S2"] += d * d
        st["mn"] = np.where(r < st["mn"], r, st["mn"])
        st["mx"] = np.where(r > st["mx"], r, st["mx"])
        st["G"] += 1
    return st


def row_tree(A, op=np.add):
    """for w = 1, 2, 4, ... < N: A[i] = op(A[i], A[i + w]) for every i that is a multiple of 2w with
    i + w < N; the result is A[0].  A: [N][...]; any N."""
    A = np.array(A, dtype=np.float64)
    N = A.shape[0]
    w = 1
    while w < N:
        i = np.arange(0, N - w, 2 * w)                     # multiples of 2w with i + w < N
        A[i] = op(A[i], A[i + w])
        w *= 2
    return A[0]


def _pick_min(a, b):
    return np.where(b < a, b, a)


def _pick_max(a, b):
    return np.where(b > a, b, a)


def finish(st):
    D, full = st["D"], st["full"]
    n = st["G"] * st["N"]
    T1 = row_tree(st["S1"])
    T2 = row_tree(st["S2"])
    if full:                                               # the lower triangle is what was kept
        T2 = np.tril(T2) + np.tril(T2, -1).T
    mn, mx = row_tree(st["mn"], _pick_min), row_tree(st["mx"], _pick_max)
    dn = np.float64(n)
    mean = st["pivot"] + T1 / dn
    if full:
        cov = (T2 - (T1[:, None] * T1[None, :]) / dn) / np.float64(n - 1)
    else:
        cov = (T2 - (T1 * T1) / dn) / np.float64(n - 1)
    return {"n": n, "pivot": st["pivot"].copy(), "sum1": T1, "sum2": T2, "min": mn, "max": mx,
            "mean": mean, "cov": cov}


def summarize(trace, full=True):
    trace = np.asarray(trace, dtype=np.float64)
    return finish(fold(begin(trace.shape[1], trace.shape[2], full), trace))


FIELDS = ("n", "pivot", "sum1", "sum2", "min", "max", "mean", "cov")


def mismatches(got, want):
    """the FIELDS in which a PosteriorSummary (or a dict) differs from finish()'s dict, bit for bit"""
    bad = []
    for f in FIELDS:
        g = got[f] if isinstance(got, dict) else getattr(got, f)
        if f == "n":
            if int(g) != int(want[f]):
                bad.append(f"n: {g} != {want[f]}")
            continue
        g, w = np.asarray(g, dtype=np.float64), np.asarray(want[f], dtype=np.float64)
        if g.shape != w.shape or not np.array_equal(g.view(np.uint64), w.view(np.uint64)):
            bad.append(f"{f}: {g!r} != {w!r}")
    return bad
