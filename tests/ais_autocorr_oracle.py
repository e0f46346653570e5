"""numpy restatement of the AIS summary's autocorrelation (include/kabc.h, "autocorrelation time and
effective sample size of a summarised trace") on top of ais_summary_oracle: the lagged products, the first
window and the ring the device keeps per element, the row tree over them, and the finalisation in the
header's order.  numpy's elementwise fp64 operations are IEEE operations and nothing here is fused or
reordered, so the device's result equals this one bit for bit.

    st = begin(N, D, L, full)      the summary's accumulators and the autocorrelation's
    fold(st, trace)                one or several times: the generations in order
    out = finish(st)               the summary's fields and lagsum, first, last, acov, rho, tau, ess,
                                   window, converged, nlags
    summarize(trace, L, full)      the three in one go
"""
import numpy as np

import ais_summary_oracle as so


def begin(N, D, L, full=True):
    st = so.begin(N, D, full)
    st.update(L=int(L), P=np.zeros((L + 1, N, D)),          # P[t], t = 1 ... L (P[0] stays unused: lag 0 is S2)
              F=np.zeros((L, N, D)), R=np.zeros((L, N, D)))
    return st


def fold(st, trace):
    trace = np.asarray(trace, dtype=np.float64)
    L = st["L"]
    for r in trace:
        g = st["G"]
        so.fold(st, r[None])                               # (takes the pivot at g = 0; G += 1)
        d = r - st["pivot"]
        for t in range(1, min(g, L) + 1):
            st["P"][t] += d * st["R"][(g - t) % L]          # the product is rounded, then added
        if g < L:
            st["F"][g] = d
        st["R"][g % L] = d
    return st


def finish(st):
    out = so.finish(st)
    G, N, D, L = st["G"], st["N"], st["D"], st["L"]
    Lm, Lw = min(L, G - 1), min(L, G)
    TP = np.stack([so.row_tree(st["P"][t]) for t in range(L + 1)])         # [t][k]
    TF = np.stack([so.row_tree(st["F"][g]) for g in range(Lw)])            # [g][k]
    TL = np.stack([so.row_tree(st["R"][(G - j) % L]) for j in range(1, Lw + 1)])   # [j - 1][k]
    T1 = out["sum1"]
    T2 = np.diagonal(out["sum2"]) if st["full"] else out["sum2"]
    n = np.float64(G * N)
    lagsum, acov, rho = (np.full((D, Lm + 1), np.nan) for _ in range(3))
    tau, ess = np.full(D, np.nan), np.full(D, np.nan)
    window, converged = np.zeros(D, dtype=np.int32), np.zeros(D, dtype=np.int32)
    for k in range(D):
        m = T1[k] / n
        head = tail = np.float64(0.0)
        for t in range(Lm + 1):
            if t > 0:
                head = head + TF[t - 1][k]
                tail = tail + TL[t - 1][k]
            tp = T2[k] if t == 0 else TP[t][k]
            A, B = T1[k] - tail, T1[k] - head
            u = A + B
            v = m * u
            w = tp - v
            q = m * m
            x = np.float64(N * (G - t)) * q
            y = w + x
            lagsum[k, t], acov[k, t] = tp, y / n
        if acov[k, 0] == 0.0 or G < 2:
            continue
        s, win, conv, tw = np.float64(0.0), Lm, 0, None
        for M in range(Lm + 1):
            rho[k, M] = acov[k, M] / acov[k, 0]
            if M > 0:
                s = s + rho[k, M]
            tm = 1.0 + 2.0 * s
            if not conv and np.float64(M) >= 5.0 * tm:
                win, conv, tw = M, 1, tm
            if not conv and M == Lm:
                tw = tm
        tau[k], ess[k], window[k], converged[k] = tw, n / tw, win, conv
    out.update(nlags=Lm + 1, lagsum=lagsum, first=TF, last=TL, acov=acov, rho=rho, tau=tau, ess=ess,
               window=window, converged=converged)
    return out


def summarize(trace, L, full=True):
    trace = np.asarray(trace, dtype=np.float64)
    return finish(fold(begin(trace.shape[1], trace.shape[2], L, full), trace))


# PosteriorSummary's names for the fields above
AC_FIELDS = {"lagsum": "lagsum", "first": "first", "last": "last", "acov": "acov", "rho": "acf", "tau": "tau",
             "ess": "ess", "window": "window"}


def mismatches(got, want):
    """so.mismatches plus the autocorrelation's fields (a PosteriorSummary or finish()'s dict against
    finish()'s dict), bit for bit; NaN equals NaN of the same bits"""
    bad = so.mismatches(got, want)
    for f, attr in AC_FIELDS.items():
        g = got[f] if isinstance(got, dict) else getattr(got, attr)
        if g is None:
            bad.append(f"{f}: None")
            continue
        if f == "window":
            if not np.array_equal(np.asarray(g, dtype=np.int64), np.asarray(want[f], dtype=np.int64)):
                bad.append(f"window: {g!r} != {want[f]!r}")
            continue
        g, w = np.asarray(g, dtype=np.float64), np.asarray(want[f], dtype=np.float64)
        if g.shape != w.shape:
            bad.append(f"{f}: shape {g.shape} != {w.shape}")
        elif not np.array_equal(np.isnan(g), np.isnan(w)) or not np.array_equal(
                np.where(np.isnan(g), 0.0, g).view(np.uint64), np.where(np.isnan(w), 0.0, w).view(np.uint64)):
            bad.append(f"{f}: max |diff| {np.nanmax(np.abs(g - w))!r}")
    conv = got["converged"] if isinstance(got, dict) else getattr(got, "tau_converged")
    if not np.array_equal(np.asarray(conv).astype(bool), np.asarray(want["converged"]).astype(bool)):
        bad.append(f"converged: {conv!r} != {want['converged']!r}")
    return bad
