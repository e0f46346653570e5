"""numpy restatement of the marginal histograms of a summarised AIS trace and of the quantile rule
(include/kabc.h, "marginal histograms and quantiles of a summarised trace"), with the same operation order:
every fp64 operation below is one rounded numpy operation, and counts are integers."""
import numpy as np


def histogram(trace, lo, hi, B):
    """trace [G][N][D] (one chain), lo / hi [D]  ->  counts [D][B + 2] uint64: underflow, the bins, overflow"""
    trace = np.asarray(trace, dtype=np.float64)
    D = trace.shape[-1]
    r = trace.reshape(-1, D)
    lo, hi = np.broadcast_to(np.asarray(lo, dtype=np.float64), (D,)), np.broadcast_to(np.asarray(hi, np.float64), (D,))
    B = int(B)
    counts = np.zeros((D, B + 2), dtype=np.uint64)
    for k in range(D):
        width = hi[k] - lo[k]
        scale = np.float64(B) / width
        assert np.isfinite(scale) and scale > 0
        x = r[:, k]
        under = x < lo[k]
        over = ~under & ~(x < hi[k])                      # (a NaN lands here)
        mid = ~under & ~over
        d = x[mid] - lo[k]
        u = d * scale
        b = u.astype(np.int64)                            # (int)u: truncation
        b = np.where(b > B - 1, B - 1, b)
        counts[k, 0] = np.count_nonzero(under)
        counts[k, B + 1] = np.count_nonzero(over)
        counts[k, 1:B + 1] = np.bincount(b, minlength=B).astype(np.uint64)
    return counts


def quantile(counts, B, lo, hi, mn, mx, q):
    """one parameter: counts [B + 2], q a scalar in [0, 1]  ->  the quantile (a Python float)"""
    c = [int(v) for v in np.asarray(counts).reshape(-1)]
    B = int(B)
    assert len(c) == B + 2
    lo, hi, mn, mx, q = (np.float64(v) for v in (lo, hi, mn, mx, q))
    if not (0.0 <= q <= 1.0):
        raise ValueError("q outside [0, 1]")
    n = sum(c)
    if n == 0:
        raise ArithmeticError("n = 0")
    span = hi - lo
    w = span / np.float64(B)
    h = q * np.float64(n)
    cum, j = 0, 0
    while j < B + 1:
        if c[j] > 0 and h <= np.float64(cum + c[j]):
            break
        cum += c[j]
        j += 1
    if j == 0:
        return float(mn)
    if j == B + 1:
        return float(mx)
    num = h - np.float64(cum)
    f = num / np.float64(c[j])
    pos = np.float64(j - 1) + f
    off = pos * w
    v = lo + off
    v = v if v > mn else mn
    v = v if v < mx else mx
    return float(v)


QS = (0.0, 0.025, 0.25, 0.5, 0.75, 0.975, 1.0)


def random_cases(ncases=300, seed=20):
    """(x, lo, hi, B): Normal and rounded-Normal samples, B from 1 to 200, ranges that hold all of the data,
    cut into it on either side, or miss most of it"""
    rng = np.random.default_rng(seed)
    for i in range(ncases):
        n = int(rng.integers(1, 500))
        B = int(rng.integers(1, 201))
        mu, sd = rng.normal(0, 5), float(np.exp(rng.normal(0, 1.5)))
        x = rng.normal(mu, sd, n)
        if i % 2:
            x = np.round(x)
        kind = i % 5
        if kind == 0:                                        # all of the data, with room
            lo, hi = x.min() - sd, x.max() + sd
        elif kind == 1:                                      # integer-aligned around the data
            lo, hi = np.floor(x.min()) - 0.5, np.ceil(x.max()) + 0.5
        elif kind == 2:                                      # cuts both tails
            lo, hi = mu - 1.1 * sd, mu + 0.9 * sd
        elif kind == 3:                                      # misses most of it
            lo, hi = mu + 1.5 * sd, mu + 1.5 * sd + 0.3 * sd
        else:                                                # exactly the data's own range: the maximum overflows
            lo, hi = x.min(), x.max() if x.max() > x.min() else x.min() + 1.0
        yield x, float(lo), float(hi), B


def edges(lo, hi, B):
    lo, hi = np.float64(lo), np.float64(hi)
    e = lo + np.arange(B + 1) * ((hi - lo) / B)
    e[-1] = hi
    return e


def mismatches(got, trace, lo, hi, B):
    """where a one-chain PosteriorSummary's histogram differs from histogram(trace, lo, hi, B), bit for bit;
    also that every parameter's counts add up to n"""
    bad = []
    want = histogram(trace, lo, hi, B)
    if got.hist is None:
        return ["hist: None"]
    full = np.concatenate([got.underflow[:, None], got.hist, got.overflow[:, None]], axis=1)
    if full.dtype != np.uint64:
        bad.append(f"dtype {full.dtype}")
    if full.shape != want.shape:
        return bad + [f"shape {full.shape} != {want.shape}"]
    if not np.array_equal(full, want):
        k, j = np.argwhere(full != want)[0]
        bad.append(f"counts differ in {np.count_nonzero(full != want)} places, first at parameter {k} counter {j}: "
                   f"{full[k, j]} != {want[k, j]}")
    if not np.all(full.sum(axis=1) == np.uint64(got.n)):
        bad.append(f"sums {full.sum(axis=1)} != n = {got.n}")
    D = want.shape[0]
    if not (np.array_equal(got.histogram["lo"], np.broadcast_to(np.asarray(lo, np.float64), (D,)))
            and np.array_equal(got.histogram["hi"], np.broadcast_to(np.asarray(hi, np.float64), (D,)))):
        bad.append("lo / hi are not the ones given")
    return bad
