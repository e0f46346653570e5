"""No GPU: the numpy restatement of the AIS posterior summary (tests/ais_summary_oracle.py) computes the
moments it claims to, within the error a recursive summation can make, and has the properties the device
relies on: the pivot keeps a far-off column accurate, a constant column is exact, the accumulators carry
over any split of the generations, and the row tree is the expression it is said to be.

The tolerances are worked out in the tests, per entry, from u = 2^-53 and the terms summed.  A sum of n
terms taken in any order is off by at most n * u * sum|terms| (Higham, Accuracy and Stability of Numerical
Algorithms, eq. 4.4, with gamma_n <= n * u rounded up generously); both sides of a comparison get their
own share: the restatement sums the deviations from the pivot, the extended-precision reference the values."""
import numpy as np
import pytest

import ais_summary_oracle as so

U = 2.0 ** -53


def _traces():
    rng = np.random.default_rng(12)
    G, N = 9, 37
    cols = [rng.normal(0.0, 1.0, (G, N)),                  # plain
            np.full((G, N), 2.75),                         # constant
            1e9 + rng.normal(0.0, 1.0, (G, N)),            # offset by 1e9, unit spread
            rng.integers(-4, 9, (G, N)).astype(float),     # integer-valued
            rng.integers(0, 3, (G, N)).astype(float)]
    mixed = np.stack(cols, axis=-1)
    return {"mixed": mixed, "odd_rows": rng.normal(3.0, 2.0, (5, 13, 3)), "one_generation": mixed[:1],
            "two_rows": rng.normal(0.0, 1.0, (4, 2, 2))}


TRACES = _traces()


def _reference(x):
    """mean and cov(ddof=1) of rows x [n][D] in extended precision, centred first"""
    xl = x.astype(np.longdouble)
    mean = xl.sum(axis=0) / xl.shape[0]
    c = xl - mean
    return mean, (c.T @ c) / (xl.shape[0] - 1)


def _bounds(trace, s):
    """per-entry bounds on |restatement - exact| + |reference - exact| for mean [D] and cov [D][D]"""
    x = trace.reshape(-1, trace.shape[-1])
    n = x.shape[0]
    d = np.abs(x - s["pivot"])
    c = np.abs(x - x.mean(axis=0))
    e1 = n * U * d.sum(axis=0)                               # error of T1 (and the deviations' own rounding)
    mean_tol = (e1 + n * U * np.abs(x).sum(axis=0)) / n + 4 * U * (np.abs(s["pivot"]) + np.abs(s["mean"]))
    t1 = np.abs(s["sum1"])
    e2 = n * U * (d.T @ d + c.T @ c)                         # T2, and the reference's centred products
    ecross = (np.outer(t1, e1) + np.outer(e1, t1) + np.outer(e1, e1) + 4 * U * np.outer(t1, t1)) / n
    cov_tol = (e2 + ecross) / (n - 1) + 4 * U * np.abs(s["cov"])
    return mean_tol, cov_tol


def _numpy_cov_share(x):
    """what np.cov adds in float64: it centres on its own mean, whose n terms are the VALUES -- off by
    delta <= n * u * sum|x| / n -- and a centre shifted by delta moves sum(c_k c_l) by at most
    delta_k sum|c_l| + delta_l sum|c_k| + n delta_k delta_l.  (At 1e9 this is what the pivot avoids.)"""
    n = x.shape[0]
    delta = U * np.abs(x).sum(axis=0)
    c = np.abs(x - x.mean(axis=0)).sum(axis=0)
    return (np.outer(delta, c) + np.outer(c, delta) + n * np.outer(delta, delta)) / (n - 1)


@pytest.mark.parametrize("name", sorted(TRACES))
def test_moments_agree_with_numpy_within_the_summation_bound(name):
    trace = TRACES[name]
    x = trace.reshape(-1, trace.shape[-1])
    s = so.summarize(trace, full=True)
    sd = so.summarize(trace, full=False)
    assert s["n"] == x.shape[0] == sd["n"]
    mean, cov = _reference(x)
    mean_tol, cov_tol = _bounds(trace, s)
    assert np.all(np.abs(s["mean"] - mean) <= mean_tol), (s["mean"] - mean, mean_tol)
    assert np.all(np.abs(s["cov"] - cov) <= cov_tol), (np.abs(s["cov"] - cov).max(), cov_tol)
    # numpy's own float64 moments lie inside the same bounds
    assert np.all(np.abs(s["mean"] - np.mean(x, axis=0)) <= mean_tol)
    np_cov = np.cov(x, rowvar=False, ddof=1).reshape(cov.shape)
    assert np.all(np.abs(s["cov"] - np_cov) <= cov_tol + _numpy_cov_share(x))
    assert np.array_equal(s["cov"], s["cov"].T) and np.array_equal(s["sum2"], s["sum2"].T)
    # "diag" is the diagonal of "full", bit for bit; min / max are the plain ones
    assert np.array_equal(sd["cov"], np.diagonal(s["cov"])) and np.array_equal(sd["sum2"], np.diagonal(s["sum2"]))
    for t in (s, sd):
        assert np.array_equal(t["min"], x.min(axis=0)) and np.array_equal(t["max"], x.max(axis=0))
        assert np.array_equal(t["pivot"], trace[0, 0])


def test_the_pivot_keeps_a_far_off_column_accurate():
    """a column at 1e9 with unit spread: the deviations from the pivot are of order 1, so the variance is good
    to the bound -- where the textbook sum of squares about zero loses every digit of it"""
    trace = TRACES["mixed"][..., 2:3]
    x = trace.reshape(-1, 1)
    n = x.shape[0]
    s = so.summarize(trace)
    _, cov = _reference(x)
    _, cov_tol = _bounds(trace, s)
    err = abs(s["cov"][0, 0] - cov[0, 0])
    assert err <= cov_tol[0, 0] and cov_tol[0, 0] < 1e-12, (err, cov_tol)
    naive = (np.sum(x * x) - np.sum(x) ** 2 / n) / (n - 1)
    assert abs(naive - float(cov[0, 0])) > 1e6 * cov_tol[0, 0]


def test_a_constant_column_gives_exactly_zero():
    for full in (True, False):
        s = so.summarize(TRACES["mixed"], full=full)
        assert s["mean"][1] == 2.75 and s["sum1"][1] == 0.0 and s["min"][1] == s["max"][1] == 2.75
        if full:
            assert np.all(s["cov"][1, :] == 0.0) and np.all(s["cov"][:, 1] == 0.0)
        else:
            assert s["cov"][1] == 0.0


def test_integer_columns_sum_exactly():
    trace = TRACES["mixed"][..., 3:5]
    x = trace.reshape(-1, 2).astype(np.int64)
    s = so.summarize(trace)
    p = trace[0, 0].astype(np.int64)
    d = x - p
    assert np.array_equal(s["sum1"], d.sum(axis=0).astype(float))
    assert np.array_equal(s["sum2"], (d.T @ d).astype(float))


@pytest.mark.parametrize("full", [True, False])
def test_splitting_the_generations_anywhere_gives_the_same_bits(full):
    trace = TRACES["mixed"]
    whole = so.summarize(trace, full)
    for cut in range(1, trace.shape[0]):
        st = so.begin(trace.shape[1], trace.shape[2], full)
        so.fold(st, trace[:cut])
        so.fold(st, trace[cut:])
        assert so.mismatches(so.finish(st), whole) == []
    st = so.begin(trace.shape[1], trace.shape[2], full)
    for g in range(trace.shape[0]):
        so.fold(st, trace[g:g + 1])
    assert so.mismatches(so.finish(st), whole) == []


def test_row_trees_are_the_expressions_written_out():
    rng = np.random.default_rng(3)
    a = rng.normal(0.0, 1.0, 13) * 10.0 ** rng.integers(-8, 9, 13)   # (the order of the additions shows)
    assert so.row_tree(a[:1]) == a[0]
    assert so.row_tree(a[:2]) == a[0] + a[1]
    assert so.row_tree(a[:3]) == (a[0] + a[1]) + a[2]
    want13 = ((((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7])))
              + (((a[8] + a[9]) + (a[10] + a[11])) + a[12]))
    assert so.row_tree(a) == want13
    # vector-valued rows, min and max
    b = rng.normal(0.0, 1.0, (13, 2, 2))
    want = ((((b[0] + b[1]) + (b[2] + b[3])) + ((b[4] + b[5]) + (b[6] + b[7])))
            + (((b[8] + b[9]) + (b[10] + b[11])) + b[12]))
    assert np.array_equal(so.row_tree(b), want)
    assert so.row_tree(a, so._pick_min) == a.min() and so.row_tree(a, so._pick_max) == a.max()
