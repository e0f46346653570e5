"""No GPU: the numpy restatement of the histogram and of the quantile rule (tests/ais_hist_oracle.py) against
independent statements of what they mean -- np.bincount, np.histogram, the sample's minimum and maximum, and
the order statistics of the sample."""
import math

import numpy as np

import ais_hist_oracle as ho


def _trace(x):
    return np.asarray(x, dtype=np.float64).reshape(-1, 1, 1)


def test_integer_data_on_an_integer_aligned_range_is_bincount():
    rng = np.random.default_rng(1)
    K = 17
    x = rng.poisson(4.0, (9, 50, 2)).astype(np.float64)     # [G][N][D]
    x[..., 1] = np.minimum(x[..., 1], K)
    c = ho.histogram(x, -0.5, K + 0.5, K + 1)
    for k in range(2):
        col = x[..., k].astype(np.int64).ravel()
        want = np.bincount(col[col <= K], minlength=K + 1)
        assert np.array_equal(c[k, 1:-1], want.astype(np.uint64))
        assert c[k, 0] == 0 and c[k, -1] == np.count_nonzero(col > K)
        assert c[k].sum() == col.size


def test_data_away_from_the_edges_is_np_histogram():
    rng = np.random.default_rng(2)
    for B in (1, 2, 7, 128, 1024):
        lo, hi = rng.normal(0, 3), None
        hi = lo + float(np.exp(rng.normal(0, 2)))
        w = (hi - lo) / B
        j = rng.integers(0, B, 4000)
        x = lo + (j + 0.5 + rng.uniform(-0.4, 0.4, j.size)) * w   # (a tenth of a bin from every edge)
        c = ho.histogram(_trace(x), lo, hi, B)
        want, _ = np.histogram(x, bins=B, range=(lo, hi))
        assert np.array_equal(c[0, 1:-1], want.astype(np.uint64)), B
        assert c[0, 0] == 0 and c[0, -1] == 0


def test_the_ends_of_the_range_and_nan():
    x = np.array([-1.0, 0.0, np.nextafter(0.0, -1), np.nextafter(1.0, 0), 1.0, 2.0, np.nan, np.inf, -np.inf])
    c = ho.histogram(_trace(x), 0.0, 1.0, 4)
    #          under: -1, -tiny, -inf | bin 0: 0.0 | bin 3: 1 - tiny | over: 1.0, 2.0, nan, +inf
    assert c[0].tolist() == [3, 1, 0, 0, 1, 4]
    assert c[0].sum() == x.size


def test_quantile_0_and_1_are_the_minimum_and_the_maximum():
    """... exactly, with the one exception the rule itself makes: a range that lies wholly above the sample
    puts every count into the underflow, whose answer is the minimum for every q (q = 1 included), and a
    range wholly below it answers the maximum for every q.  Nothing but [min, max] is known there."""
    degenerate = 0
    for x, lo, hi, B in ho.random_cases():
        c = ho.histogram(_trace(x), lo, hi, B)[0]
        q0 = ho.quantile(c, B, lo, hi, x.min(), x.max(), 0.0)
        q1 = ho.quantile(c, B, lo, hi, x.min(), x.max(), 1.0)
        all_under, all_over = c[0] == x.size, c[-1] == x.size
        degenerate += bool(all_under or all_over)
        assert q0 == (x.max() if all_over else x.min())
        assert q1 == (x.min() if all_under else x.max())
    assert degenerate < 30                                   # (the cases are not mostly the exception)


def test_a_range_that_misses_the_whole_sample_answers_from_min_and_max_alone():
    x = np.array([3.0, 4.0, 5.0])
    under = ho.histogram(_trace(x), 10.0, 11.0, 4)[0]
    over = ho.histogram(_trace(x), -2.0, -1.0, 4)[0]
    assert under.tolist() == [3, 0, 0, 0, 0, 0] and over.tolist() == [0, 0, 0, 0, 0, 3]
    for q in ho.QS:
        assert ho.quantile(under, 4, 10.0, 11.0, 3.0, 5.0, q) == 3.0
        assert ho.quantile(over, 4, -2.0, -1.0, 3.0, 5.0, q) == 5.0


def test_quantile_is_within_one_bin_width_of_the_order_statistic():
    """Where the order statistic x_(max(ceil(q n), 1)) lies inside [lo, hi), the located counter is the bin
    that holds it and the rule answers from inside that bin (and from inside [min, max]): the distance is at
    most w.  The bin of a sample comes from (x - lo) * scale, the rule's position from lo + j * w: both are
    rounded, so the bound is w plus a few units in the last place of the numbers involved."""
    worst, checked = 0.0, 0
    for x, lo, hi, B in ho.random_cases():
        c = ho.histogram(_trace(x), lo, hi, B)[0]
        xs, n, w = np.sort(x), x.size, (hi - lo) / B
        slack = 8 * np.spacing(max(abs(lo), abs(hi), abs(xs[0]), abs(xs[-1])))
        for q in ho.QS:
            v = ho.quantile(c, B, lo, hi, xs[0], xs[-1], q)
            assert xs[0] <= v <= xs[-1]
            stat = xs[max(math.ceil(q * n), 1) - 1]
            if lo <= stat < hi:
                checked += 1
                assert abs(v - stat) <= w + slack, (q, v, stat, w, lo, hi, B)
                worst = max(worst, abs(v - stat) / w)
    assert checked > 500                                     # (the bound was put to the test)
    print(f"worst |quantile - order statistic| / w = {worst:.3f} over {checked} checks")


def test_quantile_is_monotone_in_q_and_refuses_what_the_rule_excludes():
    import pytest
    x, lo, hi, B = next(iter(ho.random_cases(1, seed=3)))
    c = ho.histogram(_trace(x), lo, hi, B)[0]
    vs = [ho.quantile(c, B, lo, hi, x.min(), x.max(), q) for q in np.linspace(0, 1, 41)]
    assert all(a <= b for a, b in zip(vs, vs[1:]))
    for q in (-0.1, 1.0001, np.nan):
        with pytest.raises(ValueError):
            ho.quantile(c, B, lo, hi, x.min(), x.max(), q)
    with pytest.raises(ArithmeticError):
        ho.quantile(np.zeros(B + 2, dtype=np.uint64), B, lo, hi, 0.0, 0.0, 0.5)


def test_edges():
    e = ho.edges(-1.0, 2.0, 3)
    assert e.tolist() == [-1.0, 0.0, 1.0, 2.0]
    e = ho.edges(0.1, 0.7, 7)
    assert e[0] == 0.1 and e[-1] == 0.7 and e.shape == (8,) and np.all(np.diff(e) > 0)
