"""No GPU: the numpy restatement of the summary's autocorrelation (tests/ais_autocorr_oracle.py) computes the
autocovariance it claims to -- within the error its sums and an independent FFT estimate can make -- finds a
known integrated autocorrelation time, carries over any split of the generations bit for bit, and behaves
at the edges as include/kabc.h says.

The tolerance against the FFT estimate is worked out in the test from u = 2^-53 and the terms summed, the way
tests/test_ais_summary_oracle.py does it: a sum of n terms taken in any order is off by at most
n * u * sum|terms| (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4, gamma_n <= n * u rounded up
generously)."""
import numpy as np
import pytest

import ais_autocorr_oracle as ao
import ais_summary_oracle as so

U = 2.0 ** -53


def _ar1(phi, G, N, D, seed, scale=1.0, offset=0.0):
    """stationary AR(1) per walker and column: x[g] = phi x[g-1] + e, var 1 / (1 - phi^2)"""
    rng = np.random.default_rng(seed)
    x = np.empty((G, N, D))
    x[0] = rng.normal(0.0, 1.0 / np.sqrt(1.0 - phi * phi), (N, D))
    e = rng.normal(0.0, 1.0, (G, N, D))
    for g in range(1, G):
        x[g] = phi * x[g - 1] + e[g]
    return offset + scale * x


def _fft_acov(x, nlags):
    """the two-pass estimate, written independently: subtract the global mean, autocovariance of every
    walker by FFT (zero-padded, so the correlation is not circular), sum over walkers, divide by n.
    x: [G][N]; returns [nlags] and the transform length"""
    G, N = x.shape
    c = x - x.mean()
    M = 1 << int(np.ceil(np.log2(2 * G)))
    f = np.fft.rfft(c, n=M, axis=0)
    ac = np.fft.irfft(f * np.conj(f), n=M, axis=0)[:nlags]
    return ac.sum(axis=1) / (G * N), M


def _acov_bound(x, pivot, s, k, M):
    """per lag, a bound on |restatement - exact| + |FFT estimate - exact| for column k of x [G][N]"""
    G, N = x.shape
    n = G * N
    d = np.abs(x - pivot)
    c = np.abs(x - x.mean())
    t1, m = abs(s["sum1"][k]), abs(s["sum1"][k]) / n
    e1 = n * U * d.sum()                                   # T1, head and tail: sums of up to n deviations
    nl = s["nlags"]
    tol = np.empty(nl)
    for t in range(nl):
        # restatement: TP[t] sums n products |d d'|; m carries e1 / n; A + B is 2 |T1| at most, off by 2 e1;
        # then a handful of roundings of terms no larger than |TP| + 2 m |T1| + n m^2
        prods = (d[t:] * d[:G - t]).sum()
        big = prods + 2.0 * m * (t1 + d.sum()) + n * m * m
        rest = n * U * prods + (e1 / n) * 2.0 * (t1 + d.sum()) + m * 2.0 * e1 + 2.0 * m * e1 + 16.0 * U * big
        # FFT estimate: its mean is off by delta <= u * sum|x| (n terms / n), which moves a sum of centred
        # products by at most 2 delta sum|c| + n delta^2; each of its three passes (forward transform,
        # pointwise product, inverse) is normwise within log2(M) * 6u of its input (Higham, Theorem 24.2,
        # rounded up), and an output element is at most the walker's sum of squares
        delta = U * np.abs(x).sum()
        fft = 2.0 * delta * c.sum() + n * delta * delta + 3.0 * 6.0 * np.log2(M) * U * (c * c).sum() * 2.0
        tol[t] = (rest + fft) / n
    return tol


@pytest.fixture(scope="module")
def mixed():
    """three columns, [G = 60][N = 13]: AR(1) phi = 0.6; AR(1) phi = 0.9 far from zero (1e6, unit scale:
    the pivot matters); white noise with a large scale"""
    a = _ar1(0.6, 60, 13, 1, 1)
    b = _ar1(0.9, 60, 13, 1, 2, offset=1e6)
    c = _ar1(0.0, 60, 13, 1, 3, scale=250.0)
    return np.concatenate([a, b, c], axis=-1)


@pytest.mark.parametrize("L", [1, 7, 59, 64])
def test_acov_agrees_with_an_independent_fft_estimate(mixed, L):
    s = ao.summarize(mixed, L)
    G = mixed.shape[0]
    assert s["nlags"] == min(L, G - 1) + 1
    for k in range(mixed.shape[2]):
        want, M = _fft_acov(mixed[..., k], s["nlags"])
        tol = _acov_bound(mixed[..., k], s["pivot"][k], s, k, M)
        err = np.abs(s["acov"][k] - want)
        print(f"L {L} column {k}: max err {err.max():.3e}, tol at it {tol[err.argmax()]:.3e}, acov0 {want[0]:.3e}")
        assert np.all(err <= tol), (k, err.max(), tol)
        # the bound says something: it is far below the autocovariance itself
        assert tol.max() < 1e-5 * want[0]
    # lag 0 is the biased variance the summary's own moments give
    n = s["n"]
    var0 = np.diagonal(s["cov"]) * (n - 1) / n
    assert np.allclose(s["acov"][:, 0], var0, rtol=1e-9, atol=0)
    assert np.array_equal(s["rho"][:, 0], np.ones(3))


@pytest.fixture(scope="module")
def ar1_long():
    return ao.summarize(_ar1(0.8, 2000, 64, 1, 2024), 128)


def test_known_tau_of_an_ar1_trace(ar1_long):
    """phi = 0.8: tau = (1 + phi) / (1 - phi) = 9; Sokal's variance of the windowed estimate,
    var(tau) ~ 2 (2M + 1) / n * tau^2, at five standard deviations"""
    s = ar1_long
    M, n = int(s["window"][0]), 2000 * 64
    bound = 5.0 * 9.0 * np.sqrt(2.0 * (2 * M + 1) / n)
    print(f"tau {s['tau'][0]!r}, window {M}, bound {bound!r}")
    assert s["converged"][0] == 1 and M >= 5.0 * s["tau"][0]
    assert abs(s["tau"][0] - 9.0) <= bound
    assert s["ess"][0] == n / s["tau"][0]
    # the autocorrelation itself: phi^t, to the same statistical accuracy at short lags
    assert np.allclose(s["rho"][0, :6], 0.8 ** np.arange(6), atol=0.02)


def test_splitting_the_generations_anywhere_gives_the_same_bits(mixed):
    trace = mixed[:23]
    N, D = trace.shape[1:]
    for L in (5, 40):                                       # (pieces shorter than L; G <= L)
        whole = ao.summarize(trace, L)
        for cuts in ([1], [22], [3, 4], [7, 8, 20], [5, 10, 15, 20], list(range(1, 23))):
            st = ao.begin(N, D, L)
            for piece in np.split(trace, cuts):
                ao.fold(st, piece)
            assert ao.mismatches(ao.finish(st), whole) == [], (L, cuts)
        # "diag" keeps the same autocorrelation: lag 0 is S2[k][k] in both modes
        diag = ao.summarize(trace, L, full=False)
        for f in ao.AC_FIELDS:
            assert np.array_equal(diag[f], whole[f], equal_nan=True), f


def test_fewer_generations_than_lags(mixed):
    s = ao.summarize(mixed[:6], 8)
    assert s["nlags"] == 6 and s["acov"].shape == (3, 6) and s["first"].shape == (6, 3) == s["last"].shape
    assert np.all(np.isfinite(s["tau"])) and np.all(s["window"] <= 5)
    # the windows are the tree sums of the deviations, first generations and last ones
    d = mixed[:6] - s["pivot"]
    assert np.array_equal(s["first"], np.stack([so.row_tree(d[g]) for g in range(6)]))
    assert np.array_equal(s["last"], np.stack([so.row_tree(d[5 - j]) for j in range(6)]))
    one = ao.summarize(mixed[:1], 8)
    assert one["nlags"] == 1 and np.all(np.isnan(one["tau"])) and np.all(np.isnan(one["ess"]))
    assert np.all(np.isnan(one["rho"])) and np.all(one["window"] == 0) and np.all(one["converged"] == 0)
    assert np.all(one["acov"][:, 0] > 0)                    # (the spread over the walkers is still there)


def test_a_constant_column_is_nan_with_window_zero(mixed):
    trace = mixed.copy()
    trace[..., 1] = 2.75
    s = ao.summarize(trace, 7)
    assert np.all(s["acov"][1] == 0.0) and np.all(np.isnan(s["rho"][1]))
    assert np.isnan(s["tau"][1]) and np.isnan(s["ess"][1]) and s["window"][1] == 0 and s["converged"][1] == 0
    assert np.all(np.isfinite(s["tau"][[0, 2]]))


def test_white_noise_has_tau_near_one():
    G, N = 400, 32
    s = ao.summarize(_ar1(0.0, G, N, 2, 77), 32)
    for k in range(2):
        M = int(s["window"][k])
        # (0 >= 5 tau_0 = 5 never holds: the smallest window white noise can get is 5 or so)
        assert s["converged"][k] == 1 and M <= 8
        assert abs(s["tau"][k] - 1.0) <= 5.0 * np.sqrt(2.0 * (2 * M + 1) / (G * N))


def test_a_slow_column_does_not_converge_inside_a_short_window():
    s = ao.summarize(_ar1(0.99, 300, 16, 1, 5), 8)
    assert s["converged"][0] == 0 and s["window"][0] == 8 and s["nlags"] == 9
    assert np.isclose(s["tau"][0], 1.0 + 2.0 * s["rho"][0, 1:].sum(), rtol=1e-12)   # tau at the last lag kept
    assert s["tau"][0] > 8.0 / 5.0
