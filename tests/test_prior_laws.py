"""CPU: the LAW of every prior family's draws (include/kabc_sampling.h, kabc_sampling_base.h and the
user-family snippets of kissabc_jl_amd/distributions.py), against scipy / mpmath, on a grid of edge
parameters -- the part of the stream contract that bit parity with the oracle cannot check, since the
device and the oracle compile the same sampler text.  Also the truncated Normal's normaliser at its
edges and the Dirichlet's support test along a chain (both shared between the host and the oracle).

check_law (tests/helpers.py) is the protocol; test_gpu_prior_laws.py runs it on device draws."""
import hashlib
import math

import numpy as np
import pytest

from helpers import check_law, make_dist, prior_law

N = 200_000
INF = float("inf")


def _tn_grid():
    g = [(0, 0.1, 0, 100), (0, 0.05, 0, 100)]                     # the half-normals of test_priors.py
    for z in (0.5, 1, 2, 3, 5, 8, 20, 37):                         # one-sided tails, both signs
        g += [(0, 1, z, INF), (0, 1, -INF, -z)]
    for z in (0.5, 1, 2, 3, 5, 8, 20, 37):                         # two-sided tail windows
        for w in (1e-3, 0.1, 1, 5):
            g += [(0, 1, z, z + w), (0, 1, -z - w, -z)]
    for w in (1e-9, 1e-6):                                         # narrow: centre, z = 0.5, 3
        g += [(0, 1, -w / 2, w / 2)]
        for z in (0.5, 3):
            g += [(0, 1, z, z + w), (0, 1, -z - w, -z)]
    for w in (0.01, 0.5, 4):                                       # across the mean
        g += [(0, 1, -w / 3, 2 * w / 3)]
    g += [(2.0, 0.5, 2.0 + 0.5 * 3, 2.0 + 0.5 * 3.1), (-1.0, 3.0, -INF, -1.0 - 3.0 * 8)]   # scaled
    return [("TruncNormal", p) for p in g]


GRID = _tn_grid() + [
    ("Gamma", (a, 1.0)) for a in (1e-3, 0.05, 0.999999, 1.0, 1.000001, 1e8)] + [
    ("Gamma", (0.5, 1e-300)), ("Gamma", (3.0, 1e-300)), ("Gamma", (0.5, 1e300)), ("Gamma", (3.0, 1e300)),
] + [("Beta", ab) for ab in ((1e-3, 1e-3), (0.01, 0.01), (1e-3, 2), (2, 1e-3), (0.5, 0.5), (1, 1), (1e4, 1e4))] + [
    ("Poisson", (lam,)) for lam in (9.999, 10.0, 10.001, 0.1, 1e6, 1e12)] + [
    ("NegativeBinomial", rp) for rp in ((2.0, 1e-9), (2.0, 0.999999), (0.01, 0.3), (1e4, 0.3), (1e4, 0.999))] + [
    ("DiscreteUniform", (0, n - 1)) for n in (1, 2, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40)] + [
    ("DiscreteUniform", (-7, 2 ** 40 - 8)),
    ("Exponential", (1e-300,)), ("Exponential", (1e300,)), ("Exponential", (1.0,)),
    ("LogNormal", (0.0, 1.0)), ("LogNormal", (-650.0, 2.0)), ("LogNormal", (650.0, 2.0)), ("LogNormal", (0.0, 1e-3)),
    ("Laplace", (0.0, 1.0)), ("Laplace", (1e300, 1e295)), ("Laplace", (0.0, 1e-200)),
    ("TruncatedGamma", (2.0, 1.5, 0.5, 6.0)), ("TruncatedGamma", (0.3, 1.0, 0.0, 0.5)), ("TruncatedGamma", (0.3, 1.0, 1e-4, 1e-3)),
    ("TruncatedGamma", (5.0, 1.0, 20.0, 20.5)), ("TruncatedGamma", (50.0, 1.0, 30.0, 31.0)),
]


def _id(case):
    return f"{case[0]}{tuple(case[1])}"


@pytest.mark.parametrize("case", GRID, ids=_id)
def test_prior_draws_follow_the_reference_law(orc, k, case):
    kind, params = case
    seed = int.from_bytes(hashlib.sha256(_id(case).encode()).digest()[:4], "little")
    x = orc.factored_rand(make_dist(k, kind, params), N, seed=seed)[:, 0]
    check_law(x, prior_law(kind, params), _id(case))


# ---- draws that were right before the samplers were fixed stay bit-identical -------------------
# sha256 of 10^4 oracle draws (seed 20261015) of the parameters test_priors.py, test_user_priors.py and
# bench.py sample, recorded before the truncated-Normal and Beta samplers changed
REGULAR_DRAWS = {
    ("Uniform", (1, 3)): "2df0ee7096d31dae5c1bdc83825fb0c62de59a6e35417bff5b8cbdd9421caef2",
    ("Uniform", (0, 1)): "0a21b5439538e4b6f72e7dcd96d113f776801211db801f68a62d2e7708da0355",
    ("Uniform", (100, 101)): "ce3240122a21d246750f584d7ecf6c226181fdb49acc2e48e41d84451ebbeef5",
    ("Normal", (1, 0.5)): "b18041a28442c56981a4446e3b3cfb24c5631a53f8ba22425ca49d39858db418",
    ("TruncNormal", (0, 0.1, 0, 100)): "3039c02813bbef45e5cd34ca9b0cc2108f54757c678cebc5742e538a0e2d1899",
    ("TruncNormal", (1, 2, -1, 4)): "8613fa05c78ca538085ddbbba4ace8c57a6eada7067f87f3d55be3d042794dbf",
    ("Beta", (15, 2)): "00fbf708428b3417777ed6bf9e3d8bec1a026247903c165e9c990cb0ca58a8cd",
    ("Beta", (0.5, 0.7)): "658c1c083f71e08a0f2bf65cc83dd3dbed716bf7b70466e772c028ff53317f14",
    ("Beta", (2, 3)): "971a1c4914b95987fb05d40e67f5c9b9a67486c31bc7b7fe39aa8197caaa2edf",
    ("Exponential", (2.5,)): "810485ec805fe3d636c42ef062c0598a9c4fdaa7b8d63cdf80fb96dd15a38158",
    ("Gamma", (0.4, 3.0)): "f2c2fc96c9a1cb270ae3e1b95c54d6d2a3af5f1203c1c469bd6c65848692e806",
    ("Gamma", (7.5, 0.5)): "baead8186f51bf7a30273d78d6a14713c7ac164c318d2d8b1f73b6fe191e7aef",
    ("Gamma", (2.5, 0.7)): "fd303a4bfe3b6740c5733345ba0c5c9035e640708fc98a411c20c8b005300c72",
    ("LogNormal", (0.3, 0.6)): "2923e6f2fbf9d53db200f2ea2a0065252529ef04cb4b29ee6225bc86611c19cd",
    ("DiscreteUniform", (1, 10)): "ac4d71ab71ea58249bc1302e2fdfc184bdf595a4951f77aff9856a673c0ff0d4",
    ("DiscreteUniform", (1, 2)): "60524601e16f4fafc15a1374bf264fc0356e6db8ad4f197a5892cfc6e3413cc3",
    ("NegativeBinomial", (900 / 195, (900 / 195) / (30 + 900 / 195))):
        "41201f6113c14513530c6dbd7e155d95a0fdebedf1d05a527af8f0f1369c369d",
    ("NegativeBinomial", (3.0, 0.6)): "e375c4e6f3563f0df61cf73904f4d4493b2b41e4ad99aba26ba5f4bd6fe260f7",
    ("Laplace", (0.5, 2.0)): "a1150bdf81aa168bc6665ffc9f8213b345b2e01b8d71e4c5b66bd65b899819d5",
    ("TruncatedGamma", (2.0, 1.5, 0.5, 6.0)): "dcd4a5c1b2be5a95cc049d270b8c411a7d0f4f53c03a7766793ffaec2d07e515",
    ("Poisson", (3.0,)): "26ab7c3d58aa88f1030420b3d05f6fc188a21c2f82e1fe14a3747d94b28d532b",
    ("Poisson", (40.0,)): "73533168b052adc8f4c228114914f4def72fcb292f5abb3a3f85ba078e32ab99",
}


def test_sampler_changes_leave_regular_draws_unchanged(orc, k):
    bad = []
    for (kind, params), want in REGULAR_DRAWS.items():
        x = orc.factored_rand(make_dist(k, kind, params), 10_000, seed=20261015)
        if hashlib.sha256(x.tobytes()).hexdigest() != want:
            bad.append(f"{kind}{params}")
    assert not bad, f"draws changed: {bad}"


# ---- the truncated Normal's normaliser ------------------------------------------------------------
def test_truncnormal_logpdf_is_finite_beyond_erfc_underflow(orc, k):
    """(0,1,40,41): erfc(40/sqrt2) is 0 in doubles; log(0) once made the logpdf +Inf everywhere"""
    import mpmath as mp
    mp.mp.dps = 50
    x = np.array([40.0, 40.25, 40.5, 41.0])
    got = orc.factored_logpdf(k.TruncatedNormal(0, 1, 40, 41), x.reshape(-1, 1))
    lm = mp.log(mp.ncdf(-40) - mp.ncdf(-41))
    ref = np.array([float(-mp.mpf(v) ** 2 / 2 - mp.log(mp.sqrt(2 * mp.pi)) - lm) for v in x])
    assert np.all(np.isfinite(got)) and np.allclose(got, ref, rtol=1e-12, atol=1e-12)


# ---- Dirichlet: the support test along a chain ---------------------------------------------------
def _dirichlet_chain_proposals(alpha, walkers=40, moves=20_000, seed=7):
    """Proposals of an ensemble chain on the simplex, built in numpy with the reference's rules (stretch
    move, Z = ((a - 1) U + 1)^2 / a with a = 2, and a walk move), each accepted whenever the reference
    accepts it (log-density ratio + the stretch's (D - 1) log Z), the density's sum taken in the
    snippet's order.  Rounding in x_i + Z (x_j - x_i) drifts the sum of the coordinates away from 1 as a
    real run does, which a fresh draw does not show."""
    rng = np.random.default_rng(seed)
    D = len(alpha)
    X = rng.dirichlet(alpha, size=walkers)

    def logp(x):
        if np.any(x < 0):
            return -np.inf
        s = 0.0
        for v in x:
            s += v
        if abs(s - 1.0) > 2.0 ** -26 * max(s, 1.0):
            return -np.inf
        return float(np.sum((alpha - 1) * np.log(x)))
    lp = np.array([logp(x) for x in X])
    props = []
    for t in range(moves):
        i = t % walkers
        j = rng.integers(walkers - 1)
        j += j >= i
        if t % 2 == 0:
            Z = ((2.0 - 1.0) * rng.random() + 1.0) ** 2 / 2.0
            y = X[j] + Z * (X[i] - X[j])
            extra = (D - 1) * math.log(Z)
        else:
            k1, k2 = rng.choice([m for m in range(walkers) if m != i], 2, replace=False)
            y = X[i] + rng.normal() * (X[k1] - X[k2]) * 0.5
            extra = 0.0
        props.append(y)
        ly = logp(y)
        if np.isfinite(ly) and math.log(rng.random()) < ly - lp[i] + extra:
            X[i], lp[i] = y, ly
    return np.array(props)


DIR_ALPHA = np.array([2.0, 3.0, 1.5, 4.0, 2.5])


def test_dirichlet_support_is_isprobvec(orc, k):
    d = k.Dirichlet(DIR_ALPHA)
    base = np.array([0.1, 0.2, 0.3, 0.15, 0.25])
    for eps, finite in ((1e-9, True), (-1e-9, True), (1e-7, False), (-1e-7, False), (0.0, True)):
        x = base.copy()
        x[2] += eps
        got = orc.factored_logpdf(d, x.reshape(1, -1))[0]
        assert np.isfinite(got) == finite, (eps, got)


def _isprobvec(P):
    """the reference's support test: all x >= 0 and isapprox(sum(x), 1) (rtol sqrt(eps) = 2^-26),
    the sum taken left to right as the snippet takes it"""
    s = np.zeros(len(P))
    for c in range(P.shape[1]):
        s = s + P[:, c]
    return np.all(P >= 0, axis=1) & (np.abs(s - 1) <= 2.0 ** -26 * np.maximum(s, 1)), s


def test_dirichlet_chain_proposals_in_support_have_finite_logpdf(orc, k):
    d = k.Dirichlet(DIR_ALPHA)
    P = _dirichlet_chain_proposals(DIR_ALPHA)
    ok, s = _isprobvec(P)
    # the chain drifts far beyond the 12-ulp rule the snippet once had: most proposals are past it
    assert np.mean(np.abs(s[ok] - 1) > len(DIR_ALPHA) * 2.0 ** -50) > 0.5
    got = orc.factored_logpdf(d, P)
    assert np.array_equal(np.isfinite(got), ok), \
        f"{np.sum(ok & ~np.isfinite(got))} of {ok.sum()} in-support proposals rejected, {np.sum(~ok & np.isfinite(got))} accepted outside"
