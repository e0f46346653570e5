"""CPU: the arithmetic contract (include/kabc_math.h, kabc_philox.h) against
independent implementations: glibc libm through numpy, mpmath, and the
Random123 known-answer vectors for Philox4x32-10."""
import ctypes as C

import numpy as np
import pytest

from helpers import philox_py as _philox_py   # (the Python Philox lives with the population restatements)
from helpers import ulp_diff

rng = np.random.default_rng(1)


def test_philox_kat_oracle_restatement(orc):
    # Random123 kat_vectors, philox4x32 10 rounds
    assert orc.philox([0] * 4, [0] * 2) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert orc.philox([0xffffffff] * 4, [0xffffffff] * 2) == \
        [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert orc.philox([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344],
                      [0xa4093822, 0x299f31d0]) == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_philox_round_count_is_a_contract_parameter(orc):
    """KABC_PHILOX_ROUNDS (include/kabc_philox.h): the Python restatement reproduces the
    Random123 10-round vectors, and agrees with the C restatement at 7 and 10 rounds on random
    inputs -- so a build with 7 rounds is pinned as firmly as the default."""
    assert _philox_py([0] * 4, [0] * 2, 10) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert _philox_py([0xffffffff] * 4, [0xffffffff] * 2, 10) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    r = np.random.default_rng(3)
    for _ in range(200):
        c = [int(v) for v in r.integers(0, 2 ** 32, 4)]
        kk = [int(v) for v in r.integers(0, 2 ** 32, 2)]
        for R in (7, 10):
            assert orc.philox(c, kk, R) == _philox_py(c, kk, R)
    assert orc.philox_rounds() in (7, 10)


def test_philox_shared_header_matches_restatement(orc, k):
    """kabc_philox.h (used by costs/sampling on host AND device) vs the oracle's
    independent Philox: a Uniform(0,1) prior draw is u01(lo64(block))."""
    from kissabc_jl_amd import _cdefs as cd
    seed = 0x0123456789ABCDEF
    n = 64
    draws = orc.factored_rand(k.Factored(k.Uniform(0, 1), k.Uniform(0, 1)), n, seed=seed,
                              domain=cd.DOM_SMC_INIT, first_walker=5, attempt=3)
    for i in range(n):
        for dim in range(2):
            w = orc.philox([5 + i, 3, dim * 128, cd.DOM_SMC_INIT],
                           [seed & 0xffffffff, seed >> 32], orc.philox_rounds())
            lo = (w[1] << 32) | w[0]
            u = ((lo >> 12) + 0.5) * 2.0 ** -52
            assert draws[i, dim] == u


# the transition counter where it leaves 32 bits: word 1 holds its low half, word 3 the domain byte and the
# upper 24 bits (include/kabc_philox.h).  The device and the oracle's costs and prior samplers compile the same
# kabc_stream_block, so a wrong word 3 there is invisible to device-oracle parity: it is pinned here.
_HIGH_T = [2 ** 32 - 1, 2 ** 32, 2 ** 32 + 3, 0xABCDEF00000003, 2 ** 56 - 1]
_DOM_ABCDE_MOVE, _DOM_PF_INIT, _DOM_PF_MOVE, _DOM_PF_COST = 11, 13, 15, 16   # (include/kabc_philox.h)


def _block_py(orc, seed, walker, t, slot, domain):
    return _philox_py([walker, t & 0xffffffff, slot, domain | ((t >> 32) << 8)],
                      [seed & 0xffffffff, seed >> 32], orc.philox_rounds())


def _lo_hi(w):
    return (w[1] << 32) | w[0], (w[3] << 32) | w[2]


def _u01(r):
    return ((r >> 12) + 0.5) * 2.0 ** -52


@pytest.mark.parametrize("t", _HIGH_T)
def test_philox_shared_header_upper_counter_word_prior_draws(orc, k, t):
    """orc.factored_rand draws through kabc_stream_block of the shared header: a Uniform(0,1) component is
    u01(lo64(block)) of the block at (walker, t lo32, slot, domain | t hi24 << 8)"""
    from kissabc_jl_amd import _cdefs as cd
    seed, n = 0x0123456789ABCDEF, 16
    for domain in (cd.DOM_SMC_INIT, _DOM_PF_INIT):
        draws = orc.factored_rand(k.Factored(k.Uniform(0, 1), k.Uniform(0, 1)), n, seed=seed, domain=domain,
                                  first_walker=5, attempt=t)
        for i in range(n):
            for dim in range(2):
                lo, _ = _lo_hi(_block_py(orc, seed, 5 + i, t, dim * 128, domain))
                assert draws[i, dim] == _u01(lo), (hex(t), i, dim)
    if t >= 2 ** 32:     # the upper word takes part: not the draws of the counter's low half alone
        low = orc.factored_rand(k.Factored(k.Uniform(0, 1)), n, seed=seed, domain=domain, first_walker=5,
                                attempt=t & 0xffffffff)
        high = orc.factored_rand(k.Factored(k.Uniform(0, 1)), n, seed=seed, domain=domain, first_walker=5, attempt=t)
        assert not np.any(low == high)


@pytest.mark.parametrize("t", _HIGH_T)
def test_philox_shared_header_upper_counter_word_cost_draws(orc, k, t):
    """orc.cost_eval hands the cost a kabc_cost_rng_t at (seed, walker, t, domain): NoisyBanana takes the
    normal pair of slot 0 and the uniforms of slot 1 (include/kabc_costs.h); its value is recomputed from the
    blocks of the restatement, the Inf coin included"""
    from kissabc_jl_amd import _cdefs as cd
    seed = 0xFEDCBA9876543210
    x = np.array([0.3, -0.7])
    coins = []
    for domain in (cd.DOM_AIS_COST, cd.DOM_SMC_COST, _DOM_PF_COST):
        for walker in (0, 7, 2 ** 31 + 3):
            z0, z1 = orc.normal_pairs(np.array(_lo_hi(_block_py(orc, seed, walker, t, 0, domain)), dtype=np.uint64))[0]
            u0 = _u01(_lo_hi(_block_py(orc, seed, walker, t, 1, domain))[0])
            a = x[0] + z0 * 0.01 - x[1] * x[1]
            b = x[1] - 1.0 + z1 * 0.01
            c = 50.0 * a * a + b * b
            assert orc.cost_eval(k.costs.NoisyBanana(0.0), x, seed=seed, walker=walker, t=t, domain=domain) == c
            want = np.inf if u0 < 0.5 else c
            assert orc.cost_eval(k.costs.NoisyBanana(0.5), x, seed=seed, walker=walker, t=t, domain=domain) == want
            coins.append(u0 < 0.5)
    assert len(coins) == 9


@pytest.mark.parametrize("t", _HIGH_T)
def test_oracle_stream_upper_counter_word(orc, t):
    """the oracle composes the counter words of its move streams itself (stream(), oracle/kabc_oracle.c):
    the same address, against the restatement"""
    from kissabc_jl_amd import _cdefs as cd
    r = np.random.default_rng(t % 1000)
    for _ in range(20):
        seed = int(r.integers(0, 2 ** 63)) * 2 + 1
        walker, slot = int(r.integers(0, 2 ** 32)), int(r.integers(0, 2 ** 32))
        for domain in (cd.DOM_AIS_MOVE, cd.DOM_SMC_MOVE, _DOM_ABCDE_MOVE, _DOM_PF_MOVE):
            assert orc.stream_block(seed, walker, t, slot, domain) == _block_py(orc, seed, walker, t, slot, domain)
    # bits 56..63 of a counter are not part of the address (the entry points refuse such counters)
    assert orc.stream_block(1, 2, 2 ** 56 + 5, 0, cd.DOM_AIS_MOVE) == orc.stream_block(1, 2, 5, 0, cd.DOM_AIS_MOVE)
    assert orc.stream_block(1, 2, 2 ** 55 + 5, 0, cd.DOM_AIS_MOVE) != orc.stream_block(1, 2, 5, 0, cd.DOM_AIS_MOVE)


def test_log_exp_log1p_within_1ulp_of_libm(orc):
    u = rng.random(200000)
    e = rng.integers(-300, 300, 200000)
    x = np.ldexp(u + 0.5, e)
    assert ulp_diff(orc.math_vec("log", x), np.log(x)).max() <= 1.0
    assert ulp_diff(orc.math_vec("log", u), np.log(u)).max() <= 1.0
    y = (u - 0.5) * 1400
    assert ulp_diff(orc.math_vec("exp", y), np.exp(y)).max() <= 1.0
    y = (u - 0.5) * 4
    assert ulp_diff(orc.math_vec("exp", y), np.exp(y)).max() <= 1.0
    z = np.ldexp(2 * u - 1, -rng.integers(0, 60, 200000))
    z = z[z > -1]
    assert ulp_diff(orc.math_vec("log1p", z), np.log1p(z)).max() <= 1.0


def test_exp_bounded_is_exp_on_its_domain(orc):
    # kabc_exp without the special cases (DE's gamma = c exp(0.1 randn), |arg| < 0.86)
    x = np.concatenate([rng.uniform(-700, 700, 300000), rng.normal(0, 1, 300000),
                        [0.0, -0.0, 700.0, -700.0]])
    assert np.array_equal(orc.math_vec("exp_bounded", x), orc.math_vec("exp", x))


def test_log_pn_is_log_on_positive_normals(orc):
    x = np.ldexp(rng.random(300000) + 0.5, rng.integers(-1020, 1020, 300000))
    assert np.array_equal(orc.math_vec("log_pn", x), orc.math_vec("log", x))
    u = (rng.integers(0, 2 ** 52, 300000).astype(np.float64) + 0.5) * 2.0 ** -52
    assert np.array_equal(orc.math_vec("log_pn", u), orc.math_vec("log", u))


def test_math_special_values(orc):
    with np.errstate(all="ignore"):
        x = np.array([0.0, -0.0, -1.0, np.inf, np.nan, 5e-324, 1.0, 2.2250738585072014e-308])
        got, ref = orc.math_vec("log", x), np.log(x)
    assert np.array_equal(got, ref, equal_nan=True)
    x = np.array([710.0, -746.0, 0.0, -0.0, np.inf, -np.inf, 709.7, -745.0, -710.0])
    with np.errstate(all="ignore"):
        assert np.array_equal(orc.math_vec("exp", x), np.exp(x))
    x = np.array([-1.0, -2.0, 0.0, 1e-300, np.inf])
    with np.errstate(all="ignore"):
        assert np.array_equal(orc.math_vec("log1p", x), np.log1p(x), equal_nan=True)


def test_sqrt_rint_are_ieee(orc):
    x = np.ldexp(rng.random(100000) + 0.5, rng.integers(-500, 500, 100000))
    assert np.array_equal(orc.math_vec("sqrt", x), np.sqrt(x))
    y = np.concatenate([rng.normal(0, 100, 1000), [0.5, 1.5, 2.5, -0.5, -1.5, 1e300]])
    assert np.array_equal(orc.math_vec("rint", y), np.rint(y))  # ties to even = round(Int, x)


def test_sincos2pi(orc):
    import mpmath as mp
    mp.mp.dps = 40
    u = np.concatenate([rng.random(2000), [0.0, 0.125, 0.25, 0.5, 0.75, 1.0 - 2 ** -53]])
    sc = orc.math_vec("sincos2pi", u)
    for ui, (s, c) in zip(u, sc):
        a = 2 * mp.pi * mp.mpf(float(ui))
        assert abs(mp.sin(a) - s) < 5e-16 and abs(mp.cos(a) - c) < 5e-16


def test_lgamma(orc):
    from scipy.special import gammaln
    x = np.concatenate([np.ldexp(rng.random(20000) + 0.5, rng.integers(-10, 14, 20000)),
                        np.arange(1, 200, dtype=float), [0.5, 1.5]])
    got, ref = orc.math_vec("lgamma", x), gammaln(x)
    assert np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))) < 4e-14


def test_lgamma1_table_holds_the_contract_functions_bits(orc):
    """include/kabc_lgamma1_table.h (the lookup of lgamma(x + 1) for the integer arguments of the
    NegativeBinomial log-density, kabc_lgamma1p_int_t) against kabc_lgamma itself as the oracle
    build computes it: all 256 entries, bit for bit."""
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                        "kabc_lgamma1_table.h")
    text = open(path).read()
    body = text[text.index("KABC_LGAMMA1_VALUES") + len("KABC_LGAMMA1_VALUES"):text.rindex("#endif")]
    vals = np.array([float.fromhex(t) for t in re.findall(r"-?0x[0-9a-f.]+p[+-]?\d+", body)])
    assert vals.size == 256
    ref = orc.math_vec("lgamma", np.arange(1, 257, dtype=float))
    assert np.array_equal(vals.view(np.uint64), ref.view(np.uint64))


def test_box_muller_moments(orc):
    r = rng.integers(0, 2 ** 64, size=400000, dtype=np.uint64)
    z = orc.normal_pairs(r).ravel()
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1) < 0.01
    from scipy import stats
    assert stats.kstest(z[:50000], "norm").pvalue > 1e-3
    assert np.all(np.isfinite(z))


def test_cdf_g_inv_closed_forms(orc):
    # src/transition.jl:46: cdf_g_inv(0,a) = 1/a, cdf_g_inv(1,a) = a
    for a in (2.0, 3.0, 7.5):
        assert orc.cdf_g_inv(0.0, a) == pytest.approx(1 / a, rel=4e-16)
        assert orc.cdf_g_inv(1.0, a) == pytest.approx(a, rel=4e-16)
    z = np.array([orc.cdf_g_inv(u, 3.0) for u in rng.random(1000)])
    assert z.min() >= 1 / 3 - 1e-15 and z.max() <= 3 + 1e-15


def test_div_rc_equals_ieee_division(orc):
    """kabc_div_rc(x, c, RN(1/c)) (Markstein: 1 mul + 2 fma) must equal the correctly
    rounded IEEE quotient x / c: the contract uses it for `/ 300`, `/ 3`
    (src/transition.jl:13,35), `cost / scale` (src/types.jl:55) and (x - mu) / sigma."""
    n = 4_000_000
    x = np.ldexp(rng.random(n) + 0.5, rng.integers(-300, 300, n)) * rng.choice([-1.0, 1.0], n)
    for c in (3.0, 300.0, 0.1, 0.005, 0.001, 1.0, 5.0, 0.2, 0.5, 0.01 / np.sqrt(2), 12.0):
        assert np.array_equal(orc.div_rc(x, c), x / c), c
    c = np.ldexp(rng.random(n) + 0.5, rng.integers(-100, 100, n))
    got, ref = orc.div_rc(x, c), x / c
    bad = np.flatnonzero(got != ref)
    # Markstein's theorem leaves room for rare 1-ulp misses for arbitrary c; none of the
    # constants the path divides by may miss, and random divisors must agree to <= 1 ulp
    assert bad.size <= n * 1e-3
    assert ulp_diff(got, ref).max() <= 1.0
