"""CPU: abc_reject / kabc_abc_reject -- the refusals that need no device (Python's, and the C entry point's own,
made with ctx = NULL as tests/test_cost_eval_args.py makes them), the two struct layouts, the exported symbols,
Particles.quantile / var, and the pure-oracle restatement of both modes (tests/abc_reject_oracle.py: the helper
the GPU tests compare against) checked against a table filtered by hand."""
import ctypes as C
import math

import numpy as np
import pytest

from abc_reject_oracle import oracle_reject, oracle_table, select_keep, select_threshold


# ---- Python refusals: before the library is touched --------------------------------------------
def test_python_refusals(k, monkeypatch):
    from kissabc_jl_amd import _lib

    def no_library(*a, **kw):
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(_lib, "default_context", no_library)
    prior = k.Factored(k.Normal(0, 1), k.Normal(0, 1))
    g = k.costs.GaussDist([0.0, 1.0])
    with pytest.raises(TypeError, match="must be a DeviceCost"):
        k.abc_reject(prior, lambda x: 0.0, 0.1, 10)
    with pytest.raises(ValueError, match="takes rows of 1 parameters, got 2"):
        k.abc_reject(prior, k.costs.Mixture(0.0), 0.1, 10)
    with pytest.raises(ValueError, match=r"either \(eps, n\) or \(draws, keep\)"):
        k.abc_reject(prior, g)
    with pytest.raises(ValueError, match=r"either \(eps, n\) or \(draws, keep\)"):
        k.abc_reject(prior, g, 0.1)                              # eps without n
    with pytest.raises(ValueError, match=r"either \(eps, n\) or \(draws, keep\)"):
        k.abc_reject(prior, g, n=10)                             # n without eps
    with pytest.raises(ValueError, match="not both"):
        k.abc_reject(prior, g, 0.1, 10, draws=100, keep=5)
    with pytest.raises(ValueError, match="not both"):
        k.abc_reject(prior, g, n=10, draws=100, keep=5)
    with pytest.raises(ValueError, match="keep needs draws"):
        k.abc_reject(prior, g, keep=5)
    with pytest.raises(ValueError, match="keep must be >= 1"):
        k.abc_reject(prior, g, draws=100, keep=0)
    with pytest.raises(ValueError, match="draws must be >= keep"):
        k.abc_reject(prior, g, draws=4, keep=5)
    with pytest.raises(ValueError, match="eps is NaN"):
        k.abc_reject(prior, g, math.nan, 10)
    with pytest.raises(ValueError, match="n must be >= 0"):
        k.abc_reject(prior, g, 0.1, -1)
    with pytest.raises(ValueError, match="draws must be >= 1"):
        k.abc_reject(prior, g, 0.1, 10, draws=0)
    with pytest.raises(ValueError, match="first_row must be >= 0"):
        k.abc_reject(prior, g, 0.1, 10, first_row=-1)
    with pytest.raises(ValueError, match=r"first_row \+ draws <= 2\^32"):
        k.abc_reject(prior, g, 0.1, 10, draws=100, first_row=(1 << 32) - 99)
    with pytest.raises(ValueError, match=r"first_row \+ draws <= 2\^32"):
        k.abc_reject(prior, g, draws=100, keep=5, first_row=(1 << 32) - 99)
    with pytest.raises(ValueError, match=r"first_row \+ draws <= 2\^32"):
        k.abc_reject(prior, g, 0.1, 10, first_row=(1 << 32) + 1)  # no budget: the stream is empty from there
    # prior_predictive shares the row check (costs.check_rows)
    with pytest.raises(ValueError, match=r"first_row \+ n <= 2\^32"):
        k.prior_predictive(prior, g, 100, first_row=(1 << 32) - 99)


def test_public_surface(k):
    assert "abc_reject" in k.__all__ and callable(k.abc_reject)
    from kissabc_jl_amd import api
    assert api.RejectResult._fields == ("P", "C", "logprior", "eps", "info")


# ---- the C entry point's own refusals (no device needed: ctx = NULL) ---------------------------
def _abi_args(k, D=2, cap=8):
    from kissabc_jl_amd import _cdefs as cd, _lib
    lib = _lib.load()
    cost = k.costs.GaussDist([0.25] * D)
    cc = cost.to_c()
    o = cd.RejectOpts()
    lib.kabc_reject_default_opts(C.byref(o))
    o.eps, o.n_accept = 0.5, 4
    bufs = (np.zeros((cap, D)), np.zeros(cap), np.zeros(cap), np.zeros(cap, dtype=np.int64))
    r = cd.RejectResult()
    r.theta = bufs[0].ctypes.data_as(cd.c_double_p)
    r.cost = bufs[1].ctypes.data_as(cd.c_double_p)
    r.logprior = bufs[2].ctypes.data_as(cd.c_double_p)
    r.index = bufs[3].ctypes.data_as(C.POINTER(C.c_int64))
    r.capacity = cap
    return lib, cd, cost, cc, o, r, bufs


def test_default_opts(k):
    lib, cd, _, _, _, _, _ = _abi_args(k)
    o = cd.RejectOpts()
    o.n_accept = o.max_draws = o.keep = o.first_row = 7
    o.seed = 7
    lib.kabc_reject_default_opts(C.byref(o))
    assert math.isnan(o.eps)
    assert (o.n_accept, o.max_draws, o.keep, o.seed, o.first_row) == (0, 0, 0, 0, 0)
    lib.kabc_reject_default_opts(None)                           # NULL is ignored


def test_abi_refusals(k):
    lib, cd, cost, cc, o, r, bufs = _abi_args(k)
    prior = k.Factored(k.Normal(0, 1), k.Uniform(-1, 1)).to_c()
    f = lib.kabc_abc_reject
    fake = C.c_void_p(8)      # never dereferenced: every case below is refused before the context is used

    def refused(msg, ctx=None, prior_=prior, D=2, cost_=None, opts=o, res=r, status=cd.KABC_ERR_INVALID_ARG):
        got = f(ctx, prior_, D, C.byref(cc) if cost_ is None else cost_, C.byref(opts) if opts is not None else None,
                C.byref(res) if res is not None else None)
        assert got == status, (msg, got, lib.kabc_last_error())
        assert msg in lib.kabc_last_error(), (msg, lib.kabc_last_error())

    refused(b"ctx is NULL")                                      # everything else is in order
    refused(b"NULL argument", ctx=fake, prior_=None)
    refused(b"NULL argument", ctx=fake, opts=None)
    refused(b"NULL argument", ctx=fake, res=None)
    assert f(fake, prior, 2, None, C.byref(o), C.byref(r)) == cd.KABC_ERR_INVALID_ARG
    assert b"NULL argument" in lib.kabc_last_error()
    refused(b"D = 0 outside 1..256", D=0)
    refused(b"D = 257 outside 1..256", D=257)

    def with_opts(**kw):
        o2 = cd.RejectOpts()
        C.memmove(C.byref(o2), C.byref(o), C.sizeof(o))
        for name, v in kw.items():
            setattr(o2, name, v)
        return o2
    refused(b"n_accept = -1", opts=with_opts(n_accept=-1))
    refused(b"max_draws = -5", opts=with_opts(max_draws=-5))
    refused(b"keep = -2", opts=with_opts(keep=-2))
    refused(b"result.capacity = 8 below n_accept = 9", opts=with_opts(n_accept=9))
    refused(b"result.capacity = 8 below keep = 9", opts=with_opts(keep=9, max_draws=100))
    refused(b"1 <= keep <= max_draws", opts=with_opts(keep=5, max_draws=4))
    refused(b"1 <= keep <= max_draws", opts=with_opts(keep=5, max_draws=0))
    refused(b"first_row + max_draws <= 2^32", opts=with_opts(max_draws=100, first_row=(1 << 32) - 99))
    refused(b"first_row + max_draws <= 2^32", opts=with_opts(first_row=-1))
    refused(b"first_row + max_draws <= 2^32", opts=with_opts(first_row=(1 << 32) + 1))
    refused(b"eps is NaN", opts=with_opts(eps=math.nan))
    # keep mode ignores eps; the last row that fits passes the range check (and stops at the NULL context)
    refused(b"ctx is NULL", opts=with_opts(eps=math.nan, keep=4, max_draws=100, first_row=(1 << 32) - 100))
    # a result array missing behind a non-zero demand
    r2 = cd.RejectResult()
    C.memmove(C.byref(r2), C.byref(r), C.sizeof(r))
    r2.index = None
    refused(b"NULL argument", res=r2)
    # the cost's arrays
    cc2 = cost.to_c()
    cc2.params = None
    refused(b"NULL params / data array", cost_=C.byref(cc2))
    cc3 = cost.to_c()
    cc3.ndata = -1
    refused(b"NULL params / data array", cost_=C.byref(cc3))
    assert not any(b.any() for b in bufs)


def test_struct_layouts_and_symbols(k):
    from kissabc_jl_amd import _cdefs as cd, _lib
    lib = _lib.load()
    for which, T in ((cd.ABI_REJECT_OPTS, cd.RejectOpts), (cd.ABI_REJECT_RESULT, cd.RejectResult)):
        assert C.sizeof(T) == lib.kabc_abi_sizeof(which), T
        for f, (name, _) in enumerate(T._fields_):
            assert getattr(T, name).offset == lib.kabc_abi_offsetof(which, f), (T, name)
        assert lib.kabc_abi_offsetof(which, len(T._fields_)) == -1
    assert C.sizeof(cd.RejectOpts) == 48 and C.sizeof(cd.RejectResult) == 96
    assert lib.kabc_abi_sizeof(31) == -1 and lib.kabc_abi_sizeof(34) == -1
    for sym in ("kabc_abc_reject", "kabc_reject_default_opts"):
        assert hasattr(lib, sym) and sym in cd.PROTOTYPES


# ---- Particles.quantile / var ------------------------------------------------------------------
def test_particles_quantile_and_var(k):
    x = np.random.default_rng(3).normal(size=1001) * 2.5 + 1.0
    p = k.Particles(x)
    for q in (0.0, 0.025, 0.5, 0.9, 1.0):
        got = p.quantile(q)
        assert isinstance(got, float) and got == float(np.quantile(x, q))
    qs = [0.05, 0.5, 0.95]
    assert np.array_equal(p.quantile(qs), np.quantile(x, qs))
    assert p.var() == float(np.var(x, ddof=1)) and abs(p.var() - p.std() ** 2) < 1e-12


# ---- the oracle restatement --------------------------------------------------------------------
def test_selection_rules_on_a_table_written_by_hand():
    nan, inf = math.nan, math.inf
    C_ = [0.5, nan, 0.2, inf, 0.2, 0.1]
    idx, draws, ex = select_threshold(C_, 0.2, 2)
    assert idx.tolist() == [2, 4] and draws == 5 and not ex
    idx, draws, ex = select_threshold(C_, 0.2, 3)
    assert idx.tolist() == [2, 4, 5] and draws == 6 and not ex
    idx, draws, ex = select_threshold(C_, 0.2, 4)
    assert idx.tolist() == [2, 4, 5] and draws == 6 and ex
    idx, draws, ex = select_threshold(C_, inf, 6)                # NaN never accepts, +Inf does at eps = +Inf
    assert idx.tolist() == [0, 2, 3, 4, 5] and draws == 6 and ex
    idx, draws, ex = select_threshold(C_, 0.05, 1)
    assert idx.tolist() == [] and draws == 6 and ex
    idx, draws, ex = select_threshold(C_, 0.2, 0)
    assert idx.tolist() == [] and draws == 0 and not ex
    idx, eps = select_keep(C_, 1)
    assert idx.tolist() == [5] and eps == 0.1
    idx, eps = select_keep(C_, 2)                                # the tie at 0.2 goes to the lower index
    assert idx.tolist() == [2, 5] and eps == 0.2
    idx, eps = select_keep(C_, 3)
    assert idx.tolist() == [2, 4, 5] and eps == 0.2
    idx, eps = select_keep(C_, 5)                                # +Inf only when nothing cheaper is left
    assert idx.tolist() == [0, 2, 3, 4, 5] and eps == inf
    idx, eps = select_keep(C_, 6)                                # NaN is never kept
    assert idx.tolist() == [0, 2, 3, 4, 5]
    idx, eps = select_keep([nan, nan], 1)
    assert idx.size == 0 and math.isnan(eps)


def test_oracle_restatement_against_a_hand_filtered_table(orc, k):
    from kissabc_jl_amd import _cdefs as cd
    prior = k.Factored(k.Normal(1, 0.5), k.DiscreteUniform(1, 10))
    cost = k.costs.NoisyQuadDU(5.5)
    seed, first_row, N = 3, (1 << 31) + 5, 60
    # the table, row by row, each of the four oracle calls made for ONE row
    rows = []
    for i in range(N):
        x = orc.push_p(prior, orc.factored_rand(prior, 1, seed, domain=cd.DOM_EVAL_DRAW, first_walker=first_row + i))[0]
        rows.append((x, orc.factored_logpdf(prior, x[None, :])[0],
                     orc.cost_eval(cost, x, seed=seed, walker=first_row + i, t=0, domain=cd.DOM_EVAL_COST)))
    P, lp, C_ = oracle_table(orc, prior, cost, N, seed, first_row)
    assert all(np.array_equal(P[i], rows[i][0]) and lp[i] == rows[i][1] and C_[i] == rows[i][2] for i in range(N))
    assert np.all(P[:, 1] == np.rint(P[:, 1])) and P[:, 1].min() >= 1 and P[:, 1].max() <= 10   # push_p happened
    eps = float(np.sort(C_)[14])
    # threshold mode by hand: walk the rows, stop at the 10th acceptance
    want, draws = [], None
    for i in range(N):
        if rows[i][2] <= eps:
            want.append(i)
            if len(want) == 10:
                draws = i + 1
                break
    Pg, Cg, lpg, eg, idx, d, ex = oracle_reject(orc, prior, cost, eps=eps, n=10, draws=N, seed=seed, first_row=first_row)
    assert idx.tolist() == want and d == draws and not ex and eg == eps
    assert np.array_equal(Pg, P[want]) and np.array_equal(Cg, C_[want]) and np.array_equal(lpg, lp[want])
    # more than the table holds: exhausted
    _, _, _, _, idx, d, ex = oracle_reject(orc, prior, cost, eps=eps, n=16, draws=N, seed=seed, first_row=first_row)
    assert idx.size == 15 and d == N and ex
    # keep mode by hand: sort (C, i) pairs
    best = sorted(sorted((rows[i][2], i) for i in range(N))[:7], key=lambda t: t[1])
    Pg, Cg, lpg, eg, idx, d, ex = oracle_reject(orc, prior, cost, draws=N, keep=7, seed=seed, first_row=first_row)
    assert idx.tolist() == [i for _, i in best] and eg == max(c for c, _ in best) and d == N
    assert np.array_equal(Pg, P[idx]) and np.array_equal(Cg, C_[idx])
