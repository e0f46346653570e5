"""No GPU: what the histogram entry points of the posterior summary refuse before a context is used, their
prototypes, kabc_hist_quantile (host arithmetic only) against the numpy restatement bit for bit, the
Python-side checks of `hist`, and the histogram fields of PosteriorSummary / ChainSummaries."""
import ctypes as C
import os

import numpy as np
import pytest

import ais_hist_oracle as ho
import ais_summary_oracle as so

U64P = C.POINTER(C.c_uint64)


def _model(k, D=3):
    return k.ApproxKernelizedPosterior(k.Factored(*[k.Normal(0, 3)] * D), k.costs.GaussDist(np.zeros(D)), 1.0)


def _quantile(lib, counts, B, lo, hi, mn, mx, q):
    from kissabc_jl_amd import _cdefs as cd
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    q = np.ascontiguousarray(np.atleast_1d(q), dtype=np.float64)
    out = np.full(q.size, -7.0)
    st = lib.kabc_hist_quantile(counts.ctypes.data_as(U64P), B, lo, hi, mn, mx, q.ctypes.data_as(cd.c_double_p),
                                q.size, out.ctypes.data_as(cd.c_double_p))
    return st, out


def test_prototypes(k):
    from kissabc_jl_amd import _cdefs as cd
    assert cd.KABC_HIST_MAX_BINS == 1024
    assert cd.KABC_VERSION == 321                            # (no struct, no version change)
    dp = cd.c_double_p
    res, args = cd.PROTOTYPES["kabc_ais_hist_begin"]
    assert res is C.c_int and args == [C.c_void_p, C.c_int32, dp, dp]
    res, args = cd.PROTOTYPES["kabc_ais_hist_get"]
    assert res is C.c_int and len(args) == 5 and args[0] is C.c_void_p and args[3] is dp and args[4] is dp
    assert args[1]._type_ is C.c_int32 and args[2]._type_ is C.c_uint64
    res, args = cd.PROTOTYPES["kabc_hist_quantile"]
    assert res is C.c_int and len(args) == 9 and args[0]._type_ is C.c_uint64
    assert args[1] is C.c_int32 and args[7] is C.c_int32 and args[2:6] == [C.c_double] * 4
    assert args[6] is dp and args[8] is dp
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "kabc.h")) as f:
        assert "#define KABC_HIST_MAX_BINS 1024" in f.read()


def test_null_handle_is_refused_by_both_entry_points(k):
    from kissabc_jl_amd import _cdefs as cd, _lib
    lib = _lib.load()
    nb = C.c_int32(-7)
    counts = np.full(12, 99, dtype=np.uint64)
    lo, hi = np.full(3, -1.0), np.full(3, 1.0)
    p = lambda a: a.ctypes.data_as(cd.c_double_p)           # noqa: E731
    calls = [lambda: lib.kabc_ais_hist_begin(None, 8, p(lo), p(hi)),
             lambda: lib.kabc_ais_hist_begin(None, 0, None, None),    # (the handle's check comes first)
             lambda: lib.kabc_ais_hist_get(None, C.byref(nb), counts.ctypes.data_as(U64P), p(lo), p(hi))]
    for call in calls:
        assert call() == cd.KABC_ERR_INVALID_ARG
        assert b"NULL" in lib.kabc_last_error()
    assert nb.value == -7 and np.all(counts == 99) and np.all(lo == -1.0) and np.all(hi == 1.0)


def test_library_quantile_equals_the_oracle_bit_for_bit(k):
    from kissabc_jl_amd import _cdefs as cd, _lib
    lib = _lib.load()
    ncases = 0
    for x, lo, hi, B in ho.random_cases():
        c = ho.histogram(x.reshape(-1, 1, 1), lo, hi, B)[0]
        st, got = _quantile(lib, c, B, lo, hi, x.min(), x.max(), ho.QS)
        assert st == cd.KABC_OK
        want = np.array([ho.quantile(c, B, lo, hi, x.min(), x.max(), q) for q in ho.QS])
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (lo, hi, B, got, want)
        ncases += 1
    assert ncases == 300
    # q values that fall between the tabulated ones, and counts beyond 2^32
    rng = np.random.default_rng(6)
    c = rng.integers(0, 2 ** 40, 12).astype(np.uint64)
    qs = rng.uniform(0, 1, 50)
    st, got = _quantile(lib, c, 10, -3.0, 7.0, -4.0, 8.5, qs)
    want = np.array([ho.quantile(c, 10, -3.0, 7.0, -4.0, 8.5, q) for q in qs])
    assert st == cd.KABC_OK and np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_library_quantile_refusals_leave_out_untouched(k):
    from kissabc_jl_amd import _cdefs as cd, _lib
    lib = _lib.load()
    c = np.array([1, 2, 3, 4, 0, 5], dtype=np.uint64)       # B = 4
    ok = (c, 4, 0.0, 1.0, -1.0, 2.0)
    st, out = _quantile(lib, *ok, [0.0, 0.5, 1.0])
    assert st == cd.KABC_OK and out[0] == -1.0 and out[2] == 2.0
    for q in ([0.5, -1e-9], [1.0000001], [0.2, np.nan], [np.inf]):
        st, out = _quantile(lib, *ok, q)
        assert st == cd.KABC_ERR_INVALID_ARG and np.all(out == -7.0), q
        assert b"outside [0, 1]" in lib.kabc_last_error()
    st, out = _quantile(lib, np.zeros(6, dtype=np.uint64), 4, 0.0, 1.0, -1.0, 2.0, 0.5)
    assert st == cd.KABC_ERR_INVALID_STATE and np.all(out == -7.0) and b"n = 0" in lib.kabc_last_error()
    for B in (0, -1, cd.KABC_HIST_MAX_BINS + 1):
        st, out = _quantile(lib, np.ones(cd.KABC_HIST_MAX_BINS + 3, dtype=np.uint64), B, 0.0, 1.0, -1.0, 2.0, 0.5)
        assert st == cd.KABC_ERR_INVALID_ARG and np.all(out == -7.0) and b"nbins" in lib.kabc_last_error()
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (np.nan, 1.0), (0.0, np.inf), (-np.inf, 0.0)):
        st, out = _quantile(lib, c, 4, lo, hi, -1.0, 2.0, 0.5)
        assert st == cd.KABC_ERR_INVALID_ARG and np.all(out == -7.0), (lo, hi)
    q = np.array([0.5])
    assert lib.kabc_hist_quantile(None, 4, 0.0, 1.0, -1.0, 2.0, q.ctypes.data_as(cd.c_double_p), 1,
                                  out.ctypes.data_as(cd.c_double_p)) == cd.KABC_ERR_INVALID_ARG
    assert b"NULL" in lib.kabc_last_error() and np.all(out == -7.0)


def test_python_side_exclusions(k):
    for kw in ({"hist": True}, {"hist": 16}, {"hist": (-1.0, 1.0)}, {"hist": (-1.0, 1.0, 8)}):
        with pytest.raises(ValueError, match="needs summary=True"):
            k.sample(_model(k), k.AIS(20), 40, **kw)
        with pytest.raises(ValueError, match="needs summary=True"):
            k.sample(_model(k), k.AIS(20), k.MCMCThreads(), 40, 2, **kw)
        with pytest.raises(ValueError, match="needs summary=True"):
            k.sample_batch(_model(k), k.AIS(20), 40, nruns=2, **kw)
    for bad in (0, -3, 1025, 2.5, "128", (1.0,), (0.0, 1.0, 0), (0.0, 1.0, 1025), (0.0, 1.0, 2.5), (0.0, 1.0, 8, 9),
                ("a", "b")):
        with pytest.raises(ValueError, match="hist must be"):
            k.sample(_model(k), k.AIS(20), 40, summary=True, hist=bad)
        with pytest.raises(ValueError, match="hist must be"):
            k.sample_batch(_model(k), k.AIS(20), 40, nruns=2, summary=True, hist=bad)
    for bad in ((np.nan, 1.0), (0.0, np.inf), ([0.0, -np.inf, 0.0], 1.0)):
        with pytest.raises(ValueError, match="must be finite"):
            k.sample(_model(k), k.AIS(20), 40, summary=True, hist=bad)
    with pytest.raises(TypeError):                          # (the sampler's check still comes first)
        k.sample(_model(k), "AIS", 40, hist=True)


def test_summary_begin_checks_come_before_the_handle(k):
    ens = object.__new__(k.AisEnsemble)                     # (no handle: the checks come first)
    ens._h = C.c_void_p()
    ens.D, ens.nchains, ens.batched = 3, 2, True
    for bad in (0, 1025, "auto", (1.0,), 0.5):
        with pytest.raises(ValueError, match="hist must be"):
            ens.summary_begin(hist=bad)
    with pytest.raises(ValueError, match="must be finite"):
        ens.summary_begin(hist=(np.nan, 1.0))
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), ([0.0, 0.0, 5.0], [1.0, 1.0, 5.0]),
                   (np.zeros((2, 3)), [[1, 1, 1], [1, 0, 1]])):
        with pytest.raises(ValueError, match="is not below") as ei:
            ens.summary_begin(hist=(lo, hi, 8))
        assert "chain" in str(ei.value) and "parameter" in str(ei.value)
    with pytest.raises(ValueError, match="chain 1, parameter 1"):
        ens.summary_begin(hist=(np.zeros((2, 3)), [[1, 1, 1], [1, 0, 1]]))
    for lo, hi in ((np.zeros(2), 1.0), (0.0, np.ones(4)), (np.zeros((3, 2)), 1.0), (np.zeros((1, 3)), 1.0),
                   (np.zeros((2, 3, 1)), 1.0)):
        with pytest.raises(ValueError, match="must be a scalar"):
            ens.summary_begin(hist=(lo, hi))
    with pytest.raises(ValueError, match='cov must be'):
        ens.summary_begin("Full", hist=8)
    with pytest.raises(ValueError, match="autocorr must be"):
        ens.summary_begin(autocorr=0, hist=8)
    ens._h = None                                           # (nothing for __del__ to destroy)


def test_automatic_range_convention(k):
    from kissabc_jl_amd.api import _hist_auto_range
    x = np.array([[[0.0, 5.0, 2.0], [1.0, 5.0, -2.0], [0.25, 5.0, 0.0]]])     # [chain][N][D]
    lo, hi = _hist_auto_range(x)
    assert lo.tolist() == [[-1.0, 4.5, -6.0]] and hi.tolist() == [[2.0, 5.5, 6.0]]


def test_a_per_chain_range_gives_each_sequential_run_its_row(k):
    from kissabc_jl_amd.api import _chain_kw
    lo, hi = np.array([[0.0, 1.0, 2.0], [3.0, 4.0, 5.0]]), np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])
    kw = _chain_kw({"autocorr": 8, "hist": (lo, hi, 9)}, 1, 2, 3)
    assert kw["autocorr"] == 8 and kw["hist"][2] == 9
    assert kw["hist"][0].tolist() == [3.0, 4.0, 5.0] and kw["hist"][1].tolist() == [4.0, 5.0, 6.0]
    shared = {"hist": ([0.0, 1.0, 2.0], 7.0)}               # [D] and a scalar: the same for every run
    kw = _chain_kw(shared, 1, 2, 3)
    assert kw["hist"][0].tolist() == [0.0, 1.0, 2.0] and kw["hist"][1] == 7.0 and kw["hist"][2] == 128
    for same in ({"hist": 16}, {"hist": True}, {"autocorr": 8}, {}):
        assert _chain_kw(same, 1, 2, 3) is same


def _summary(k, tr, hist=None):
    s = so.summarize(tr)
    return k.PosteriorSummary(s["n"], s["mean"], s["cov"], s["min"], s["max"], s["pivot"], s["sum1"], s["sum2"],
                              hist=hist)


def _hist_of(tr, lo, hi, B):
    D = tr.shape[-1]
    return {"counts": ho.histogram(tr, lo, hi, B), "lo": np.broadcast_to(np.float64(lo), (D,)).copy(),
            "hi": np.broadcast_to(np.float64(hi), (D,)).copy()}


def test_summary_without_hist_reports_none_and_prints_as_before(k):
    tr = np.random.default_rng(0).normal(0, 1, (4, 9, 2))
    ps = _summary(k, tr)
    for f in ("hist", "edges", "underflow", "overflow", "median", "nbins"):
        assert getattr(ps, f) is None, f
    with pytest.raises(ValueError, match="no histogram"):
        ps.quantile(0.5)
    with pytest.raises(ValueError, match="no histogram"):
        ps.interval()
    with_hist = _summary(k, tr, _hist_of(tr, -4.0, 4.0, 16))
    assert repr(with_hist) == repr(ps)                      # (__repr__ is unchanged)
    cs = k.ChainSummaries([ps, ps])
    assert cs.pooled.hist is None


def test_fields_quantiles_and_chain_slices(k):
    rng = np.random.default_rng(4)
    B, lo, hi = 20, np.array([-5.0, -1.0]), np.array([5.0, 3.0])
    trs = [rng.normal(c, 1.0, (12, 9, 2)) for c in range(3)]
    one = _summary(k, trs[0], {"counts": ho.histogram(trs[0], lo, hi, B), "lo": lo, "hi": hi})
    assert one.hist.shape == (2, B) and one.hist.dtype == np.uint64 and one.nbins == B
    assert one.edges.shape == (2, B + 1)
    for d in range(2):
        assert np.array_equal(one.edges[d], ho.edges(lo[d], hi[d], B)) and one.edges[d, -1] == hi[d]
    assert np.array_equal(one.hist.sum(axis=1) + one.underflow + one.overflow, [one.n] * 2)
    c = one.histogram["counts"]
    for q in ho.QS:
        want = [ho.quantile(c[d], B, lo[d], hi[d], one.min[d], one.max[d], q) for d in range(2)]
        assert one.quantile(q).tolist() == want
    assert one.quantile([0.1, 0.9]).shape == (2, 2)
    assert np.array_equal(one.median, one.quantile(0.5))
    assert np.array_equal(one.interval(0.9), one.quantile([0.05, 0.95]))
    assert np.array_equal(one.interval(), one.quantile([(1 - 0.95) / 2, (1 + 0.95) / 2]))
    assert np.array_equal(one.quantile(0.0), one.min) and np.array_equal(one.quantile(1.0), one.max)
    with pytest.raises(k.KabcError):
        one.quantile(1.5)
    # a batch summary: a leading chain axis, chain(c) slices the histogram too
    parts = [so.summarize(t) for t in trs]
    stack = lambda f: np.stack([p[f] for p in parts])   # noqa: E731
    hs = {"counts": np.stack([ho.histogram(t, lo, hi, B) for t in trs]), "lo": np.stack([lo] * 3),
          "hi": np.stack([hi] * 3)}
    both = k.PosteriorSummary(parts[0]["n"], stack("mean"), stack("cov"), stack("min"), stack("max"), hist=hs)
    assert both.hist.shape == (3, 2, B) and both.edges.shape == (3, 2, B + 1) and both.median.shape == (3, 2)
    assert both.interval().shape == (3, 2, 2)
    for ci in range(3):
        ch = both.chain(ci)
        assert np.array_equal(ch.hist, hs["counts"][ci][:, 1:-1]) and ch.median.shape == (2,)
        assert np.array_equal(ch.median, both.median[ci])


def test_pooled_histogram_needs_equal_ranges(k):
    rng = np.random.default_rng(5)
    trs = [rng.normal(c, 1.0, (6, 9, 2)) for c in range(3)]
    same = [_summary(k, t, _hist_of(t, -5.0, 6.0, 12)) for t in trs]
    cs = k.ChainSummaries(same)
    assert np.array_equal(cs.pooled.histogram["counts"], ho.histogram(np.concatenate(trs), -5.0, 6.0, 12))
    assert cs.pooled.hist.dtype == np.uint64 and cs.pooled.n == 3 * 54
    allx = np.sort(np.concatenate(trs).reshape(-1, 2), axis=0)
    assert np.all(np.abs(cs.pooled.median - allx[81 - 1]) <= 11.0 / 12)
    assert np.array_equal(cs.pooled.quantile(1.0), allx[-1])
    for other in (_hist_of(trs[2], -5.0, np.nextafter(6.0, 7.0), 12), _hist_of(trs[2], -5.0, 6.0, 13)):
        differ = same[:2] + [_summary(k, trs[2], other)]
        cs = k.ChainSummaries(differ)
        assert cs.pooled.hist is None and cs.pooled.median is None
        with pytest.raises(ValueError, match=r"hist=\(lo, hi\)"):
            cs.pooled.quantile(0.5)
        assert cs[2].hist is not None                       # (the chains keep their own)
