"""No GPU: what the autocorrelation entry points of the posterior summary refuse before a context is used,
their prototypes, and the Python-side checks of `autocorr`."""
import ctypes as C

import numpy as np
import pytest

import ais_autocorr_oracle as ao


def _model(k, D=3):
    return k.ApproxKernelizedPosterior(k.Factored(*[k.Normal(0, 3)] * D), k.costs.GaussDist(np.zeros(D)), 1.0)


def test_null_handle_is_refused_by_both_entry_points(k):
    from kissabc_jl_amd import _cdefs as cd, _lib
    lib = _lib.load()
    nl = C.c_int32(-7)
    tau = np.full(3, -1.0)
    calls = [lambda: lib.kabc_ais_autocorr_begin(None, 8),
             lambda: lib.kabc_ais_autocorr_begin(None, 0),           # (the handle's check comes first)
             lambda: lib.kabc_ais_autocorr_get(None, C.byref(nl), None, None, None, None, None,
                                               tau.ctypes.data_as(cd.c_double_p), None, None, None)]
    for call in calls:
        assert call() == cd.KABC_ERR_INVALID_ARG
        assert b"NULL" in lib.kabc_last_error()
    assert nl.value == -7 and np.all(tau == -1.0)           # (outputs are left untouched)


def test_prototypes(k):
    from kissabc_jl_amd import _cdefs as cd
    assert cd.KABC_AUTOCORR_MAX_LAG == 256
    assert cd.PROTOTYPES["kabc_ais_autocorr_begin"] == (C.c_int, [C.c_void_p, C.c_int32])
    res, args = cd.PROTOTYPES["kabc_ais_autocorr_get"]
    assert res is C.c_int and len(args) == 11
    assert args[1] is args[9] is args[10] and args[1]._type_ is C.c_int32
    assert all(a is cd.c_double_p for a in args[2:9])
    assert cd.KABC_VERSION == 321                            # (no struct, no version change)


def test_python_side_exclusions(k):
    with pytest.raises(ValueError, match="needs summary=True"):
        k.sample(_model(k), k.AIS(20), 40, autocorr=True)
    with pytest.raises(ValueError, match="needs summary=True"):
        k.sample(_model(k), k.AIS(20), k.MCMCThreads(), 40, 2, autocorr=16)
    with pytest.raises(ValueError, match="needs summary=True"):
        k.sample_batch(_model(k), k.AIS(20), 40, nruns=2, autocorr=True)
    for bad in (0, -3, 257, 2.5, "64"):
        with pytest.raises(ValueError, match="autocorr must be"):
            k.sample(_model(k), k.AIS(20), 40, summary=True, autocorr=bad)
    with pytest.raises(TypeError):                          # (the sampler's check still comes first)
        k.sample(_model(k), "AIS", 40, autocorr=True)
    ens = object.__new__(k.AisEnsemble)                     # (no handle: the checks come first)
    ens._h = C.c_void_p()
    for bad in (0, 257, "all"):
        with pytest.raises(ValueError, match="autocorr must be"):
            ens.summary_begin(autocorr=bad)
    with pytest.raises(ValueError, match='cov must be'):
        ens.summary_begin("Full", autocorr=8)
    ens._h = None                                           # (nothing for __del__ to destroy)


def test_summary_without_autocorr_reports_none(k):
    s = ao.so.summarize(np.random.default_rng(0).normal(0, 1, (4, 9, 2)))
    ps = k.PosteriorSummary(s["n"], s["mean"], s["cov"], s["min"], s["max"], s["pivot"], s["sum1"], s["sum2"])
    for f in ("tau", "ess", "mcse", "acf", "acov", "window", "tau_converged", "maxlag"):
        assert getattr(ps, f) is None, f
    assert k.ChainSummaries([ps, ps]).ess is None


def test_fields_chain_slices_and_chain_ess(k):
    rng = np.random.default_rng(4)
    parts = [ao.summarize(rng.normal(c, 1.0, (12, 9, 2)), 5) for c in range(3)]

    def ac_of(p):
        return {"tau": p["tau"], "ess": p["ess"], "acf": p["rho"], "acov": p["acov"], "window": p["window"],
                "tau_converged": p["converged"].astype(bool), "maxlag": 5, "lagsum": p["lagsum"],
                "first": p["first"], "last": p["last"]}

    stack = lambda f: np.stack([p[f] for p in parts])   # noqa: E731
    acs = [ac_of(p) for p in parts]
    both = {f: (5 if f == "maxlag" else np.stack([a[f] for a in acs])) for f in acs[0]}
    s = k.PosteriorSummary(parts[0]["n"], stack("mean"), stack("cov"), stack("min"), stack("max"), stack("pivot"),
                           stack("sum1"), stack("sum2"), autocorr=both)
    assert s.tau.shape == (3, 2) and s.acf.shape == (3, 2, 6) and s.maxlag == 5
    before = repr(k.PosteriorSummary(parts[0]["n"], stack("mean"), stack("cov"), stack("min"), stack("max")))
    assert repr(s) == before                                # (__repr__ is unchanged)
    chains = [s.chain(c) for c in range(3)]
    for c, one in enumerate(chains):
        assert ao.mismatches(one, parts[c]) == [] and one.maxlag == 5
        assert np.array_equal(one.mcse, one.std * np.sqrt(one.tau / one.n))
        assert np.allclose(one.mcse, np.sqrt(one.var * one.tau / one.n), rtol=1e-14)
    cs = k.ChainSummaries(chains)
    assert np.array_equal(cs.ess, (parts[0]["ess"] + parts[1]["ess"]) + parts[2]["ess"])
    assert cs.pooled.tau is None and cs.pooled.ess is None
