"""No GPU: what the posterior-summary entry points refuse before a context is used, the Python-side
exclusions of summary=True, and the course sample(..., summary=True) takes over an ensemble -- on a fake
AisEnsemble whose summary is the numpy restatement (tests/ais_summary_oracle.py) of a trace that is a
function of the seed alone, so that ChainSummaries' `.pooled` and `.rhat` are checked against numpy."""
import ctypes as C

import numpy as np
import pytest

import ais_summary_oracle as so


def _model(k, D=3):
    return k.ApproxKernelizedPosterior(k.Factored(*[k.Normal(0, 3)] * D), k.costs.GaussDist(np.zeros(D)), 1.0)


def test_null_handle_is_refused_by_every_entry_point(k):
    from kissabc_jl_amd import _cdefs as cd, _lib
    lib = _lib.load()
    n = C.c_int64(-7)
    calls = [lambda: lib.kabc_ais_summary_begin(None, cd.SUMMARY_AUTO),
             lambda: lib.kabc_ais_advance_summary(None, 1, 1, None),
             lambda: lib.kabc_ais_summary_get(None, C.byref(n), None, None, None, None, None, None, None),
             lambda: lib.kabc_ais_summary_end(None)]
    for call in calls:
        assert call() == cd.KABC_ERR_INVALID_ARG
        assert b"NULL" in lib.kabc_last_error()
    assert n.value == -7                                    # (outputs are left untouched)


def test_prototypes_and_modes(k):
    from kissabc_jl_amd import _cdefs as cd
    assert (cd.SUMMARY_AUTO, cd.SUMMARY_FULL, cd.SUMMARY_DIAG) == (0, 1, 2)
    assert len(cd.PROTOTYPES["kabc_ais_summary_get"][1]) == 9
    assert k.AisEnsemble.COV_MODES == {None: 0, "full": 1, "diag": 2}


def test_python_side_exclusions(k):
    ens = object.__new__(k.AisEnsemble)                     # (no handle: the checks come first)
    ens._h = C.c_void_p()
    with pytest.raises(ValueError, match="excludes collect / out"):
        ens.advance(1, 1, collect=True, summary=True)
    with pytest.raises(ValueError, match="excludes collect / out"):
        ens.advance(1, 1, out=np.empty((1, 8, 2)), summary=True)
    for cov in ("Full", "diagonal", 1, True):
        with pytest.raises(ValueError, match='cov must be "full", "diag" or None'):
            ens.summary_begin(cov)
    with pytest.raises(ValueError, match="excludes return_array"):
        k.sample(_model(k), k.AIS(20), 40, summary=True, return_array=True)
    with pytest.raises(ValueError, match="excludes return_array"):
        k.sample(_model(k), k.AIS(20), k.MCMCThreads(), 40, 2, summary=True, return_array=True)
    with pytest.raises(ValueError, match="excludes return_array"):
        k.sample_batch(_model(k), k.AIS(20), 40, nruns=2, summary=True, return_array=True)
    with pytest.raises(TypeError):                          # (the sampler's check still comes first)
        k.sample(_model(k), "AIS", 40, summary=True, return_array=True)
    ens._h = None                                           # (nothing for __del__ to destroy)


def _trace_of(seed, G, N, D):
    rng = np.random.default_rng(seed % 1009)
    return rng.normal(seed % 7, 1.0 + seed % 3, (G, N, D))


class _FakeEnsemble:
    """AisEnsemble without a device: a batch handle is refused with `status`; a single chain's kept
    generations are a function of its seed, and its summary is the restatement's"""
    status = None
    log = []

    def __init__(self, model, nparticles, seed=0, ctx=None, seeds=None, costs=None, **kw):
        from kissabc_jl_amd import _lib
        if seeds is not None:
            raise _lib.KabcError(type(self).status, "refused")
        self.N, self.D, self.seed, self.calls = int(nparticles), len(model), int(seed), []
        self.driver = "halves"
        type(self).log.append(self.calls)

    def init(self, retry_sampling=100):
        self.calls.append(("init", retry_sampling))
        return self

    def advance(self, ngenerations, ntransitions=1, collect=False, out=None, summary=False):
        self.calls.append(("advance", ngenerations, ntransitions, summary))
        if summary:
            self.kept = _trace_of(self.seed, ngenerations, self.N, self.D)

    def summary_begin(self, cov=None):
        self.calls.append(("begin", cov))
        return self

    def summary(self):
        self.calls.append(("summary",))
        s = so.summarize(self.kept)
        return type(self).k.PosteriorSummary(s["n"], s["mean"], s["cov"], s["min"], s["max"], s["pivot"], s["sum1"],
                                             s["sum2"])

    def close(self):
        self.calls.append(("close",))


@pytest.fixture
def fake(k, monkeypatch):
    from kissabc_jl_amd import api, _cdefs as cd
    monkeypatch.setattr(api, "AisEnsemble", _FakeEnsemble)
    _FakeEnsemble.k, _FakeEnsemble.log, _FakeEnsemble.status = k, [], cd.KABC_ERR_UNSUPPORTED
    return _FakeEnsemble


def test_sample_summary_discards_then_summarises_whole_generations(k, fake):
    s = k.sample(_model(k), k.AIS(20), 45, ntransitions=4, discard_initial=30, retry_sampling=7, seed=3, summary=True)
    assert fake.log == [[("init", 7), ("advance", 2, 4, False), ("begin", None), ("advance", 3, 4, True),
                         ("summary",), ("close",)]]
    assert isinstance(s, k.PosteriorSummary) and s.n == 60          # ceil(45 / 20) * 20 > Ns
    assert so.mismatches(s, so.summarize(_trace_of(3, 3, 20, 3))) == []
    assert np.array_equal(s.std, np.sqrt(np.diagonal(s.cov))) and s.nchains is None
    assert repr(s) == "[" + ", ".join(f"{m:.4g} ± {sd:.2g}" for m, sd in zip(s.mean, s.std)) + "]"
    assert s.isapprox(s.mean).all() and not s.isapprox(s.mean + 3 * s.std).any()
    assert s.isapprox(s.mean + 2.5 * s.std, nsigma=3.0).all()


def test_mcmcthreads_summary_per_chain_pooled_and_rhat(k, fake):
    from kissabc_jl_amd.api import chain_seeds
    Nc, N, D, Ns = 4, 20, 3, 60
    out = k.sample(_model(k), k.AIS(N), k.MCMCThreads(), Ns, Nc, seed=5, summary=True)
    seeds = chain_seeds(5, Nc)
    assert isinstance(out, k.ChainSummaries) and len(out) == Nc
    traces = [_trace_of(sd, 3, N, D) for sd in seeds]
    for s, tr in zip(out, traces):
        assert so.mismatches(s, so.summarize(tr)) == []
    x = np.concatenate([t.reshape(-1, D) for t in traces])
    assert out.pooled.n == x.shape[0]
    # (host arithmetic on well-scaled data: a few hundred roundings of unit-size terms)
    assert np.allclose(out.pooled.mean, x.mean(axis=0), rtol=1e-12, atol=1e-12)
    assert np.allclose(out.pooled.cov, np.cov(x, rowvar=False, ddof=1), rtol=1e-12, atol=1e-12)
    assert np.array_equal(out.pooled.min, x.min(axis=0)) and np.array_equal(out.pooled.max, x.max(axis=0))
    n = 3 * N
    means = np.stack([t.reshape(-1, D).mean(axis=0) for t in traces])
    W = np.mean([t.reshape(-1, D).var(axis=0, ddof=1) for t in traces], axis=0)
    rhat = np.sqrt(((n - 1) / n * W + means.var(axis=0, ddof=1)) / W)
    assert np.allclose(out.rhat, rhat, rtol=1e-12)
    assert np.all(out.rhat > 1.0)                                   # (the fake chains sit at different centres)


def test_sample_batch_summary_on_the_sequential_course(k, fake):
    out = k.sample_batch(_model(k), k.AIS(20), 40, nruns=3, seeds=[4, 5, 6], summary=True)
    assert out.info["course"] == "sequential" and len(out) == 3
    for s, sd in zip(out, (4, 5, 6)):
        assert so.mismatches(s, so.summarize(_trace_of(sd, 2, 20, 3))) == []


def test_batch_axis_and_chain(k):
    rng = np.random.default_rng(1)
    parts = [so.summarize(rng.normal(c, 1.0, (3, 9, 2))) for c in range(3)]
    stack = lambda f: np.stack([p[f] for p in parts])   # noqa: E731
    s = k.PosteriorSummary(parts[0]["n"], stack("mean"), stack("cov"), stack("min"), stack("max"), stack("pivot"),
                           stack("sum1"), stack("sum2"))
    assert s.nchains == 3 and s.std.shape == (3, 2)
    for c in range(3):
        assert so.mismatches(s.chain(c), parts[c]) == []
    assert repr(s).count("±") == 6
    with pytest.raises(ValueError):
        s.chain(0).chain(0)
