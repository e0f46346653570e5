"""No GPU: sample_batch's `course` argument is checked before anything touches the device, and
sample(model, AIS(N), MCMCThreads(), Ns, Nc) falls back to one sample() call per chain, with
chain_seeds(seed, Nc), when the batch handle answers KABC_ERR_UNSUPPORTED (beyond KABC_MAX_DIM
parameters: an ensemble too large for one workgroup's LDS, a user cost)."""
import numpy as np
import pytest


def _model(k, D=20):
    return k.ApproxKernelizedPosterior(k.Factored(*[k.Normal(0, 3)] * D), k.costs.GaussDist(np.zeros(D)), 1.0)


class _FakeEnsemble:
    """AisEnsemble without a device: a batch handle is refused with `status`; a single chain's trace is
    a function of its seed alone"""
    status = None
    created = []

    def __init__(self, model, nparticles, seed=0, ctx=None, seeds=None, costs=None, **kw):
        from kissabc_jl_amd import _lib
        type(self).created.append(("batch", list(seeds)) if seeds is not None else ("single", int(seed)))
        if seeds is not None:
            raise _lib.KabcError(type(self).status, "refused")
        self.N, self.D, self.seed = int(nparticles), len(model), int(seed)
        self.driver = "halves"

    def init(self, retry_sampling=100):
        return self

    def advance(self, ngenerations, ntransitions=1, collect=False, out=None):
        if out is not None:
            out[...] = (self.seed % 1009) + np.arange(out.size, dtype=np.float64).reshape(out.shape)
        return out

    def close(self):
        pass


@pytest.fixture
def fake(k, monkeypatch):
    from kissabc_jl_amd import api
    monkeypatch.setenv("KABC_PINNED_TRACE", "0")
    monkeypatch.setattr(api, "AisEnsemble", _FakeEnsemble)
    _FakeEnsemble.created = []
    return _FakeEnsemble


@pytest.mark.parametrize("course", ["Grid", "auto", 0, True, "batch"])
def test_sample_batch_course_is_checked_first(k, course):
    with pytest.raises(ValueError, match="course must be None"):
        k.sample_batch(_model(k), k.AIS(60), 60, nruns=2, course=course)
    with pytest.raises(TypeError):                      # (the sampler's check still comes before it)
        k.sample_batch(_model(k), "AIS", 60, nruns=2, course=course)


def test_mcmcthreads_falls_back_to_one_call_per_chain(k, fake):
    from kissabc_jl_amd import _cdefs as cd
    fake.status = cd.KABC_ERR_UNSUPPORTED
    model, Ns, Nc = _model(k), 60, 3
    out = k.sample(model, k.AIS(60), k.MCMCThreads(), Ns, Nc, seed=5, return_array=True)
    from kissabc_jl_amd.api import chain_seeds
    seeds = chain_seeds(5, Nc)
    assert fake.created == [("batch", seeds)] + [("single", s) for s in seeds]
    assert out.shape == (Nc * Ns, 20)
    for c, s in enumerate(seeds):                        # chainsstack: chain after chain
        ref = k.sample(model, k.AIS(60), Ns, seed=s, return_array=True)
        assert np.array_equal(out[c * Ns:(c + 1) * Ns], ref)


def test_mcmcthreads_other_errors_are_raised(k, fake):
    from kissabc_jl_amd import _cdefs as cd
    fake.status = cd.KABC_ERR_INVALID_ARG
    with pytest.raises(k.KabcError, match="refused"):
        k.sample(_model(k), k.AIS(60), k.MCMCThreads(), 60, 3, return_array=True)
    assert len(fake.created) == 1


def test_sample_batch_courses_without_a_batch_handle(k, fake):
    """"grid" raises where the batch handle is refused, at any length(prior); "sequential" never asks for it;
    None asks for it up to KABC_MAX_DIM parameters only"""
    from kissabc_jl_amd import _cdefs as cd
    fake.status = cd.KABC_ERR_UNSUPPORTED
    for D in (4, 20):
        fake.created = []
        with pytest.raises(k.KabcError, match="refused"):
            k.sample_batch(_model(k, D), k.AIS(60), 60, nruns=2, course="grid", return_array=True)
        assert [c[0] for c in fake.created] == ["batch"]
        fake.created = []
        out = k.sample_batch(_model(k, D), k.AIS(60), 60, nruns=2, course="sequential", return_array=True)
        assert out.info["course"] == "sequential" and [c[0] for c in fake.created] == ["single", "single"]
        fake.created = []
        out = k.sample_batch(_model(k, D), k.AIS(60), 60, nruns=2, return_array=True)
        assert out.info["course"] == "sequential"
        assert [c[0] for c in fake.created] == (["batch"] if D <= cd.KABC_MAX_DIM else []) + ["single", "single"]


def test_oracle_refuses_a_transition_counter_beyond_the_streams(k, orc):
    """the stream address holds 56 bits of the transition counter (include/kabc_philox.h): the oracle refuses
    set_state at or beyond 2^56, and an advance that would count past it, as kabc_ais_set_state and
    kabc_ais_advance do (the library's refusals need a handle: tests/test_gpu_stream_counter.py)"""
    from kissabc_jl_amd import _cdefs as cd
    model = k.ApproxKernelizedPosterior(k.Factored(k.Uniform(-5, 5), k.Uniform(-5, 5)), k.costs.Rosenbrock(), 1.0)
    o = orc.OracleAIS(model, 12, seed=1).init()
    x, lp, ll, t = o.state()
    assert t == 0
    for bad in (2 ** 56, 2 ** 56 + 5, 2 ** 64 - 1):
        with pytest.raises(orc.OracleError, match=r"kabc_ais_set_state: t = %d, the transition counter must be below 2\^56" % bad) as e:
            o.set_state(x, lp, ll, bad)
        assert e.value.status == cd.KABC_ERR_INVALID_ARG
    assert o.state()[3] == 0                       # (a refused state changes nothing)
    o.set_state(x, lp, ll, 2 ** 56 - 16)
    with pytest.raises(orc.OracleError, match=r"kabc_ais_advance: the transition counter t = %d would pass 2\^56" % (2 ** 56 - 16)):
        o.generations_sync(3, 8)
    assert o.state()[3] == 2 ** 56 - 16 and np.array_equal(o.state()[0], x)
    o.generations_sync(2, 8)                       # the last two admissible generations
    assert o.state()[3] == 2 ** 56
    with pytest.raises(orc.OracleError, match="would pass"):
        o.generations_sync(1, 1)
    with pytest.raises(orc.OracleError, match="kabc_ais_half_generation"):
        o.half_generation(0, 1, 0, 6)
    with pytest.raises(orc.OracleError, match="kabc_ais_end_generation"):
        o.end_generation(1)
    o.generations_sync(0, 8)                       # (nothing to count)
