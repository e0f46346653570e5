"""-m gpu: the wide geometry of the AIS half-generation kernel (csrc/ais_kernels.hpp WideGeom: 512
threads, two batches per workgroup, producer shares by SIMD placement) against
  (a) the CPU oracle's sync schedule, bit for bit,
  (b) the existing geometry (KABC_AIS_WIDE=0) on trace, state, counters and the per-transition
      debug records, bit for bit,
  (c) itself: one handle advanced in two calls against one call.
KABC_AIS_WIDE=2 takes the wide kernel below its cut-over and makes a launch that cannot take it an
error, so no case passes on the existing kernel by accident; =1 quietly keeps the existing kernel
there.  Shapes: rows per half around the two-batch workgroup (128 = one full workgroup), sub-steps
around the chunk of kWideK = 4.

Not covered: the equal-shares branch of the task table (a placement other than the two consumers on
two SIMDs with one producer beside each).  Nobody controls where the hardware puts a wave, and the
shipped variant has n_c = 1, so no case here can make the kernel take it.  It deals the same 2K
tasks, and a record is a pure function of (seed, walker, t, slot), so it cannot change a value; it
is not exercised."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 4  # csrc/ais_kernels.hpp kWideK


def _models(k):
    return {
        "box8": k.ApproxKernelizedPosterior(k.Factored(*[k.Uniform(-5, 5)] * 8), k.costs.Rosenbrock(), 1.0),
        "box2": k.ApproxKernelizedPosterior(k.Factored(*[k.Uniform(-5, 5)] * 2), k.costs.Rosenbrock(), 1.0),
        "normal4": k.ApproxKernelizedPosterior(k.Factored(*[k.Normal(0, 2)] * 4), k.costs.Rosenbrock(), 1.0),
        "simple4": k.ApproxKernelizedPosterior(
            k.Factored(k.Uniform(-3, 3), k.Normal(0, 2), k.TruncatedNormal(0, 2, -3, 3), k.Uniform(-4, 4)),
            k.costs.Rosenbrock(), 1.0),
        "general4": k.ApproxKernelizedPosterior(
            k.Factored(k.Gamma(2.5, 0.7), k.LogNormal(0.3, 0.6), k.Exponential(2.0), k.Beta(2, 3)),
            k.costs.Rosenbrock(), 2.0),
        # a discrete component: push_p rounds it (BOX class)
        "discrete3": k.ApproxKernelizedPosterior(
            k.Factored(k.Uniform(-3, 3), k.DiscreteUniform(-3, 3), k.Uniform(-3, 3)), k.costs.Rosenbrock(), 2.0),
        # ApproxPosterior (threshold acceptance, posterior kind 2)
        "threshold2": k.ApproxPosterior(k.Factored(*[k.Uniform(-5, 5)] * 2), k.costs.Rosenbrock(), 30.0),
    }


def _run(k, monkeypatch, model, N, nt, seed, wide, split=False):
    monkeypatch.setenv("KABC_AIS_WIDE", wide)
    ens = k.AisEnsemble(model, N, seed=seed).init()
    assert ens.driver == "halves"
    ens.set_debug(nt)
    g1 = ens.advance(1, nt, collect=True)
    dbg = ens.get_debug(nt)
    ens.set_debug(0)
    if split:
        g2 = np.concatenate([ens.advance(1, nt, collect=True), ens.advance(1, nt, collect=True)])
    else:
        g2 = ens.advance(2, nt, collect=True)
    xs, lps, lls, t = ens.state()
    out = {"g1": g1, "dbg": dbg, "g2": g2, "x": xs, "lp": lps, "ll": lls, "t": t, "stats": ens.stats()}
    ens.close()
    return out


def _same(a, b, what):
    for key in ("g1", "dbg", "g2", "x", "lp", "ll"):
        assert np.array_equal(a[key], b[key]), (what, key)
    assert a["t"] == b["t"] and a["stats"] == b["stats"], what


def _check(k, orc, monkeypatch, name, rows, nt, force="2"):
    monkeypatch.setenv("KABC_AIS_SMALL", "0")
    monkeypatch.setenv("KABC_SPECIALIZE", "0")   # the prebuilt kernels: the model's own have one geometry
    model, N = _models(k)[name], 2 * rows
    for seed in (1, 2):
        wide = _run(k, monkeypatch, model, N, nt, seed, force)
        # (b) the existing geometry, (c) two calls against one
        _same(wide, _run(k, monkeypatch, model, N, nt, seed, "0"), f"wide != existing, seed {seed}")
        _same(wide, _run(k, monkeypatch, model, N, nt, seed, force, split=True), f"resume, seed {seed}")
        # (a) the oracle: trace, move ids, accept and evaluated flags, partner rows, state, counters
        o = orc.OracleAIS(model, N, seed=seed).init()
        ref, tr = o.generations_sync(1, nt, trace=True)
        dbg = wide["dbg"]
        assert np.array_equal(wide["g1"], ref)
        for col in (0, 1, 5):
            assert np.array_equal(dbg[:, :, col], tr[0, :, :, col]), col
        base = np.where(np.arange(N) < rows, rows, 0)[:, None]
        for col in (2, 3, 4):
            d = dbg[:, :, col].astype(np.int64)
            assert np.array_equal(np.where(d >= 0, d + base, -1), tr[0, :, :, col].astype(np.int64)), col
        assert np.array_equal(wide["g2"], o.generations_sync(2, nt))
        xo, lpo, llo, to = o.state()
        assert wide["t"] == to == 3 * nt
        assert np.array_equal(wide["x"], xo) and np.array_equal(wide["lp"], lpo) and np.array_equal(wide["ll"], llo)
        assert wide["stats"] == o.stats()
        # the records cover stretch, DE and walk
        assert set(np.unique(dbg[:, :, 0]).tolist()) == {1, 2, 3}


@pytest.mark.parametrize("rows", [128, 129, 191, 192, 193, 255])
def test_wide_rows_around_the_workgroup(k, orc, gpu_ctx, monkeypatch, rows):
    """the second batch of the last workgroup full, empty but one row, ragged, absent"""
    _check(k, orc, monkeypatch, "box8", rows, K + 1)


def test_wide_below_two_batches_keeps_existing_kernel(k, orc, gpu_ctx, monkeypatch):
    """127 rows per half: KABC_AIS_WIDE=1 quietly takes the existing kernel; =2 says so"""
    _check(k, orc, monkeypatch, "box8", 127, K + 1, force="1")
    monkeypatch.setenv("KABC_AIS_WIDE", "2")
    ens = k.AisEnsemble(_models(k)["box8"], 254, seed=1).init()
    with pytest.raises(k.KabcError, match="wide"):
        ens.advance(1, K + 1)
    ens.close()


@pytest.mark.parametrize("nt", [1, K - 1, K, 2 * K, 2 * K + 1])
def test_wide_substeps_around_the_chunk(k, orc, gpu_ctx, monkeypatch, nt):
    """below the cut-over, forced; 1 and 2K + 1 end on a single-sub-step chunk (K + 1: the rows test)"""
    _check(k, orc, monkeypatch, "box8", 193, nt)


@pytest.mark.parametrize("name", ["box2", "normal4", "simple4", "general4", "discrete3", "threshold2"])
def test_wide_prior_classes_and_kinds(k, orc, gpu_ctx, monkeypatch, name):
    _check(k, orc, monkeypatch, name, 129, K + 1)


def test_wide_placement_independence(k, orc, gpu_ctx, monkeypatch):
    """one case twice in one process (the hardware may place the waves differently): equal"""
    monkeypatch.setenv("KABC_AIS_SMALL", "0")
    monkeypatch.setenv("KABC_SPECIALIZE", "0")
    model = _models(k)["box8"]
    first = _run(k, monkeypatch, model, 386, 2 * K + 1, 1, "2")
    _same(first, _run(k, monkeypatch, model, 386, 2 * K + 1, 1, "2"), "second run")


def test_wide_default_dispatch(k, orc, gpu_ctx, monkeypatch):
    """the default rule (no KABC_AIS_WIDE) at the smallest launch that takes the wide kernel on a
    256-unit device -- 32 sub-steps, two batches per compute unit and half -- against the existing
    geometry: equal trace, state and counters.  The unit count is the MI355X's; on a device with
    more units the default rule keeps the existing kernel and this compares that kernel with itself
    (nothing the library exports says which kernel ran; the forced cases above cannot pass on the
    existing one)."""
    monkeypatch.setenv("KABC_AIS_SMALL", "0")
    monkeypatch.setenv("KABC_SPECIALIZE", "0")
    monkeypatch.delenv("KABC_AIS_WIDE", raising=False)
    model, N, nt = _models(k)["box8"], 2 * 2 * 64 * 256, 32
    runs = []
    for wide in (None, "0"):
        if wide is not None:
            monkeypatch.setenv("KABC_AIS_WIDE", wide)
        ens = k.AisEnsemble(model, N, seed=2).init()
        runs.append((ens.advance(1, nt, collect=True), ens.state(), ens.stats()))
        ens.close()
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][2] == runs[1][2]
    for a, b in zip(runs[0][1][:3], runs[1][1][:3]):
        assert np.array_equal(a, b)
