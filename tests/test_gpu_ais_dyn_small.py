"""GPU: the one-workgroup AIS driver beyond KABC_MAX_DIM = 16 parameters (csrc/ais_dyn_small_kernel.hpp):
one workgroup per chain, a team of lanes per walker, every generation of a call in one launch, many
chains per handle.  Same draws, same operation order: every comparison is np.array_equal -- against the
oracle, against the launch-per-half-generation driver (KABC_AIS_SMALL=0) and against single-chain handles."""
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S5 = [11, 12, 13, 14, 15]


def _models(k):
    """the shapes of tests/test_gpu_dyn_dim.py at small ensembles"""
    rng = np.random.default_rng(4)
    return {
        "rosen_d17_box": (k.ApproxKernelizedPosterior(k.Factored(*[k.Uniform(-5, 5)] * 17),
                                                      k.costs.Rosenbrock(), 2.0), 50),
        "gauss_d40_normal": (k.ApproxKernelizedPosterior(k.MvNormal(40, 3.0),
                                                         k.costs.GaussDist(rng.normal(size=40)), 0.5), 100),
        "shell_d24_threshold": (k.ApproxPosterior(k.Factored(*[k.Normal(0, 1)] * 24),
                                                  k.costs.NormShell(4.0), 0.5), 64),
        "hier_d34_mixed": (k.ApproxKernelizedPosterior(
            k.Factored(k.Normal(0, 5), k.Uniform(0, 5), *[k.Normal(0, 1)] * 30, k.Gamma(2.0, 1.0),
                       k.DiscreteUniform(-3, 3)),
            k.costs.HierGaussSim(rng.normal(size=32)), 1.0), 100),
        "gauss_d128": (k.ApproxPosterior(k.Product([k.Uniform(-2, 2)] * 128),
                                         k.costs.GaussDist(np.zeros(128)), 12.0), 140),
    }


def _d20(k, centre=0.0):
    return k.ApproxKernelizedPosterior(k.Factored(*[k.Normal(0, 3)] * 20), k.costs.GaussDist(np.full(20, centre)), 1.0)


def _halves(k, monkeypatch, *a, **kw):
    """a handle on the launch-per-half-generation driver"""
    with monkeypatch.context() as m:
        m.setenv("KABC_AIS_SMALL", "0")
        e = k.AisEnsemble(*a, **kw)
    assert e.driver == "halves"
    return e


def _same(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


# ---- 1. oracle parity ---------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [1, 6])
@pytest.mark.parametrize("name", ["rosen_d17_box", "gauss_d40_normal", "shell_d24_threshold",
                                  "hier_d34_mixed", "gauss_d128"])
def test_oracle_parity(k, orc, gpu_ctx, monkeypatch, name, nt):
    monkeypatch.delenv("KABC_AIS_SMALL", raising=False)
    model, N = _models(k)[name]
    gens, seed = 4, 21
    if name == "gauss_d128":
        # 160 KiB hold one team of 64 lanes beside this ensemble: 70 rounds per half-step.  A single chain
        # takes the driver by default only where a half is ONE round of teams (the rest is not measured),
        # and on request beyond that
        d = k.AisEnsemble(model, N, seed=seed)
        assert d.driver == "halves"
        d.close()
        monkeypatch.setenv("KABC_AIS_SMALL", "1")
    _oracle_parity(k, orc, monkeypatch, model, N, nt, gens, seed)


@pytest.mark.parametrize("N", [30, 200])
def test_oracle_parity_team_widths(k, orc, gpu_ctx, monkeypatch, N):
    """teams of 32 and of 4 lanes (the sizes above land on 8, 16 and 64).  ais_dyn_small_plan at D = 17: the
    coordinates can use Tcap = 32 lanes; T halves from there while a workgroup of 512 has fewer than
    rows0 = ceil(N / 2) teams.  N = 30: 512 / 32 = 16 >= 15, T = 32.  N = 200: 16, 32, 64 < 100, T = 4
    (128 teams, one round; 118 KB of LDS)"""
    monkeypatch.delenv("KABC_AIS_SMALL", raising=False)
    model, _ = _models(k)["rosen_d17_box"]
    _oracle_parity(k, orc, monkeypatch, model, N, nt=3, gens=4, seed=21)


def _oracle_parity(k, orc, monkeypatch, model, N, nt, gens, seed):
    e = k.AisEnsemble(model, N, seed=seed).init()
    assert e.driver == "small"
    h = _halves(k, monkeypatch, model, N, seed=seed).init()
    c = k.AisEnsemble(model, N, seed=seed).init()          # advanced in several chunks
    o = orc.OracleAIS(model, N, seed=seed).init()
    assert _same(e.state()[:3], o.state()[:3]) and _same(h.state()[:3], o.state()[:3])     # step(init)
    for x in (e, h):
        x.set_debug(nt)
    tr1, trh = e.advance(1, nt, collect=True), h.advance(1, nt, collect=True)
    tro, reco = o.generations_sync(1, nt, trace=True)
    assert np.array_equal(tr1, tro) and np.array_equal(trh, tro)
    n0 = (N + 1) // 2
    ro = reco[0].copy()
    ro[:n0, :, 2:5] = np.where(ro[:n0, :, 2:5] >= 0, ro[:n0, :, 2:5] - n0, -1)   # partner ids -> rows
    assert np.array_equal(e.get_debug(nt), ro) and np.array_equal(h.get_debug(nt), ro)
    for x in (e, h):
        x.set_debug(0)
    tr, trh = e.advance(gens, nt, collect=True), h.advance(gens, nt, collect=True)
    tro = o.generations_sync(gens, nt)
    assert np.array_equal(tr, tro) and np.array_equal(trh, tro)
    # gen 0 and the four that follow, as calls of 1 + 3 + 1 generations
    trc = np.concatenate([c.advance(1, nt, collect=True), c.advance(3, nt, collect=True), c.advance(1, nt, collect=True)])
    assert np.array_equal(trc[0], tr1[0]) and np.array_equal(trc[1:], tro)
    assert _same(e.state(), o.state()) and _same(h.state(), o.state()) and _same(c.state(), o.state())
    assert e.stats() == o.stats() == h.stats() == c.stats()
    for x in (e, h, c):
        x.close()


# ---- 2. chains ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_chain_costs", [False, True])
def test_chains_equal_single_chain_handles(k, gpu_ctx, per_chain_costs):
    costs = [k.costs.GaussDist(np.full(20, 0.1 * r)) for r in range(5)] if per_chain_costs else None
    ens = k.AisEnsemble(_d20(k), 60, seeds=S5, costs=costs).init()
    assert ens.driver == "small" and ens.nchains == 5
    tr = ens.advance(3, 2, collect=True)                    # [gen][chain][N][D]
    st = ens.state()
    for c, sd in enumerate(S5):
        one = k.AisEnsemble(_d20(k, 0.1 * c if per_chain_costs else 0.0), 60, seed=sd).init()
        assert np.array_equal(tr[:, c], one.advance(3, 2, collect=True)), c
        assert _same([a[c] for a in st[:3]], one.state()[:3]), c
        one.close()
    ens.close()


def test_mcmcthreads_beyond_16_parameters(k, gpu_ctx):
    """sample(model, AIS(60), MCMCThreads(), 60, 4) at D = 20: refused before this driver existed"""
    from kissabc_jl_amd.api import chain_seeds
    model, kw = _d20(k, 0.3), dict(ntransitions=2, discard_initial=120, return_array=True)
    out = k.sample(model, k.AIS(60), k.MCMCThreads(), 60, 4, seed=9, **kw)
    ref = np.concatenate([k.sample(model, k.AIS(60), 60, seed=s, **kw) for s in chain_seeds(9, 4)])
    assert out.shape == (240, 20) and np.array_equal(out, ref)


def test_failed_initial_draw_names_its_chain(k, gpu_ctx):
    prior = k.Factored(*[k.Uniform(-1, 1)] * 20)
    costs = [k.costs.GaussDist(np.full(20, 0.1 * r)) for r in range(5)]
    costs[3] = k.costs.GaussDist(np.full(20, 1e200))        # +Inf on the whole support
    ens = k.AisEnsemble(k.ApproxPosterior(prior, costs[0], 3.0), 60, seeds=S5, costs=costs)
    with pytest.raises(k.KabcError, match=r"^chain 3: Prior leads to ∞ costs too often"):
        ens.init(5)
    ens.close()


# ---- 3. fallbacks -------------------------------------------------------------------------------------
def test_shapes_too_large_for_lds(k, orc, gpu_ctx):
    from kissabc_jl_amd.api import chain_seeds
    model, N = _d20(k, 0.2), 4096
    e = k.AisEnsemble(model, N, seed=3).init()
    assert e.driver == "halves"
    o = orc.OracleAIS(model, N, seed=3).init()
    assert np.array_equal(e.advance(2, 3, collect=True), o.generations_sync(2, 3)) and _same(e.state(), o.state())
    e.close()
    with pytest.raises(k.KabcError, match="bytes of LDS") as err:
        k.AisEnsemble(model, N, seeds=S5[:2])
    assert err.value.status == k._cdefs.KABC_ERR_UNSUPPORTED
    out = k.sample(model, k.AIS(N), k.MCMCThreads(), 100, 2, seed=4, return_array=True)
    ref = np.concatenate([k.sample(model, k.AIS(N), 100, seed=s, return_array=True) for s in chain_seeds(4, 2)])
    assert np.array_equal(out, ref)


def test_sample_batch_courses(k, gpu_ctx):
    models = [_d20(k, 0.1 * r) for r in range(3)]
    kw = dict(seeds=S5[:3], ntransitions=2, discard_initial=60, return_array=True)
    dflt = k.sample_batch(models, k.AIS(60), 60, **kw)
    grid = k.sample_batch(models, k.AIS(60), 60, course="grid", **kw)
    seq = k.sample_batch(models, k.AIS(60), 60, course="sequential", **kw)
    assert (dflt.info["course"], grid.info["course"], seq.info["course"]) == ("sequential", "grid", "sequential")
    assert grid.info["driver"] == "small"
    for r in range(3):
        assert np.array_equal(grid[r], dflt[r]) and np.array_equal(seq[r], dflt[r]), r
    with pytest.raises(k.KabcError, match="bytes of LDS"):
        k.sample_batch(models, k.AIS(4096), 60, course="grid", **kw)


# ---- 4. plumbing --------------------------------------------------------------------------------------
def test_resume_launch_count_trace_blocks_discard(k, orc, gpu_ctx, monkeypatch):
    monkeypatch.delenv("KABC_AIS_SMALL", raising=False)
    model, N = _d20(k, 0.1), 100
    a = k.AisEnsemble(model, N, seed=5).init()
    o = orc.OracleAIS(model, N, seed=5).init()
    a.set_timing(64, stride=1)
    for gens, nt in ((5, 4), (3, 1)):                       # one launch per call (test_gpu_ais_small.py)
        a.advance(gens, nt)
        o.generations_sync(gens, nt, collect=False)
        ms, n = a.kernel_ms()
        assert n == 1 and ms > 0
    b = k.AisEnsemble(model, N, seed=5)                    # AISState round trip into a new handle (the seed
    #                                                        addresses the streams and is the handle's, not the state's)
    b.set_state(*a.state())
    assert b.driver == "small"
    monkeypatch.setenv("KABC_TRACE_CHUNK_MIB", "1")         # 16 000 B per generation: 3 blocks
    got = b.advance(150, 1, collect=True)
    monkeypatch.delenv("KABC_TRACE_CHUNK_MIB")
    assert np.array_equal(got, o.generations_sync(150, 1)) and _same(b.state(), o.state())
    assert np.array_equal(got, a.advance(150, 1, collect=True))
    out = k.sample(model, k.AIS(N), 250, seed=5, discard_initial=350, ntransitions=2, return_array=True)
    o2 = orc.OracleAIS(model, N, seed=5).init()
    o2.generations_sync(4, 2, collect=False)
    assert np.array_equal(out, o2.generations_sync(3, 2).reshape(-1, 20)[:250])
    a.close()
    b.close()


# ---- 5. cancel ----------------------------------------------------------------------------------------
def test_cancel_from_a_host_thread(k, orc):
    """as tests/test_gpu_cancel.py: a call sized to ~5 s is cancelled after 0.3 s, raises Cancelled within
    0.25 s, leaves the state of a completed generation, and goes on from there like the oracle"""
    model, N, nt = _d20(k, 0.1), 60, 1
    ctx = k.Context(0)
    try:
        ens = k.AisEnsemble(model, N, seed=11, ctx=ctx).init()
        assert ens.driver == "small"
        t0 = time.perf_counter()
        ens.advance(2000, nt)
        G = max(int(5.0 / ((time.perf_counter() - t0) / 2000)), 2)
        box = {}

        def fire():
            box["t"] = time.perf_counter()
            ctx.cancel()

        tm = threading.Timer(0.3, fire)
        tm.start()
        with pytest.raises(k.Cancelled):
            ens.advance(G, nt)
        lat = time.perf_counter() - box["t"]
        tm.join()
        print(f"[cancel latency] ais one-workgroup driver, D 20: {lat * 1e3:.2f} ms")
        assert lat < 0.25
        x, lp, ll, t = ens.state()
        kg = t // nt - 2000
        assert t % nt == 0 and 0 < kg < G
        tr = ens.advance(20, nt, collect=True)
        ens.close()
    finally:
        ctx.close()
    # the state is that of a completed generation: the uncancelled run of exactly that length
    ref = k.AisEnsemble(model, N, seed=11).init()
    ref.advance(2000 + kg, nt)
    assert _same((x, lp, ll, t), ref.state())
    ref.close()
    # ... and advancing further equals the oracle from that generation
    o = orc.OracleAIS(model, N, seed=11)
    o.set_state(x, lp, ll, t)
    assert np.array_equal(tr, o.generations_sync(20, nt))


@pytest.mark.parametrize("waves", ["1", "16"])
def test_lds_waves_knob_same_bits(k, orc, gpu_ctx, monkeypatch, waves):
    """KABC_DYN_LDS_WAVES (A/B runs: the wavefronts per CU the rows in LDS leave room for, hence the team width)
    promises the same bits: D = 20, N = 2048 on the launch-per-half-generation driver"""
    monkeypatch.setenv("KABC_DYN_LDS_WAVES", waves)
    model, N = _d20(k, 0.2), 2048
    e = k.AisEnsemble(model, N, seed=3).init()
    assert e.driver == "halves"
    o = orc.OracleAIS(model, N, seed=3).init()
    assert np.array_equal(e.advance(2, 3, collect=True), o.generations_sync(2, 3)) and _same(e.state(), o.state())
    assert e.stats() == o.stats()
    e.close()
