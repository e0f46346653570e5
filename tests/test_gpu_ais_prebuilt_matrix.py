"""-m gpu: every prebuilt AIS kernel instantiation (csrc/ais_inst.hip: ais_half_kernel, ais_half_wide_kernel
and the one-workgroup kernel, for every cost x D x prior class x posterior kind the tables hold) against the
CPU oracle's sync schedule, bit for bit: the initial state, the first generation with its debug records
(trace, move ids, accept and cost-evaluated flags, partner rows), two more generations, the final state and
the counters.  One test per (family, cost, D) over the whole grid, the variants in a loop inside; every
message names the tuple.  After a run kabc_ctx_last_kernel must name the instantiation the case meant, wave
count included: that is what proves the sweep complete.  Where a table holds no kernel the documented refusal
is asserted and nothing runs.  Cases, shapes and environment: prebuilt_matrix.py."""
import numpy as np
import pytest

import prebuilt_matrix as pm

pytestmark = pytest.mark.gpu

_launched = {f: set() for f in pm.AIS_FAMILIES}   # the tuples kabc_ctx_last_kernel reported, per family
_ran = {f: set() for f in pm.AIS_FAMILIES}        # the (cost, D) ids that ran


def _run_case(k, orc, family, c, D, cls, kind):
    from kissabc_jl_amd import _lib
    who = pm.tuple_name(family, c, D, cls, kind)
    model, N, nt = pm.model(k, c, D, cls, kind), pm.AIS_N[family], pm.AIS_NT
    ens = k.AisEnsemble(model, N, seed=pm.AIS_SEED).init()
    assert ens.driver == ("small" if family == "AIS_SMALL" else "halves"), who
    o = orc.OracleAIS(model, N, seed=pm.AIS_SEED).init()
    for name, a, b in zip(("x", "lp", "ll"), ens.state(), o.state()):
        assert np.array_equal(a, b), (who, "initial", name)
    ens.set_debug(nt)
    g1 = ens.advance(1, nt, collect=True)
    dbg = ens.get_debug(nt)
    ens.set_debug(0)
    ref, tr = o.generations_sync(1, nt, trace=True)
    assert np.array_equal(g1, ref), (who, "trace of generation 1")
    for col, name in ((0, "move ids"), (1, "accept flags"), (5, "cost-evaluated flags")):
        assert np.array_equal(dbg[:, :, col], tr[0, :, :, col]), (who, name)
    rows0 = (N + 1) // 2   # (the device reports partner rows inside the complementary half)
    base = np.where(np.arange(N) < rows0, rows0, 0)[:, None]
    for col in (2, 3, 4):
        d = dbg[:, :, col].astype(np.int64)
        assert np.array_equal(np.where(d >= 0, d + base, -1), tr[0, :, :, col].astype(np.int64)), (who, "partner rows", col)
    assert np.array_equal(ens.advance(2, nt, collect=True), o.generations_sync(2, nt)), (who, "generations 2, 3")
    xs, lps, lls, t = ens.state()
    xo, lpo, llo, to = o.state()
    assert t == to == 3 * nt, who
    for name, a, b in (("x", xs, xo), ("lp", lps, lpo), ("ll", lls, llo)):
        assert np.array_equal(a, b), (who, "final", name)
    assert ens.stats() == o.stats(), who
    got = _lib.last_kernel(ens.ctx)
    ens.close()
    o.close()
    assert got == pm.ais_expected_kernel(family, c, D, cls, kind), (who, "kabc_ctx_last_kernel", got)
    _launched[family].add(got)


def _refused(k, family, c, D, cls, kind):
    """the table holds no kernel: the model is refused for its dimension, or KABC_AIS_WIDE=2 refuses the launch"""
    who = pm.tuple_name(family, c, D, cls, kind)
    if not pm.cost_dim_ok(c, D):
        d_ok = min(d for d in range(1, pm.MAX_DIM + 1) if pm.cost_dim_ok(c, d))
        p, cc = pm.prior(k, D, cls), pm.cost(k, c, d_ok)
        model = (k.CommonLogDensity(D, p, cc) if kind == pm.COMMON else
                 (k.ApproxPosterior if kind == pm.THRESHOLD else k.ApproxKernelizedPosterior)(p, cc, 1.0))
        with pytest.raises(k.KabcError, match=f"does not accept D = {D}"):
            k.AisEnsemble(model, pm.AIS_N[family], seed=pm.AIS_SEED)
        return
    assert family == "AIS_WIDE", who   # (the other tables hold every accepted dimension)
    ens = k.AisEnsemble(pm.model(k, c, D, cls, kind), pm.AIS_N[family], seed=pm.AIS_SEED).init()
    before = ens.stats()
    with pytest.raises(k.KabcError, match="KABC_AIS_WIDE=2: no wide half-generation kernel"):
        ens.advance(1, pm.AIS_NT)
    assert ens.stats() == before, who   # (raised before anything is enqueued)
    ens.close()


@pytest.mark.parametrize("cd", pm.grid_ids(), ids=pm.grid_id_name)
@pytest.mark.parametrize("family", pm.AIS_FAMILIES)
def test_ais_prebuilt(k, orc, gpu_ctx, monkeypatch, family, cd):
    from kissabc_jl_amd import _lib
    c, D = cd
    monkeypatch.setenv("KABC_SPECIALIZE", "0")
    monkeypatch.delenv("KABC_PREBUILT_CLASS", raising=False)
    for name, value in pm.AIS_ENV[family].items():
        monkeypatch.setenv(name, value)
    for cls, kind in pm.ais_variants(family):
        if _lib.prebuilt_has(family, c, D, pm.pcx(cls, kind)):
            _run_case(k, orc, family, c, D, cls, kind)
        else:
            _refused(k, family, c, D, cls, kind)
    _ran[family].add(cd)


@pytest.mark.parametrize("family", pm.AIS_FAMILIES)
def test_ais_sweep_is_complete(k, family):
    """after the whole sweep of a family (this file run as a whole): the instantiations that
    kabc_ctx_last_kernel reported are exactly the ones the drivers can dispatch -- every entry of the
    AIS_HALF and AIS_WIDE tables; of AIS_SMALL's all but the NORMAL class above seven parameters, which
    the one-workgroup driver runs on its GENERAL kernel"""
    from kissabc_jl_amd import _lib
    want = {pm.ais_expected_kernel(family, c, D, cls, kind) for c, D in pm.grid_ids()
            for cls, kind in pm.ais_variants(family) if _lib.prebuilt_has(family, c, D, pm.pcx(cls, kind))}
    print(family, "launched", len(_launched[family]), "of", len(want), "dispatchable tuples;",
          len(_ran[family]), "of", len(pm.grid_ids()), "ids ran")
    if len(_ran[family]) == len(pm.grid_ids()):
        assert _launched[family] == want, (family, sorted(want - _launched[family])[:8])
    else:   # (a selection of the sweep ran: what it launched is part of the table)
        assert _launched[family] <= want
