"""-m gpu: the support test of the BOX prior class in the AIS half-generation kernels
(csrc/ais_kernels.hpp loglike): a box (-a_k, a_k)^D of continuous components takes ONE comparison per
component, |y_k| <= a_k (box_contains_sym), every other box the general chain of two, a box with a
discrete component the rounding path.  All three against the CPU oracle's sync schedule, bit for bit:
trace, state, the three counters and the per-transition debug records, the `ev` flag among them.

The boxes are narrow, Uniform(-0.5, 0.5)^D under a unit-scale gauss_dist cost, so that BOTH outcomes
of the test occur often: every case asserts, on the oracle's own records, that between 20 % and 80 %
of the proposals fall outside the support (a condition on the inputs, not a tolerance).

Both geometries, forced: KABC_AIS_WIDE=0 (one batch of 64 rows per workgroup) and =2 (two batches
per workgroup; a launch that cannot take it is an error).  Sub-steps 7 and 25: a ragged last chunk
for both chunk lengths (3 and 6), the second past the default cut-over of 24.  Rows per half: a
ragged batch and two full batches -- 64 + 37 and 128 for the existing geometry; the wide one needs
two full batches per launch (capi_ais.hip ais_can_wide), so its ragged case is 128 + 37."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS = {"0": (64 + 37, 2 * 64), "2": (2 * 64, 2 * 64 + 37)}
NTS = (7, 25)


def _prior(k, name):
    u = k.Uniform(-0.5, 0.5)
    if name in ("sym2", "sym5", "sym8"):
        return k.Factored(*[u] * int(name[3:]))
    if name == "skew8":     # one component off centre: the general chain
        return k.Factored(*([u] * 5 + [k.Uniform(-0.5, 0.75)] + [u] * 2))
    if name == "discrete3":  # push_p rounds the second component: the discrete path
        return k.Factored(u, k.DiscreteUniform(-3, 3), u)
    raise KeyError(name)


def _model(k, name, kind):
    post = k.ApproxKernelizedPosterior if kind == "kernelized" else k.ApproxPosterior
    return post(_prior(k, name), k.costs.GaussDist(np.zeros(int(name[-1]))), 1.0)


_ORACLE = {}


def _oracle(orc, k, name, kind, N, nt, seed):
    """one oracle run per (model, shape), shared by the two geometries"""
    key = (name, kind, N, nt, seed)
    if key not in _ORACLE:
        o = orc.OracleAIS(_model(k, name, kind), N, seed=seed).init()
        ref, tr = o.generations_sync(1, nt, trace=True)
        g2 = o.generations_sync(2, nt)
        _ORACLE[key] = (ref, tr, g2, o.state(), o.stats())
    return _ORACLE[key]


def _device(k, monkeypatch, model, N, nt, seed, wide):
    monkeypatch.setenv("KABC_AIS_SMALL", "0")
    monkeypatch.setenv("KABC_SPECIALIZE", "0")   # the prebuilt kernels of both geometries
    monkeypatch.setenv("KABC_AIS_WIDE", wide)
    ens = k.AisEnsemble(model, N, seed=seed).init()
    assert ens.driver == "halves"
    ens.set_debug(nt)
    g1 = ens.advance(1, nt, collect=True)
    dbg = ens.get_debug(nt)
    ens.set_debug(0)
    g2 = ens.advance(2, nt, collect=True)
    out = (g1, dbg, g2, ens.state(), ens.stats())
    ens.close()
    return out


def _check(k, orc, monkeypatch, name, kind, wide, rows, nt, seed=3):
    N = 2 * rows
    ref, tr, ref2, (xo, lpo, llo, to), so = _oracle(orc, k, name, kind, N, nt, seed)
    out_share = 1.0 - tr[0, :, :, 5].mean()
    print(f"{name} {kind} rows {rows} nt {nt}: {100 * out_share:.1f} % of the proposals outside the support")
    assert 0.2 <= out_share <= 0.8, out_share
    g1, dbg, g2, (x, lp, ll, t), st = _device(k, monkeypatch, _model(k, name, kind), N, nt, seed, wide)
    assert np.array_equal(g1, ref)
    for col in (0, 1, 5):   # move id, accepted, evaluated
        assert np.array_equal(dbg[:, :, col], tr[0, :, :, col]), col
    base = np.where(np.arange(N) < rows, rows, 0)[:, None]
    for col in (2, 3, 4):   # partner rows
        d = dbg[:, :, col].astype(np.int64)
        assert np.array_equal(np.where(d >= 0, d + base, -1), tr[0, :, :, col].astype(np.int64)), col
    assert np.array_equal(g2, ref2)
    assert t == to == 3 * nt
    assert np.array_equal(x, xo) and np.array_equal(lp, lpo) and np.array_equal(ll, llo)
    assert st == so   # proposals, cost evaluations, accepted


def test_wide_refuses_a_ragged_single_batch(k, gpu_ctx, monkeypatch):
    """64 + 37 rows per half cannot take the wide geometry: forced, the launch is an error (so the
    wide cases above start at two full batches)"""
    monkeypatch.setenv("KABC_AIS_SMALL", "0")
    monkeypatch.setenv("KABC_SPECIALIZE", "0")
    monkeypatch.setenv("KABC_AIS_WIDE", "2")
    ens = k.AisEnsemble(_model(k, "sym8", "kernelized"), 2 * (64 + 37), seed=3).init()
    with pytest.raises(k.KabcError, match="wide"):
        ens.advance(1, 7)
    ens.close()


CASES = [(name, kind) for name in ("sym2", "sym5", "sym8", "skew8", "discrete3")
         for kind in ("kernelized", "threshold")]


@pytest.mark.parametrize("wide", ["0", "2"])
@pytest.mark.parametrize("name,kind", CASES)
def test_box_paths_match_oracle(k, orc, gpu_ctx, monkeypatch, name, kind, wide):
    for rows in ROWS[wide]:
        for nt in NTS:
            _check(k, orc, monkeypatch, name, kind, wide, rows, nt)
