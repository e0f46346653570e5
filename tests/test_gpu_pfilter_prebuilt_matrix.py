"""-m gpu: every prebuilt pfilter kernel instantiation (csrc/capi_pfilter.hip: abcde_init_kernel<D> with
pfilter's stream domains + pf_attempt_kernel<D> on the loop-in-kernel and on the launch-per-attempt course,
pf_small_kernel<D>, pf_batch_kernel<D> of kabc_pfilter_run_batch's launch grid, D = 1..16, every built-in cost
that accepts D behind kabc_cost_eval's switch, a simple and a general prior) against the CPU oracle, bit for
bit: the population, its costs, eps, eff, iterations, nreps and cost_evals of four iterations.  One test per
(family, cost, D) over the whole grid; kabc_ctx_last_kernel must name the family, the course and the workgroup
the case meant, so that a run served by a run-time compiled kernel cannot pass for the prebuilt one.  Where
the cost does not accept the dimension the refusal is asserted and nothing is launched.  Cases, shapes and
environment: prebuilt_matrix.py."""
import numpy as np
import pytest

import prebuilt_matrix as pm
from test_gpu_pfilter_batch import _user_cost

pytestmark = pytest.mark.gpu

_launched = {f: set() for f in pm.PF_FAMILIES}
_ran = {f: set() for f in pm.PF_FAMILIES}


def _env(monkeypatch, env=()):
    monkeypatch.setenv("KABC_SPECIALIZE", "0")
    for name in pm.PF_ENV_CLEARED:
        monkeypatch.delenv(name, raising=False)
    for name, value in dict(env).items():
        monkeypatch.setenv(name, value)


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _same_as_oracle(got, ref, who):
    assert got.P.shape == ref["P"].shape, who
    assert np.array_equal(_bits(got.P), _bits(ref["P"])), (who, "P")
    assert np.array_equal(_bits(got.C), _bits(ref["C"])), (who, "C")
    assert _bits(got.info["eps"]) == _bits(ref["eps"]), (who, "eps", got.info["eps"], ref["eps"])
    eff, ref_eff = float(got.info["eff"]), float(ref["eff"])
    assert eff == ref_eff or (eff != eff and ref_eff != ref_eff), (who, "eff", eff, ref_eff)
    for f in ("iterations", "nreps", "cost_evals"):
        assert got.info[f] == ref[f], (who, f, got.info[f], ref[f])
    assert ref["iterations"] == pm.PF_MAX_ITERS + 1, who


def _run_case(k, orc, gpu_ctx, monkeypatch, family, c, D, simple):
    from kissabc_jl_amd import _lib
    prior, cost, legs = pm.pop_case(k, c, D, simple, family)
    refs = {}   # (the legs of PF_PHASES are one problem on two courses)
    for env, kw in legs:
        who = (pm.pop_name(family, c, D, simple), tuple(sorted(env.items())))
        _env(monkeypatch, env)
        kw = dict(kw)
        N = kw.pop("N")
        if family == "PF_BATCH":
            got = k.pfilter_batch(prior, cost, N, len(pm.POP_SEEDS), seeds=list(pm.POP_SEEDS), return_array=True,
                                  ctx=gpu_ctx, **kw)
            last = _lib.last_kernel(gpu_ctx)
            assert got.info["course"] == "grid" and got.info["launches"] == 1, (who, got.info)
            assert len(got) == len(pm.POP_SEEDS), who
        else:
            got = [k.pfilter(prior, cost, N, return_array=True, ctx=gpu_ctx, **kw)]
            last = _lib.last_kernel(gpu_ctx)
        for run, seed in zip(got, pm.pop_seeds(family, dict(kw))):
            if seed not in refs:
                refs[seed] = orc.pfilter(prior, cost, N, **dict(kw, seed=seed))
            assert run.P.shape == (pm.pf_effective_n(N, D), D), who
            _same_as_oracle(run, refs[seed], who + (seed,))
        assert last == pm.pop_expected_kernel(family, c, D, env, dict(kw, N=N)), (who, "kabc_ctx_last_kernel", last)
        _launched[family].add(last)


def _refused(k, gpu_ctx, monkeypatch, family, c, D, simple):
    """the cost's own refusal of D, before anything is launched: the recorder keeps what it held (a launch of
    this (cost, D) would have written a tuple no table entry has)"""
    from kissabc_jl_amd import _lib
    d_ok = min(d for d in range(1, pm.MAX_DIM + 1) if pm.cost_dim_ok(c, d))
    prior, cost = pm.smc_prior(k, D, simple), pm.cost(k, c, d_ok)
    for env, kw in pm.POP_LEGS[family]:
        _env(monkeypatch, env)
        before = _lib.last_kernel(gpu_ctx)
        with pytest.raises(k.KabcError, match=f"does not accept D = {D}") as e:
            if family == "PF_BATCH":
                k.pfilter_batch(prior, cost, kw["N"], 3, max_iters=1, ctx=gpu_ctx)
            else:
                k.pfilter(prior, cost, kw["N"], max_iters=1, ctx=gpu_ctx)
        if family == "PF_BATCH":
            assert e.value.results.info["launches"] == 0 and e.value.results == [None] * 3
        assert _lib.last_kernel(gpu_ctx) == before


@pytest.mark.parametrize("cd", pm.grid_ids(), ids=pm.grid_id_name)
@pytest.mark.parametrize("family", pm.PF_FAMILIES)
def test_pfilter_prebuilt(k, orc, gpu_ctx, monkeypatch, family, cd):
    from kissabc_jl_amd import _lib
    c, D = cd
    _env(monkeypatch)
    for simple in (1, 0):
        if _lib.prebuilt_has(family, c, D, 0):
            _run_case(k, orc, gpu_ctx, monkeypatch, family, c, D, simple)
        else:
            assert not pm.cost_dim_ok(c, D), (family, c, D)   # (the tables hold every accepted dimension)
            _refused(k, gpu_ctx, monkeypatch, family, c, D, simple)
    _ran[family].add(cd)


@pytest.mark.parametrize("family", pm.PF_FAMILIES)
def test_pfilter_sweep_is_complete(k, family):
    """after the whole sweep of a family (this file run as a whole): every entry of the table was launched, on
    every leg of its case (PF_PHASES: on both courses)"""
    from kissabc_jl_amd import _lib
    want = {pm.pop_expected_kernel(family, c, D, env, kw) for c, D in pm.grid_ids() for env, kw in pm.POP_LEGS[family]
            if _lib.prebuilt_has(family, c, D, 0)}
    entries = {t[1:3] for t in _launched[family]}
    print(family, "launched", len(entries), "of", len({t[1:3] for t in want}), "table entries,",
          len(_launched[family]), "tuples;", len(_ran[family]), "of", len(pm.grid_ids()), "ids ran")
    if len(_ran[family]) == len(pm.grid_ids()):
        assert _launched[family] == want, (family, sorted(want - _launched[family])[:8])
        assert len(entries) == 68
    else:
        assert _launched[family] <= want


def test_recorder_says_no(k, gpu_ctx, monkeypatch):
    """all six words are zero after a run on a run-time-dimension kernel (17 parameters), on a user cost's
    kernels and on a specialised model's own kernels; a prebuilt run in between sets them again"""
    from kissabc_jl_amd import _lib
    _env(monkeypatch)
    zeros = (0,) * 6
    N2 = k.Factored(k.Normal(0, 5), k.Normal(0, 5))
    g2 = k.costs.GaussDist([1.0, -0.5])
    kw = dict(max_iters=2, seed=3, ctx=gpu_ctx)

    def prebuilt_again():
        k.pfilter(N2, g2, 130, **kw)
        assert _lib.last_kernel(gpu_ctx) == (pm.FAMILY_ID["PF_SMALL"], 1, 2, 0, 0, 4)

    prebuilt_again()
    big, gbig = k.Factored(*[k.Normal(0, 2)] * 17), k.costs.GaussDist(np.linspace(-1, 1, 17))
    k.pfilter(big, gbig, 130, **kw)   # (the one-workgroup kernel's D = 0 instantiation)
    assert _lib.last_kernel(gpu_ctx) == zeros, "17 parameters, one workgroup"
    prebuilt_again()
    k.pfilter(big, gbig, 300, **kw)   # (the launches per phase)
    assert _lib.last_kernel(gpu_ctx) == zeros, "17 parameters, phases"
    prebuilt_again()
    user = _user_cost(k)   # (the noisy L1 cost of the batch tests: its code objects are theirs)
    k.pfilter(N2, user, 130, **kw)   # (a user cost never takes the one-workgroup kernel)
    assert _lib.last_kernel(gpu_ctx) == zeros, "user cost"
    out = k.pfilter_batch(N2, user, 65, 3, max_iters=2, ctx=gpu_ctx)
    assert out.info["course"] == "grid" and _lib.last_kernel(gpu_ctx) == zeros, "user cost, launch grid"
    out = k.pfilter_batch(N2, g2, 65, 3, max_iters=2, ctx=gpu_ctx)
    assert out.info["course"] == "grid" and _lib.last_kernel(gpu_ctx) == (pm.FAMILY_ID["PF_BATCH"], 1, 2, 0, 0, 2)
    # a specialised model: KABC_SPECIALIZE=1 compiles its unit inside the call, and the attempt kernel is the
    # unit's (the one-workgroup course asks for no unit: 300 particles); two plain Normals are not eligible
    mixed = k.Factored(k.Normal(0.25, 5), k.Uniform(-4, 6))
    monkeypatch.setenv("KABC_SPECIALIZE", "1")
    k.pfilter(mixed, g2, 300, **kw)
    assert _lib.last_kernel(gpu_ctx) == zeros, "specialised model"
    prebuilt_again()
    monkeypatch.setenv("KABC_SPECIALIZE", "0")
    k.pfilter(mixed, g2, 300, **kw)
    assert _lib.last_kernel(gpu_ctx) == (pm.FAMILY_ID["PF_PHASES"], 1, 2, 0, 0, 1)
