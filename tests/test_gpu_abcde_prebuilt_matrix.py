"""-m gpu: every prebuilt ABCDE kernel instantiation (csrc/capi_abcde.hip: abcde_init_kernel<D> +
abcde_gen_kernel<D> of kabc_abcde_run, abcde_small_kernel<D> of kabc_abcde_run_batch's launch grid, D = 1..16,
every built-in cost that accepts D behind kabc_cost_eval's switch, a simple and a general prior) against the CPU
oracle, bit for bit: the population, its costs, reached_eps, generations_run and nsims of four generations.
One test per (family, cost, D) over the whole grid; kabc_ctx_last_kernel must name the family, the donor scheme
and the workgroup the case meant, so that a run served by a run-time compiled kernel cannot pass for the
prebuilt one.  Where the cost does not accept the dimension the refusal is asserted and nothing is launched.
Cases, shapes and environment: prebuilt_matrix.py."""
import numpy as np
import pytest

import prebuilt_matrix as pm
from test_gpu_abcde_batch import _user_cost

pytestmark = pytest.mark.gpu

_launched = {f: set() for f in pm.ABCDE_FAMILIES}
_ran = {f: set() for f in pm.ABCDE_FAMILIES}


def _env(monkeypatch, env=()):
    monkeypatch.setenv("KABC_SPECIALIZE", "0")
    for name in pm.ABCDE_ENV_CLEARED:
        monkeypatch.delenv(name, raising=False)
    for name, value in dict(env).items():
        monkeypatch.setenv(name, value)


def _same_as_oracle(got, ref, who):
    assert got.P.shape == ref["P"].shape, who
    assert np.array_equal(got.P.view(np.uint64), ref["P"].view(np.uint64)), (who, "P")
    assert np.array_equal(got.C.view(np.uint64), ref["C"].view(np.uint64)), (who, "C")
    assert got.reached_ϵ == ref["reached_eps"], (who, "reached_eps")
    assert got.info["generations_run"] == ref["generations_run"] == pm.ABCDE_GENERATIONS, (who, "generations_run")
    assert got.info["nsims"] == ref["nsims"], (who, "nsims", got.info["nsims"], ref["nsims"])


def _run_case(k, orc, gpu_ctx, monkeypatch, family, c, D, simple):
    from kissabc_jl_amd import _lib
    prior, cost, legs = pm.pop_case(k, c, D, simple, family)
    for env, kw in legs:
        who = (pm.pop_name(family, c, D, simple), kw["nparticles"])
        _env(monkeypatch, env)
        if family == "ABCDE_GEN":
            got = [k.ABCDE(prior, cost, pm.ABCDE_EPS, return_array=True, ctx=gpu_ctx, **kw)]
            last = _lib.last_kernel(gpu_ctx)
        else:
            got = k.ABCDE_batch(prior, cost, pm.ABCDE_EPS, len(pm.POP_SEEDS), seeds=list(pm.POP_SEEDS),
                                return_array=True, ctx=gpu_ctx, **kw)
            last = _lib.last_kernel(gpu_ctx)
            assert got.info["course"] == "grid" and got.info["launches"] == 1, (who, got.info)
            assert len(got) == len(pm.POP_SEEDS), who
        for run, seed in zip(got, pm.pop_seeds(family, kw)):
            _same_as_oracle(run, orc.abcde(prior, cost, pm.ABCDE_EPS, **dict(kw, seed=seed)), who + (seed,))
        assert last == pm.pop_expected_kernel(family, c, D, env, kw), (who, "kabc_ctx_last_kernel", last)
        _launched[family].add(last)


def _refused(k, gpu_ctx, family, c, D, simple):
    """the cost's own refusal of D, before anything is launched: the recorder keeps what it held (a launch of
    this (cost, D) would have written a tuple no table entry has)"""
    from kissabc_jl_amd import _lib
    d_ok = min(d for d in range(1, pm.MAX_DIM + 1) if pm.cost_dim_ok(c, d))
    prior, cost = pm.smc_prior(k, D, simple), pm.cost(k, c, d_ok)
    before = _lib.last_kernel(gpu_ctx)
    with pytest.raises(k.KabcError, match=f"does not accept D = {D}") as e:
        if family == "ABCDE_GEN":
            k.ABCDE(prior, cost, pm.ABCDE_EPS, nparticles=130, generations=1, ctx=gpu_ctx)
        else:
            k.ABCDE_batch(prior, cost, pm.ABCDE_EPS, 3, nparticles=65, generations=1, ctx=gpu_ctx)
    if family == "ABCDE_SMALL":
        assert e.value.results.info["launches"] == 0 and e.value.results == [None] * 3
    assert _lib.last_kernel(gpu_ctx) == before


@pytest.mark.parametrize("cd", pm.grid_ids(), ids=pm.grid_id_name)
@pytest.mark.parametrize("family", pm.ABCDE_FAMILIES)
def test_abcde_prebuilt(k, orc, gpu_ctx, monkeypatch, family, cd):
    from kissabc_jl_amd import _lib
    c, D = cd
    _env(monkeypatch)
    for simple in (1, 0):
        if _lib.prebuilt_has(family, c, D, 0):
            _run_case(k, orc, gpu_ctx, monkeypatch, family, c, D, simple)
        else:
            assert not pm.cost_dim_ok(c, D), (family, c, D)   # (the tables hold every accepted dimension)
            _refused(k, gpu_ctx, family, c, D, simple)
    _ran[family].add(cd)


@pytest.mark.parametrize("family", pm.ABCDE_FAMILIES)
def test_abcde_sweep_is_complete(k, family):
    """after the whole sweep of a family (this file run as a whole): every entry of the table was launched, on
    every leg of its case (ABCDE_GEN: under both donor schemes)"""
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
    kw = dict(nparticles=130, generations=2, seed=3, ctx=gpu_ctx)

    def prebuilt_again():
        k.ABCDE(N2, g2, 0.05, **kw)
        assert _lib.last_kernel(gpu_ctx) == (pm.FAMILY_ID["ABCDE_GEN"], 1, 2, 0, 0, 1)

    prebuilt_again()
    k.ABCDE(k.Factored(*[k.Normal(0, 2)] * 17), k.costs.GaussDist(np.linspace(-1, 1, 17)), 0.1, **kw)
    assert _lib.last_kernel(gpu_ctx) == zeros, "17 parameters"
    prebuilt_again()
    user = _user_cost(k)   # (the noisy L1 cost of the batch tests: its code objects are theirs)
    k.ABCDE(N2, user, 0.05, **kw)
    assert _lib.last_kernel(gpu_ctx) == zeros, "user cost"
    out = k.ABCDE_batch(N2, user, 0.05, 3, nparticles=65, generations=2, ctx=gpu_ctx)
    assert out.info["course"] == "grid" and _lib.last_kernel(gpu_ctx) == zeros, "user cost, launch grid"
    out = k.ABCDE_batch(N2, g2, 0.05, 3, nparticles=65, generations=2, ctx=gpu_ctx)
    assert out.info["course"] == "grid" and _lib.last_kernel(gpu_ctx) == (pm.FAMILY_ID["ABCDE_SMALL"], 1, 2, 0, 0, 2)
    # a specialised model (test_gpu_abcde_resume.py's): KABC_SPECIALIZE=1 compiles its unit inside the call, and
    # the generation kernel is the unit's; two plain Normals are not eligible and stay on the table's entry
    mixed = k.Factored(k.Normal(0.25, 5), k.Uniform(-4, 6))
    monkeypatch.setenv("KABC_SPECIALIZE", "1")
    k.ABCDE(mixed, g2, 0.05, **kw)
    assert _lib.last_kernel(gpu_ctx) == zeros, "specialised model"
    prebuilt_again()
    monkeypatch.setenv("KABC_SPECIALIZE", "0")
    k.ABCDE(mixed, g2, 0.05, **kw)
    assert _lib.last_kernel(gpu_ctx) == (pm.FAMILY_ID["ABCDE_GEN"], 1, 2, 0, 0, 1)
