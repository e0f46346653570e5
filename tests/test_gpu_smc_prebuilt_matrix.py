"""-m gpu: every prebuilt smc kernel instantiation (csrc/smc_inst.hip: smc_mcmc_kernel of the kernel-per-phase
driver, the persistent loop kernel and the one-workgroup kernel, for every cost x D x {simple, general}
prior) against the CPU oracle, bit for bit: theta, cost, the alive mask and the per-iteration log of three
iterations with default options.  One test per (family, cost, D) over the whole grid; kabc_ctx_last_kernel
must name the family and flavour the case meant.  Where the cost does not accept the dimension the refusal is
asserted and nothing runs.  Cases, shapes and environment: prebuilt_matrix.py."""
import numpy as np
import pytest

import prebuilt_matrix as pm

pytestmark = pytest.mark.gpu

_launched = {f: set() for f in pm.SMC_FAMILIES}
_ran = {f: set() for f in pm.SMC_FAMILIES}


def _run_case(k, orc, gpu_ctx, family, c, D, simple):
    from kissabc_jl_amd import _lib
    who = f"({family}, {pm.COSTS[c]}, D={D}, {'simple' if simple else 'general'})"
    prior, cost, kw = pm.smc_case(k, c, D, simple, family)
    got = k.smc(prior, cost, return_array=True, ctx=gpu_ctx, **kw)
    last = _lib.last_kernel(gpu_ctx)
    ref = orc.smc(prior, cost, **kw)
    assert got.info["iterations"] == ref["iterations"] == pm.SMC_ITERATIONS, who
    assert got.info["log"] == ref["log"], (who, "iteration log")
    assert got.eps == ref["eps"], who
    assert np.array_equal(got.info["alive"], ref["alive"]), (who, "alive mask")
    assert np.array_equal(got.info["theta_all"], ref["theta_all"]), (who, "theta")
    assert np.array_equal(got.C, ref["C"]), (who, "cost")
    assert got.info["cost_evals"] == ref["cost_evals"] and got.info["proposals"] == ref["proposals"], who
    assert last == pm.smc_expected_kernel(family, c, D, simple), (who, "kabc_ctx_last_kernel", last)
    _launched[family].add(last)


@pytest.mark.parametrize("cd", pm.grid_ids(), ids=pm.grid_id_name)
@pytest.mark.parametrize("family", pm.SMC_FAMILIES)
def test_smc_prebuilt(k, orc, gpu_ctx, monkeypatch, family, cd):
    from kissabc_jl_amd import _lib
    c, D = cd
    monkeypatch.setenv("KABC_SPECIALIZE", "0")
    for name in ("KABC_SMC_LOOP", "KABC_SMC_SMALL", "KABC_SMC_SPEC_SELECT"):
        monkeypatch.delenv(name, raising=False)
    for name, value in pm.SMC_ENV[family].items():
        monkeypatch.setenv(name, value)
    for simple in (1, 0):
        if _lib.prebuilt_has(family, c, D, simple):
            _run_case(k, orc, gpu_ctx, family, c, D, simple)
        else:
            assert not pm.cost_dim_ok(c, D), (family, c, D)   # (the tables hold every accepted dimension)
            d_ok = min(d for d in range(1, pm.MAX_DIM + 1) if pm.cost_dim_ok(c, d))
            with pytest.raises(k.KabcError, match=f"does not accept D = {D}"):
                k.smc(pm.smc_prior(k, D, simple), pm.cost(k, c, d_ok), nparticles=pm.SMC_N[family], max_iterations=1)
    _ran[family].add(cd)


@pytest.mark.parametrize("family", pm.SMC_FAMILIES)
def test_smc_sweep_is_complete(k, family):
    """after the whole sweep of a family (this file run as a whole): every entry of the table was launched --
    but for SMC_LOOP's two of the prepared cost, which the driver keeps on the kernel per phase"""
    from kissabc_jl_amd import _lib
    want = {pm.smc_expected_kernel(family, c, D, s) for c, D in pm.grid_ids() for s in (0, 1)
            if _lib.prebuilt_has(family, c, D, s)}
    own = {t for t in _launched[family] if t[0] == pm.FAMILY_ID[family]}
    print(family, "launched", len(own), "of its own tuples,", len(_launched[family]), "in all;",
          len(_ran[family]), "of", len(pm.grid_ids()), "ids ran")
    if len(_ran[family]) == len(pm.grid_ids()):
        assert _launched[family] == want, (family, sorted(want - _launched[family])[:8])
    else:
        assert _launched[family] <= want
