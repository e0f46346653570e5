"""CPU: the tables of prebuilt kernels (kabc_prebuilt_has, no device) against the written rules, and the
cases of the GPU sweeps (prebuilt_matrix.py) on the oracle alone: a case in which nothing is accepted, or
everything is, cannot see a wrong kernel."""
import math

import pytest

import prebuilt_matrix as pm

FAMILIES = pm.AIS_FAMILIES + pm.SMC_FAMILIES + pm.POP_FAMILIES
# what csrc/ais_inst.hip and csrc/smc_inst.hip instantiate: 68 (cost, D) pairs; x 12 variants; the wide
# kernel's 26 pairs x 12; x 9 without the SIMPLE class; x 2 flavours of each smc driver.  The population
# samplers: one instantiation per D, every cost that accepts D behind its run-time switch, 68 pairs
TOTALS = {"AIS_HALF": 816, "AIS_WIDE": 312, "AIS_SMALL": 612, "SMC_PHASES": 136, "SMC_LOOP": 136, "SMC_SMALL": 136,
          "ABCDE_GEN": 68, "ABCDE_SMALL": 68, "PF_PHASES": 68, "PF_SMALL": 68, "PF_BATCH": 68}


def _variants(family):
    return range(12) if family in pm.AIS_FAMILIES else range(1) if family in pm.POP_FAMILIES else range(2)


@pytest.mark.parametrize("family", FAMILIES)
def test_table_is_the_written_rule(k, family):
    """kabc_prebuilt_has over the whole grid, and a margin of arguments out of range around it"""
    from kissabc_jl_amd import _lib
    total = 0
    for c in range(-1, 14):
        for D in range(-1, 19):
            for v in range(-1, len(_variants(family)) + 1):
                has = _lib.prebuilt_has(family, c, D, v)
                assert has == pm.rule_has(family, c, D, v), (family, c, D, v)
                total += has
    assert total == TOTALS[family]
    assert not _lib.prebuilt_has(0, 1, 1, 0) and not _lib.prebuilt_has(12, 1, 1, 0)
    assert sorted(pm.FAMILY_ID.values()) == list(range(1, 12)) and pm.FAMILY_ID == _lib.PREBUILT_FAMILY


def test_twelve_wave_rule_edges():
    """BOX D <= 8, NORMAL D <= 6, SIMPLE D <= 4, GENERAL D <= 2 take 12 waves; the sweep visits both sides"""
    edges = {pm.NORMAL: (6, 7), pm.SIMPLE: (4, 5), pm.GENERAL: (2, 3)}
    for cls, (lo, hi) in edges.items():
        assert pm.wide_waves(lo, cls) == 12 and pm.wide_waves(hi, cls) == 8
        assert pm.wide_ok(1, lo) and pm.wide_ok(1, hi)
    assert pm.wide_waves(8, pm.BOX) == 12


def test_dispatched_tuples():
    """the kernels a sweep can reach by the drivers' own dispatch: every entry of the AIS_HALF, AIS_WIDE,
    SMC_PHASES and SMC_SMALL tables; AIS_SMALL without its NORMAL entries above seven parameters (4 costs x
    9 dimensions x 3 kinds), SMC_LOOP without the prepared cost's two"""
    for family in pm.AIS_FAMILIES:
        seen = {pm.ais_expected_kernel(family, c, D, cls, kind) for c, D in pm.grid_ids()
                for cls, kind in pm.ais_variants(family) if pm.rule_has(family, c, D, pm.pcx(cls, kind))}
        assert all(t[0] == pm.FAMILY_ID[family] for t in seen)
        assert len(seen) == TOTALS[family] - (108 if family == "AIS_SMALL" else 0), family
    for family in pm.SMC_FAMILIES:
        seen = {pm.smc_expected_kernel(family, c, D, s) for c, D in pm.grid_ids() for s in (0, 1)
                if pm.rule_has(family, c, D, s)}
        own = [t for t in seen if t[0] == pm.FAMILY_ID[family]]
        assert len(own) == TOTALS[family] - (2 if family == "SMC_LOOP" else 0), family


@pytest.mark.parametrize("family", pm.AIS_FAMILIES)
def test_ais_cases_are_informative(k, orc, family):
    """at the shapes of the GPU sweep: the oracle's initial draw succeeds, the debug records of the first
    generation hold all three moves, and accepted and rejected proposals each make up at least 5 % of them"""
    n_cases = n_excused = 0
    for c, D in pm.grid_ids():
        for cls, kind in pm.ais_variants(family):
            if not pm.rule_has(family, c, D, pm.pcx(cls, kind)):
                continue
            n_cases += 1
            name = pm.tuple_name(family, c, D, cls, kind)
            if name in pm.AIS_UNINFORMATIVE:
                n_excused += 1
                continue
            moves, accepted = pm.ais_informative(orc, k, c, D, cls, kind, pm.AIS_N[family])
            print(name, moves, accepted)
            assert moves == {1, 2, 3}, name
            assert 0.05 <= accepted <= 0.95, (name, accepted)
    assert n_cases == TOTALS[family]
    assert n_excused <= 0.05 * n_cases
    assert all(reason for reason in pm.AIS_UNINFORMATIVE.values())


@pytest.mark.parametrize("family", pm.SMC_FAMILIES)
def test_smc_cases_are_informative(k, orc, family):
    """at least two iterations run and epsilon falls, some but not all particles move in an MCMC step, and
    an iteration kills particles so that the resample runs"""
    n_cases = n_excused = 0
    for c, D in pm.grid_ids():
        for simple in (1, 0):
            if not pm.rule_has(family, c, D, simple):
                continue
            n_cases += 1
            name = f"({family}, {pm.COSTS[c]}, D={D}, {'simple' if simple else 'general'})"
            if name in pm.SMC_UNINFORMATIVE:
                n_excused += 1
                continue
            ref = pm.smc_informative(orc, k, c, D, simple, family)
            log, eps = ref["log"], [rec["eps"] for rec in ref["log"]]
            print(name, log)
            assert len(log) >= 2 and ref["iterations"] == len(log), name
            assert all(b < a for a, b in zip(eps, eps[1:])), (name, eps)   # (NoisyBanana starts from +Inf)
            assert any(0 < rec["accepted"] < pm.SMC_N[family] for rec in log), name
            assert any(rec["resampled"] for rec in log), name
    assert n_cases == TOTALS[family]
    assert n_excused <= 0.05 * n_cases
    assert all(reason for reason in pm.SMC_UNINFORMATIVE.values())


def test_pop_table_entries_are_the_grid():
    """each population-sampler family holds the (cost, D) pairs grid_ids() accepts, and the sweeps' expected
    tuples are one per entry and leg-specific sub-course: both donor schemes of ABCDE_GEN, both PF_PHASES courses"""
    for family in pm.POP_FAMILIES:
        held = [cd for cd in pm.grid_ids() if pm.rule_has(family, *cd, 0)]
        assert len(held) == TOTALS[family] == 68
        subs = {pm.pop_expected_kernel(family, 1, 1, env, kw)[3] for env, kw in pm.POP_LEGS[family]}
        assert subs == ({0, 1} if family in ("ABCDE_GEN", "PF_PHASES") else {0}), family
    # the batch sweep crosses pfilter's N q <= 4 length(prior) rule between D = 11 and D = 12
    assert [pm.pf_effective_n(65, D) for D in (11, 12, 16)] == [65, 70, 93]
    assert pm.pop_expected_kernel("PF_BATCH", 1, 16, {}, dict(N=65))[5] == 2


def _pop_cases(family):
    for c, D in pm.grid_ids():
        for simple in (1, 0):
            if pm.rule_has(family, c, D, 0):
                yield c, D, simple, pm.pop_name(family, c, D, simple)


@pytest.mark.parametrize("family", pm.ABCDE_FAMILIES)
def test_abcde_cases_are_informative(k, orc, family):
    """at every shape (and seed of the batch) of the GPU sweep: all four generations run, and between a tenth
    and nine tenths of the particles have left the row of their initial draw"""
    n_cases = n_excused = 0
    for c, D, simple, name in _pop_cases(family):
        n_cases += 1
        if name in pm.POP_UNINFORMATIVE:
            n_excused += 1
            continue
        prior, cost, legs = pm.pop_case(k, c, D, simple, family)
        for _, kw in legs:
            for seed in pm.pop_seeds(family, kw):
                gens, moved = pm.abcde_informative(orc, prior, cost, kw, seed)
                print(name, kw["nparticles"], seed, gens, moved)
                assert gens == pm.ABCDE_GENERATIONS, name
                assert 0.1 <= moved <= 0.9, (name, kw["nparticles"], seed, moved)
    assert n_cases == 2 * TOTALS[family]
    assert n_excused <= 0.05 * n_cases
    assert all(reason for reason in pm.POP_UNINFORMATIVE.values())


@pytest.mark.parametrize("family", pm.PF_FAMILIES)
def test_pfilter_cases_are_informative(k, orc, family):
    """at every shape (and seed of the batch) of the GPU sweep: max_iters + 1 iterations run; some proposals
    fail the prior's Metropolis gate and some pass (nreps > cost_evals > 0); at least 0.3 replacements per
    particle were proposed; eps is finite"""
    n_cases = n_excused = 0
    for c, D, simple, name in _pop_cases(family):
        n_cases += 1
        if name in pm.POP_UNINFORMATIVE:
            n_excused += 1
            continue
        prior, cost, legs = pm.pop_case(k, c, D, simple, family)
        kw = legs[0][1]   # (the legs of a family differ by their environment only: one oracle run)
        assert all(leg_kw == kw for _, leg_kw in legs)
        n_eff = pm.pf_effective_n(kw["N"], D)
        for seed in pm.pop_seeds(family, kw):
            ref = pm.pf_informative(orc, prior, cost, kw, seed)
            print(name, seed, {f: ref[f] for f in ("iterations", "nreps", "cost_evals", "eps", "eff")})
            assert ref["P"].shape == (n_eff, D), name
            assert ref["iterations"] == pm.PF_MAX_ITERS + 1, name
            assert ref["nreps"] > ref["cost_evals"] > 0, (name, seed, ref["nreps"], ref["cost_evals"])
            assert ref["nreps"] >= 0.3 * n_eff, (name, seed, ref["nreps"])
            assert math.isfinite(ref["eps"]), (name, seed)
    assert n_cases == 2 * TOTALS[family]
    assert n_excused <= 0.05 * n_cases
    assert all(reason for reason in pm.POP_UNINFORMATIVE.values())


def test_smc_priors_are_what_the_dispatch_calls_simple(k):
    """capi_smc.hip takes the simple kernels when every component is Uniform, Normal, TruncatedNormal,
    DiscreteUniform or Exponential (kabc_device.hpp prior_is_simple)"""
    from kissabc_jl_amd import _cdefs as cd
    simple_kinds = {cd.PRIOR_UNIFORM, cd.PRIOR_NORMAL, cd.PRIOR_TRUNCNORMAL, cd.PRIOR_DISCRETE_UNIFORM,
                    cd.PRIOR_EXPONENTIAL}
    for D in range(1, pm.MAX_DIM + 1):
        assert {c.kind for c in pm.smc_prior(k, D, True).p} <= simple_kinds
        assert not {c.kind for c in pm.smc_prior(k, D, False).p} <= simple_kinds
    assert {c.kind for c in pm.smc_prior(k, 5, True).p} == simple_kinds


def test_ais_priors_have_their_class(k):
    """capi_ais.hip ais_prepare_prior: BOX all uniform, NORMAL all Normal, SIMPLE uniform / Normal /
    TruncatedNormal (not all of one of the former), GENERAL anything else -- at every D, D = 1 included"""
    from kissabc_jl_amd import _cdefs as cd
    box, gauss = {cd.PRIOR_UNIFORM, cd.PRIOR_DISCRETE_UNIFORM}, {cd.PRIOR_NORMAL, cd.PRIOR_TRUNCNORMAL}

    def cls_of(p):
        kinds = {c.kind for c in p.p}
        if kinds <= box:
            return pm.BOX
        if kinds == {cd.PRIOR_NORMAL}:
            return pm.NORMAL
        return pm.SIMPLE if kinds <= box | gauss else pm.GENERAL
    for D in range(1, pm.MAX_DIM + 1):
        for cls in (pm.BOX, pm.SIMPLE, pm.GENERAL, pm.NORMAL):
            assert cls_of(pm.prior(k, D, cls)) == cls, (D, cls)
    # from five parameters on the GENERAL prior holds a NegativeBinomial: its lgamma table in LDS
    assert cd.PRIOR_NEGBINOMIAL in {c.kind for c in pm.prior(k, 5, pm.GENERAL).p}
