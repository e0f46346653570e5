"""The matrix of prebuilt kernel instantiations (csrc/ais_inst.hip, csrc/smc_inst.hip, the per-D tables of
csrc/capi_abcde.hip and csrc/capi_pfilter.hip) as test cases: for every (cost id, D, prior class, posterior
kind) one model, for every (cost id, D, simple / general) one smc problem and one problem of the two
population samplers (ABCDE, pfilter).  Builders depend on nothing but that tuple.  A helper module, used by
test_prebuilt_matrix_cases.py (CPU: the tables' contents; the cases are informative on the oracle alone),
test_gpu_ais_prebuilt_matrix.py, test_gpu_smc_prebuilt_matrix.py, test_gpu_abcde_prebuilt_matrix.py and
test_gpu_pfilter_prebuilt_matrix.py (the kernels against the oracle)."""
import math

import numpy as np

MAX_DIM = 16
COSTS = {1: "GaussDist", 2: "Rosenbrock", 3: "HierGaussSim", 4: "NormalMeanStdSim", 5: "DiracSq", 6: "AbsDiff",
         7: "NormShell", 8: "NoisyQuadDU", 9: "Mixture", 10: "NoisyBanana", 11: "WienerRms"}
# prior classes of the AIS kernels, by their id (csrc/ais_kernels.hpp kPriorBox ...)
BOX, SIMPLE, GENERAL, NORMAL = 0, 1, 2, 3
CLASS_NAME = {BOX: "BOX", SIMPLE: "SIMPLE", GENERAL: "GENERAL", NORMAL: "NORMAL"}
KERNELIZED, THRESHOLD, COMMON = 1, 2, 3
KIND_NAME = {KERNELIZED: "KERNELIZED", THRESHOLD: "THRESHOLD", COMMON: "COMMON"}
AIS_FAMILIES = ("AIS_HALF", "AIS_WIDE", "AIS_SMALL")
SMC_FAMILIES = ("SMC_PHASES", "SMC_LOOP", "SMC_SMALL")
ABCDE_FAMILIES = ("ABCDE_GEN", "ABCDE_SMALL")
PF_FAMILIES = ("PF_PHASES", "PF_SMALL", "PF_BATCH")
POP_FAMILIES = ABCDE_FAMILIES + PF_FAMILIES
FAMILY_ID = {"AIS_HALF": 1, "AIS_WIDE": 2, "AIS_SMALL": 3, "SMC_PHASES": 4, "SMC_LOOP": 5, "SMC_SMALL": 6,
             "ABCDE_GEN": 7, "ABCDE_SMALL": 8, "PF_PHASES": 9, "PF_SMALL": 10, "PF_BATCH": 11}
# the shapes of the GPU sweeps.  AIS: 13 sub-steps end on a single-sub-step chunk for K = 3, 4 and 6 and pass
# the 8 sub-steps from which the NegativeBinomial table is staged.  AIS_HALF: 65 rows per half, a full
# 64-row workgroup and one of one row.  AIS_WIDE: 129 rows per half, the second batch of the wide workgroup
# holds one row.  AIS_SMALL: halves of 66 and 65 rows.
AIS_NT, AIS_SEED = 13, 1
AIS_N = {"AIS_HALF": 130, "AIS_WIDE": 258, "AIS_SMALL": 131}
AIS_ENV = {"AIS_HALF": {"KABC_AIS_SMALL": "0", "KABC_AIS_WIDE": "0"},
           "AIS_WIDE": {"KABC_AIS_SMALL": "0", "KABC_AIS_WIDE": "2"},
           "AIS_SMALL": {"KABC_AIS_SMALL": "1"}}
SMC_N = {"SMC_PHASES": 300, "SMC_LOOP": 300, "SMC_SMALL": 101}
SMC_ENV = {"SMC_PHASES": {"KABC_SMC_LOOP": "0"}, "SMC_LOOP": {"KABC_SMC_LOOP": "1"}, "SMC_SMALL": {}}
SMC_SEED, SMC_ITERATIONS = 1, 3
# The population samplers.  A family's sweep makes one or more "legs" per case: (environment, keywords).
# ABCDE_GEN: 130 particles are three 64-lane workgroups, the last of two particles, and take the generation
# kernel's own scans for the donor draw; 257 put abcde_donor_kernel's teams in front of it, the last team range
# holding one particle.  ABCDE_SMALL: 65 particles are two wavefronts, the second of one lane; three runs, one
# launch.  PF_SMALL: 130 particles in the one-workgroup kernel; eff_tol = 0 keeps a poor early efficiency from
# ending the run before max_iters does.  PF_PHASES: the same call on the loop-in-kernel course and on the
# launch-per-attempt course.  PF_BATCH: 65 particles; from D = 12 on N q <= 4 length(prior) raises N to 70..93.
POP_SEED, POP_SEEDS = 1, (1, 2, 3)
ABCDE_EPS, ABCDE_GENERATIONS = 0.0, 4
PF_Q, PF_MAX_ITERS = 0.7, 3
ABCDE_ENV_CLEARED = ("KABC_ABCDE_DONOR", "KABC_ABCDE_BLOCKS_FROM", "KABC_ABCDE_RANK", "KABC_ABCDE_SMALL")
PF_ENV_CLEARED = ("KABC_PF_SMALL", "KABC_PF_PASSES", "KABC_PF_BATCH", "KABC_PF_BATCH_SPREAD")
_PF_KW = dict(max_iters=PF_MAX_ITERS, eff_tol=0.0)
POP_LEGS = {
    "ABCDE_GEN": [({}, dict(nparticles=130, generations=ABCDE_GENERATIONS, seed=POP_SEED)),
                  ({}, dict(nparticles=257, generations=ABCDE_GENERATIONS, seed=POP_SEED))],
    "ABCDE_SMALL": [({}, dict(nparticles=65, generations=ABCDE_GENERATIONS))],
    "PF_SMALL": [({}, dict(N=130, seed=POP_SEED, **_PF_KW))],
    "PF_PHASES": [({"KABC_PF_SMALL": "0"}, dict(N=130, seed=POP_SEED, **_PF_KW)),
                  ({"KABC_PF_SMALL": "0", "KABC_PF_PASSES": "1"}, dict(N=130, seed=POP_SEED, **_PF_KW))],
    "PF_BATCH": [({}, dict(N=65, **_PF_KW))],
}


def pcx(cls, kind):
    return cls + 4 * (kind - 1)


def ais_variants(family):
    """(class, kind) the sweep of a family loops over: the one-workgroup kernel has no SIMPLE class"""
    classes = (BOX, NORMAL, GENERAL) if family == "AIS_SMALL" else (BOX, SIMPLE, GENERAL, NORMAL)
    return [(c, kd) for kd in (KERNELIZED, THRESHOLD, COMMON) for c in classes]


# ---- the written rules, restated (the library's tables are the authority: test_prebuilt_matrix_cases.py) ----
def cost_dim_ok(cost, D):
    """kabc_cost_dim_ok (include/kabc_costs.h)"""
    if not 1 <= D <= MAX_DIM:
        return False
    return {1: D >= 1, 2: D >= 2, 3: D >= 3, 4: D == 2, 5: D == 1, 6: D == 1, 7: D >= 1, 8: D == 2, 9: D == 1,
            10: D == 2, 11: D == 2}.get(cost, False)


def wide_ok(cost, D):
    """the wide kernel: no prepared words (NormalMeanStdSim), no leading normal blocks of the cost's stream
    (HierGaussSim, NoisyQuadDU, Mixture, NoisyBanana), at most eight parameters"""
    return cost_dim_ok(cost, D) and D <= 8 and cost in (1, 2, 5, 6, 7, 11)


def wide_waves(D, cls):
    """12 waves (K = 6) up to these dimensions by class, else the eight-wave kernel (K = 4)"""
    return 12 if D <= {BOX: 8, NORMAL: 6, SIMPLE: 4, GENERAL: 2}[cls] else 8


def rule_has(family, cost, D, variant):
    if family in POP_FAMILIES:   # (one instantiation per D, the cost behind a run-time switch)
        return cost_dim_ok(cost, D) and variant == 0
    if family in SMC_FAMILIES:
        return cost_dim_ok(cost, D) and variant in (0, 1)
    if not 0 <= variant < 12:
        return False
    if family == "AIS_WIDE":
        return wide_ok(cost, D)
    if family == "AIS_SMALL":
        return cost_dim_ok(cost, D) and variant % 4 != SIMPLE
    return cost_dim_ok(cost, D)


def ais_expected_kernel(family, cost, D, cls, kind):
    """kabc_ctx_last_kernel after a run of the case.  The one-workgroup driver runs a NORMAL prior of more
    than seven parameters on its GENERAL kernel (capi_ais.hip ais_resolve_kernels: the NORMAL class is the
    low translation unit's): those NORMAL entries of the table are never dispatched."""
    if family == "AIS_SMALL":
        if cls == SIMPLE or (cls == NORMAL and D > 7):
            cls = GENERAL
        return (FAMILY_ID[family], cost, D, cls, kind, 8)
    waves = wide_waves(D, cls) if family == "AIS_WIDE" else 4
    return (FAMILY_ID[family], cost, D, cls, kind, waves)


def smc_expected_kernel(family, cost, D, simple):
    """a prepared cost (NormalMeanStdSim: a grid-wide pre-pass per pass) does not take the persistent loop
    kernel (capi_smc.hip run_loop): KABC_SMC_LOOP=1 leaves it on the kernel per phase"""
    if family == "SMC_LOOP" and cost == 4:
        family = "SMC_PHASES"
    return (FAMILY_ID[family], cost, D, int(simple), 0, {"SMC_PHASES": 1, "SMC_LOOP": 4, "SMC_SMALL": 4}[family])


def pf_effective_n(N, D, q=PF_Q):
    """kabc_pfilter_nparticles (src/smc.jl:276-279): N q <= 4 length(prior) raises N"""
    return math.ceil((4 * D + 1) / q) if N * q <= 4 * D else N


def pop_expected_kernel(family, cost, D, env, kw):
    """kabc_ctx_last_kernel after a leg of the case: {family, cost, D, sub-course, 0, waves per workgroup}.
    The sub-course: ABCDE_GEN, the donor scheme by size with the knobs unset (capi_abcde.hip
    abcde_donor_scheme: 0 the generation kernel's scans below 256 particles, 1 the teams up to 4096);
    PF_PHASES, 1 with KABC_PF_PASSES=1, else 0."""
    if family == "ABCDE_GEN":
        N = kw["nparticles"]
        assert N < 1536, N   # (sorted blocks and the wavelet matrix: not these shapes)
        return (FAMILY_ID[family], cost, D, 1 if N >= 256 else 0, 0, 1)
    if family == "ABCDE_SMALL":
        return (FAMILY_ID[family], cost, D, 0, 0, -(-kw["nparticles"] // 64))
    if family == "PF_PHASES":
        return (FAMILY_ID[family], cost, D, 1 if env.get("KABC_PF_PASSES") == "1" else 0, 0, 1)
    if family == "PF_SMALL":
        return (FAMILY_ID[family], cost, D, 0, 0, 4)
    return (FAMILY_ID[family], cost, D, 0, 0, -(-pf_effective_n(kw["N"], D) // 64))


# ---- builders -------------------------------------------------------------------------------------------
def prior(k, D, cls):
    """component j differs a little from component j - 1 in every class, so that a wrong index shows"""
    def uni(j):
        return k.Uniform(-1.0 - 0.05 * j, 2.0 + 0.03 * j)

    def nrm(j):
        return k.Normal(0.5 + 0.02 * j, 0.8 + 0.01 * j)

    def tnr(j):
        return k.TruncatedNormal(0.5 - 0.01 * j, 0.9 + 0.01 * j, -1.5, 2.5 + 0.02 * j)

    def gen(j):
        return (lambda: k.Gamma(2.0 + 0.05 * j, 0.4), lambda: k.LogNormal(-0.4 + 0.01 * j, 0.5),
                lambda: k.Exponential(0.8 + 0.01 * j), lambda: k.Beta(2.0, 2.0 + 0.05 * j),
                lambda: k.NegativeBinomial(3.0 + 0.1 * j, 0.6))[j % 5]()
    comp = {BOX: uni, NORMAL: nrm, SIMPLE: lambda j: (tnr, uni, nrm)[j % 3](j), GENERAL: gen}[cls]
    return k.Factored(*[comp(j) for j in range(D)])


def cost(k, cost_id, D):
    """fixed parameters / seeded data inside the support of every class"""
    rng = np.random.default_rng(1000 * cost_id + D)
    if cost_id == 1:
        return k.costs.GaussDist([0.35 + 0.3 * ((7 * j) % 5) / 5 for j in range(D)])
    if cost_id == 2:
        return k.costs.Rosenbrock()
    if cost_id == 3:
        return k.costs.HierGaussSim(0.6 + 0.5 * rng.normal(size=D - 2))
    if cost_id == 4:
        return k.costs.NormalMeanStdSim(37, 0.6, 0.5)
    if cost_id == 5:
        return k.costs.DiracSq(1.3)
    if cost_id == 6:
        return k.costs.AbsDiff(0.55)
    if cost_id == 7:
        return k.costs.NormShell(0.8 * np.sqrt(D))
    if cost_id == 8:
        return k.costs.NoisyQuadDU(1.5)
    if cost_id == 9:
        return k.costs.Mixture(0.4)
    if cost_id == 10:
        return k.costs.NoisyBanana(0.1)
    if cost_id == 11:
        t = np.arange(10.0)
        return k.costs.WienerRms(np.sqrt(0.36 * t * t + 0.8 * t) * (1.0 + 0.05 * rng.normal(size=10)))
    raise ValueError(cost_id)


# one eps per (cost, kind): chosen on the oracle so that every case of the sweep is informative
# (test_prebuilt_matrix_cases.py).  CommonLogDensity has no eps.
EPS = {
    (1, KERNELIZED): 1.0, (1, THRESHOLD): 4.5,
    (2, KERNELIZED): 1.0, (2, THRESHOLD): 100.0,
    (3, KERNELIZED): 0.5, (3, THRESHOLD): 4.0,
    (4, KERNELIZED): 3.0, (4, THRESHOLD): 10.0,
    (5, KERNELIZED): 0.4, (5, THRESHOLD): 0.6,
    (6, KERNELIZED): 0.4, (6, THRESHOLD): 0.7,
    (7, KERNELIZED): 0.5, (7, THRESHOLD): 4.0,
    (8, KERNELIZED): 1.0, (8, THRESHOLD): 1.5,
    (9, KERNELIZED): 0.4, (9, THRESHOLD): 0.8,
    (10, KERNELIZED): 1.0, (10, THRESHOLD): 3.0,
    (11, KERNELIZED): 1.0, (11, THRESHOLD): 1.0,
}


def model(k, cost_id, D, cls, kind):
    p, c = prior(k, D, cls), cost(k, cost_id, D)
    if kind == KERNELIZED:
        return k.ApproxKernelizedPosterior(p, c, EPS[cost_id, kind])
    if kind == THRESHOLD:
        return k.ApproxPosterior(p, c, EPS[cost_id, kind])
    return k.CommonLogDensity(D, p, c)   # (its docstring: lπ may be a built-in cost)


def smc_prior(k, D, simple):
    """capi_smc.hip: a prior is "simple" when every component is Uniform, Normal, TruncatedNormal,
    DiscreteUniform or Exponential (kabc_device.hpp prior_is_simple).  The simple prior cycles all five; the
    general one puts a Gamma first (one component that is not simple is enough) and cycles the other
    families behind it."""
    def simple_c(j):
        return (lambda: k.Uniform(-1.0 - 0.05 * j, 2.0 + 0.03 * j), lambda: k.Normal(0.5 + 0.02 * j, 0.8),
                lambda: k.TruncatedNormal(0.5, 0.9 + 0.01 * j, -1.5, 2.5), lambda: k.Exponential(0.8 + 0.01 * j),
                lambda: k.DiscreteUniform(-1, 2 + j % 2))[j % 5]()

    def general_c(j):
        return (lambda: k.Gamma(2.0 + 0.05 * j, 0.4), lambda: k.LogNormal(-0.4 + 0.01 * j, 0.5),
                lambda: k.Beta(2.0, 2.0 + 0.05 * j), lambda: k.NegativeBinomial(3.0 + 0.1 * j, 0.6),
                lambda: k.Normal(0.5 + 0.02 * j, 0.8))[j % 5]()
    return k.Factored(*[(simple_c if simple else general_c)(j) for j in range(D)])


def smc_case(k, cost_id, D, simple, family):
    """(prior, cost, keywords of k.smc / orc.smc): default options, three iterations"""
    return smc_prior(k, D, simple), cost(k, cost_id, D), dict(nparticles=SMC_N[family], seed=SMC_SEED,
                                                               max_iterations=SMC_ITERATIONS)


def pop_case(k, cost_id, D, simple, family):
    """(prior, cost, legs) of a population-sampler case; a leg is (environment, keywords of k.ABCDE /
    k.ABCDE_batch / k.pfilter / k.pfilter_batch and of the oracle's run; the batch families run POP_SEEDS)"""
    return smc_prior(k, D, simple), cost(k, cost_id, D), POP_LEGS[family]


def pop_name(family, cost_id, D, simple):
    return f"({family}, {COSTS[cost_id]}, D={D}, {'simple' if simple else 'general'})"


# ---- the grid ---------------------------------------------------------------------------------------------
def grid_ids():
    """(cost, D) over the full grid, cost 1..11 x D 1..16"""
    return [(c, D) for c in COSTS for D in range(1, MAX_DIM + 1)]


def grid_id_name(cd):
    return f"{COSTS[cd[0]]}-D{cd[1]}"


def tuple_name(family, cost_id, D, cls, kind):
    return f"({family}, {COSTS[cost_id]}, D={D}, {CLASS_NAME[cls]}, {KIND_NAME[kind]})"


# cases that cannot be made informative for any eps / parameters, by name with the reason; at most 5 % of a
# family's cases (asserted by test_prebuilt_matrix_cases.py)
AIS_UNINFORMATIVE = {}
SMC_UNINFORMATIVE = {}
POP_UNINFORMATIVE = {}


# ---- informativeness, on the oracle alone -------------------------------------------------------------------
def ais_informative(orc, k, cost_id, D, cls, kind, N):
    """runs the oracle's first generation of the case; returns (moves seen, accepted fraction)"""
    o = orc.OracleAIS(model(k, cost_id, D, cls, kind), N, seed=AIS_SEED).init()
    _, tr = o.generations_sync(1, AIS_NT, trace=True)
    o.close()
    return set(np.unique(tr[0, :, :, 0]).tolist()), float(np.mean(tr[0, :, :, 1] != 0))


def smc_informative(orc, k, cost_id, D, simple, family):
    """the oracle's run of the case: its iteration log"""
    p, c, kw = smc_case(k, cost_id, D, simple, family)
    return orc.smc(p, c, **kw)


def pop_seeds(family, kw):
    """the seeds a leg runs: its own, or the three of the batch families"""
    return (kw["seed"],) if "seed" in kw else POP_SEEDS


def abcde_informative(orc, prior, cost, kw, seed):
    """the oracle's run of one ABCDE leg and seed: (generations run, the share of particles whose row differs
    from the run of no generations, i.e. from the initial draw)"""
    kw = dict(kw, seed=seed)
    ref = orc.abcde(prior, cost, ABCDE_EPS, **kw)
    ref0 = orc.abcde(prior, cost, ABCDE_EPS, **dict(kw, generations=0))
    return ref["generations_run"], float(np.mean(np.any(ref["P"] != ref0["P"], axis=1)))


def pf_informative(orc, prior, cost, kw, seed):
    """the oracle's run of one pfilter leg and seed"""
    kw = dict(kw, seed=seed)
    return orc.pfilter(prior, cost, kw.pop("N"), **kw)
