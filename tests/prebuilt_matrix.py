"""The matrix of prebuilt kernel instantiations (csrc/ais_inst.hip, csrc/smc_inst.hip) as test cases: for
every (cost id, D, prior class, posterior kind) one model, for every (cost id, D, simple / general) one smc
problem.  Builders depend on nothing but that tuple.  A helper module, used by
test_prebuilt_matrix_cases.py (CPU: the tables' contents; the cases are informative on the oracle alone),
test_gpu_ais_prebuilt_matrix.py and test_gpu_smc_prebuilt_matrix.py (the kernels against the oracle)."""
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
FAMILY_ID = {"AIS_HALF": 1, "AIS_WIDE": 2, "AIS_SMALL": 3, "SMC_PHASES": 4, "SMC_LOOP": 5, "SMC_SMALL": 6}
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
