"""Adversarial cost laws for smc's ε-selection (src/smc.jl:131-153), shared by
test_smc_selection_edges.py (CPU, the oracle) and test_gpu_smc_selection_edges.py (every device course).

Each scenario is a table of costs and a one-parameter prior x[0] ~ DiscreteUniform(0, M - 1); the cost of a
particle is table[x[0]], so every cost is an exact table entry and C = table[θ] can be recomputed from the
positions.  Runs last exactly K iterations (r_epstol = 0, mcmc_tol = 0, epstol = -1e308, max_iterations = K)
unless the scenario is about a stop rule or an error.  Where a scenario needs a particular rank of the
initial ensemble's costs (γ = 0, the last key of a range, an Inf at rank j + 1), α is solved for that rank and
N α + (1 - α) is checked to evaluate to the intended double."""
import math

import numpy as np

SEED = 11
SOURCE = '''
KABC_HD double kabc_user_cost(const double* x, int D, const double* params,
                              const double* data, int64_t ndata, kabc_cost_rng_t* rng) {
    int64_t i = (int64_t)x[0];
    i = i < 0 ? 0 : (i >= ndata ? ndata - 1 : i);
    return data[i];
}'''
K_DEFAULT = 5

NAMES = ["neg_mixed", "signed_zero", "signed_zero_floor", "inf_tail", "inf_nan_eps", "inf_bracket",
         "neg_inf_head", "subnormal", "plateau_ties", "dead_pile", "cliff", "cluster_outliers", "gap_needmin"]
ERRORS = {"inf_nan_eps", "inf_bracket"}       # ESS = 0 at iteration 1: "no alive particle to resample from"


class Scenario:
    def __init__(self, name, N, table, alpha, K=K_DEFAULT, min_r_ess=None, epstol=-1e308):
        self.name, self.N, self.K = name, int(N), int(K)
        self.table = np.asarray(table, dtype=np.float64)
        self.alpha = float(alpha)
        self.min_r_ess = float(alpha * alpha if min_r_ess is None else min_r_ess)
        self.epstol = epstol

    def prior(self, k):
        return k.DiscreteUniform(0, self.table.size - 1)

    def cost(self, k):
        return k.costs.UserCost(SOURCE, dims=[1], data=self.table, name="table")

    def kw(self, max_iterations=None):
        return dict(nparticles=self.N, alpha=self.alpha, min_r_ess=self.min_r_ess, r_epstol=0.0, mcmc_tol=0.0,
                    epstol=self.epstol, seed=SEED,
                    max_iterations=self.K if max_iterations is None else max_iterations)

    def initial(self, orc):
        """(θ, C) of the initial ensemble (domain DOM_SMC_INIT)"""
        from kissabc_jl_amd import _cdefs as cd
        import kissabc_jl_amd as k
        th = orc.factored_rand(self.prior(k), self.N, seed=SEED, domain=cd.DOM_SMC_INIT)
        return th, self.costs_of(th)

    def costs_of(self, theta):
        return self.table[np.asarray(theta)[:, 0].astype(np.int64)]


def _alpha_for(N, j, gamma):
    """α with trunc(N α + (1 - α)) == j (the 1-based rank of order statistic a) and γ = aleph - j: exactly 0
    when gamma == 0, else strictly inside (0, 1)"""
    target = float(j) + gamma
    a = (target - 1.0) / (N - 1.0)
    for _ in range(200):
        v = N * a + (1.0 - a)
        if v == target or (gamma > 0 and 0.0 < v - j < 1.0):
            return a
        a = np.nextafter(a, math.inf if v < target else -math.inf)
    raise AssertionError(f"no α puts aleph at {target} for N = {N}")


def _init_costs(table, N, orc):
    s = Scenario("probe", N, table, 0.5)
    return s.initial(orc)[1]


def build(name, N, orc):
    """the Scenario `name` at N particles (the initial ensemble decides α where a rank is designed)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "neg_mixed":             # costs in [-1e3, 1e3]: ε crosses zero
        t = rng.uniform(-1e3, 1e3, 4096)
        return Scenario(name, N, t, 0.75)
    if name == "signed_zero":           # ±0 between negatives and positives: ε = 0 exactly, flag 0
        t = np.concatenate([-rng.uniform(1e-3, 1, 300), np.full(500, -0.0), np.full(500, 0.0),
                            rng.uniform(1e-3, 1, 2700)])
        return Scenario(name, N, rng.permutation(t), 0.75)
    if name == "signed_zero_floor":     # minimum -0.0 while ε = +0.0: the flag is set by value (0 > -0 is false)
        t = np.concatenate([np.full(1800, -0.0), np.full(1800, 0.0), rng.uniform(1e-3, 1, 400)])
        return Scenario(name, N, rng.permutation(t), 0.5)
    if name in ("inf_tail", "inf_nan_eps"):   # +Inf at rank j + 1: γ > 0 -> ε = +Inf, flag 0; γ = 0 -> NaN
        t = np.concatenate([rng.uniform(1, 2, 2800), np.full(1200, np.inf)])
        t = rng.permutation(t)
        nfin = int(np.isfinite(_init_costs(t, N, orc)).sum())
        return Scenario(name, N, t, _alpha_for(N, nfin, 0.5 if name == "inf_tail" else 0.0),
                        min_r_ess=0.5)
    if name == "inf_bracket":           # -Inf at rank j, +Inf at rank j + 1: -Inf + Inf -> NaN
        t = rng.permutation(np.concatenate([np.full(2000, -np.inf), np.full(2000, np.inf)]))
        nneg = int((_init_costs(t, N, orc) < 0).sum())
        return Scenario(name, N, t, _alpha_for(N, nneg, 0.5), min_r_ess=0.5)
    if name == "neg_inf_head":          # -Inf at ranks j and j + 1: ε = -Inf <= epstol stops the run
        t = rng.permutation(np.concatenate([np.full(2400, -np.inf), rng.uniform(-1, 1, 1600)]))
        return Scenario(name, N, t, _alpha_for(N, int(0.3 * N), 0.5))
    if name == "subnormal":             # γ-interpolation among subnormals and zeros
        t = np.concatenate([rng.integers(1, 1 << 40, 3000) * 5e-324, np.zeros(500), np.full(500, -0.0)])
        return Scenario(name, N, rng.permutation(t), 0.7)
    if name == "plateau_ties":          # most costs equal: ε constant (d = 0), every key of the range equal
        t = np.concatenate([np.full(3200, 1.0), rng.uniform(2, 10, 800)])
        return Scenario(name, N, rng.permutation(t), 0.5)
    if name == "dead_pile":             # > 1024 particles die tied at ε (flag 0, no resample); the next target
        # lies in the top bin of the loop kernel's window, which always holds key(ε): error 4 there
        t = np.concatenate([rng.uniform(0.01, 0.5, 3800), rng.uniform(0.999, 1, 1000), np.full(4000, 1.0),
                            rng.uniform(2, 3, 1200)])
        return Scenario(name, N, rng.permutation(t), 0.9, K=4, min_r_ess=0.02)
    if name == "cliff":                 # log-uniform 1e-300 .. 1e300, small α: ε falls by tens of decades
        t = 10.0 ** rng.uniform(-300, 300, 8192)
        return Scenario(name, N, t, 0.1, K=6, min_r_ess=0.5)
    if name == "cluster_outliers":      # > 4096 distinct keys around the target + outliers near ±1e300
        base = np.float64(1.0).view(np.int64)
        cl = (base + rng.integers(0, 1 << 22, 60000)).view(np.float64)
        t = np.concatenate([cl, rng.uniform(0.5, 1, 2000) * 1e300, -rng.uniform(0.5, 1, 2000) * 1e300])
        return Scenario(name, N, rng.permutation(t), 0.6, K=4)
    if name == "gap_needmin":           # rank j the last key of a dense cluster, rank j + 1 far above it
        base = np.float64(1.0).view(np.int64)
        t = np.concatenate([(base + rng.integers(0, 1 << 20, 3000)).view(np.float64), 1e6 + rng.uniform(0, 1, 1000)])
        t = rng.permutation(t)
        ncl = int((_init_costs(t, N, orc) < 2).sum())
        return Scenario(name, N, t, _alpha_for(N, ncl, 0.5), min_r_ess=0.5)
    raise KeyError(name)
