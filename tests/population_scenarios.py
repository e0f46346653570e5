"""Adversarial cost laws for the two population samplers, ABCDE (src/smc.jl:347-430) and pfilter (:275-340),
shared by test_population_cost_edges.py (CPU: the oracle against the restatements of tests/helpers.py, and the
gate that decides what may run on a GPU) and test_gpu_population_cost_edges.py (every device course).

As in smc_scenarios.py each scenario is a table of costs under x[0] ~ DiscreteUniform(0, M - 1) with
cost = table[x[0]] -- the same source, so one run-time compilation serves every scenario --: every cost is an
exact table entry, recomputable from the positions, and the log-prior is one constant or -Inf.  The tables put
in front of the ranking code what the built-in costs (distances, all >= 0) never do: negative costs, signed
zeros, subnormals, plateaus, +-Inf, NaN, 1e308-scale costs and clusters of neighbouring doubles."""
import numpy as np

from helpers import DOM_ABCDE_INIT, DOM_PF_INIT, TableProblem
from smc_scenarios import SOURCE

SEED = 11
NAMES = ["neg_mixed", "signed_zero", "subnormal", "plateau_ties", "inf_holes", "neg_inf_sink", "nan_holes", "cliff",
         "huge_span", "cluster"]
GENERATIONS = 6
ABCDE_LEGS = {"a0": dict(alpha=0.0, earlystop=False), "a03-earlystop": dict(alpha=0.3, earlystop=True)}
PF_KW = dict(q=0.7, eff_tol=0.0, max_iters=4)
PF_NAN_ERROR = "pfilter: quantile of the costs is undefined (NaN or empty)"

# the smallest shapes at which each course's structure is ragged.  course: (environment, N, scenarios or None)
ABCDE_ENV = ("KABC_ABCDE_SMALL", "KABC_ABCDE_RANK", "KABC_ABCDE_DONOR", "KABC_ABCDE_BLOCKS_FROM")
ABCDE_COURSES = {
    "one-workgroup": ({}, 65, None),
    "scans": ({"KABC_ABCDE_SMALL": "0"}, 130, None),
    "teams": ({}, 257, None),
    "blocks": ({}, 1537, None),
    "blocks-two-per-lane": ({}, 16500, ("signed_zero", "plateau_ties")),
    "wavelet": ({"KABC_ABCDE_RANK": "wavelet"}, 4100, None),      # three radix tiles, the last of four keys; 13 levels
}
ABCDE_BATCH_N, BATCH_SEEDS = 65, (SEED, 12, 15)     # (seeds at which every scenario passes the gate)
PF_ENV = ("KABC_PF_SMALL", "KABC_PF_PASSES", "KABC_PF_BATCH")
PF_COURSES = {
    # (the default course of <= 256 particles is pf_small_kernel with a built-in cost; a run-time compiled
    # cost has no such kernel and goes phase by phase)
    "default-130": ({}, 130),
    "loop-130": ({"KABC_PF_SMALL": "0"}, 130),
    "loop-1000": ({"KABC_PF_SMALL": "0"}, 1000),
    "passes-130": ({"KABC_PF_SMALL": "0", "KABC_PF_PASSES": "1"}, 130),
    "passes-1000": ({"KABC_PF_SMALL": "0", "KABC_PF_PASSES": "1"}, 1000),
}
PF_BATCH_N = 65
# huge_span: the table's seed offset by N, and the seeds of its batch runs (see build)
HUGE_SPAN_TABLE = {130: 6, 1537: 4, 4100: 6}
HUGE_SPAN_BATCH_SEEDS = (SEED, 15, 16)


def abcde_cases():
    """(scenario, N) of every ABCDE case some test runs (the batch runs at ABCDE_BATCH_N are one-workgroup's)"""
    out = []
    for _, n, only in ABCDE_COURSES.values():
        out += [(name, n) for name in (only or NAMES) if (name, n) not in out]
    return out


def pfilter_cases():
    out = [(name, PF_BATCH_N) for name in NAMES]
    for _, n in PF_COURSES.values():
        out += [(name, n) for name in NAMES if (name, n) not in out]
    return out


class Scenario:
    def __init__(self, name, table, batch_seeds):
        self.name, self.batch_seeds = name, tuple(batch_seeds)
        self.table = np.asarray(table, dtype=np.float64)
        fin = self.table[np.isfinite(self.table)]
        self.eps_target = float(np.quantile(fin, 0.05))     # ABCDE's ϵ_target: the 5 % quantile of the finite entries

    def prior(self, k):
        return k.DiscreteUniform(0, self.table.size - 1)

    def cost(self, k):
        return k.costs.UserCost(SOURCE, dims=[1], data=self.table, name="table")

    def abcde_kw(self, N, leg, generations=GENERATIONS, seed=SEED):
        return dict(nparticles=N, generations=generations, seed=seed, **ABCDE_LEGS[leg])

    def pf_kw(self, max_iters=PF_KW["max_iters"], seed=SEED):
        return dict(PF_KW, max_iters=max_iters, seed=seed)

    def problem(self, k, orc, seed=SEED):
        lp0 = float(orc.factored_logpdf(self.prior(k), np.zeros((1, 1)))[0])
        return TableProblem(self.table, lp0, seed, orc.philox_rounds(), orc.normal_pairs)

    def initial(self, k, orc, N, algo, seed=SEED):
        """the state after the initial draw (:349-366 ABCDE, :280-294 pfilter): attempt k of particle i is
        rand(prior) from the stream (seed, i, k, DOM_*_INIT), drawn again while its cost is not finite (the
        log-prior is finite everywhere on the support)"""
        pb = self.problem(k, orc, seed)
        dom = DOM_ABCDE_INIT if algo == "abcde" else DOM_PF_INIT
        th = orc.factored_rand(self.prior(k), N, seed=seed, domain=dom)[:, 0]
        C = pb.cost(th)
        attempt = 0
        while not np.isfinite(C).all():
            attempt += 1
            assert attempt < 1000
            again = ~np.isfinite(C)
            th[again] = orc.factored_rand(self.prior(k), N, seed=seed, domain=dom, attempt=attempt)[again, 0]
            C = pb.cost(th)
        st = dict(theta=th, C=C, logpi=np.full(N, pb.lp0))
        st.update(dict(generation=0, nsims=0) if algo == "abcde" else dict(iteration=0, nreps=0, cost_evals=0))
        return st


def build(name, N):
    """the Scenario `name` for runs of N particles; its table is seeded by the name (huge_span: and sized by N)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "neg_mixed":             # costs of both signs: ϵ_l < 0, ranks across zero
        t = rng.uniform(-1e3, 1e3, 4096)
    elif name == "signed_zero":         # -0.0 == +0.0 by value, two keys by bits
        t = rng.permutation(np.concatenate([-rng.uniform(1e-3, 1, 300), np.full(500, -0.0), np.full(500, 0.0),
                                            rng.uniform(1e-3, 1, 2700)]))
    elif name == "subnormal":           # integer multiples of 5e-324 with both zeros
        t = rng.permutation(np.concatenate([rng.integers(1, 1 << 40, 3000) * 5e-324, np.zeros(500),
                                            np.full(500, -0.0)]))
    elif name == "plateau_ties":        # 80 % equal to 1.0
        t = rng.permutation(np.concatenate([np.full(3200, 1.0), rng.uniform(2, 10, 800)]))
    elif name == "inf_holes":           # 30 % +Inf: proposals that are never accepted, re-draws at the start
        t = rng.permutation(np.concatenate([rng.uniform(0, 1, 2800), np.full(1200, np.inf)]))
    elif name == "neg_inf_sink":        # about 2 % -Inf: accepted by every threshold, then ϵ_l = -Inf
        t = rng.permutation(np.concatenate([rng.uniform(-1, 1, 4014), np.full(82, -np.inf)]))
    elif name == "nan_holes":           # 25 % NaN: compares false both ways
        t = rng.permutation(np.concatenate([rng.uniform(-1, 1, 3072), np.full(1024, np.nan)]))
    elif name == "cliff":               # ±10^U(-300, 300)
        t = rng.choice([-1.0, 1.0], 8192) * 10.0 ** rng.uniform(-300, 300, 8192)
    elif name == "huge_span":
        # ±[0.85, 1.7]e308: ϵ_h - ϵ_l overflows as soon as both signs are in the population, and then ϵ_pop is NaN
        # (α = 0: 0 Inf) or +Inf (α > 0) and no particle needs a donor.  So that the donor draws see 1e308-scale
        # costs too, the negative entries are few -- about M / (2 N) of them, table and seeds chosen so that the
        # initial population holds none and a proposal finds one within the run (the gate of
        # test_population_cost_edges.py checks both)
        M = max(4096, 4 * N)
        rng = np.random.default_rng(sum(map(ord, name)) + 1000 * HUGE_SPAN_TABLE.get(N, 0))
        t = rng.uniform(0.85, 1.7, M) * 1e308
        t[rng.choice(M, max(1, round(M / (2 * N))), replace=False)] *= -1.0
    elif name == "cluster":             # 60 000 neighbouring doubles at 1.0, outliers at ±1e300
        base = np.float64(1.0).view(np.int64)
        cl = (base + rng.integers(0, 1 << 22, 60000)).view(np.float64)
        t = rng.permutation(np.concatenate([cl, rng.uniform(0.5, 1, 2000) * 1e300, -rng.uniform(0.5, 1, 2000) * 1e300]))
    else:
        raise KeyError(name)
    return Scenario(name, t, HUGE_SPAN_BATCH_SEEDS if name == "huge_span" else BATCH_SEEDS)


# ---- the restated runs (tests/helpers.py abcde_step, pfilter_step) and the gate: a case is informative and ends,
# or it runs nowhere.  Computed once per case and shared by the tests of both files.
_replays = {}


def replay_abcde(k, orc, name, N, leg, seed=SEED):
    """[S_0 .. S_6]: the initial state and abcde_step of each; asserts the gate"""
    from helpers import abcde_step
    key = ("abcde", name, N, leg, seed)
    if key not in _replays:
        sc = build(name, N)
        pb = sc.problem(k, orc, seed)
        states = [sc.initial(k, orc, N, "abcde", seed)]
        for _ in range(GENERATIONS):
            states.append(abcde_step(pb, states[-1], eps_target=sc.eps_target, **ABCDE_LEGS[leg]))
            assert not states[-1]["broke"], (key, "the earlystop break: not every generation runs")
        W = [s["w"] for s in states[1:]]
        moved = float(np.mean(states[-1]["theta"] != states[0]["theta"]))
        assert moved >= 0.15, (key, f"{moved:.2f} of the rows differ from the initial population")
        assert sum(w["n_donor"] for w in W) >= 1, (key, "no donor draw")
        witness = {
            "neg_mixed": any(w["neg_donor"] for w in W),
            "signed_zero": any(w["zero_needs_donor"] for w in W),
            "plateau_ties": max(w["tie_frac"] for w in W) > 0.5,
            "inf_holes": any(w["inf_eval"] for w in W),
            # -Inf entered the state, and ϵ_pop was NaN in a generation after that
            "neg_inf_sink": any(w["neg_inf_state"] and w["eps_pop_nan"] for w in W),
            "huge_span": any(w["span_overflow"] for w in W),
            "nan_holes": sum(w["nan_refused"] for w in W) >= 1,
        }
        assert witness.get(name, True), (key, "the scenario's witness")
        _replays[key] = states
    return _replays[key]


def replay_pfilter(k, orc, name, N, seed=SEED):
    """([S_0 .. S_n], nan): the initial state and pfilter_step of each until a stop rule of :330-332 (or
    "nothing was bad": eff = 0 / 0); nan: the next quantile met a NaN cost instead.  Asserts the gate."""
    from helpers import pfilter_step
    key = ("pfilter", name, N, seed)
    if key not in _replays:
        sc = build(name, N)
        pb = sc.problem(k, orc, seed)
        states, nan = [sc.initial(k, orc, N, "pfilter", seed)], False
        while True:
            try:
                st = pfilter_step(pb, states[-1], q=PF_KW["q"])   # (asserts nok >= 3 wherever a particle is bad)
            except ValueError:
                nan = True
                break
            states.append(st)
            assert st["max_attempts"] <= 4096, (key, st["max_attempts"])
            if st["eff"] != st["eff"] or st["eff"] < PF_KW["eff_tol"] or st["iteration"] > PF_KW["max_iters"]:
                break
        assert any(s["nbad"] > 0 for s in states[1:]), (key, "nothing was ever bad")
        assert nan == (name == "nan_holes"), (key, "a NaN cost is accepted in nan_holes and nowhere else")
        _replays[key] = (states, nan)
    return _replays[key]


# ---- pf_small_kernel (at most 256 particles, built-in costs only) never meets a table cost.  Its selection --
# ϵ = quantile(C, q) by key rank counting, idxok from ballots -- sees the finite tables through a state handed
# to resume=: costs drawn from the table on particles of DiscreteUniform(0, 9) under AbsDiff(3), whose
# proposals reach the cost 0 (θ[d] == θ[c] and θ[b] == 3), below every ϵ the tables give at q = 0.7.
CRAFTED_NAMES = ["neg_mixed", "signed_zero", "subnormal", "plateau_ties", "cliff", "huge_span", "cluster"]
CRAFTED_N, CRAFTED_TARGET, CRAFTED_M = 130, 3.0, 10
CRAFTED_KW = dict(q=PF_KW["q"], eff_tol=0.0, max_iters=1)      # one more iteration from a state at iteration 1


class AbsDiffProblem(TableProblem):
    """|x[0] - target| under x[0] ~ DiscreteUniform(0, M - 1) (include/kabc_costs.h kabc_cost_abs_diff)"""

    def __init__(self, target, M, lp0, seed, rounds, normal_pairs):
        super().__init__(np.zeros(M), lp0, seed, rounds, normal_pairs)
        self.target = float(target)

    def cost(self, x):
        return np.abs(np.asarray(x, dtype=np.float64) - self.target)


def crafted_pfilter_case(k, orc, name):
    """(prior, cost, state, next): a PfilterState at iteration 1 whose costs are table entries, and pfilter_step
    of it -- asserting the gate: it ends within 4096 attempts, something is bad, b, c and d can differ"""
    from helpers import pfilter_step
    from kissabc_jl_amd import api
    key = ("crafted", name)
    if key not in _replays:
        N = CRAFTED_N
        table = build(name, N).table
        rng = np.random.default_rng(sum(map(ord, name)) + 1)
        prior = k.DiscreteUniform(0, CRAFTED_M - 1)
        theta = rng.integers(0, CRAFTED_M, N).astype(np.float64).reshape(N, 1)
        C = rng.choice(table[np.isfinite(table)], N)
        lp = orc.factored_logpdf(prior, theta)
        pb = AbsDiffProblem(CRAFTED_TARGET, CRAFTED_M, lp[0], SEED, orc.philox_rounds(), orc.normal_pairs)
        st = dict(theta=theta[:, 0], C=C, logpi=lp, iteration=1, nreps=N, cost_evals=N)
        nxt = pfilter_step(pb, st, q=CRAFTED_KW["q"])
        assert nxt["nbad"] > 0 and nxt["max_attempts"] <= 4096, (key, nxt["nbad"], nxt["max_attempts"])
        _replays[key] = (theta, C, lp, nxt)
    theta, C, lp, nxt = _replays[key]
    state = api.PfilterState(theta.copy(), C.copy(), lp.copy(), seed=SEED, iteration=1, nreps=CRAFTED_N,
                             cost_evals=CRAFTED_N, eps=np.inf, eff=0.5)
    return k.DiscreteUniform(0, CRAFTED_M - 1), k.costs.AbsDiff(CRAFTED_TARGET), state, nxt
