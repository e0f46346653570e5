"""Timing of abc_reject_batch (kabc_abc_reject_batch) against what existed before it: K abc_reject calls one after
another (and, for the record, prior_predictive + numpy on one shared table).

Shapes: GaussDist D = 8 and Mixture at acceptance 1e-4 and 1e-2, NormalMeanStdSim(1000) at 1e-4, keep = 5000 on
GaussDist; K datasets in {1, 8, 64, 1024}; budgets of 1e5, 2^20 and 2e7 draws per run (the large budgets with the
small K only: the one-after-another leg has to fit the probe's time).  Every run draws its whole budget (n is above
what the budget accepts), all runs share the seed.  Legs, ALTERNATING in one process after a warm-up of each:
  sequential   K abc_reject calls                      (the baseline)
  table        abc_reject_batch, the default course for a shared seed, wavefront compaction
  table_wg     the same with KABC_REJECT_BATCH_COMPACT=wg
  grid         KABC_REJECT_BATCH_COURSE=grid
A host clock around calls that end in a device synchronise; median, min, max of --reps repeats; kernel_ms
(KABC_EVAL_TIMING=1) from one extra repeat per leg.  `table_holds`: the table's median is below the MINIMUM of the
sequential leg.  The results of the legs are compared (same indices and costs for every run) before timing.
   python tools/abc_reject_batch_probe.py [--out profiles/abc_reject_batch_probe.json] [--reps 5] [--quick]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kissabc_jl_amd as k  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--quick", action="store_true", help="K <= 64 and budgets <= 2^20 only")
args = ap.parse_args()
SEED = 1
KMAX = 64 if args.quick else 1024
rng = np.random.default_rng(7)


def stats(ws):
    ws = sorted(ws)
    return {"median_ms": round(ws[len(ws) // 2] * 1e3, 3), "min_ms": round(ws[0] * 1e3, 3),
            "max_ms": round(ws[-1] * 1e3, 3)}


class env:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        os.environ.update(self.kw)

    def __exit__(self, *a):
        for name in self.kw:
            os.environ.pop(name, None)


sim_prior = k.Factored(k.Uniform(1, 3), k.Truncated(k.Normal(0, 0.1), 0, 100))
base8 = np.linspace(-1, 1, 8)
shapes = {
    "gauss_d8": (k.Factored(*[k.Normal(0, 5)] * 8),
                 [k.costs.GaussDist(base8 + 0.05 * rng.normal(size=8)) for _ in range(KMAX)]),
    "mixture": (k.Normal(0, 1), [k.costs.Mixture(0.02 * rng.normal()) for _ in range(KMAX)]),
    "readme_sim": (sim_prior, [k.costs.NormalMeanStdSim(1000, 2.0 + 0.01 * rng.normal(), 0.04) for _ in range(64)]),
}
# (shape, mode, K, budget)
plan = []
for shape in ("gauss_d8", "mixture"):
    for q in (1e-4, 1e-2):
        for K in (1, 8, 64, 1024):
            plan.append((shape, q, K, 100_000))
        for K in (1, 8, 64):
            plan.append((shape, q, K, 1 << 20))
        if not args.quick:
            for K in (1, 8):
                plan.append((shape, q, K, 20_000_000))
for K in (1, 8, 64):
    plan.append(("readme_sim", 1e-4, K, 100_000))
for K, budget in ((1, 100_000), (64, 100_000), (1024, 100_000), (1, 1 << 20), (8, 1 << 20), (64, 1 << 20)):
    plan.append(("gauss_d8", "keep5000", K, budget))
plan = [p for p in plan if p[2] <= KMAX]

pilot_eps = {}


def eps_of(shape, q):
    """per-run eps: the q-quantile of each dataset's own pilot run"""
    if (shape, q) not in pilot_eps:
        prior, costs = shapes[shape]
        pilot_eps[(shape, q)] = [float(np.quantile(k.prior_predictive(prior, c, 1 << 17, seed=SEED + 1,
                                                                      return_array=True).C, q)) for c in costs]
    return pilot_eps[(shape, q)]


out = {"cases": [], "table_from_one_shared_prior_predictive": []}
for shape, q, K, budget in plan:
    prior, costs = shapes[shape]
    costs = costs[:K]
    if q == "keep5000":
        kw, eps = dict(draws=budget, keep=5000), None
    else:
        eps = eps_of(shape, q)[:K]
        kw = dict(draws=budget, n=int(4 * q * budget) + 64)

    def sequential():
        return [k.abc_reject(prior, c, None if eps is None else eps[r], seed=SEED, return_array=True, **kw)
                for r, c in enumerate(costs)]

    def batch():
        return k.abc_reject_batch(prior, costs, eps, seed=SEED, return_array=True, **kw)

    legs = {"sequential": (sequential, {}), "table": (batch, {}),
            "table_wg": (batch, {"KABC_REJECT_BATCH_COMPACT": "wg"}), "grid": (batch, {"KABC_REJECT_BATCH_COURSE": "grid"})}
    res, info = {}, {}
    for name, (fn, e) in legs.items():       # warm-up, and the legs agree
        with env(**e):
            res[name] = fn()
        if name != "sequential":
            info[name] = res[name].info
            assert info[name]["course"] == name.split("_")[0], info[name]
            for a, b in zip(res[name], res["sequential"]):
                assert np.array_equal(a.info["index"], b.info["index"]) and np.array_equal(a.C, b.C)
                assert a.info["draws"] == b.info["draws"] == budget
    walls = {name: [] for name in legs}
    for _ in range(args.reps):
        for name, (fn, e) in legs.items():
            with env(**e):
                t0 = time.perf_counter()
                fn()
                walls[name].append(time.perf_counter() - t0)
    entry = {"shape": shape, "mode": q, "K": K, "budget": budget,
             "accepted_per_run": round(float(np.mean([r.C.size for r in res["sequential"]])), 1)}
    for name, (fn, e) in legs.items():
        with env(KABC_EVAL_TIMING="1", **e):
            r = fn()
        kms = sum(x.info["kernel_ms"] for x in r) if name == "sequential" else r.info["kernel_ms"]
        entry[name] = dict(stats(walls[name]), kernel_ms=round(kms, 3))
        if name != "sequential":
            entry[name].update(launches=info[name]["launches"], rows_drawn=info[name]["rows_drawn"])
    entry["speedup_table"] = round(entry["sequential"]["median_ms"] / entry["table"]["median_ms"], 2)
    entry["speedup_grid"] = round(entry["sequential"]["median_ms"] / entry["grid"]["median_ms"], 2)
    entry["table_holds"] = entry["table"]["median_ms"] < entry["sequential"]["min_ms"]
    entry["table_below_grid"] = entry["table"]["median_ms"] < entry["grid"]["min_ms"]
    out["cases"].append(entry)
    print(json.dumps(entry), flush=True)

# for the record: one shared prior_predictive table (theta over PCIe once), every dataset scored by numpy on the host
for K in (8, 64):
    prior, costs = shapes["gauss_d8"]
    eps = eps_of("gauss_d8", 1e-2)[:K]
    ws = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        t = k.prior_predictive(prior, costs[0], 1 << 20, seed=SEED, return_array=True)
        for r in range(K):
            c = np.sqrt(((t.P - costs[r].params) ** 2).sum(axis=1))
            np.flatnonzero(c <= eps[r])
        ws.append(time.perf_counter() - t0)
    e = dict(shape="gauss_d8", K=K, budget=1 << 20, **stats(ws))
    out["table_from_one_shared_prior_predictive"].append(e)
    print(json.dumps(e), flush=True)

print(json.dumps(out))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
