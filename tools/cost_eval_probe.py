"""Timing of DeviceCost.evaluate / prior_predictive (kabc_cost_eval, kabc_prior_predictive) for
   (a) GaussDist, D = 8, n = 2^20, one replicate,
   (b) the README simulator NormalMeanStdSim(1000, ...), D = 2, n = 65 536, nrep = 16,
   (c) the same simulator at n = 100, one replicate (a posterior predictive of a default smc):
wall time of the call (median of 20 after 3 warm-up calls), device time of the evaluation kernel (event pairs
around it: KABC_EVAL_TIMING=1, a separate set of calls), evaluations per second, and for (a) the bytes the
kernel moves over its time as a share of 8.0 TB/s.  Beside them the one-core oracle's evaluations per second on
a slice ("extrapolated": the slice's rate stands for the whole).
The bar: prior_predictive(prior, cost, N) against smc(prior, cost, nparticles=N, max_iterations=1) of the same
library, same process, alternating -- the smc call makes the same N draws and N evaluations in its initial step
and a selection, a pass and a result copy on top.
   python tools/cost_eval_probe.py [--out profiles/cost_eval_probe.json] [--reps 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kissabc_jl_amd as k  # noqa: E402
from oracle import oracle as orc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warm", type=int, default=3)
args = ap.parse_args()
HBM = 8.0e12


def med(ws):
    return sorted(ws)[len(ws) // 2]


def wall(fn):
    for _ in range(args.warm):
        fn()
    ws = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        fn()
        ws.append(time.perf_counter() - t0)
    return ws


def kernel_ms(prior, cost, n, nrep):
    os.environ["KABC_EVAL_TIMING"] = "1"
    try:
        ks = []
        for _ in range(args.warm + 7):
            ks.append(k.prior_predictive(prior, cost, n, nrep=nrep, seed=1, return_array=True).info)
        ks = ks[args.warm:]
        return med([i["kernel_ms"] for i in ks]), med([i["prior_kernel_ms"] for i in ks])
    finally:
        os.environ.pop("KABC_EVAL_TIMING", None)


def oracle_rate(cost, theta, nrep, budget_s=2.0):
    from kissabc_jl_amd import _cdefs as cd
    t0, m = time.perf_counter(), 0
    for i in range(theta.shape[0]):
        for j in range(nrep or 1):
            orc.cost_eval(cost, theta[i], seed=1, walker=i, t=j, domain=cd.DOM_EVAL_COST)
            m += 1
        if time.perf_counter() - t0 > budget_s:
            break
    return m / (time.perf_counter() - t0), m


sim = k.costs.NormalMeanStdSim(1000, 2.0, 0.04)
sim_prior = k.Factored(k.Uniform(1, 3), k.Truncated(k.Normal(0, 0.1), 0, 100))
cases = [
    ("a_gauss_d8_n2^20", k.Factored(*[k.Normal(0, 5)] * 8), k.costs.GaussDist(np.linspace(-1, 1, 8)), 1 << 20, None),
    ("b_readme_sim_n65536_x16", sim_prior, sim, 65536, 16),
    ("c_readme_sim_n100", sim_prior, sim, 100, None),
]
out = {"cases": {}, "bar": {}}
for name, prior, cost, n, nrep in cases:
    R = nrep or 1
    theta = k.prior_predictive(prior, cost, n, seed=1, return_array=True).P
    e = {"n": n, "nrep": R, "D": theta.shape[1]}
    ws = wall(lambda: cost.evaluate(theta, nrep=nrep, seed=1))
    e["evaluate_wall_ms"] = round(med(ws) * 1e3, 3)
    ws = wall(lambda: k.prior_predictive(prior, cost, n, nrep=nrep, seed=1, return_array=True))
    e["prior_predictive_wall_ms"] = round(med(ws) * 1e3, 3)
    km, pm = kernel_ms(prior, cost, n, nrep)
    e["eval_kernel_ms"] = round(km, 4)
    e["prior_kernels_ms"] = round(pm, 4)
    e["evals_per_s_kernel"] = round(n * R / (km * 1e-3), 0)
    e["evals_per_s_evaluate_call"] = round(n * R / (e["evaluate_wall_ms"] * 1e-3), 0)
    if name.startswith("a_"):
        nbytes = n * theta.shape[1] * 8 + n * R * 8      # rows read once, results written once
        e["kernel_bytes"] = nbytes
        e["kernel_share_of_8TBs"] = round(nbytes / (km * 1e-3) / HBM, 4)
    rate, m = oracle_rate(cost, theta, nrep)
    e["oracle_one_core_evals_per_s"] = round(rate, 0)
    e["oracle_note"] = f"extrapolated from a slice of {m} evaluations" if m < n * R else "whole input"
    out["cases"][name] = e
    print(name, json.dumps(e), flush=True)

# the bar: prior_predictive(N) against smc(N, max_iterations=1), alternating, same process
for name, prior, cost, n, nrep in cases[:2]:
    def pp():
        return k.prior_predictive(prior, cost, n, seed=1, return_array=True)

    def sm():
        return k.smc(prior, cost, nparticles=n, max_iterations=1, seed=1, return_array=True)
    for _ in range(args.warm):
        pp()
        sm()
    wp, wsm = [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        pp()
        wp.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        sm()
        wsm.append(time.perf_counter() - t0)
    b = {"N": n, "prior_predictive_ms": round(med(wp) * 1e3, 3), "smc_max_iterations_1_ms": round(med(wsm) * 1e3, 3),
         "prior_predictive_min_ms": round(min(wp) * 1e3, 3), "smc_min_ms": round(min(wsm) * 1e3, 3)}
    b["ratio"] = round(b["prior_predictive_ms"] / b["smc_max_iterations_1_ms"], 3)
    b["holds"] = b["prior_predictive_ms"] <= b["smc_max_iterations_1_ms"]
    out["bar"][name] = b
    print("bar", name, json.dumps(b), flush=True)
print(json.dumps(out))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
