"""Timing of abc_reject (kabc_abc_reject) against the path that existed before it: prior_predictive over the same
rows in chunks of 2^20 plus a numpy filter on the host, which ships every draw over PCIe.

Shapes: (a) GaussDist, D = 8; (b) the README simulator NormalMeanStdSim(1000, ...); (c) Mixture, D = 1.
For each, eps is the quantile of a pilot run (2^20 rows) at acceptance 1e-1, 1e-2 and 1e-4, and n is chosen so
that the run draws about 2^22 rows (2^24 at 1e-4).  Both paths return the first n accepted rows of the same
stream (checked: same indices).  Timing: every shape is warmed up on both paths, then the two ALTERNATE in one
process; a host clock around calls that end in a device synchronise; median, min and max of --reps repeats.
`holds`: the median of abc_reject is below the median of the parent path by more than the spread (max - min)
of either.
Also: the device time of the fused kernel per 2^20 rows (KABC_EVAL_TIMING=1) beside the evaluation kernel's of
prior_predictive for the same cost and the phases course's (KABC_REJECT_COURSE=phases), and the register / LDS /
scratch use of the kernels (--resources: the output of tools/kernel_resources.py on build/capi_abc_reject.o).
   python tools/abc_reject_probe.py [--out profiles/abc_reject_probe.json] [--reps 7]"""
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
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warm", type=int, default=2)
ap.add_argument("--resources", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                    "profiles", "abc_reject_resources.txt"))
args = ap.parse_args()
CHUNK = 1 << 20
SEED = 1


def parent_path(prior, cost, eps, n, max_draws):
    """what a user wrote before abc_reject: pilot chunks to the host, a filter there"""
    P, C_, L, I = [], [], [], []
    got, off = 0, 0
    while got < n and off < max_draws:
        m = min(CHUNK, max_draws - off)
        t = k.prior_predictive(prior, cost, m, seed=SEED, first_row=off, return_array=True)
        keep = np.flatnonzero(t.C <= eps)[:n - got]
        P.append(t.P[keep])
        C_.append(t.C[keep])
        L.append(t.logprior[keep])
        I.append(keep + off)
        got += keep.size
        off += m
    return np.concatenate(P), np.concatenate(C_), np.concatenate(L), np.concatenate(I)


def stats(ws):
    ws = sorted(ws)
    return {"median_ms": round(ws[len(ws) // 2] * 1e3, 3), "min_ms": round(ws[0] * 1e3, 3),
            "max_ms": round(ws[-1] * 1e3, 3), "spread_ms": round((ws[-1] - ws[0]) * 1e3, 3)}


sim_prior = k.Factored(k.Uniform(1, 3), k.Truncated(k.Normal(0, 0.1), 0, 100))
shapes = [
    ("gauss_d8", k.Factored(*[k.Normal(0, 5)] * 8), k.costs.GaussDist(np.linspace(-1, 1, 8)), True),
    ("readme_sim", sim_prior, k.costs.NormalMeanStdSim(1000, 2.0, 0.04), False),
    ("mixture", k.Normal(0, 1), k.costs.Mixture(0.0), True),
]
out = {"cases": {}, "kernel": {}, "resources": []}
for name, prior, cost, cheap in shapes:
    pilot = k.prior_predictive(prior, cost, CHUNK, seed=SEED + 1, return_array=True).C
    for q in (1e-1, 1e-2, 1e-4):
        eps = float(np.quantile(pilot, q))
        target = 1 << (24 if q < 1e-3 else 22)
        n = max(1, int(round(q * target)))
        budget = 8 * target

        def new():
            return k.abc_reject(prior, cost, eps, n, draws=budget, seed=SEED, return_array=True)

        def old():
            return parent_path(prior, cost, eps, n, budget)
        for _ in range(args.warm):
            r, o = new(), old()
        assert np.array_equal(r.info["index"], o[3]) and np.array_equal(r.P, o[0]) and np.array_equal(r.C, o[1])
        wn, wo = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            r = new()
            wn.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            old()
            wo.append(time.perf_counter() - t0)
        sn, so = stats(wn), stats(wo)
        draws = r.info["draws"]
        e = {"eps": eps, "n": n, "draws": draws, "acceptance": r.info["acceptance"], "launches": r.info["launches"],
             "course": r.info["course"], "abc_reject": sn, "parent_path": so,
             "abc_reject_draws_per_s": round(draws / (sn["median_ms"] * 1e-3), 0),
             "parent_draws_per_s": round(draws / (so["median_ms"] * 1e-3), 0),
             "ratio_parent_over_new": round(so["median_ms"] / sn["median_ms"], 2)}
        gap = so["median_ms"] - sn["median_ms"]
        if cheap:      # required at acceptance <= 1e-2: faster by more than the spread of either
            e["holds"] = gap > max(sn["spread_ms"], so["spread_ms"])
        else:          # the kernel time is the simulator's: not slower beyond the spread
            e["holds"] = gap > -max(sn["spread_ms"], so["spread_ms"])
        out["cases"][f"{name}@{q:g}"] = e
        print(name, q, json.dumps(e), flush=True)

# device time per 2^20 rows: the fused kernel, the phases course, and the evaluation kernel alone
os.environ["KABC_EVAL_TIMING"] = "1"
for name, prior, cost, _ in shapes:
    N = 1 << 24
    e = {}
    for course in ("fused", "phases"):
        if course == "phases":
            os.environ["KABC_REJECT_COURSE"] = "phases"
        ks = []
        for _ in range(args.warm + 5):
            r = k.abc_reject(prior, cost, draws=N, keep=1000, seed=SEED, return_array=True)
            ks.append(r.info["kernel_ms"])
        os.environ.pop("KABC_REJECT_COURSE", None)
        assert r.info["course"] == course
        e[f"{course}_us_per_2^20_rows"] = round(sorted(ks[args.warm:])[2] * 1e3 * CHUNK / N, 2)
        e[f"{course}_launches"] = r.info["launches"]
    ps = [k.prior_predictive(prior, cost, CHUNK, seed=SEED, return_array=True).info for _ in range(args.warm + 5)]
    e["cost_eval_kernel_us_per_2^20_rows"] = round(sorted(i["kernel_ms"] for i in ps[args.warm:])[2] * 1e3, 2)
    e["prior_kernels_us_per_2^20_rows"] = round(sorted(i["prior_kernel_ms"] for i in ps[args.warm:])[2] * 1e3, 2)
    out["kernel"][name] = e
    print("kernel", name, json.dumps(e), flush=True)
os.environ.pop("KABC_EVAL_TIMING", None)

if os.path.exists(args.resources):
    with open(args.resources) as f:
        out["resources"] = [" ".join(line.split()) for line in f if "abc_reject" in line and "vgpr" in line]
print(json.dumps(out))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
