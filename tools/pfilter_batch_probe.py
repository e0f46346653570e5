"""Wall time of pfilter_batch (kabc_pfilter_run_batch: R independent runs as the workgroups of one launch)
against the same R runs as pfilter() calls one after another, for three problems -- the easy Gaussian one
(final eff 0.6-0.7) and the two low-acceptance ones (the README simulator, discrete_256: final eff
0.07-0.10) --, R in {1, 64, 256, 1024, 4096}; one pfilter() call at each problem; and the
attempt-parallel rejection phase against KABC_PF_BATCH_SPREAD=0 at R = 1024.
   python tools/pfilter_batch_probe.py [--out profiles/<name>.json] [--rs 1,64,256] [--only name]
The sequential time is measured for R <= 64 runs (every run once) and extrapolated from the mean of
those 64 above ("seq_ms_est")."""
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
ap.add_argument("--rs", default="1,64,256,1024,4096")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--only")
ap.add_argument("--ab-r", type=int, default=1024)
args = ap.parse_args()
RS = [int(x) for x in args.rs.split(",")]
NSEQ = 64

N2 = k.Factored(k.Normal(0, 5), k.Normal(0, 5))
problems = [
    ("gauss_n100", N2, k.costs.GaussDist([1.0, -0.5]), 100, dict(epstol=0.05)),
    ("readme_sim_n100", k.Factored(k.Uniform(1, 3), k.Truncated(k.Normal(0, 0.1), 0, 100)),
     k.costs.NormalMeanStdSim(1000, 2.0, 0.04), 100, dict(max_iters=30)),
    ("discrete_n256", k.Factored(k.Normal(1, 0.5), k.DiscreteUniform(1, 10)), k.costs.NoisyQuadDU(5.5), 256,
     dict(max_iters=15)),
]


def timed_batch(pr, co, N, R, kw, reps):
    k.pfilter_batch(pr, co, N, R, seed=1, return_array=True, **kw)  # (warm: allocations, pools)
    ws = []
    for _ in range(reps):
        t0 = time.perf_counter()
        b = k.pfilter_batch(pr, co, N, R, seed=1, return_array=True, **kw)
        ws.append(time.perf_counter() - t0)
    return ws, b


out = {"single": {}, "batch": {}, "spread_ab": {}}
for name, pr, co, N, kw in problems:
    if args.only and args.only != name:
        continue
    # one kabc_pfilter_run call (its own course)
    for _ in range(3):
        k.pfilter(pr, co, N, seed=1, return_array=True, **kw)
    ws = []
    for _ in range(9):
        t0 = time.perf_counter()
        k.pfilter(pr, co, N, seed=1, return_array=True, **kw)
        ws.append(time.perf_counter() - t0)
    out["single"][name] = {"ms": round(sorted(ws)[4] * 1e3, 3)}
    seeds_all = k.api.chain_seeds(1, max(max(RS), NSEQ))
    seq = []  # the sequential course: every run once
    for s in seeds_all[:NSEQ]:
        t0 = time.perf_counter()
        k.pfilter(pr, co, N, seed=s, return_array=True, **kw)
        seq.append(time.perf_counter() - t0)
    os.environ.pop("KABC_PF_BATCH_SPREAD", None)
    for R in RS:
        ws, b = timed_batch(pr, co, N, R, kw, args.reps)
        e = {"batch_ms": round(sorted(ws)[len(ws) // 2] * 1e3, 3), "course": b.info["course"],
             "launches": b.info["launches"], "nreps_mean": round(float(np.mean([x.info["nreps"] for x in b])), 1),
             "iterations_mean": round(float(np.mean([x.info["iterations"] for x in b])), 2)}
        if R <= len(seq):
            e["seq_ms"] = round(sum(seq[:R]) * 1e3, 3)
        else:
            e["seq_ms_est"] = round(float(np.mean(seq)) * R * 1e3, 3)
        seq_ms = e.get("seq_ms", e.get("seq_ms_est"))
        e["speedup"] = round(seq_ms / e["batch_ms"], 2)
        e["batch_over_one_run"] = round(e["batch_ms"] / out["single"][name]["ms"], 2)
        out["batch"][f"{name}_R{R}"] = e
        print(name, R, json.dumps(e), flush=True)
    # the attempt-parallel phase against one lane per particle: best of `reps` each, with their spread
    ab = {}
    for label, val in (("spread", None), ("one_lane_per_particle", "0"), ("spread_again", None)):
        if val is None:
            os.environ.pop("KABC_PF_BATCH_SPREAD", None)
        else:
            os.environ["KABC_PF_BATCH_SPREAD"] = val
        ws, _ = timed_batch(pr, co, N, args.ab_r, kw, max(args.reps, 7))
        ab[label] = {"best_ms": round(min(ws) * 1e3, 3), "median_ms": round(sorted(ws)[len(ws) // 2] * 1e3, 3),
                     "worst_ms": round(max(ws) * 1e3, 3)}
    os.environ.pop("KABC_PF_BATCH_SPREAD", None)
    ab["R"] = args.ab_r
    ab["one_lane_over_spread"] = round(ab["one_lane_per_particle"]["best_ms"] /
                                       min(ab["spread"]["best_ms"], ab["spread_again"]["best_ms"]), 3)
    out["spread_ab"][name] = ab
    print(name, "spread_ab", json.dumps(ab), flush=True)
print(json.dumps(out))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
