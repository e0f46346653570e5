"""Wall time of ABCDE_batch (kabc_abcde_run_batch: R independent runs as the workgroups of one launch)
against the same R runs as ABCDE() calls one after another, for the reference's defaults (gauss,
50 particles x 20 generations) and 256 particles x 200 generations, R in {1, 64, 256, 1024, 4096}; and
one ABCDE() call at each shape, as a check against a run of R = 1.
   python tools/abcde_batch_probe.py [--out profiles/<name>.json] [--rs 1,64,256]
The sequential time is measured for R <= 256 runs (every run once) and extrapolated from the mean of
those 256 above ("seq_ms_est")."""
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
args = ap.parse_args()
RS = [int(x) for x in args.rs.split(",")]

N2 = k.Factored(k.Normal(0, 5), k.Normal(0, 5))
gauss = k.costs.GaussDist([1.0, -0.5])
problems = [("gauss_n50_g20", N2, gauss, 0.05, dict(nparticles=50, generations=20)),
            ("gauss_n256_g200", N2, gauss, 0.05, dict(nparticles=256, generations=200))]
out = {"single": {}, "batch": {}}
for name, pr, co, eps, kw in problems:
    # one kabc_abcde_run call (its own course: a few launches per generation)
    for _ in range(3):
        k.ABCDE(pr, co, eps, seed=1, return_array=True, **kw)
    ws = []
    for _ in range(9):
        t0 = time.perf_counter()
        k.ABCDE(pr, co, eps, seed=1, return_array=True, **kw)
        ws.append(time.perf_counter() - t0)
    out["single"][name] = {"ms": round(sorted(ws)[4] * 1e3, 3)}
    seeds_all = k.api.chain_seeds(1, max(RS))
    seq = []  # the sequential course: every run once, R <= 256
    for s in seeds_all[:min(256, max(RS))]:
        t0 = time.perf_counter()
        k.ABCDE(pr, co, eps, seed=s, return_array=True, **kw)
        seq.append(time.perf_counter() - t0)
    for R in RS:
        k.ABCDE_batch(pr, co, eps, R, seed=1, return_array=True, **kw)  # (warm: allocations, pools)
        ws = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            b = k.ABCDE_batch(pr, co, eps, R, seed=1, return_array=True, **kw)
            ws.append(time.perf_counter() - t0)
        e = {"batch_ms": round(sorted(ws)[len(ws) // 2] * 1e3, 3), "course": b.info["course"],
             "launches": b.info["launches"], "nsims_mean": round(float(np.mean([x.info["nsims"] for x in b])), 1)}
        if R <= len(seq):
            e["seq_ms"] = round(sum(seq[:R]) * 1e3, 3)
        else:
            e["seq_ms_est"] = round(float(np.mean(seq)) * R * 1e3, 3)
        seq_ms = e.get("seq_ms", e.get("seq_ms_est"))
        e["speedup"] = round(seq_ms / e["batch_ms"], 2)
        e["batch_over_one_run"] = round(e["batch_ms"] / out["single"][name]["ms"], 2)
        out["batch"][f"{name}_R{R}"] = e
        print(name, R, json.dumps(e), flush=True)
print(json.dumps(out))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
