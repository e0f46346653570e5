"""Wall time of sample_batch (one AIS handle with a cost per run: kabc_ais_create_batch_costs) against the
same R runs as sample() calls one after another, R in {1, 64, 256, 1024, 4096}, on three problems:
  readme  the reference's README model (AIS(10), 1000 samples, ntransitions = 100, NormalMeanStdSim with
          1000 draws) with a per-run observed mean / std;
  gauss   AIS(12), D = 2, 1200 samples after 1200 discarded, per-run GaussDist centres;
  halves  AIS(4096), D = 8, 4096 samples after 16 384 discarded, ntransitions = 2, per-run GaussDist
          centres (the launch per half-generation).
   python tools/ais_batch_probe.py [--out profiles/<name>.json] [--rs 1,64,256] [--problems readme,gauss]
The sequential time is measured for the first `--seq` runs (every run once) and extrapolated from their
mean above that ("seq_ms_est")."""
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
ap.add_argument("--problems", default="readme,gauss,halves")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--seq", type=int, default=64)
args = ap.parse_args()
RS = [int(x) for x in args.rs.split(",")]


def readme(r):
    rng = np.random.default_rng(r)
    t = rng.normal(2.0 + 0.1 * rng.random(), 0.04, 1000)
    prior = k.Factored(k.Uniform(1, 3), k.Truncated(k.Normal(0, 0.1), 0, 100))
    return k.ApproxKernelizedPosterior(prior, k.costs.NormalMeanStdSim(1000, t.mean(), t.std(ddof=1)), 0.005)


def gauss(D):
    def make(r):
        c = np.random.default_rng(r).uniform(-1, 1, D)
        return k.ApproxKernelizedPosterior(k.Factored(*[k.Normal(0, 5)] * D), k.costs.GaussDist(c), 0.1)
    return make


problems = {
    "readme": (readme, 10, 1000, dict(ntransitions=100)),
    "gauss": (gauss(2), 12, 1200, dict(ntransitions=1, discard_initial=1200)),
    "halves": (gauss(8), 4096, 4096, dict(ntransitions=2, discard_initial=4 * 4096)),
}
out = {"problems": {}, "batch": {}}
seeds_all = k.api.chain_seeds(1, max(RS))
for name in args.problems.split(","):
    make, N, Ns, kw = problems[name]
    out["problems"][name] = {"N": N, "Ns": Ns, **kw}
    models_all = [make(r) for r in range(max(RS))]
    k.sample(models_all[0], k.AIS(N), Ns, seed=1, return_array=True, **kw)   # (warm)
    seq = []   # the sequential course: the first --seq runs once each
    for r in range(min(args.seq, max(RS))):
        t0 = time.perf_counter()
        k.sample(models_all[r], k.AIS(N), Ns, seed=seeds_all[r], return_array=True, **kw)
        seq.append(time.perf_counter() - t0)
    out["problems"][name]["sample_ms_mean"] = round(float(np.mean(seq)) * 1e3, 3)
    for R in RS:
        models = models_all[:R]
        k.sample_batch(models, k.AIS(N), Ns, seeds=seeds_all[:R], return_array=True, **kw)   # (warm)
        ws = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            b = k.sample_batch(models, k.AIS(N), Ns, seeds=seeds_all[:R], return_array=True, **kw)
            ws.append(time.perf_counter() - t0)
            info = b.info
            del b   # (the next call's trace buffers may be large: release this one first)
        e = {"batch_ms": round(sorted(ws)[len(ws) // 2] * 1e3, 3), "course": info["course"],
             "driver": info["driver"]}
        if R <= len(seq):
            e["seq_ms"] = round(sum(seq[:R]) * 1e3, 3)
        else:
            e["seq_ms_est"] = round(float(np.mean(seq)) * R * 1e3, 3)
        seq_ms = e.get("seq_ms", e.get("seq_ms_est"))
        e["speedup"] = round(seq_ms / e["batch_ms"], 2)
        out["batch"][f"{name}_R{R}"] = e
        print(name, R, json.dumps(e), flush=True)
print(json.dumps(out))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
