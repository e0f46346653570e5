"""The one-workgroup AIS driver beyond KABC_MAX_DIM parameters (csrc/ais_dyn_small_kernel.hpp) against the
launch per half-generation (KABC_AIS_SMALL=0, the path every such call took before), two legs alternated in
one process:
  (a) one sample() call: AIS(100) / 11 000 steps at D = 20 and D = 40, AIS(50) / 50 100 steps at D = 20,
      AIS(140) / 2800 steps at D = 128 (steps = discarded + kept samples, ntransitions = 1);
  (b) Nc chains of AIS(60) at D = 20 (660 steps each) in ONE handle -- sample(model, AIS(60), MCMCThreads(),
      60, Nc) -- against Nc sample() calls with KABC_AIS_SMALL=0, Nc in {4, 64, 1024}; the sequential leg
      runs at most --seq calls per repetition and is extrapolated from their mean above that ("seq_ms_est").
   python tools/ais_dyn_small_probe.py [--out profiles/ais_dyn_small_probe.json] [--reps 9]
Wall milliseconds per call (host side, handle creation and init included), median and minimum per leg.
The rule the default follows: the new driver serves a (D, N) region where its MEDIAN is below the MINIMUM of
the other leg ("wins")."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kissabc_jl_amd as k  # noqa: E402
from kissabc_jl_amd.api import chain_seeds  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--ncs", default="4,64,1024")
ap.add_argument("--seq", type=int, default=64)
args = ap.parse_args()


def gauss(D, eps=1.0):
    c = np.random.default_rng(D).uniform(-1, 1, D)
    return k.ApproxKernelizedPosterior(k.Factored(*[k.Normal(0, 3)] * D), k.costs.GaussDist(c), eps)


def leg(small, fn):
    """fn() with the driver chosen: returns (milliseconds, the driver the handles report)"""
    if small:
        os.environ["KABC_AIS_SMALL"] = "1"   # (also where a single chain does not take the driver by default)
    else:
        os.environ["KABC_AIS_SMALL"] = "0"
    try:
        t0 = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t0) * 1e3, r
    finally:
        os.environ.pop("KABC_AIS_SMALL", None)


def summary(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "n": len(ms)}


out = {"one_call": [], "chains": []}
for D, N, steps in ((20, 100, 11000), (40, 100, 11000), (20, 50, 50100), (128, 140, 2800)):
    model = gauss(D, 12.0 if D > 100 else 1.0)
    run = lambda: k.sample(model, k.AIS(N), N, discard_initial=steps - N, seed=3, return_array=True)  # noqa: E731
    drivers = []
    for small in (True, False):
        os.environ["KABC_AIS_SMALL"] = "1" if small else "0"
        e = k.AisEnsemble(model, N, seed=3)
        drivers.append(e.driver)
        e.close()
    os.environ.pop("KABC_AIS_SMALL", None)
    ref = [leg(s, run)[1] for s in (True, False)]   # (warm; the two drivers give the same bits)
    assert np.array_equal(ref[0], ref[1])
    ms = {True: [], False: []}
    for _ in range(args.reps):
        for small in (True, False):
            ms[small].append(leg(small, run)[0])
    a, b = summary(ms[True]), summary(ms[False])
    gens = -(-(steps - N) // N) + 1
    row = {"D": D, "N": N, "steps": steps, "drivers": drivers, "small": a, "halves": b,
           "small_us_per_generation": a["median_ms"] * 1e3 / gens,   # (against the cancel model's estimate)
           "wins": a["median_ms"] < b["min_ms"]}
    out["one_call"].append(row)
    print(json.dumps(row), flush=True)

D, N, Ns, disc = 20, 60, 60, 600
model = gauss(D)
for Nc in [int(x) for x in args.ncs.split(",")]:
    seeds = chain_seeds(7, Nc)
    nseq = min(Nc, args.seq)
    grid = lambda: k.sample(model, k.AIS(N), k.MCMCThreads(), Ns, Nc, seed=7, discard_initial=disc,  # noqa: E731
                            return_array=True)
    seq = lambda: np.concatenate([k.sample(model, k.AIS(N), Ns, seed=s, discard_initial=disc,  # noqa: E731
                                           return_array=True) for s in seeds[:nseq]])
    g0, s0 = leg(True, grid)[1], leg(False, seq)[1]
    assert np.array_equal(g0[:nseq * Ns], s0)
    reps = max(3, args.reps // 3)
    mg, msq = [], []
    for _ in range(reps):
        mg.append(leg(True, grid)[0])
        msq.append(leg(False, seq)[0] * (Nc / nseq))
    a, b = summary(mg), summary(msq)
    row = {"D": D, "N": N, "steps": disc + Ns, "Nc": Nc, "grid": a, "seq_ms_est": b, "seq_calls_timed": nseq,
           "wins": a["median_ms"] < b["min_ms"]}
    out["chains"].append(row)
    print(json.dumps(row), flush=True)

if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
