"""What a posterior summary on the device costs beside the trace it replaces.  Three legs alternate in one
process on handles of one seed: advance() without a trace, advance(out=<page-locked buffer>) (the two paths
that exist without the summary: the yardstick), advance(summary=True).  Per leg the median, minimum and
maximum microseconds per generation over the rounds; the spread of the no-trace leg says how far two medians
must lie apart to differ.  Shapes: C3 (65 536 walkers x 8 parameters) at ntransitions 1, 16 and 100, and the
4096 fits of the README problem (AIS(10), 1000 samples, ntransitions = 100) as the chains of one handle.

    python tools/ais_summary_probe.py [--out profiles/ais_summary_probe.json] [--rounds 7] [--shapes c3_nt1,...]

The claim under test: the summary leg lies nearer the no-trace leg than the trace leg does, at ntransitions
1 and 16 (`summary_nearer_than_trace`)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kissabc_jl_amd as k  # noqa: E402
from kissabc_jl_amd import _lib  # noqa: E402
from kissabc_jl_amd.api import AisEnsemble, chain_seeds  # noqa: E402


def c3():
    model = k.ApproxKernelizedPosterior(k.Factored(*[k.Uniform(-5, 5)] * 8), k.costs.Rosenbrock(), 1.0)
    return dict(model=model, N=65536, kw=dict(seed=1))


def readme_batch(runs=4096):
    prior = k.Factored(k.Uniform(1, 3), k.Truncated(k.Normal(0, 0.1), 0, 100))
    rng = np.random.default_rng(7)
    costs = []
    for _ in range(runs):
        t = rng.normal(2.0, 0.05, 1000)
        costs.append(k.costs.NormalMeanStdSim(1000, t.mean(), t.std(ddof=1)))
    model = k.ApproxKernelizedPosterior(prior, costs[0], 0.005)
    return dict(model=model, N=10, kw=dict(seeds=chain_seeds(0, runs), costs=costs))


SHAPES = {
    "c3_nt1": (c3, 64, 1), "c3_nt16": (c3, 64, 16), "c3_nt100": (c3, 64, 100),
    "readme_4096_runs": (readme_batch, 100, 100),
}


def probe(name, rounds):
    make, gens, nt = SHAPES[name]
    sh = make()
    ctx = _lib.default_context()
    legs = ("none", "trace", "summary")
    ens = {leg: AisEnsemble(sh["model"], sh["N"], **sh["kw"]).init() for leg in legs}
    e0 = ens["none"]
    lead = (e0.nchains,) if e0.batched else ()
    buf = _lib.pinned_empty((gens,) + lead + (e0.N, e0.D))
    ens["summary"].summary_begin()

    def run(leg):
        if leg == "none":
            ens[leg].advance(gens, nt)
        elif leg == "trace":
            ens[leg].advance(gens, nt, out=buf)
        else:
            ens[leg].advance(gens, nt, summary=True)

    for leg in legs:                                       # warm-up: allocations, first launches
        run(leg)
    ctx.synchronize()
    us = {leg: [] for leg in legs}
    for _ in range(rounds):
        for leg in legs:
            t0 = time.perf_counter()
            run(leg)
            ctx.synchronize()
            us[leg].append((time.perf_counter() - t0) / gens * 1e6)
    t0 = time.perf_counter()
    s = ens["summary"].summary()
    get_ms = (time.perf_counter() - t0) * 1e3
    # the three handles walked the same chain: the trace's last generation is everybody's state
    x = ens["none"].state()[0]
    assert np.array_equal(buf[-1], x) and np.array_equal(ens["summary"].state()[0], x)
    assert s.n == (rounds + 1) * gens * e0.N
    driver = e0.driver
    for e in ens.values():
        e.close()
    out = {"N": e0.N, "D": e0.D, "chains": e0.nchains, "ntransitions": nt, "generations_per_call": gens,
           "rounds": rounds, "driver": driver, "trace_MiB_per_call": buf.nbytes / 2 ** 20,
           "summary_get_ms": get_ms, "us_per_generation": {}}
    for leg in legs:
        v = us[leg]
        out["us_per_generation"][leg] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    med = {leg: out["us_per_generation"][leg]["median"] for leg in legs}
    out["no_trace_spread"] = (max(us["none"]) - min(us["none"])) / med["none"]
    out["summary_over_none"] = med["summary"] / med["none"]
    out["trace_over_none"] = med["trace"] / med["none"]
    out["summary_nearer_than_trace"] = abs(med["summary"] - med["none"]) < abs(med["trace"] - med["none"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    a = ap.parse_args()
    res = {}
    for name in a.shapes.split(","):
        res[name] = probe(name, a.rounds if not name.startswith("readme") else min(a.rounds, 3))
        print(name, json.dumps(res[name]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
