"""What the autocorrelation of a device summary costs beside the summary alone.  Two legs alternate in one
process on handles of one seed: advance(summary=True) on a summary opened without autocorr, and on one opened
with autocorr=64.  Per leg the median, minimum and maximum microseconds per generation over the rounds; the
spread of the summary leg says how far two medians must lie apart to differ.  Shapes: C3 (65 536 walkers x 8
parameters) at ntransitions 1, 16 and 100, and the 4096 fits of the README problem (AIS(10), 1000 samples,
ntransitions = 100) as the chains of one handle.

    python tools/ais_autocorr_probe.py [--out profiles/ais_autocorr_probe.json] [--rounds 7] [--shapes c3_nt1,...]
                                       [--maxlag 64]

The cost is reported, not gated.  `--legs summary` times the summary-alone leg only: run in fresh processes
alternately on two builds of the library (KABC_LIB), it says whether that leg moved between them."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kissabc_jl_amd as k  # noqa: E402,F401
from kissabc_jl_amd import _lib  # noqa: E402
from kissabc_jl_amd.api import AisEnsemble  # noqa: E402
from ais_summary_probe import SHAPES  # noqa: E402


def probe(name, rounds, maxlag, legs):
    make, gens, nt = SHAPES[name]
    sh = make()
    ctx = _lib.default_context()
    ens = {leg: AisEnsemble(sh["model"], sh["N"], **sh["kw"]).init() for leg in legs}
    e0 = ens[legs[0]]
    for leg in legs:
        ens[leg].summary_begin(autocorr=maxlag if leg == "autocorr" else None)
    for leg in legs:                                       # warm-up: allocations, first launches
        ens[leg].advance(gens, nt, summary=True)
    ctx.synchronize()
    us = {leg: [] for leg in legs}
    for _ in range(rounds):
        for leg in legs:
            t0 = time.perf_counter()
            ens[leg].advance(gens, nt, summary=True)
            ctx.synchronize()
            us[leg].append((time.perf_counter() - t0) / gens * 1e6)
    get_ms = {}
    res = {}
    for leg in legs:
        t0 = time.perf_counter()
        res[leg] = ens[leg].summary()
        get_ms[leg] = (time.perf_counter() - t0) * 1e3
        assert res[leg].n == (rounds + 1) * gens * e0.N
    if len(legs) == 2:                                     # the two handles walked the same chain
        assert np.array_equal(ens["summary"].state()[0], ens["autocorr"].state()[0])
        assert np.array_equal(res["summary"].mean, res["autocorr"].mean)
        assert np.array_equal(res["summary"].cov, res["autocorr"].cov)
    out = {"N": e0.N, "D": e0.D, "chains": e0.nchains, "ntransitions": nt, "generations_per_call": gens,
           "rounds": rounds, "driver": e0.driver, "maxlag": maxlag, "summary_get_ms": get_ms,
           "accumulators_MiB": 3 * maxlag * e0.N * e0.D * e0.nchains * 8 / 2 ** 20, "us_per_generation": {}}
    for e in ens.values():
        e.close()
    for leg in legs:
        v = us[leg]
        out["us_per_generation"][leg] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    med = {leg: out["us_per_generation"][leg]["median"] for leg in legs}
    out["summary_spread"] = (max(us["summary"]) - min(us["summary"])) / med["summary"]
    if "autocorr" in legs:
        out["autocorr_over_summary"] = med["autocorr"] / med["summary"]
        out["autocorr_extra_us_per_generation"] = med["autocorr"] - med["summary"]
        tau = np.asarray(res["autocorr"].tau)
        out["tau_range"] = [float(np.nanmin(tau)), float(np.nanmax(tau))]
        out["tau_converged"] = float(np.mean(res["autocorr"].tau_converged))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--maxlag", type=int, default=64)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--legs", default="summary,autocorr")
    a = ap.parse_args()
    legs = tuple(a.legs.split(","))
    assert legs in (("summary", "autocorr"), ("summary",)), legs
    res = {}
    for name in a.shapes.split(","):
        res[name] = probe(name, a.rounds if not name.startswith("readme") else min(a.rounds, 3), a.maxlag, legs)
        print(name, json.dumps(res[name]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
