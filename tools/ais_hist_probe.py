"""What the marginal histograms of a device summary cost beside the summary alone.  The legs alternate in one
process on handles of one seed: advance(summary=True) on a summary opened without hist, with hist=128 over the
automatic range, with 128 bins over a range so wide that every sample shares one bin (the worst case for the
atomics), and with hist=1024.  Per leg the median, minimum and maximum microseconds per generation over the
rounds, and its own spread (max - min over the median): two medians nearer than that do not differ.  Shapes:
C3 (65 536 walkers x 8 parameters) at ntransitions 1, 16 and 100, and the 4096 fits of the README problem
(AIS(10), ntransitions = 100) as the chains of one handle -- there the shape rule picks the direct kernel, and
a further leg forces the LDS kernel (KABC_HIST_PATH) to show what the rule avoids.

    python tools/ais_hist_probe.py [--out profiles/ais_hist_probe.json] [--rounds 7] [--shapes c3_nt1,...]

The cost is reported, not gated; the comparison is against the summary-alone leg of the same run."""
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

ONE_BIN = (-100.0, 1e4, 128)        # bin 1 = [-21.1, 57.8) holds every sample of both problems
# leg -> (hist, KABC_HIST_PATH or None: the shape rule)
LEGS = {"summary": (None, None), "hist128": (128, None), "hist128_one_bin": (ONE_BIN, None), "hist1024": (1024, None),
        "hist128_lds": (128, "lds"), "hist128_direct": (128, "direct")}


def _advance(e, path, gens, nt):
    if path is None:
        os.environ.pop("KABC_HIST_PATH", None)
    else:
        os.environ["KABC_HIST_PATH"] = path
    e.advance(gens, nt, summary=True)


def probe(name, rounds, legs):
    make, gens, nt = SHAPES[name]
    sh = make()
    ctx = _lib.default_context()
    ens = {leg: AisEnsemble(sh["model"], sh["N"], **sh["kw"]).init() for leg in legs}
    e0 = ens["summary"]
    for leg in legs:
        ens[leg].summary_begin(hist=LEGS[leg][0])
    for leg in legs:                                       # warm-up: allocations, first launches
        _advance(ens[leg], LEGS[leg][1], gens, nt)
    ctx.synchronize()
    us = {leg: [] for leg in legs}
    for _ in range(rounds):
        for leg in legs:
            t0 = time.perf_counter()
            _advance(ens[leg], LEGS[leg][1], gens, nt)
            ctx.synchronize()
            us[leg].append((time.perf_counter() - t0) / gens * 1e6)
    os.environ.pop("KABC_HIST_PATH", None)
    res, get_ms = {}, {}
    for leg in legs:
        t0 = time.perf_counter()
        res[leg] = ens[leg].summary()
        get_ms[leg] = (time.perf_counter() - t0) * 1e3
        s = res[leg]
        assert s.n == (rounds + 1) * gens * e0.N
        # the handles walked the same chain; every sample was counted once
        assert np.array_equal(s.mean, res["summary"].mean) and np.array_equal(s.cov, res["summary"].cov)
        if leg != "summary":
            assert np.all(s.hist.sum(axis=-1) + s.underflow + s.overflow == s.n)
    if "hist128_one_bin" in legs:
        assert np.all(res["hist128_one_bin"].hist[..., 1] == e0.N * (rounds + 1) * gens)
    for a, b in (("hist128", "hist128_lds"), ("hist128", "hist128_direct")):
        if a in legs and b in legs:
            assert np.array_equal(res[a].hist, res[b].hist)
    out = {"N": e0.N, "D": e0.D, "chains": e0.nchains, "ntransitions": nt, "generations_per_call": gens,
           "rounds": rounds, "driver": e0.driver, "summary_get_ms": get_ms, "us_per_generation": {},
           "spread": {}, "extra_us_per_generation": {}}
    if "hist128" in legs:
        h = res["hist128"]
        out["hist128_bins_in_use_per_parameter"] = float(np.mean(np.count_nonzero(h.hist, axis=-1)))
        out["hist128_missed_fraction"] = float(np.max((h.underflow + h.overflow) / h.n))
    for e in ens.values():
        e.close()
    for leg in legs:
        v = us[leg]
        med = statistics.median(v)
        out["us_per_generation"][leg] = {"median": med, "min": min(v), "max": max(v)}
        out["spread"][leg] = (max(v) - min(v)) / med
    for leg in legs:
        if leg != "summary":
            out["extra_us_per_generation"][leg] = (out["us_per_generation"][leg]["median"]
                                                   - out["us_per_generation"]["summary"]["median"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    a = ap.parse_args()
    res = {}
    for name in a.shapes.split(","):
        batch = name.startswith("readme")
        legs = (("summary", "hist128", "hist128_lds", "hist1024") if batch
                else ("summary", "hist128", "hist128_one_bin", "hist1024", "hist128_direct"))
        res[name] = probe(name, min(a.rounds, 3) if batch else a.rounds, legs)
        print(name, json.dumps(res[name]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
