"""What derived quantities g(θ) on the device cost beside the summary alone.  The legs alternate in one process on
handles of one seed: advance(summary=True) on a summary opened without derived, with a two-output snippet (the
ratio θ₁/θ₂ and the indicator θ₁ > θ₂), and with the identity at G = D -- by arithmetic one more fold plus the
trace read once and written once.  Further legs run the identity through each memory-access form of the map
kernel (KABC_DERIVED_PATH=direct / lds: one thread per row on the global rows, or rows staged through LDS).  Per
leg the median, minimum and maximum microseconds per generation over the rounds, and its own spread
(max - min over the median): two medians nearer than that do not differ.  Shapes: C3 (65 536 walkers x 8
parameters) at ntransitions 1, 16 and 100, and the 4096 fits of the README problem (AIS(10), ntransitions = 100)
as the chains of one handle (its D = 2: the identity is G = 2 there).

    python tools/ais_derived_probe.py [--out profiles/ais_derived_probe.json] [--rounds 7] [--shapes c3_nt1,...]

The cost is reported, not gated.  `--legs none,summary` times the two untouched paths only (advance() without
a trace, and the summary alone): run in fresh processes alternately on two builds of the library, it says
whether they moved between them (`--label` names the build in the output)."""
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

HEAD = "KABC_HD void kabc_user_derived(const double* x, int D, const double* params, int nparams, double* g, int G) {\n"
RATIO_SRC = HEAD + "    g[0] = x[0] / x[1];\n    g[1] = x[0] > x[1] ? 1.0 : 0.0;\n}\n"
IDENTITY_SRC = HEAD + "    for (int j = 0; j < G; ++j) g[j] = x[j];\n}\n"
# leg -> (snippet or None, G or None: D, KABC_DERIVED_PATH or None: the library's default)
LEGS = {"none": None, "summary": (None, 0, None), "ratio_indicator": (RATIO_SRC, 2, None),
        "identity": (IDENTITY_SRC, None, None), "identity_direct": (IDENTITY_SRC, None, "direct"),
        "identity_lds": (IDENTITY_SRC, None, "lds")}


def _advance(e, leg, gens, nt):
    if leg == "none":
        e.advance(gens, nt)
        return
    path = LEGS[leg][2]
    if path is None:
        os.environ.pop("KABC_DERIVED_PATH", None)
    else:
        os.environ["KABC_DERIVED_PATH"] = path
    e.advance(gens, nt, summary=True)


def probe(name, rounds, legs):
    make, gens, nt = SHAPES[name]
    sh = make()
    ctx = _lib.default_context()
    ens = {leg: AisEnsemble(sh["model"], sh["N"], **sh["kw"]).init() for leg in legs}
    e0 = ens[legs[0]]
    for leg in legs:
        if leg == "none":
            continue
        src, G, _ = LEGS[leg]
        ens[leg].summary_begin(**({} if src is None else {"derived": k.Derived(src, G or e0.D)}))
    for leg in legs:                                       # warm-up: allocations, compilations, first launches
        _advance(ens[leg], leg, gens, nt)
    ctx.synchronize()
    us = {leg: [] for leg in legs}
    for _ in range(rounds):
        for leg in legs:
            t0 = time.perf_counter()
            _advance(ens[leg], leg, gens, nt)
            ctx.synchronize()
            us[leg].append((time.perf_counter() - t0) / gens * 1e6)
    os.environ.pop("KABC_DERIVED_PATH", None)
    res = {}
    for leg in legs:
        if leg == "none":
            continue
        s = res[leg] = ens[leg].summary()
        assert s.n == (rounds + 1) * gens * e0.N
        # the handles walked the same chain
        assert np.array_equal(s.mean, res[[x for x in legs if x != "none"][0]].mean)
        if leg.startswith("identity"):                       # the derived set IS the parameters' set
            assert np.array_equal(s.derived.mean, s.mean) and np.array_equal(s.derived.cov, s.cov)
            assert np.array_equal(s.derived.min, s.min) and np.array_equal(s.derived.max, s.max)
    out = {"N": e0.N, "D": e0.D, "chains": e0.nchains, "ntransitions": nt, "generations_per_call": gens,
           "rounds": rounds, "driver": e0.driver, "us_per_generation": {}, "spread": {}}
    if "ratio_indicator" in res:
        out["P_theta1_gt_theta2"] = float(np.atleast_2d(res["ratio_indicator"].derived.mean)[:, 1].mean())
    for e in ens.values():
        e.close()
    for leg in legs:
        v = us[leg]
        med = statistics.median(v)
        out["us_per_generation"][leg] = {"median": med, "min": min(v), "max": max(v)}
        out["spread"][leg] = (max(v) - min(v)) / med
    if "summary" in legs:
        out["extra_us_per_generation"] = {
            leg: out["us_per_generation"][leg]["median"] - out["us_per_generation"]["summary"]["median"]
            for leg in legs if leg not in ("none", "summary")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--legs", default="summary,ratio_indicator,identity,identity_direct,identity_lds")
    ap.add_argument("--label", default=None)
    a = ap.parse_args()
    legs = tuple(a.legs.split(","))
    assert all(leg in LEGS for leg in legs), legs
    res = {}
    for name in a.shapes.split(","):
        res[name] = probe(name, min(a.rounds, 3) if name.startswith("readme") else a.rounds, legs)
        if a.label:
            res[name]["build"] = a.label
        print(name, json.dumps(res[name]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
