"""Timing of abc_pmc (kabc_abc_pmc): what a generation costs and where the time goes.

Shapes: GaussDist D = 8 under Normal(0, 5)^8 and the README simulator (NormalMeanStdSim(1000)); N in {512, 4096, 65 536};
the adaptive schedule (q = 0.5) over --gens generations.  Per shape and N:
  generation   wall time of a run of G generations minus that of generation 0 alone, over G - 1: host clock around
               calls that end in a device synchronise; median, min, max of --reps repeats
  split        one extra run with KABC_EVAL_TIMING=1: device time of the proposal launches and of the weight kernel
               (event pairs), host time in the rules between them (kabc_pmc_stats), per generation g >= 1
  proposal vs abc_reject
               the proposal launches' device time per row drawn, beside abc_reject's fused kernel on the same number
               of rows from the prior (eps chosen so that it draws them all), ALTERNATING in one process
  weight kernel vs numpy
               kabc_pmc_kernel_sums on the last generation's whitened populations (device time, and the host clock
               around the call with its copies) beside the numpy restatement of tests/abc_pmc_oracle.py, N <= 4096;
               the sums are compared bit for bit first.  Both forms of the launch (KABC_PMC_WEIGHT_SPLIT=0|1).
   python tools/abc_pmc_probe.py [--out profiles/abc_pmc_probe.json] [--reps 5] [--gens 5] [--quick]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kissabc_jl_amd as k  # noqa: E402
from kissabc_jl_amd import _cdefs as cd, _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--gens", type=int, default=5)
ap.add_argument("--quick", action="store_true", help="N <= 4096 only")
args = ap.parse_args()
SEED = 1


def stats(ws):
    ws = sorted(ws)
    return {"median_ms": round(ws[len(ws) // 2] * 1e3, 3), "min_ms": round(ws[0] * 1e3, 3),
            "max_ms": round(ws[-1] * 1e3, 3)}


class env:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        os.environ.update(self.kw)

    def __exit__(self, *a):
        for name in self.kw:
            os.environ.pop(name, None)


def kernel_sums(y_new, y_anc, w_anc):
    """(S, device ms of the weight kernel, wall ms of the call) through kabc_pmc_kernel_sums"""
    lib, ctx = _lib.load(), _lib.default_context()
    S = np.empty(y_new.shape[0])
    dp = lambda a: a.ctypes.data_as(cd.c_double_p)
    with env(KABC_EVAL_TIMING="1"):
        t0 = time.perf_counter()
        _lib.check(lib.kabc_pmc_kernel_sums(ctx.handle, y_new.shape[1], y_new.shape[0], dp(y_new), y_anc.shape[0],
                                            dp(y_anc), dp(w_anc), dp(S)))
        wall = time.perf_counter() - t0
    st = (C.c_double * 4)()
    lib.kabc_pmc_stats(st)
    return S, st[1], wall * 1e3


shapes = {
    "gauss_d8": (k.Factored(*[k.Normal(0, 5)] * 8), k.costs.GaussDist(np.linspace(-1, 1, 8))),
    "readme_sim": (k.Factored(k.Uniform(1, 3), k.Uniform(0, 0.1)), k.costs.NormalMeanStdSim(1000, 2.0, 0.04)),
}
out = {"gens": args.gens, "reps": args.reps, "cases": []}
for shape, (prior, cost) in shapes.items():
    for N in (512, 4096) if args.quick else (512, 4096, 65536):
        G = args.gens
        run = lambda g=G: k.abc_pmc(prior, cost, N, q=0.5, generations=g, seed=SEED)
        r = run()                                         # warm-up
        run(1)
        assert r.info["generations_run"] == G and r.info["course"] == "fused", r.info
        walls, walls0 = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            run(1)
            walls0.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            run()
            walls.append(time.perf_counter() - t0)
        per_gen = [(a - b) / (G - 1) for a, b in zip(walls, walls0)]
        with env(KABC_EVAL_TIMING="1"):
            rt = run()
        draws = sum(rec["draws"] for rec in rt.info["log"][1:])
        entry = {"shape": shape, "N": N, "generations": G, "eps": [rec["eps"] for rec in rt.info["log"]],
                 "draws": [rec["draws"] for rec in rt.info["log"]], "ess": [round(rec["ess"], 1) for rec in rt.info["log"]],
                 "run": stats(walls), "generation_0_alone": stats(walls0), "per_generation": stats(per_gen),
                 "split_per_generation_ms": {
                     "proposal_kernels": round(rt.info["proposal_kernel_ms"] / (G - 1), 4),
                     "weight_kernel": round(rt.info["weight_kernel_ms"] / (G - 1), 4),
                     "host_rules": round(rt.info["host_rules_ms"] / (G - 1), 4),
                     "weight_launches": rt.info["weight_launches"] / (G - 1)}}
        # the proposal launches beside abc_reject's fused kernel on as many rows, alternating
        rows = int(draws / (G - 1))
        pm, rj = [], []
        for _ in range(args.reps):
            with env(KABC_EVAL_TIMING="1"):
                pm.append(run().info["proposal_kernel_ms"] / (G - 1) * 1e-3)
                a = k.abc_reject(prior, cost, -1.0, 1, draws=rows, seed=SEED, return_array=True)   # (accepts nothing)
                assert a.info["draws"] == rows and a.info["course"] == "fused"
                rj.append(a.info["kernel_ms"] * 1e-3)
        entry["proposal_vs_abc_reject"] = {"rows": rows, "abc_pmc_proposal_kernels": stats(pm), "abc_reject_kernel": stats(rj)}
        # the weight kernel beside numpy
        if N <= 4096:
            import abc_pmc_oracle as po
            from oracle import oracle as orc
            orc.load()
            mu, c = po.moments(r.theta, r.w)
            rc, L, W = po.mvn_prepare(orc, po.proposal_cov(c, 2.0, "full"))
            assert rc == 0
            y = po.whiten(r.theta, mu, W)
            w = np.ascontiguousarray(r.w)
            t0 = time.perf_counter()
            want = po.kernel_sums(orc, y, y, w)
            numpy_ms = (time.perf_counter() - t0) * 1e3
            wk = {"numpy_ms": round(numpy_ms, 2)}
            for split in ("0", "1"):
                with env(KABC_PMC_WEIGHT_SPLIT=split):
                    got, _, _ = kernel_sums(y, y, w)
                    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (shape, N, split)
                    dev, wall = [], []
                    for _ in range(args.reps):
                        _, d, wl = kernel_sums(y, y, w)
                        dev.append(d * 1e-3)
                        wall.append(wl * 1e-3)
                wk["split" if split == "1" else "one_launch"] = {"device": stats(dev), "call_with_copies": stats(wall)}
            entry["weight_kernel_vs_numpy"] = wk
        else:
            entry["weight_kernel_vs_numpy"] = "not measured (the numpy restatement holds N x N terms)"
        out["cases"].append(entry)
        print(json.dumps(entry), flush=True)

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
