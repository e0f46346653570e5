"""Does a call that is never cancelled pay for the stop? kabc_abcde_run's one-workgroup kernel at the head of every
generation reads the context's cancel word (host memory) and pf_small_kernel looks at it at every iteration
boundary; the host enqueues ABCDE generations in blocks.  This probe times ABCDE() and pfilter() on the library
of the commit before (built apart, `--parent-lib`) and on the current one, in fresh child processes that ALTERNATE
between the two (KABC_LIB), so that drift of the box hits both alike:
    ABCDE    50 x 20 generations, 2000 x 50, 16 384 x 50   (Normal^2 + gauss_dist)
    pfilter  N = 100 (one-workgroup kernel), N = 16 384     (the same problem, epstol = 0.05)
   python tools/stop_continue_probe.py --parent-lib <libkabc_hip.so of the parent> [--rounds 5]
                                       [--out profiles/stop_continue_probe.json]
Every child reports the median wall time of 15 calls per case.  Per case: the medians of the parent's children,
their spread (max - min: the parent's own run-to-run spread), the medians of the new library's children; the new
library passes where the median of its medians exceeds the parent's by no more than that spread."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("abcde_50x20", "abcde_2000x50", "abcde_16384x50", "pfilter_100", "pfilter_16384")


def child():
    sys.path.insert(0, ROOT)
    from kissabc_jl_amd import _cdefs
    # (the parent's library lacks the entry points added since: they are not bound, and not called here)
    raw = C.CDLL(os.environ["KABC_LIB"])
    for name in [n for n in _cdefs.PROTOTYPES if not hasattr(raw, n)]:
        del _cdefs.PROTOTYPES[name]
    import kissabc_jl_amd as k
    N2 = k.Factored(k.Normal(0, 5), k.Normal(0, 5))
    cost = k.costs.GaussDist([1.0, -0.5])
    calls = {
        "abcde_50x20": lambda: k.ABCDE(N2, cost, 0.01, nparticles=50, generations=20, seed=3, return_array=True),
        "abcde_2000x50": lambda: k.ABCDE(N2, cost, 0.01, nparticles=2000, generations=50, seed=3, return_array=True),
        "abcde_16384x50": lambda: k.ABCDE(N2, cost, 0.01, nparticles=16384, generations=50, seed=3, return_array=True),
        "pfilter_100": lambda: k.pfilter(N2, cost, 100, epstol=0.05, seed=4, return_array=True),
        "pfilter_16384": lambda: k.pfilter(N2, cost, 16384, epstol=0.05, seed=4, return_array=True),
    }
    out = {}
    for name in CASES:
        for _ in range(3):
            calls[name]()
        ws = []
        for _ in range(15):
            t0 = time.perf_counter()
            calls[name]()
            ws.append(time.perf_counter() - t0)
        out[name] = round(statistics.median(ws) * 1e3, 4)
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--new-lib", default=os.path.join(ROOT, "kissabc.jl_amd", "lib", "libkabc_hip.so"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    libs = {"parent": os.path.abspath(args.parent_lib), "new": os.path.abspath(args.new_lib)}
    runs = {"parent": [], "new": []}
    for r in range(args.rounds):
        for which in ("parent", "new"):
            env = dict(os.environ, KABC_LIB=libs[which], KABC_SPECIALIZE="0", KABC_NO_TORCH_PRELOAD="1")
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True,
                               text=True, timeout=300)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.exit(f"child on the {which} library failed ({p.returncode}):\n{p.stdout}\n{p.stderr}")
            runs[which].append(json.loads(line[0][7:]))
            print(r, which, line[0][7:], flush=True)
    out = {"rounds": args.rounds, "calls_per_child": 15, "unit": "ms per call (median)", "cases": {}}
    for name in CASES:
        par = [x[name] for x in runs["parent"]]
        new = [x[name] for x in runs["new"]]
        spread = max(par) - min(par)
        e = {"parent_medians": par, "new_medians": new, "parent_ms": round(statistics.median(par), 4),
             "parent_spread_ms": round(spread, 4), "new_ms": round(statistics.median(new), 4)}
        e["new_minus_parent_ms"] = round(e["new_ms"] - e["parent_ms"], 4)
        e["within_parent_spread"] = e["new_minus_parent_ms"] <= e["parent_spread_ms"]
        out["cases"][name] = e
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    child() if "--child" in sys.argv[1:] else main()
