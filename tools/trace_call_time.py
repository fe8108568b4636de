"""Host cost of one trace call: a loop of the smallest trace there is, one particle over one step of
model_full_orbit_trace (EB2B on a uniform model), so what is timed is the entry point's checks, the staging of the call's
arrays, one launch and the copies back -- the host path that every single-batch trace shares.  Compares trees: every tree
named is timed in a fresh process, `--runs` times, in alternation, and the runs go to profiles/trace_record_call_time.json.

  python tools/trace_call_time.py --trees parent=/path/to/parent/checkout new=.   (label=path; each tree needs its built
  libxpic_hip.so)
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one(tree, calls):
    sys.path.insert(0, os.path.abspath(tree))
    import numpy as np
    import xpic_amd as X

    ctx = X.Context("basic", (8, 8, 8), (0.5, 0.5, 0.5), 0.7)
    m = X.field_model("uniform", E0=(0.0, 0.01, 0.02), B0=(0.2, 0.3, 1.0))
    p = np.array([[1.0, 1.0, 1.0, 0.1, 0.2, 0.3]])
    best = float("inf")
    for _ in range(3):  # the best of three loops: the first also pays the module load and the first allocations
        t = time.perf_counter()
        for _ in range(calls):
            ctx.model_full_orbit_trace(p, 1, "EB2B", -1.0, 0.05, m)
        best = min(best, (time.perf_counter() - t) / calls)
    print(json.dumps({"us_per_call": best * 1e6}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", nargs="+", default=["this=" + ROOT])
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--one", help="(internal) time this tree in this process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trace_record_call_time.json"))
    args = ap.parse_args()
    if args.one:
        one(args.one, args.calls)
        sys.exit(0)
    trees = dict(t.split("=", 1) for t in args.trees)
    runs = {label: [] for label in trees}
    for _ in range(args.runs):
        for t, path in trees.items():
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", path, "--calls", str(args.calls)],
                                 capture_output=True, text=True, check=True, timeout=120).stdout
            runs[t].append(json.loads(out.strip().splitlines()[-1])["us_per_call"])
    result = {"call": "model_full_orbit_trace, one particle, one step, EB2B, uniform model", "calls_per_run": args.calls,
              "trees": [{"tree": t, "us_per_call": v, "median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)}
                        for t, v in runs.items()]}
    json.dump(result, open(args.out, "w"), indent=1)
    print(json.dumps(result))
