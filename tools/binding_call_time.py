"""Per-call cost of the Python binding, without a GPU: a loop of the cheapest call there is, Context.count(0) on a context
that was never created, which the library refuses at its first line (null context) -- so what is timed is the ctypes call,
the wrapper around it and the raise.  Compares trees: every tree named is timed in a fresh process, `--runs` times, in
alternation, and the runs go to profiles/binding_call_time.json.

  python tools/binding_call_time.py --trees parent=/path/to/parent/checkout new=.   (label=path; each tree needs its built
  libxpic_hip.so)
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one(tree, calls):
    sys.path.insert(0, os.path.abspath(tree))
    import xpic_amd as X

    ctx = object.__new__(X.Context)
    ctx.L, ctx.h = X.load_library(), ctypes.c_void_p(0)
    best = float("inf")
    for _ in range(3):  # the best of three loops: the first also pays the imports' tail
        t = time.perf_counter()
        for _ in range(calls):
            try:
                ctx.count(0)
            except X.XpicError:
                pass
        best = min(best, (time.perf_counter() - t) / calls)
    print(json.dumps({"us_per_call": best * 1e6}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", nargs="+", default=["this=" + ROOT])
    ap.add_argument("--calls", type=int, default=100000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--one", help="(internal) time this tree in this process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "binding_call_time.json"))
    args = ap.parse_args()
    if args.one:
        one(args.one, args.calls)
        sys.exit(0)
    trees = dict(t.split("=", 1) for t in args.trees)
    runs = {label: [] for label in trees}
    for _ in range(args.runs):
        for t, path in trees.items():
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", path, "--calls", str(args.calls)],
                                 capture_output=True, text=True, check=True).stdout
            runs[t].append(json.loads(out.strip().splitlines()[-1])["us_per_call"])
    result = {"call": "Context.count(0) on a null handle, refused by the library", "calls_per_run": args.calls,
              "trees": [{"tree": t, "us_per_call": v, "mean": sum(v) / len(v), "min": min(v), "max": max(v)}
                        for t, v in runs.items()]}
    json.dump(result, open(args.out, "w"), indent=1)
    print(json.dumps(result))
