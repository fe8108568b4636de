#!/usr/bin/env python3
"""Times the binary collisions (xpic_collide, xpic_amd/csrc/collide.hip): an intra-species call on one sort and an
inter-species call on two sorts of equal weight, ECSIM, n^3 x ppc per cell from load_synthetic, on a uniform ("poisson")
load and on the "blob" load (a quarter of the records in a Gaussian of n / 16 cells: cells far above the LDS path's limit).

Device time from the context's profile section "cmd_collide" (the whole call: the kernel, the reduction of its counters
and their host round trip).  Beside each time: the call's own traffic, one read and one write of the velocities of the
records it touches (48 B per record), at the measured device copy rate; the same state's ecsim second push ("second_push",
which streams the same records); the share of the cells that took the second path (more than XPIC_COLLIDE_LDS_CELL
records of a sort), from Context.collide_info, and the sort's occupancy.
--sorts 1 loads one sort only and times the intra-species call alone (256^3 x 64: two sorts of that size do not fit beside
the step's buffers).  Prints one JSON object; with --out it is also written to that file.  profiles/collide_time.json is
the list of such objects: --n 128, and --n 256 --sorts 1.
--weighted R times the inter-species call of xpic_collide_weighted ("cmd_collide_weighted") on two sorts whose weights
are in the ratio R (the second sort's density is R, at the same ppc); at R = 1 the same state also goes through
xpic_collide ("inter"), the call the weighted one is held against.  profiles/collide_weighted_time.json is the list of
these objects for R = 1, 0.5 and 0.125.
usage: collide_time.py [--n 128] [--ppc 64] [--reps 3] [--sorts 2] [--weighted R] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import xpic_amd as X  # noqa: E402


def run(n, ppc, reps, vth, profile, strength, sorts, weighted=None):
    d = 0.5
    ctx = X.Context("ecsim", (n, n, n), (d,) * 3, 1.0, device=0)
    cap = int(ppc * ctx.N * 1.02) + 1024
    a = ctx.add_sort(ppc, 1.0, -1.0, 1.0, capacity=cap)
    b = ctx.add_sort(ppc, 1.0 if weighted is None else weighted, 1.0, 100.0, capacity=cap if sorts == 2 else 64)
    param = (0.25, n / 16.0) if profile == "blob" else (0.0, 0.0)
    ctx.load_synthetic(a, ppc, vth, seed=1234, profile=profile, param=param)
    if sorts == 2:
        ctx.load_synthetic(b, ppc, vth / 10.0, seed=4321, profile=profile, param=param)
    B = np.zeros(ctx.fshape())
    B[..., 2] = 0.2
    ctx.set_field(X.B, B)
    ctx.set_field(X.B0, B)
    del B
    ctx.step()  # (the records in the step's own order, as tools/commands_time.py)
    bw = ctx.probe_copy_bandwidth(1 << 30, 10)
    res = {"load": profile, "records": [ctx.count(a), ctx.count(b)], "copy_GBps": bw / 1e9,
           "occupancy": ctx.occupancy(a)}
    step = [0]

    def timed(section, call, records):
        call()
        ctx.synchronize()
        ctx.profile_enable(True)
        ctx.profile_reset()
        out = None
        for _ in range(reps):
            out = call()
        ctx.synchronize()
        launches, ms = ctx.profile_get(section)
        large = ctx.collide_info()["large_cells"]  # (of the last call)
        ctx.profile_enable(False)
        per = ms / max(launches, 1)
        floor = 48 * records / bw * 1e3  # the velocities, read once and written once
        return {"ms": per, "calls": launches, "velocity_rw_ms": floor, "x_velocity_rw": per / floor,
                "large_cells_per_call": large, "large_cell_share": large / ctx.N}, out

    def collide(sa, sb):
        step[0] += 1
        return ctx.collide(sa, sb, strength, step[0], seed=7)

    def collide_weighted(sa, sb):
        step[0] += 1
        return ctx.collide_weighted(sa, sb, strength, step[0], seed=7)

    if weighted is not None:
        res["weight_ratio"] = weighted
        res["inter_weighted"], out = timed("cmd_collide_weighted", lambda: collide_weighted(a, b), ctx.count(a) + ctx.count(b))
        res["inter_weighted"].update(out)
    else:
        res["intra"], out = timed("cmd_collide", lambda: collide(a, a), ctx.count(a))
        res["intra"].update(out)
    if sorts == 2 and (weighted is None or weighted == 1.0):
        res["inter"], out = timed("cmd_collide", lambda: collide(a, b), ctx.count(a) + ctx.count(b))
        res["inter"].update(out)
    sp, _ = timed("second_push", lambda: ctx.ecsim_second_push(a), ctx.count(a))
    res["second_push_ms"] = sp["ms"]
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--ppc", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--vth", type=float, default=0.014)  # bench.py's default
    ap.add_argument("--strength", type=float, default=1e-9)
    ap.add_argument("--sorts", type=int, default=2, choices=(1, 2))
    ap.add_argument("--weighted", type=float, default=None, metavar="R")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.weighted is not None and args.sorts != 2:
        ap.error("--weighted needs two sorts")
    res = {"grid": f"{args.n}^3", "ppc": args.ppc, "reps": args.reps, "sorts": args.sorts, "lds_cell": X.COLLIDE_LDS_CELL,
           "runs": [run(args.n, args.ppc, args.reps, args.vth, p, args.strength, args.sorts, args.weighted)
                    for p in (("poisson",) if args.weighted is not None else ("poisson", "blob"))]}
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
