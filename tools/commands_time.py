#!/usr/bin/env python3
"""Times the per-step commands (xpic_remove_particles, xpic_inject_particles, xpic_fields_damping) and the SetCoilsField
set-up on the headline state: ECSIM, 256^3 x 64 per cell from load_synthetic, after one step (the records in the step's own
order), plus an empty second sort that the injection feeds.

Device time from the context's named profile sections ("cmd_remove", "cmd_inject", "cmd_damp", "cmd_coils"; a section
spans the whole call, its small host round trips included).  Each per-step call is also given as a multiple of the floor =
one read and one write of the surviving records (2 x 48 B per record) at the measured device copy rate; the damping also
against its own floor, one read and write of E and B and one read of B0 (5 x 24 B per node).  Calls:
  remove_nothing   a removal whose geometry holds every cell (counts only, no record touched), 3 reps
  remove_shell     the removal of a 2-cell shell (about 4.6 % of the records), ONE call (it changes the state)
  inject_2^20      2^20 ion / electron pairs in a cylinder, Maxwellian momenta, 3 reps
  damp_cylinder    the damping of a cylinder layer (radius 0.4 L, coefficient 0.8), 3 reps
  coils_setup      SetCoilsField with two coils into B0, ONE call
Prints one JSON object.  profiles/commands_rocprofv3_kernel_stats_256.csv is from `rocprofv3 --kernel-trace --stats -d <dir>
-o cmd --output-format csv -- python tools/commands_time.py --reps 1`, profiles/commands_time_256.json from the plain run.
usage: commands_time.py [--n 256] [--ppc 64] [--reps 3]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import xpic_amd as X  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--ppc", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--vth", type=float, default=0.014)  # bench.py's default
    ap.add_argument("--pairs", type=int, default=1 << 20)
    args = ap.parse_args()
    n, d = args.n, 0.5
    L = n * d
    ctx = X.Context("ecsim", (n, n, n), (d,) * 3, 1.0, device=0)
    extra = (args.reps + 1) * args.pairs + 1024
    e = ctx.add_sort(args.ppc, 1.0, -1.0, 1.0, capacity=int(args.ppc * ctx.N * 1.02) + extra)
    ion = ctx.add_sort(args.ppc, 1.0, 1.0, 100.0, capacity=extra)
    ctx.load_synthetic(e, args.ppc, args.vth, seed=1234)
    B = np.zeros(ctx.fshape())
    B[..., 2] = 0.2
    ctx.set_field(X.B, B)
    ctx.set_field(X.B0, B)
    del B
    ctx.step()
    res = {"grid": f"{n}^3", "ppc": args.ppc, "particles": ctx.count(e), "reps": args.reps}
    bw = ctx.probe_copy_bandwidth(1 << 30, 10)
    res["copy_GBps"] = bw / 1e9

    def timed(section, call, reps, warm=True):
        if warm:
            call()
        ctx.synchronize()
        ctx.profile_enable(True)
        ctx.profile_reset()
        out = None
        for _ in range(reps):
            out = call()
        ctx.synchronize()
        launches, ms = ctx.profile_get(section)
        ctx.profile_enable(False)
        per = ms / max(launches, 1)
        floor = 96 * ctx.count(e) / bw * 1e3  # one read and one write of the surviving records
        return {"ms": per, "calls": launches, "records_rw_floor_ms": floor, "x_records_rw": per / floor}, out

    t = {}
    whole = {"name": "box", "min": (0.0, 0.0, 0.0), "max": (L, L, L)}
    t["remove_nothing"], r = timed("cmd_remove", lambda: ctx.remove_particles(e, whole), args.reps)
    assert r[0] == 0
    before = ctx.count(e)
    shell = {"name": "box", "min": (2 * d,) * 3, "max": (L - 2 * d,) * 3}
    t["remove_shell"], r = timed("cmd_remove", lambda: ctx.remove_particles(e, shell), 1, warm=False)
    t["remove_shell"]["removed"] = r[0]
    t["remove_shell"]["removed_fraction"] = r[0] / before
    cyl = {"name": "CoordinateInCylinder", "center": (0.5 * L,) * 3, "radius": 0.3 * L, "height": 0.5 * L}
    mom = {"name": "MaxwellianMomentum", "T": (0.1, 0.1, 0.1)}
    step = [0]

    def inject():
        step[0] += 1
        return ctx.inject_particles(ion, e, args.pairs, step[0], cyl, mom, mom, seed=7)

    t[f"inject_{args.pairs}"], r = timed("cmd_inject", inject, args.reps)
    assert r[0] == args.pairs
    layer = {"name": "cylinder", "center": (0.5 * L,) * 3, "radius": 0.4 * L, "height": L}
    t["damp_cylinder"], _ = timed("cmd_damp", lambda: ctx.fields_damping(layer, 0.8), args.reps)
    ffloor = 5 * 24 * ctx.N / bw * 1e3
    t["damp_cylinder"].update({"field_floor_ms": ffloor, "x_field_floor": t["damp_cylinder"]["ms"] / ffloor})
    coils = [(0.25 * L, 0.3 * L, 1.0), (0.75 * L, 0.3 * L, 1.0)]
    t["coils_setup"], _ = timed("cmd_coils", lambda: ctx.set_coils_field(coils, X.B0), 1, warm=False)
    for k in ("records_rw_floor_ms", "x_records_rw"):  # (a set-up, not a per-step call)
        t["coils_setup"].pop(k)
    res["times"] = t
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
