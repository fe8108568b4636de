#!/usr/bin/env python3
"""Times the field-line kernel (include/xpic_field_lines.h).

--lines lines (default 2^20, one direction) x --steps steps (default 256, one launch) through a coils field on a 128^3
grid: kernel time from the context's profile section "field_lines", as line-steps/s and as field evaluations/s (four
magnetic gathers a step).  Beside it, in the same run and on the same grid, field and batch size: xpic_full_orbit_trace
with B1B for the same number of steps (profile section "fo_trace"; 64 steps a launch), the project's nearest kernel -- one
gather of E and B a step -- as particle-steps/s.  Each is repeated --reps times, alternating; reported are the values, the
median and the spread (max - min) / median.  Prints one JSON object and writes it to --out
(default profiles/field_lines_time.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import xpic_amd as X  # noqa: E402


def stats(v):
    med = float(np.median(v))
    return {"values": [float(x) for x in v], "median": med, "spread": float((max(v) - min(v)) / med)}


def section_ms(ctx, name, call):
    ctx.profile_enable(True)
    ctx.profile_reset()
    out = call()
    launches, ms = ctx.profile_get(name)
    ctx.profile_enable(False)
    return out, launches, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--lines", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_lines_time.json"))
    args = ap.parse_args()
    n, d = args.n, 0.5
    L = n * d
    ctx = X.Context("basic", (n, n, n), (d, d, d), 0.5, device=0)
    ctx.set_field(X.E, np.zeros(ctx.fshape()))
    ctx.set_field(X.B, np.zeros(ctx.fshape()) + np.array([0.0, 0.0, 0.2]))
    ctx.set_coils_field([(0.25 * L, 0.3 * L, 40.0), (0.75 * L, 0.3 * L, 40.0)], field=X.B)
    rng = np.random.default_rng(4)
    seeds = np.column_stack([L * (0.3 + 0.4 * rng.random((args.lines, 2))), L * (0.3 + 0.4 * rng.random(args.lines))])
    state = np.column_stack([seeds, rng.normal(0.0, 0.3, (args.lines, 3))])
    h, dt = 0.05, 0.05

    def lines():
        return ctx.field_lines(seeds, h=h, max_steps=args.steps, directions="+")

    def orbits():
        return ctx.full_orbit_trace(state, args.steps, "B1B", -1.0, dt)
    res = lines()  # warm-up, and what the lanes did
    orbits()
    assert (res.steps[0] == args.steps).all(), "a lane stopped early: the rates below would overstate the work"
    line_rate, orbit_rate, launches = [], [], {}
    for _ in range(args.reps):  # alternating
        _, launches["field_lines"], ms = section_ms(ctx, "field_lines", lines)
        line_rate.append(args.lines * args.steps / (ms * 1e-3))
        _, launches["fo_trace"], ms = section_ms(ctx, "fo_trace", orbits)
        orbit_rate.append(args.lines * args.steps / (ms * 1e-3))
    ctx.close()
    out = {"grid": "%d^3" % n, "lines": args.lines, "steps": args.steps, "h": h, "launches_per_call": launches,
           "line_steps_per_s": stats(line_rate), "field_evaluations_per_s": stats([4.0 * v for v in line_rate]),
           "full_orbit_B1B_particle_steps_per_s": stats(orbit_rate),
           "mirror_ratio_median": float(np.median(res.mirror_ratio)), "csrc_hash": X.csrc_hash()}
    out["evaluations_over_B1B_steps"] = out["field_evaluations_per_s"]["median"] / out["full_orbit_B1B_particle_steps_per_s"]["median"]
    out["note"] = ("kernel times from the context's profile sections (event pairs around the launches), staging and copies "
                   "excluded; one field evaluation is one magnetic gather (the B half of fo_gather), one B1B step is one "
                   "gather of E and B and the Boris rotation")
    print(json.dumps(out, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
