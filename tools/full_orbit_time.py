#!/usr/bin/env python3
"""Times the full-orbit pusher (xpic_full_orbit_trace) on static smooth fields (a base plus one box-periodic mode per
component) for the Boris scheme EB2B and for Crank-Nicolson.

Kernel time only, from the context's profile section "fo_trace" (the upload of the particles and the copy back are not
counted).  Reports particles * steps / s and, for CN, the mean iteration number per step, prints one JSON object and
writes it to profiles/full_orbit_time_<n>.json.  Run it under `rocprofv3 --kernel-trace --stats -- python
tools/full_orbit_time.py` for the kernel table.
usage: full_orbit_time.py [--n 64] [--particles 1048576] [--steps 64] [--reps 3] [--dt 0.05] [--schemes EB2B,CN]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import xpic_amd as X  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--particles", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dt", type=float, default=0.05)
    ap.add_argument("--schemes", default="EB2B,CN")
    args = ap.parse_args()
    n, d = args.n, 0.5
    L = n * d
    k = np.arange(n) / n
    z, y, x = np.meshgrid(k, k, k, indexing="ij")
    E, B = np.zeros((n, n, n, 3)), np.zeros((n, n, n, 3))
    for c, (e0, b0) in enumerate(((0.0, 0.2), (0.1, 0.3), (-0.1, 1.0))):
        E[..., c] = e0 + 0.05 * np.cos(2 * np.pi * (x + y) + c)
        B[..., c] = b0 + 0.1 * np.cos(2 * np.pi * (y + z) + c)
    rng = np.random.default_rng(7)
    npart = args.particles
    pts = np.empty((npart, 6))
    pts[:, :3] = rng.random((npart, 3)) * L
    pts[:, 3:] = rng.normal(0.0, 0.5, (npart, 3))
    res = {"grid": f"{n}^3", "particles": npart, "steps": args.steps, "reps": args.reps, "dt": args.dt,
           "launch_steps": X.FO_LAUNCH_STEPS, "cases": {}}
    ctx = X.Context("basic", (n, n, n), (d,) * 3, 1.0, device=0)
    ctx.set_field(X.E, E)
    ctx.set_field(X.B, B)
    for scheme in args.schemes.split(","):
        kw = dict(scheme=scheme, qm=-1.0, dt=args.dt)
        ctx.full_orbit_trace(pts, min(args.steps, 4), **kw)  # warm-up
        ctx.profile_enable(True)
        ctx.profile_reset()
        its, unconverged = 0, 0
        for _ in range(args.reps):
            _, _, tot, mx = ctx.full_orbit_trace(pts, args.steps, **kw)
            its += int(tot.sum())
            unconverged = max(unconverged, int((mx >= 30).sum()))
        launches, ms = ctx.profile_get("fo_trace")
        ctx.profile_enable(False)
        work = float(npart) * args.steps * args.reps
        res["cases"][scheme] = {"ms_per_trace": ms / args.reps, "launches": launches,
                                "particle_steps_per_s": work / (ms * 1e-3), "mean_iteration_number_per_step": its / work,
                                "particles_with_an_unconverged_step": unconverged}
    ctx.close()
    print(json.dumps(res, indent=1))
    out = os.path.join(ROOT, "profiles", f"full_orbit_time_{n}.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
