#!/usr/bin/env python3
"""Times the drift-kinetic pusher (xpic_drift_kinetic_trace) on static fields: a uniform field (E = (0, 0.1, -0.1),
B = (0, 0, 1), grad B = 0) and a mirror (B = (0, 0, 1 + 0.3 cos(2 pi z / Lz)) with its analytic grad |B|, E = 0).

Kernel time only, from the context's profile section "dk_trace" (the upload of the particles and the copy back are not
counted).  Reports particles * steps / s and the mean Picard iterations per step, prints one JSON object and writes it
to profiles/drift_kinetic_time_<n>.json.  Run it under `rocprofv3 --kernel-trace --stats -- python
tools/drift_kinetic_time.py` for the kernel table.
usage: drift_kinetic_time.py [--n 64] [--particles 1048576] [--steps 64] [--reps 3] [--dt 0.05]"""
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
    args = ap.parse_args()
    n, d = args.n, 0.5
    L = n * d
    shape = (n, n, n, 3)
    z = np.arange(n) * d
    cases = {}
    E, B, gB = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    E[..., 1], E[..., 2], B[..., 2] = 0.1, -0.1, 1.0
    cases["uniform"] = (E, B, None)
    E, B = np.zeros(shape), np.zeros(shape)
    B[..., 2] = (1.0 + 0.3 * np.cos(2 * np.pi * z / L))[:, None, None]
    gB[..., 2] = (-0.3 * 2 * np.pi / L * np.sin(2 * np.pi * z / L))[:, None, None]
    cases["mirror"] = (E, B, gB)
    rng = np.random.default_rng(7)
    npart = args.particles
    res = {"grid": f"{n}^3", "particles": npart, "steps": args.steps, "reps": args.reps, "dt": args.dt,
           "launch_steps": X.DK_LAUNCH_STEPS, "cases": {}}
    for name, (E, B, gB) in cases.items():
        ctx = X.Context("basic", (n, n, n), (d,) * 3, 1.0, device=0)
        ctx.set_field(X.E, E)
        ctx.set_field(X.B, B)
        gid = None
        if gB is not None:
            ctx.set_field(X.W0, gB)
            gid = X.W0
        pts = np.empty((npart, 6))
        pts[:, :3] = rng.random((npart, 3)) * L
        pts[:, 3:] = rng.normal(0.0, 0.5, (npart, 3))
        Bp = ctx.drift_kinetic_interpolate(pts[:, :3], pts[:, :3], gid)[1]
        p0 = X.guiding_centre(pts, Bp, 1.0, -1.0)
        kw = dict(qm=-1.0, mp=1.0, dt=args.dt, gradB_field=gid)
        ctx.drift_kinetic_trace(p0, min(args.steps, 4), **kw)  # warm-up
        ctx.profile_enable(True)
        ctx.profile_reset()
        its = 0
        unconverged = 0
        for _ in range(args.reps):
            _, _, tot, mx = ctx.drift_kinetic_trace(p0, args.steps, **kw)
            its += int(tot.sum())
            unconverged = max(unconverged, int((mx >= 30).sum()))
        launches, ms = ctx.profile_get("dk_trace")
        ctx.profile_enable(False)
        work = float(npart) * args.steps * args.reps
        res["cases"][name] = {"ms_per_trace": ms / args.reps, "launches": launches,
                              "particle_steps_per_s": work / (ms * 1e-3), "mean_iterations_per_step": its / work,
                              "particle_iterations_per_s": its / (ms * 1e-3),
                              "particles_with_an_unconverged_step": unconverged}
        ctx.close()
    print(json.dumps(res, indent=1))
    out = os.path.join(ROOT, "profiles", f"drift_kinetic_time_{n}.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
