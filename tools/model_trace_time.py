#!/usr/bin/env python3
"""Times the tracers on an analytic field model (xpic_model_full_orbit_trace, xpic_model_drift_kinetic_trace) against the
grid traces (xpic_full_orbit_trace, xpic_drift_kinetic_trace) on the same model, in the Gaussian mirror of the reference's
drift_kinetic_push_ex9.cpp (B_min 1, B_max 4, L 5, W 1).  The grid is the one of drift_kinetic_grid_boris_ex4.cpp:25-29
(dx = 0.1, 100^3 nodes) filled by xpic_set_model_field: E, B and grad |B| at the nodes.  A batch of one speed (0.1, ex9's)
and isotropic pitch angles starts within half a unit of the trap's centre; the guiding centres are guiding_centre(...,
orbit_centre=True) of the same points.  No region: nothing is removed on either side (the grid gathers wrap, the model
simply goes on beyond the throats), so both sides make every step of every particle.

For EB2B and for the drift-kinetic pusher the cases
  grid       the grid trace       profile section "fo_trace" / "dk_trace"
  analytic   the model trace      profile section "model_fo_trace" / "model_dk_trace"
are run --reps times, alternating, after a warm-up of both; kernel time only, from the context's profile sections (staging
and copies are not counted).  The grid traces are the kernels this build shares with its parent commit and stand for it.
Reports the medians, (max - min) / median, the ratio analytic / grid, and how far the two sides' final states are apart
(the grid's interpolation error, not a parity check).  Prints one JSON object and writes it to
profiles/model_trace_time.json.
usage: model_trace_time.py [--n 100] [--particles 1048576] [--steps 1024] [--reps 3] [--omega-dt 0.1]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import xpic_amd as X  # noqa: E402

GAUSSIAN = dict(B_min=1.0, B_max=4.0, L=5.0, W=1.0)  # tests/drift_kinetic_push/drift_kinetic_push.h:74-77


def commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              timeout=10).stdout.strip() or None
    except OSError:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--particles", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--omega-dt", type=float, default=0.1)
    ap.add_argument("--commit", default=None, help="the commit the library was built from (default: git's HEAD, if any)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "model_trace_time.json"))
    args = ap.parse_args()
    n, d = args.n, 0.1
    ctx = X.Context("basic", (n, n, n), (d,) * 3, 1.0, device=0)
    model = X.field_model("gaussian_mirror", **GAUSSIAN)
    ctx.set_model_field(model, X.E, X.B, X.W0)
    rng = np.random.default_rng(7)
    npart = args.particles
    mu = 2.0 * rng.random(npart) - 1.0  # cosine of the pitch angle: isotropic
    phi = 2 * np.pi * rng.random(npart)
    s = np.sqrt(1.0 - mu * mu)
    pts = np.empty((npart, 6))
    pts[:, :3] = GAUSSIAN["L"] + (rng.random((npart, 3)) - 0.5)
    pts[:, 3:] = 0.1 * np.column_stack([s * np.cos(phi), s * np.sin(phi), mu])
    qm, mp = -1.0, 1.0
    dt = args.omega_dt / ctx.model_fields(model, [[GAUSSIAN["L"]] * 3])[1][0, 2]  # Omega = Bz at the centre
    gcs = X.guiding_centre(pts, ctx.model_fields(model, pts[:, :3])[1], mp, qm, orbit_centre=True)
    launches = (args.steps + X.MODEL_LAUNCH_STEPS - 1) // X.MODEL_LAUNCH_STEPS
    res = {"commit": args.commit or commit(), "grid": f"{n}^3, d = {d}", "particles": npart, "steps": args.steps, "dt": dt,
           "omega_dt": args.omega_dt, "reps": args.reps, "launch_steps": X.MODEL_LAUNCH_STEPS, "model": dict(GAUSSIAN),
           "pushers": {}}

    def timed(call, section):
        ctx.profile_enable(True)
        ctx.profile_reset()
        out = call()
        ms = ctx.profile_get(section)[1]
        ctx.profile_enable(False)
        return out, ms

    pushers = {
        "EB2B": {
            "grid": (lambda p, k: ctx.full_orbit_trace(p, k, "EB2B", qm, dt)[0], "fo_trace"),
            "analytic": (lambda p, k: ctx.model_full_orbit_trace(p, k, "EB2B", qm, dt, model).state, "model_fo_trace"),
            "batch": pts},
        "drift_kinetic": {
            "grid": (lambda p, k: ctx.drift_kinetic_trace(p, k, qm, mp, dt, X.W0)[0], "dk_trace"),
            "analytic": (lambda p, k: ctx.model_drift_kinetic_trace(p, k, qm, mp, dt, model).state, "model_dk_trace"),
            "batch": gcs},
    }
    for name, P in pushers.items():
        batch = P["batch"]
        for side in ("grid", "analytic"):  # warm-up: every kernel of the timed window, once
            P[side][0](batch[:4096], 4)
        ms = {"grid": [], "analytic": []}
        outs = {}
        for rep in range(args.reps):  # alternating: a drift of the box over the run falls on both sides alike
            for side in ("grid", "analytic"):
                call, section = P[side]
                outs[side], t = timed(lambda: call(batch, args.steps), section)
                ms[side].append(t)
                print(f"{name} rep {rep} {side}: {t:.1f} ms", file=sys.stderr, flush=True)
        r = {"cases": {}}
        for side, v in ms.items():
            med = float(np.median(v))
            r["cases"][side] = {"kernel_ms": v, "median_ms": med, "spread": (max(v) - min(v)) / med,
                                "median_ms_per_launch_of_64": med / launches,
                                "ns_per_particle_step": med * 1e6 / (float(npart) * args.steps)}
        r["ratio_analytic_to_grid"] = r["cases"]["analytic"]["median_ms"] / r["cases"]["grid"]["median_ms"]
        r["grid_over_analytic"] = 1.0 / r["ratio_analytic_to_grid"]
        r["largest_spread"] = max(c["spread"] for c in r["cases"].values())
        diff = np.abs(outs["grid"][:, :3] - outs["analytic"][:, :3])
        r["final_position_difference_median"] = float(np.nanmedian(diff.max(axis=1)))
        res["pushers"][name] = r
    ctx.close()
    res["grid_is"] = ("xpic_full_orbit_trace / xpic_drift_kinetic_trace of this build on vectors filled by "
                      "xpic_set_model_field, same batch, same process, alternating with the analytic traces")
    print(json.dumps(res, indent=1))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
