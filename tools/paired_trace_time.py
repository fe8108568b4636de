#!/usr/bin/env python3
"""Times the paired trace (xpic_paired_trace) against the two closed traces it fuses, in the analytic two-coil field of
tools/open_trace_time.py: a uniform Bz plus SetApproximateMirrorField (xpic_set_mirror_field) with the coils half a box
apart, grad |B| by central differences of |B| on the nodes, E = 0.  A batch of one speed and isotropic pitch angles starts
around (L / 2, L / 2, 0); the guiding centres are guiding_centre(..., orbit_centre=True) of the same points.  Nothing is
removed: the gathers wrap.

For each scheme (EB2B, CN) the cases
  paired           xpic_paired_trace without a curve                      profile section "pair_trace"
  paired_curve     the same with the curve at every step (sample_every 1)
  closed           xpic_full_orbit_trace, then xpic_drift_kinetic_trace, on the same inputs: "fo_trace" + "dk_trace"
are run --reps times, alternating, after a warm-up of every case; kernel time only, from the context's profile sections
(staging and copies are not counted).  Reports the median and (max - min) / median of each case, the ratio of the paired
medians to the closed one, and checks on the way that the paired states are the closed traces' bits.  Prints one JSON
object and writes it to profiles/paired_trace_time.json.
usage: paired_trace_time.py [--n 64] [--particles 1048576] [--steps 1024] [--reps 3] [--dt 0.1] [--uniform 0.3]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import xpic_amd as X  # noqa: E402


def commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              timeout=10).stdout.strip() or None
    except OSError:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--particles", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dt", type=float, default=0.1)
    ap.add_argument("--uniform", type=float, default=0.3)
    ap.add_argument("--commit", default=None, help="the commit the library was built from (default: git's HEAD, if any)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paired_trace_time.json"))
    args = ap.parse_args()
    n, d = args.n, 0.5
    L = n * d
    coil = dict(D=L, R=6.0, I=1.0)
    ctx = X.Context("basic", (n, n, n), (d,) * 3, 1.0, device=0)
    shape = ctx.fshape()
    ctx.set_field(X.E, np.zeros(shape))
    ctx.set_field(X.B, np.zeros(shape) + np.array([0.0, 0.0, args.uniform]))
    ctx.set_mirror_field(field=X.B, **coil)
    B = ctx.get_field(X.B)
    absB = np.sqrt((B * B).sum(axis=-1))
    gB = np.stack([(np.roll(absB, -1, axis=2 - a) - np.roll(absB, 1, axis=2 - a)) / (2 * d) for a in range(3)], axis=-1)
    ctx.set_field(X.W0, gB)
    rng = np.random.default_rng(7)
    npart = args.particles
    mu = 2.0 * rng.random(npart) - 1.0  # cosine of the pitch angle: isotropic
    phi = 2 * np.pi * rng.random(npart)
    s = np.sqrt(1.0 - mu * mu)
    pts = np.empty((npart, 6))
    pts[:, 0] = 0.5 * L + (rng.random(npart) - 0.5)
    pts[:, 1] = 0.5 * L + (rng.random(npart) - 0.5)
    pts[:, 2] = (rng.random(npart) - 0.5)
    pts[:, 3:] = np.column_stack([s * np.cos(phi), s * np.sin(phi), mu])
    qm, mp = -1.0, 1.0
    Bp = ctx.drift_kinetic_interpolate(pts[:, :3], pts[:, :3], X.W0)[1]
    gcs = X.guiding_centre(pts, Bp, mp, qm, orbit_centre=True)
    launches = (args.steps + X.PAIR_LAUNCH_STEPS - 1) // X.PAIR_LAUNCH_STEPS
    res = {"commit": args.commit or commit(), "grid": f"{n}^3", "pairs": npart, "steps": args.steps, "dt": args.dt,
           "reps": args.reps, "launch_steps": X.PAIR_LAUNCH_STEPS, "uniform_Bz": args.uniform, "mirror": coil, "schemes": {}}

    def timed(call, sections):
        ctx.profile_enable(True)
        ctx.profile_reset()
        out = call()
        ms = sum(ctx.profile_get(s_)[1] for s_ in sections)
        ctx.profile_enable(False)
        return out, ms

    for scheme in ("EB2B", "CN"):
        pk = dict(scheme=scheme, qm=qm, mp=mp, dt=args.dt, gradB_field=X.W0)
        cases = {
            "paired": (lambda: ctx.paired_trace(pts, gcs, args.steps, **pk), ["pair_trace"]),
            "paired_curve": (lambda: ctx.paired_trace(pts, gcs, args.steps, sample_every=1, **pk), ["pair_trace"]),
            "closed": (lambda: (ctx.full_orbit_trace(pts, args.steps, scheme, qm, args.dt),
                                ctx.drift_kinetic_trace(gcs, args.steps, qm, mp, args.dt, X.W0)), ["fo_trace", "dk_trace"]),
        }
        small = (pts[:4096], gcs[:4096])  # warm-up: every kernel of the timed window, once
        ctx.paired_trace(*small, 4, **pk)
        ctx.paired_trace(*small, 4, sample_every=1, **pk)
        ctx.full_orbit_trace(small[0], 4, scheme, qm, args.dt)
        ctx.drift_kinetic_trace(small[1], 4, qm, mp, args.dt, X.W0)
        ms = {name: [] for name in cases}
        outs = {}
        for rep in range(args.reps):  # alternating: a drift of the box over the run falls on every case alike
            for name, (call, sections) in cases.items():
                outs[name], t = timed(call, sections)
                ms[name].append(t)
                print(f"{scheme} rep {rep} {name}: {t:.1f} ms", file=sys.stderr, flush=True)
        pair, curve, (fo, dk) = outs["paired"], outs["paired_curve"], outs["closed"]
        assert pair.p.tobytes() == fo[0].tobytes() and pair.state.tobytes() == dk[0].tobytes()
        assert curve.p.tobytes() == pair.p.tobytes() and curve.stats.tobytes() == pair.stats.tobytes()
        r = {"cases": {}}
        for name, v in ms.items():
            med = float(np.median(v))
            r["cases"][name] = {"kernel_ms": v, "median_ms": med, "spread": (max(v) - min(v)) / med,
                                "median_ms_per_launch_of_64": med / launches}
        base = r["cases"]["closed"]["median_ms"]
        r["ratio_paired_to_closed"] = r["cases"]["paired"]["median_ms"] / base
        r["ratio_paired_curve_to_closed"] = r["cases"]["paired_curve"]["median_ms"] / base
        r["largest_spread"] = max(c["spread"] for c in r["cases"].values())
        work = float(npart) * args.steps
        r["mean_dk_iterations_per_step"] = float(pair.dk_iterations_total.sum()) / work
        r["pairs_with_an_unconverged_dk_step"] = int((pair.dk_iterations_max >= 30).sum())
        r["mean_fo_iterations_per_step"] = float(pair.fo_iterations_sum.sum()) / work
        r["largest_stats"] = dict(zip(X.PAIR_STATS, [float(v) for v in np.nanmax(pair.stats, axis=0)]))
        r["curve_last_row"] = dict(zip(X.PAIR_STATS, [float(v) for v in curve.curve[-1]]))
        res["schemes"][scheme] = r
    ctx.close()
    res["closed_is"] = ("xpic_full_orbit_trace then xpic_drift_kinetic_trace of this build, same inputs, same process, "
                        "alternating with the paired cases")
    print(json.dumps(res, indent=1))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
