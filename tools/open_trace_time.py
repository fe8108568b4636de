#!/usr/bin/env python3
"""Times the open-trap full-orbit trace (xpic_full_orbit_trace_open, scheme EB2B) in the reference's analytic two-coil
trap: a uniform Bz plus SetApproximateMirrorField with the coils half a box apart, so that with the gathers' periodic
wrap the field is weakest in the plane z = 0 and strongest in the plane z = L / 2; a batch of one speed and isotropic
pitch angles starts around (L / 2, L / 2, 0) and is traced, unfolded, between the planes z = -0.44 L and z = +0.44 L,
just inside the two field maxima.  Whoever is in the loss cone leaves through an end.

Reports the lost fraction against the step, and kernel time (the context's profile sections "fo_trace", "fo_trace_open",
"fo_trace_open_compact"; staging and copies are not counted) per launch of at most 64 steps for
  closed          xpic_full_orbit_trace of the same batch (k_fo_trace, the closed text beside k_fo_trace_open: both run on
                  the one trace driver, batch.h's batch_trace, which reads nothing back between a closed trace's launches)
  open_everywhere the open trace with a region nobody leaves: the cost of the test
  lossy_auto / lossy_never / lossy_always   the trap's region with compact = 0, 1, 2
with each open case's ratio to `closed`, and checks on the way that the three policies return the same bits.  Prints one
JSON object and writes it to profiles/open_trace_time.json.
usage: open_trace_time.py [--n 64] [--particles 1048576] [--steps 1024] [--dt 0.2] [--uniform 0.3]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import xpic_amd as X  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--particles", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=1024)
    ap.add_argument("--dt", type=float, default=0.2)
    ap.add_argument("--uniform", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "open_trace_time.json"))
    args = ap.parse_args()
    n, d = args.n, 0.5
    L = n * d
    coil = dict(D=L, R=6.0, I=1.0)
    ctx = X.Context("basic", (n, n, n), (d,) * 3, 1.0, device=0)
    shape = ctx.fshape()
    ctx.set_field(X.E, np.zeros(shape))
    ctx.set_field(X.B, np.zeros(shape) + np.array([0.0, 0.0, args.uniform]))
    ctx.set_mirror_field(field=X.B, **coil)
    Bz = ctx.get_field(X.B)[:, n // 2, n // 2, 2]
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
    trap = {"name": "box", "min": (-8 * L, -8 * L, -0.44 * L), "max": (9 * L, 9 * L, 0.44 * L)}
    everywhere = {"name": "box", "min": (-1e9, -1e9, -1e9), "max": (1e9, 1e9, 1e9)}
    kw = dict(scheme="EB2B", qm=-1.0, dt=args.dt)
    launches = (args.steps + X.FO_LAUNCH_STEPS - 1) // X.FO_LAUNCH_STEPS
    res = {"grid": f"{n}^3", "particles": npart, "steps": args.steps, "dt": args.dt, "scheme": "EB2B",
           "launch_steps": X.FO_LAUNCH_STEPS, "uniform_Bz": args.uniform, "mirror": coil,
           "Bz_on_axis_min_max": [float(Bz.min()), float(Bz.max())], "cases": {}}

    def timed(name, call, sections):
        ctx.profile_enable(True)
        ctx.profile_reset()
        t0 = time.perf_counter()
        out = call()
        wall = time.perf_counter() - t0
        got = {s_: ctx.profile_get(s_) for s_ in sections}
        ctx.profile_enable(False)
        ms = sum(v[1] for v in got.values())
        res["cases"][name] = {"kernel_ms": ms, "kernel_ms_per_launch_of_64": ms / launches, "wall_s_with_staging": wall,
                              "sections": {k: {"launches": v[0], "ms": v[1]} for k, v in got.items()}}
        return out

    ctx.full_orbit_trace(pts[:4096], 4, **kw)  # warm-up
    ctx.full_orbit_trace_open(pts[:4096], 4, region=trap, **kw)
    closed = timed("closed", lambda: ctx.full_orbit_trace(pts, args.steps, **kw), ["fo_trace"])
    open_s = ["fo_trace_open", "fo_trace_open_compact"]
    free = timed("open_everywhere", lambda: ctx.full_orbit_trace_open(pts, args.steps, region=everywhere, **kw), open_s)
    assert free.removed == 0 and free.state.tobytes() == closed[0].tobytes()
    outs = {}
    for name in ("auto", "never", "always"):
        outs[name] = timed("lossy_" + name, lambda: ctx.full_orbit_trace_open(
            pts, args.steps, region=trap, sample_every=X.FO_LAUNCH_STEPS, keep_samples=False, compact=name, **kw), open_s)
    for name in ("never", "always"):
        assert outs[name].state.tobytes() == outs["auto"].state.tobytes()
        assert np.array_equal(outs[name].exit_step, outs["auto"].exit_step)
        assert np.array_equal(outs[name].alive, outs["auto"].alive)
    ctx.close()
    base = res["cases"]["closed"]["kernel_ms"]
    for name, case in res["cases"].items():
        case["ratio_to_closed"] = case["kernel_ms"] / base
    # one run on one box: the pool's box-to-box spread (measured on the assembly) is what a ratio
    # between two cases of this file can be trusted to
    res["box_to_box_spread_quoted"] = 0.04
    res["closed_is"] = ("xpic_full_orbit_trace of this build, same run and box; k_fo_trace is the closed text that stays beside "
                        "k_fo_trace_open (DESIGN.md 5q), on the trace driver both share")
    a = outs["auto"]
    res["lost_fraction"] = float(a.removed) / npart
    res["lost_fraction_by_step"] = [[int((k + 1) * X.FO_LAUNCH_STEPS), 1.0 - float(v) / npart] for k, v in enumerate(a.alive)]
    print(json.dumps(res, indent=1))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
