#!/usr/bin/env python3
"""Times the triplet trace (xpic_triplet_trace) against the three closed traces it fuses, and its grid-less pair against
its two, on the batch of tools/model_trace_time.py: the Gaussian mirror of the reference's drift_kinetic_push_ex9.cpp
(B_min 1, B_max 4, L 5, W 1), the grid of drift_kinetic_grid_boris_ex4.cpp:25-29 (dx = 0.1, 100^3 nodes) filled by
xpic_set_model_field with E, B and grad |B|, a batch of one speed (0.1) and isotropic pitch angles within half a unit of the
trap's centre, the guiding centres guiding_centre(..., orbit_centre=True) of the same points.  Nothing is removed.

With EB2B the cases
  triplet          xpic_triplet_trace with the grid member, no curve           profile section "triplet_trace"
  triplet_curve    the same with the curve at every step (sample_every 1)
  closed3          xpic_model_drift_kinetic_trace, xpic_drift_kinetic_trace, xpic_model_full_orbit_trace, one after the
                   other on the same inputs: "model_dk_trace" + "dk_trace" + "model_fo_trace"
  pair             xpic_triplet_trace with with_grid = 0                        "triplet_trace"
  closed2          xpic_model_drift_kinetic_trace, then xpic_model_full_orbit_trace: "model_dk_trace" + "model_fo_trace"
are run --reps times, alternating, after a warm-up of every case; kernel time only, from the context's profile sections
(staging and copies are not counted).  The closed traces are the kernels this build shares with its parent commit and stand
for it.  Reports the median and (max - min) / median of each case and the ratios fused / closed, and asserts on the way that
the final states of the fused calls are the closed traces' bits at this size.  Prints one JSON object and writes it to
profiles/triplet_trace_time.json.
usage: triplet_trace_time.py [--n 100] [--particles 1048576] [--steps 1024] [--reps 3] [--omega-dt 0.1]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "triplet_trace_time.json"))
    args = ap.parse_args()
    n, d = args.n, 0.1
    ctx = X.Context("basic", (n, n, n), (d,) * 3, 1.0, device=0)
    model = X.field_model("gaussian_mirror", **GAUSSIAN)
    ctx.set_model_field(model, X.E, X.B, X.W0)
    rng = np.random.default_rng(7)
    npart, steps = args.particles, args.steps
    mu = 2.0 * rng.random(npart) - 1.0  # cosine of the pitch angle: isotropic
    phi = 2 * np.pi * rng.random(npart)
    s = np.sqrt(1.0 - mu * mu)
    pts = np.empty((npart, 6))
    pts[:, :3] = GAUSSIAN["L"] + (rng.random((npart, 3)) - 0.5)
    pts[:, 3:] = 0.1 * np.column_stack([s * np.cos(phi), s * np.sin(phi), mu])
    qm, mp, scheme = -1.0, 1.0, "EB2B"
    dt = args.omega_dt / ctx.model_fields(model, [[GAUSSIAN["L"]] * 3])[1][0, 2]  # Omega = Bz at the centre
    gcs = X.guiding_centre(pts, ctx.model_fields(model, pts[:, :3])[1], mp, qm, orbit_centre=True)
    launches = (steps + X.TRIPLET_LAUNCH_STEPS - 1) // X.TRIPLET_LAUNCH_STEPS
    res = {"commit": args.commit or commit(), "grid": f"{n}^3, d = {d}", "triplets": npart, "steps": steps, "dt": dt,
           "omega_dt": args.omega_dt, "reps": args.reps, "launch_steps": X.TRIPLET_LAUNCH_STEPS, "model": dict(GAUSSIAN),
           "scheme": scheme}

    def timed(call, sections):
        ctx.profile_enable(True)
        ctx.profile_reset()
        out = call()
        ms = sum(ctx.profile_get(s_)[1] for s_ in sections)
        ctx.profile_enable(False)
        return out, ms

    def triplet(p, g, k, grid=True, **kw):
        return ctx.triplet_trace(p, g, g if grid else None, k, scheme, qm, mp, dt, model, gradB_field=X.W0, **kw)

    def closed(p, g, k, grid=True):
        a = ctx.model_drift_kinetic_trace(g, k, qm, mp, dt, model).state
        b = ctx.drift_kinetic_trace(g, k, qm, mp, dt, X.W0)[0] if grid else None
        return a, b, ctx.model_full_orbit_trace(p, k, scheme, qm, dt, model).state

    cases = {
        "triplet": (lambda p, g, k: triplet(p, g, k), ["triplet_trace"]),
        "triplet_curve": (lambda p, g, k: triplet(p, g, k, sample_every=1), ["triplet_trace"]),
        "closed3": (lambda p, g, k: closed(p, g, k), ["model_dk_trace", "dk_trace", "model_fo_trace"]),
        "pair": (lambda p, g, k: triplet(p, g, k, grid=False), ["triplet_trace"]),
        "closed2": (lambda p, g, k: closed(p, g, k, grid=False), ["model_dk_trace", "model_fo_trace"]),
    }
    for call, _ in cases.values():  # warm-up: every kernel of the timed window, once
        call(pts[:4096], gcs[:4096], 4)
    ms = {name: [] for name in cases}
    outs = {}
    for rep in range(args.reps):  # alternating: a drift of the box over the run falls on every case alike
        for name, (call, sections) in cases.items():
            outs[name], t = timed(lambda: call(pts, gcs, steps), sections)
            ms[name].append(t)
            print(f"rep {rep} {name}: {t:.1f} ms", file=sys.stderr, flush=True)
    tri, cur, pair = outs["triplet"], outs["triplet_curve"], outs["pair"]
    for fused, (a, b, f) in ((tri, outs["closed3"]), (pair, outs["closed2"])):
        assert fused.state_model.tobytes() == a.tobytes() and fused.p.tobytes() == f.tobytes()
        assert b is None or fused.state_grid.tobytes() == b.tobytes()
    assert cur.p.tobytes() == tri.p.tobytes() and cur.stats.tobytes() == tri.stats.tobytes()
    assert not pair.stats[:, :3].any()
    res["final_states_equal_the_closed_traces_bit_for_bit"] = True
    res["cases"] = {}
    for name, v in ms.items():
        med = float(np.median(v))
        res["cases"][name] = {"kernel_ms": v, "median_ms": med, "spread": (max(v) - min(v)) / med,
                              "median_ms_per_launch_of_64": med / launches,
                              "ns_per_triplet_step": med * 1e6 / (float(npart) * steps)}
    c = res["cases"]
    res["ratio_triplet_to_closed3"] = c["triplet"]["median_ms"] / c["closed3"]["median_ms"]
    res["ratio_triplet_curve_to_closed3"] = c["triplet_curve"]["median_ms"] / c["closed3"]["median_ms"]
    res["ratio_pair_to_closed2"] = c["pair"]["median_ms"] / c["closed2"]["median_ms"]
    res["largest_spread"] = max(v["spread"] for v in c.values())
    work = float(npart) * steps
    res["mean_dk_iterations_per_step"] = {"model": float(tri.dkm_iterations_total.sum()) / work,
                                          "grid": float(tri.dkg_iterations_total.sum()) / work}
    res["triplets_with_an_unconverged_dk_step"] = {"model": int((tri.dkm_iterations_max >= 30).sum()),
                                                   "grid": int((tri.dkg_iterations_max >= 30).sum())}
    res["largest_stats"] = dict(zip(X.TRIPLET_STATS, [float(v) for v in np.nanmax(tri.stats, axis=0)]))
    res["largest_stats_pair"] = dict(zip(X.TRIPLET_STATS[3:], [float(v) for v in np.nanmax(pair.stats[:, 3:], axis=0)]))
    res["curve_last_row"] = dict(zip(X.TRIPLET_STATS, [float(v) for v in cur.curve[-1]]))
    ctx.close()
    res["closed_is"] = ("the closed traces of this build on the same inputs, in the same process, alternating with the fused "
                        "cases; their kernels are the parent commit's, assembly for assembly")
    print(json.dumps(res, indent=1))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
