#!/usr/bin/env python3
"""Times the collisional model traces (xpic_model_full_orbit_trace_collisional,
xpic_model_drift_kinetic_trace_collisional; xpic_amd/csrc/collide_trace.hip) against the collisionless model traces of the
same call (xpic_model_full_orbit_trace, xpic_model_drift_kinetic_trace), in the Gaussian mirror and with the batch of
tools/model_trace_time.py: one speed (0.1), isotropic pitch angles, within half a unit of the trap's centre; no region, so
every particle makes every step.  The backgrounds are electrons and ions at the test particles' temperature; the
strength gives the first a sigma^2 of 1e-3 at the test particles' speed (the time does not depend on it: every collision
costs the same arithmetic).

For EB2B, Crank-Nicolson and the drift-kinetic pusher the cases
  model          the model trace                         profile section "model_fo_trace" / "model_dk_trace"
  collisional_1  the collisional trace, one background   profile section "coll_fo_trace" / "coll_dk_trace"
  collisional_2  the same with two backgrounds
are run --reps times, alternating, after a warm-up of all; kernel time only, from the context's profile sections (staging,
copies and the tallies' reduction are not counted).  Reports the medians, (max - min) / median, the ratios to the model
trace and the cost of one collision in ns per particle, with the box's device copy rate beside them.  Prints one JSON
object and writes it to profiles/collisional_trace_time.json.
usage: collisional_trace_time.py [--particles 1048576] [--steps 256] [--reps 3] [--omega-dt 0.1] [--every 1]

--grid times the collisional grid traces instead (xpic_full_orbit_trace_collisional, xpic_drift_kinetic_trace_collisional;
DESIGN.md 5u) on a --cells^3 grid with a uniform B plus xpic_set_mirror_field's field, a region nobody leaves, the same
kind of batch about the box centre.  For EB2B, Crank-Nicolson and the drift-kinetic pusher the cases
  open       the collisionless open grid trace                  profile section "fo_trace_open" / "dk_trace_open"
  uniform_1  the collisional grid trace, one uniform background  "coll_fo_grid_trace" / "coll_dk_grid_trace"
  profile_1  the same off a profile made by xpic_background_from_sort from the context's sort
and, on the sort of --ppc records per cell that the profile is made of, xpic_background_from_sort ("background_from_sort")
against xpic_collide ("cmd_collide"), which stream the same records; the moment kernel reads the three velocity arrays
twice (two passes), which the report sets against the box's device copy rate.  --reps alternating runs (five for the
record), medians and (max - min) / median; writes profiles/collisional_grid_trace_time.json.
usage: collisional_trace_time.py --grid [--particles 1048576] [--steps 128] [--reps 5] [--cells 64] [--ppc 64] [--every 1]"""
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


def summary(v):
    med = float(np.median(v))
    return {"kernel_ms": [float(x) for x in v], "median_ms": med, "spread": (max(v) - min(v)) / med}


def grid_main(args):
    n, d = (args.cells,) * 3, (0.25,) * 3
    box = args.cells * 0.25
    ctx = X.Context("ecsim", n, d, 1.0, device=0)
    shape = ctx.fshape()
    ctx.set_field(X.E, np.zeros(shape))
    ctx.set_field(X.B, np.zeros(shape) + np.array([0.0, 0.0, 1.0]))
    ctx.set_mirror_field(box, box / 3, 2.0, field=X.B)
    B = ctx.get_field(X.B)
    lB = np.sqrt((B * B).sum(axis=-1))
    g = np.zeros_like(B)
    for c, axis in enumerate((2, 1, 0)):
        g[..., c] = (np.roll(lB, -1, axis=axis) - np.roll(lB, 1, axis=axis)) / (2.0 * d[c])
    ctx.set_field(X.W0, g)
    sort = ctx.add_sort(args.ppc, 1.0, 1.0, 1836.0, capacity=int(1.25 * args.ppc * args.cells ** 3) + 1024)
    vth = 0.1 / np.sqrt(3.0)
    ctx.fill_synthetic(sort, args.ppc, vth / np.sqrt(1836.0), seed=3)
    records = ctx.count(sort)
    rng = np.random.default_rng(7)
    npart = args.particles
    mu, phi = 2.0 * rng.random(npart) - 1.0, 2 * np.pi * rng.random(npart)
    s = np.sqrt(1.0 - mu * mu)
    pts = np.empty((npart, 6))
    pts[:, :3] = box / 2 + (rng.random((npart, 3)) - 0.5)
    pts[:, 3:] = 0.1 * np.column_stack([s * np.cos(phi), s * np.sin(phi), mu])
    qm, mp = -1.0, 1.0
    Bp = ctx.drift_kinetic_interpolate(pts[:, :3], pts[:, :3])[1]
    dt = args.omega_dt / float(np.sqrt((Bp * Bp).sum(axis=1)).mean())
    gcs = X.guiding_centre(pts, Bp, mp, qm, orbit_centre=True)
    region = {"name": "box", "min": (-1e6,) * 3, "max": (1e6,) * 3}  # nobody leaves: every particle makes every step
    bg = dict(q=1.0, m=1836.0, n=1.0, vth=vth / np.sqrt(1836.0))
    strength = 1e-3 * 0.1 ** 3 / (args.every * dt)  # sigma^2 = S n dt_c / (m_ab^2 u^3) = 1e-3 at n = 1, m_ab ~ 1, u = 0.1
    coll = X.trace_collisions([bg], strength=strength, mass=1.0, every=args.every, seed=5)
    bw = ctx.probe_copy_bandwidth(1 << 30, 10)
    res = {"commit": args.commit or commit(), "grid": list(n), "d": list(d), "particles": npart, "steps": args.steps, "dt": dt,
           "every": args.every, "reps": args.reps, "launch_steps": X.FO_LAUNCH_STEPS, "background": bg, "strength": strength,
           "sort_records": records, "ppc": args.ppc, "copy_GBps": bw / 1e9, "pushers": {}}

    def timed(call, section):
        ctx.profile_enable(True)
        ctx.profile_reset()
        out = call()
        ms = ctx.profile_get(section)[1]
        ctx.profile_enable(False)
        return out, ms

    def fo(scheme):
        return {"open": (lambda p, k: ctx.full_orbit_trace_open(p, k, scheme, qm, dt, region), "fo_trace_open"),
                "uniform_1": (lambda p, k: ctx.full_orbit_trace_collisional(p, k, scheme, qm, dt, coll, None, region),
                              "coll_fo_grid_trace"),
                "profile_1": (lambda p, k: ctx.full_orbit_trace_collisional(p, k, scheme, qm, dt, coll, [0], region),
                              "coll_fo_grid_trace"),
                "batch": pts}
    pushers = {"EB2B": fo("EB2B"), "CN": fo("CN"), "drift_kinetic": {
        "open": (lambda p, k: ctx.drift_kinetic_trace_open(p, k, qm, mp, dt, region, gradB_field=X.W0), "dk_trace_open"),
        "uniform_1": (lambda p, k: ctx.drift_kinetic_trace_collisional(p, k, qm, mp, dt, coll, None, region, gradB_field=X.W0),
                      "coll_dk_grid_trace"),
        "profile_1": (lambda p, k: ctx.drift_kinetic_trace_collisional(p, k, qm, mp, dt, coll, [0], region, gradB_field=X.W0),
                      "coll_dk_grid_trace"),
        "batch": gcs}}
    # the moments against the collisions, on the same sort; the profile the traces read is made here
    ms = {"background_from_sort": [], "collide": []}
    ctx.background_from_sort(0, sort)
    ctx.collide(sort, sort, 1e-9, 0, seed=1)
    for rep in range(args.reps):
        ms["background_from_sort"].append(timed(lambda: ctx.background_from_sort(0, sort), "background_from_sort")[1])
        ms["collide"].append(timed(lambda: ctx.collide(sort, sort, 1e-9, rep + 1, seed=1), "cmd_collide")[1])
        print(f"rep {rep} from_sort {ms['background_from_sort'][-1]:.3f} ms collide {ms['collide'][-1]:.3f} ms", file=sys.stderr,
              flush=True)
    ctx.background_from_sort(0, sort)
    m = {k: summary(v) for k, v in ms.items()}
    velocity_bytes = 2 * 3 * 8 * records  # three velocity arrays, read in both passes
    m["velocity_bytes_two_passes"] = velocity_bytes
    m["from_sort_GBps_of_velocity_traffic"] = velocity_bytes / (m["background_from_sort"]["median_ms"] * 1e6)
    m["ratio_from_sort_to_collide"] = m["background_from_sort"]["median_ms"] / m["collide"]["median_ms"]
    res["moments_vs_collide"] = m
    sides = ("open", "uniform_1", "profile_1")
    for name, P in pushers.items():
        batch = P["batch"]
        for side in sides:
            P[side][0](batch[:4096], 4)
        t = {side: [] for side in sides}
        made = {}
        for rep in range(args.reps):
            for side in sides:
                call, section = P[side]
                out, x = timed(lambda: call(batch, args.steps), section)
                t[side].append(x)
                if side != "open":
                    made[side] = float(out.coll[0] + out.coll[1])
                print(f"{name} rep {rep} {side}: {x:.1f} ms", file=sys.stderr, flush=True)
        r = {"cases": {side: dict(summary(v), ns_per_particle_step=float(np.median(v)) * 1e6 / (float(npart) * args.steps))
                       for side, v in t.items()}}
        base = r["cases"]["open"]["median_ms"]
        for side in sides[1:]:
            r["ratio_%s_to_open" % side] = r["cases"][side]["median_ms"] / base
            r["ns_per_collision_%s" % side] = (r["cases"][side]["median_ms"] - base) * 1e6 / max(made[side], 1.0)
        r["largest_spread"] = max(c["spread"] for c in r["cases"].values())
        res["pushers"][name] = r
    ctx.close()
    res["open_is"] = ("xpic_full_orbit_trace_open / xpic_drift_kinetic_trace_open of this build, whose kernels and file are the "
                      "parent commit's, same batch and field, same process, alternating with the collisional grid traces")
    print(json.dumps(res, indent=1))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", action="store_true", help="time the collisional grid traces and the moments of a sort")
    ap.add_argument("--cells", type=int, default=64)
    ap.add_argument("--ppc", type=int, default=64)
    ap.add_argument("--particles", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--omega-dt", type=float, default=0.1)
    ap.add_argument("--every", type=int, default=1)
    ap.add_argument("--commit", default=None, help="the commit the library was built from (default: git's HEAD, if any)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "collisional_grid_trace_time.json" if args.grid else "collisional_trace_time.json")
    if args.grid:
        return grid_main(args)
    ctx = X.Context("basic", (8, 8, 8), (0.1,) * 3, 1.0, device=0)
    model = X.field_model("gaussian_mirror", **GAUSSIAN)
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
    vth = 0.1 / np.sqrt(3.0)
    bgs = [dict(q=-1.0, m=1.0, n=1.0, vth=vth), dict(q=1.0, m=1836.0, n=1.0, vth=vth / np.sqrt(1836.0))]
    strength = 1e-3 * 0.25 * 0.1 ** 3 / (args.every * dt)  # sigma^2 = S n dt_c / (m_ab^2 u^3), m_ab = 1 / 2
    colls = {k: X.trace_collisions(bgs[:k], strength=strength, mass=1.0, every=args.every, seed=5) for k in (1, 2)}
    bw = ctx.probe_copy_bandwidth(1 << 30, 10)
    launches = (args.steps + X.MODEL_LAUNCH_STEPS - 1) // X.MODEL_LAUNCH_STEPS
    res = {"commit": args.commit or commit(), "particles": npart, "steps": args.steps, "dt": dt, "omega_dt": args.omega_dt,
           "every": args.every, "reps": args.reps, "launch_steps": X.MODEL_LAUNCH_STEPS, "model": dict(GAUSSIAN),
           "backgrounds": bgs, "strength": strength, "copy_GBps": bw / 1e9, "pushers": {}}

    def timed(call, section):
        ctx.profile_enable(True)
        ctx.profile_reset()
        out = call()
        ms = ctx.profile_get(section)[1]
        ctx.profile_enable(False)
        return out, ms

    def fo(scheme):
        return {
            "model": (lambda p, k: ctx.model_full_orbit_trace(p, k, scheme, qm, dt, model), "model_fo_trace"),
            "collisional_1": (lambda p, k: ctx.model_full_orbit_trace_collisional(p, k, scheme, qm, dt, model, colls[1]),
                              "coll_fo_trace"),
            "collisional_2": (lambda p, k: ctx.model_full_orbit_trace_collisional(p, k, scheme, qm, dt, model, colls[2]),
                              "coll_fo_trace"),
            "batch": pts}
    pushers = {"EB2B": fo("EB2B"), "CN": fo("CN"), "drift_kinetic": {
        "model": (lambda p, k: ctx.model_drift_kinetic_trace(p, k, qm, mp, dt, model), "model_dk_trace"),
        "collisional_1": (lambda p, k: ctx.model_drift_kinetic_trace_collisional(p, k, qm, mp, dt, model, colls[1]),
                          "coll_dk_trace"),
        "collisional_2": (lambda p, k: ctx.model_drift_kinetic_trace_collisional(p, k, qm, mp, dt, model, colls[2]),
                          "coll_dk_trace"),
        "batch": gcs}}
    sides = ("model", "collisional_1", "collisional_2")
    for name, P in pushers.items():
        batch = P["batch"]
        for side in sides:  # warm-up: every kernel of the timed window, once
            P[side][0](batch[:4096], 4)
        ms = {side: [] for side in sides}
        coll = {}
        for rep in range(args.reps):  # alternating: a drift of the box over the run falls on all sides alike
            for side in sides:
                call, section = P[side]
                out, t = timed(lambda: call(batch, args.steps), section)
                ms[side].append(t)
                if side != "model":
                    coll[side] = [float(x) for x in out.coll]
                print(f"{name} rep {rep} {side}: {t:.1f} ms", file=sys.stderr, flush=True)
        r = {"cases": {}}
        for side, v in ms.items():
            med = float(np.median(v))
            r["cases"][side] = {"kernel_ms": v, "median_ms": med, "spread": (max(v) - min(v)) / med,
                                "median_ms_per_launch_of_64": med / launches,
                                "ns_per_particle_step": med * 1e6 / (float(npart) * args.steps)}
            if side in coll:
                r["cases"][side]["coll_4"] = coll[side]
                r["cases"][side]["mean_sigma2"] = coll[side][2] / max(coll[side][0], 1.0)
        base = r["cases"]["model"]["median_ms"]
        for k in (1, 2):
            c = r["cases"]["collisional_%d" % k]
            r["ratio_collisional_%d_to_model" % k] = c["median_ms"] / base
            made = c["coll_4"][0] + c["coll_4"][1]
            r["ns_per_collision_%d" % k] = (c["median_ms"] - base) * 1e6 / max(made, 1.0)
        r["largest_spread"] = max(c["spread"] for c in r["cases"].values())
        res["pushers"][name] = r
    ctx.close()
    res["model_is"] = ("xpic_model_full_orbit_trace / xpic_model_drift_kinetic_trace of this build, whose kernels are the "
                       "parent commit's, same batch, same process, alternating with the collisional traces")
    print(json.dumps(res, indent=1))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
