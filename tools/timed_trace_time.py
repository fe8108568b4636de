#!/usr/bin/env python3
"""Times the model traces with a time envelope (xpic_model_full_orbit_trace_timed) against the untimed model traces they
extend (xpic_model_full_orbit_trace), and runs the reference's crank_nicolson_push_ex3 at the step counts the test suite
leaves out.

Timing: the batch of tools/model_trace_time.py (the Gaussian mirror of drift_kinetic_push_ex9.cpp, one speed
0.1 with isotropic pitch angles within half a unit of the centre, Omega dt = 0.1, no region), EB2B and Crank-Nicolson.  Cases:
  untimed                      the model trace       profile section "model_fo_trace"
  constant / ramp / harmonic   the timed trace       profile section "timed_fo_trace"
  ... + sums                   the same with sums_4
every one warmed up, then --reps repeats alternating between the cases in one process; kernel time only, from the context's
profile sections (staging and copies are not counted).  The untimed traces are the kernels this build shares with its
parent commit and stand for it.  The constant case must return the untimed trace's bits (asserted).

Long ex3 runs: omega_dt = 1.0 (188 496 steps) and 0.1 (1 884 956 steps) on one lane with sums_4: whether the whole table
is within full_orbit_ref.table_bound(gold, 1e-11) and the two PetscChecks hold at the reference's bounds, and the wall time.
Nothing is asserted about a time.  Prints one JSON object and writes it to profiles/timed_trace_time.json.
usage: timed_trace_time.py [--particles 1048576] [--steps 1024] [--reps 3] [--omega-dt 0.1] [--no-ex3]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import full_orbit_ref as FO  # noqa: E402
import timed_trace_ref as T  # noqa: E402
import xpic_amd as X  # noqa: E402

GAUSSIAN = dict(B_min=1.0, B_max=4.0, L=5.0, W=1.0)  # tests/drift_kinetic_push/drift_kinetic_push.h:74-77
GOLD = os.path.join(ROOT, "tests", "golden", "crank_nicolson_push_ex3")


def commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              timeout=10).stdout.strip() or None
    except OSError:
        return None


def timing(ctx, args):
    model = X.field_model("gaussian_mirror", **GAUSSIAN)
    rng = np.random.default_rng(7)
    npart = args.particles
    mu = 2.0 * rng.random(npart) - 1.0  # cosine of the pitch angle: isotropic
    phi = 2 * np.pi * rng.random(npart)
    s = np.sqrt(1.0 - mu * mu)
    pts = np.empty((npart, 6))
    pts[:, :3] = GAUSSIAN["L"] + (rng.random((npart, 3)) - 0.5)
    pts[:, 3:] = 0.1 * np.column_stack([s * np.cos(phi), s * np.sin(phi), mu])
    qm = -1.0
    dt = args.omega_dt / ctx.model_fields(model, [[GAUSSIAN["L"]] * 3])[1][0, 2]  # Omega = Bz at the centre
    envelopes = {"constant": X.field_envelope("constant"), "ramp": X.field_envelope("ramp", a=0.5, b=0.3),
                 "harmonic": X.field_envelope("harmonic", omega=1.7, phase=0.4)}
    res = {"particles": npart, "steps": args.steps, "dt": dt, "omega_dt": args.omega_dt, "reps": args.reps,
           "launch_steps": X.MODEL_LAUNCH_STEPS, "model": dict(GAUSSIAN), "schemes": {}}

    def timed(call, section):
        ctx.profile_enable(True)
        ctx.profile_reset()
        out = call()
        ms = ctx.profile_get(section)[1]
        ctx.profile_enable(False)
        return out, ms

    for scheme in ("EB2B", "CN"):
        cases = {"untimed": (lambda p, k: ctx.model_full_orbit_trace(p, k, scheme, qm, dt, model).state, "model_fo_trace")}
        for ename, env in envelopes.items():
            for sums in (None, True):
                cases[ename + (" + sums" if sums else "")] = (
                    lambda p, k, env=env, sums=sums: ctx.model_full_orbit_trace_timed(p, k, scheme, qm, dt, model, env,
                                                                                      sums=sums).state, "timed_fo_trace")
        for call, _ in cases.values():  # warm-up: every kernel of the timed window, once
            call(pts[:4096], 4)
        ms = {name: [] for name in cases}
        outs = {}
        for rep in range(args.reps):  # alternating: a drift of the box over the run falls on every case alike
            for name, (call, section) in cases.items():
                outs[name], t = timed(lambda: call(pts, args.steps), section)
                ms[name].append(t)
                print(f"{scheme} rep {rep} {name}: {t:.1f} ms", file=sys.stderr, flush=True)
        assert outs["constant"].tobytes() == outs["untimed"].tobytes()
        assert outs["constant + sums"].tobytes() == outs["untimed"].tobytes()
        r = {"cases": {}}
        base = float(np.median(ms["untimed"]))
        for name, v in ms.items():
            med = float(np.median(v))
            r["cases"][name] = {"kernel_ms": v, "median_ms": med, "spread": (max(v) - min(v)) / med,
                                "ns_per_particle_step": med * 1e6 / (float(npart) * args.steps), "ratio_to_untimed": med / base}
        r["largest_spread"] = max(c["spread"] for c in r["cases"].values())
        res["schemes"][scheme] = r
    res["untimed_is"] = ("xpic_model_full_orbit_trace of this build, whose kernels are the parent commit's, same batch, same "
                         "process, alternating with the timed traces")
    return res


def ex3(ctx, omega_dt):
    dt, nt, every = T.ex3_run(omega_dt)
    gold = np.loadtxt(os.path.join(GOLD, "omega_dt_%.1f.txt" % omega_dt), skiprows=1)
    t0 = time.perf_counter()
    out = ctx.model_full_orbit_trace_timed([T.EX3_START], nt + 1, "CN", T.EX3_QM, dt, X.field_model("uniform", **T.EX3_MODEL),
                                           X.field_envelope("ramp", a=0.0, b=1.0), sample_every=every, sums=True)
    wall = time.perf_counter() - t0
    mine = T.ex3_rows(T.EX3_START, out.samples, dt, every, len(gold))
    ratio = float((np.abs(mine - gold) / FO.table_bound(gold, 1e-11)).max()) if mine.shape == gold.shape else None
    energy, drift = T.ex3_checks(out.sums[0], dt, nt)
    return {"omega_dt": omega_dt, "steps": nt + 1, "launches": (nt + X.MODEL_LAUNCH_STEPS) // X.MODEL_LAUNCH_STEPS,
            "rows": len(gold), "largest_error_over_table_bound": ratio, "table_holds": ratio is not None and ratio <= 1.0,
            "energy_balance": float(energy), "energy_holds": bool(energy <= T.EX3_ENERGY_BOUND), "drift_error": float(drift),
            "drift_holds": bool(drift < T.EX3_DRIFT_BOUND), "iterations_max": int(out.iterations_max[0]), "wall_s": wall}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--omega-dt", type=float, default=0.1)
    ap.add_argument("--no-ex3", action="store_true")
    ap.add_argument("--commit", default=None, help="the commit the library was built from (default: git's HEAD, if any)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "timed_trace_time.json"))
    args = ap.parse_args()
    ctx = X.Context("basic", (8, 8, 8), (1.0, 1.0, 1.0), 1.0, device=0)  # no grid vector is read
    res = {"commit": args.commit or commit()}
    res["timing"] = timing(ctx, args)
    if not args.no_ex3:
        res["ex3"] = []
        for omega_dt in (1.0, 0.1):
            res["ex3"].append(ex3(ctx, omega_dt))
            print("ex3", res["ex3"][-1], file=sys.stderr, flush=True)
    ctx.close()
    print(json.dumps(res, indent=1))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
