#!/usr/bin/env python3
"""Times what the tracer sets add (include/xpic_tracers.h).

(a) xpic_grad_abs_field at 128^3 and 256^3: kernel time from the context's profile section "grad_abs_field", as GB/s of
    the 48 bytes per node it must move (24 read, 24 written), beside xpic_probe_copy_bandwidth of the same process, both
    repeated --reps times; the spread of each is (max - min) / median.
(b) an ecsim run of --steps steps on 64^3 cells x 8 particles per cell with --tracers test particles, wall time per step
    (synchronised), for: no tracers; an attached full-orbit (B1B) set; the same batch driven from the host, one
    xpic_full_orbit_trace_open(steps = 1, step0 = k) after every step; an attached guiding-centre set with XPIC_GRADB_AUTO;
    and its host-driven form: xpic_field_get(B), grad |B| in numpy, xpic_field_set(W0), one-step
    xpic_drift_kinetic_trace_open.  The host-driven forms go through the package, as a user's would.
Prints one JSON object and writes it to --out (default profiles/tracers_time.json)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import xpic_amd as X  # noqa: E402


def stats(v):
    med = float(np.median(v))
    return {"values": [float(x) for x in v], "median": med, "spread": float((max(v) - min(v)) / med)}


def gradient(n, reps):
    ctx = X.Context("ecsim", (n, n, n), (0.5, 0.5, 0.5), 1.0, device=0)
    rng = np.random.default_rng(1)
    ctx.set_field(X.B, rng.normal(size=ctx.fshape()) + np.array([0.0, 0.0, 3.0]))
    ctx.grad_abs_field(X.B, X.W0)  # warm-up
    ctx.probe_copy_bandwidth(1 << 30, 2)
    nbytes = 48.0 * n ** 3
    grad, copy = [], []
    for _ in range(reps):  # alternating
        ctx.profile_enable(True)
        ctx.profile_reset()
        for _ in range(10):
            ctx.grad_abs_field(X.B, X.W0)
        launches, ms = ctx.profile_get("grad_abs_field")
        ctx.profile_enable(False)
        assert launches == 10
        grad.append(nbytes * launches / (ms * 1e-3) / 1e9)
        copy.append(ctx.probe_copy_bandwidth(1 << 30, 10) / 1e9)
    ctx.close()
    out = {"nodes": n ** 3, "bytes_per_launch": nbytes, "grad_abs_GBps": stats(grad), "copy_probe_GBps": stats(copy)}
    out["grad_over_copy"] = out["grad_abs_GBps"]["median"] / out["copy_probe_GBps"]["median"]
    return out


def run(case, args, fo, dk):
    n = args.n
    d = (0.5, 0.5, 0.5)
    ctx = X.Context("ecsim", (n, n, n), d, 0.5, device=0)
    for q, m in ((-1.0, 1.0), (1.0, 100.0)):
        s = ctx.add_sort(args.ppc // 2, 1.0, q, m, capacity=int(1.3 * (args.ppc // 2) * n ** 3))
        ctx.fill_synthetic(s, args.ppc // 2, 0.05 / np.sqrt(m), seed=3 + s)
    B0 = np.zeros(ctx.fshape()) + np.array([0.0, 0.0, 0.3])
    ctx.set_field(X.B, B0)
    ctx.set_field(X.B0, B0)
    everywhere = {"name": "box", "min": (-1e30,) * 3, "max": (1e30,) * 3}
    qm, mp, dt = -1.0, 1.0, 0.3
    state, ex, sets = None, None, []
    if case == "attached_fo":
        sets = [ctx.tracers("full_orbit", fo, "B1B", qm, dt, region=everywhere)]
    elif case == "attached_dk":
        sets = [ctx.tracers("drift_kinetic", dk, qm, mp, dt, region=everywhere, gradB_field="auto")]
    elif case == "host_fo":
        state, ex = fo, np.full(len(fo), -1, dtype=np.int64)
    elif case == "host_dk":
        state, ex = dk, np.full(len(dk), -1, dtype=np.int64)
    for s in sets:
        s.attach()
    times = []
    for k in range(args.warmup + args.steps):
        ctx.synchronize()
        t0 = time.perf_counter()
        ctx.step()
        if case == "host_fo":
            r = ctx.full_orbit_trace_open(state, 1, "B1B", qm, dt, everywhere, exit_step=ex, step0=k)
            state, ex = r.state, r.exit_step
        elif case == "host_dk":
            B = ctx.get_field(X.B)
            absB = np.sqrt((B * B).sum(axis=-1))
            ctx.set_field(X.W0, np.stack([(np.roll(absB, -1, axis=2 - a) - np.roll(absB, 1, axis=2 - a)) / (2 * d[a])
                                          for a in range(3)], axis=-1))
            r = ctx.drift_kinetic_trace_open(state, 1, qm, mp, dt, everywhere, gradB_field=X.W0, exit_step=ex, step0=k)
            state, ex = r.state, r.exit_step
        ctx.synchronize()
        if k >= args.warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    ctx.close()
    return stats(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--ppc", type=int, default=8)
    ap.add_argument("--tracers", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracers_time.json"))
    args = ap.parse_args()
    res = {"gradient": {f"{n}^3": gradient(n, args.reps) for n in (128, 256)}}
    rng = np.random.default_rng(9)
    L = args.n * 0.5
    r = L * rng.random((args.tracers, 3))
    fo = np.column_stack([r, rng.normal(0, 0.2, (args.tracers, 3))])
    dk = np.column_stack([r, rng.normal(0, 0.2, args.tracers), 0.1 + 0.2 * rng.random(args.tracers),
                          0.05 + 0.05 * rng.random(args.tracers)])
    ride = {"grid": f"{args.n}^3", "ppc": args.ppc, "tracers": args.tracers, "steps": args.steps, "warmup": args.warmup,
            "step_ms": {}}
    for case in ("no_tracers", "attached_fo", "host_fo", "attached_dk", "host_dk"):
        ride["step_ms"][case] = run(case, args, fo, dk)
        print(case, ride["step_ms"][case]["median"], file=sys.stderr, flush=True)
    base = ride["step_ms"]["no_tracers"]["median"]
    for kind in ("fo", "dk"):
        a, h = ride["step_ms"]["attached_" + kind]["median"], ride["step_ms"]["host_" + kind]["median"]
        ride[kind] = {"attached_adds_ms": a - base, "host_driven_adds_ms": h - base, "host_over_attached_added": (h - base) / (a - base)}
    ride["note"] = ("wall time per step, synchronised; every case is its own context and its own run of the plasma (the "
                    "deposits' floating-point atomics make two runs differ in the last bits, so the final tracer states of "
                    "two cases are not compared here; tests/test_gpu_tracers.py compares them inside one context)")
    res["ride"] = ride
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
