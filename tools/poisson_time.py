#!/usr/bin/env python3
"""Times the two Poisson solves (include/xpic_poisson.h: "cg" and "direct") on the same context and load:

  clean    ecsim contexts of n^3 nodes with one electron sort in the `blob` profile (tools/gauss_clean_time.py's load, DESIGN.md
           5za): the clean from E = 0 with each solver -- E is zeroed again in between, the charge is the same deposit
  es       the electrostatic scheme at 128^3 with two beams (tools/es_time.py's load): a cold step, warm steps
           with CG, warm steps with the direct solve

Device times are the context's profile sections (event pairs around the launches): gauss_* for CG's kernels,
poisson_pass_x / _y / _z for the direct solve's axis passes (two launches of each per application: forward and back).  A
pass reads one scalar and writes one; it stands beside the time a copy of two scalar vectors takes at the copy rate measured
in the same process (xpic_probe_copy_bandwidth: bytes read plus bytes written per second), as the sections of DESIGN.md 5za
and 5zb take it.  wall: time.perf_counter around the call, the charge deposit and every host round trip in it; the deposit
alone is timed by a residual call.
Writes one JSON object (profiles/poisson_time.json).
usage: poisson_time.py [--sizes 128 256] [--ppc 64 8] [--es-n 128] [--es-ppc 16] [--steps 3] [--out profiles/poisson_time.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import xpic_amd as X  # noqa: E402

CG = ("gauss_lap_dot", "gauss_update", "gauss_dir")
PASSES = ("poisson_pass_x", "poisson_pass_y", "poisson_pass_z")
AROUND = ("gauss_residual", "gauss_correct", "es_push")  # (es_push: one launch per sort)


def sections(ctx, nodes, bw):
    out, solve = {}, 0.0
    for name in CG + PASSES + AROUND:
        launches, ms = ctx.profile_get(name)
        if not launches:
            continue
        out[name] = {"launches": launches, "ms_per_launch": ms / launches}
        if name in PASSES:
            copy = 2 * 8.0 * nodes / bw * 1e3
            out[name].update(copy_ms=copy, fraction_of_copy_rate=copy / (ms / launches))
        if name not in AROUND:
            solve += ms
    out["solve_kernels_ms"] = solve
    return out


def timed(ctx, nodes, bw, call):
    ctx.synchronize()
    ctx.profile_enable(True)
    ctx.profile_reset()
    t0 = time.perf_counter()
    its = call()
    ctx.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    out = {"iterations": its, "wall_ms": wall, **sections(ctx, nodes, bw)}
    ctx.profile_enable(False)
    return out


def clean_case(n, ppc, rtol):
    ctx = X.Context("ecsim", (n, n, n), (0.5,) * 3, 0.5, device=0)
    nodes = n ** 3
    s = ctx.add_sort(ppc, 1.0, -1.0, 1.0, capacity=int(ppc * nodes * 1.3) + 1024)
    ctx.load_synthetic(s, ppc, 0.05, seed=3, profile="blob", param=(0.5, n / 8.0))
    bw = ctx.probe_copy_bandwidth(1 << 30, 10)
    out = {"grid": f"{n}^3", "ppc": ppc, "particles": ctx.count(s), "copy_GBps": bw / 1e9, "rtol": rtol}
    ctx.gauss_residual()  # (allocates the solve's vectors, warms the kernels up)
    t0 = time.perf_counter()
    ctx.gauss_residual()
    out["residual_call_with_deposit_wall_ms"] = (time.perf_counter() - t0) * 1e3
    ctx.poisson_apply(ctx.charge_density(s))  # (builds the tables, warms the pass kernel up)
    for solver in ("cg", "direct", "cg", "direct"):  # each twice, alternating: the second of each is the one to quote
        ctx.vec_set(X.E, 0.0)
        ctx.set_poisson_solver(solver)
        r = timed(ctx, nodes, bw, lambda: ctx.gauss_clean(X.E, rtol=rtol, maxit=100000))
        clean = r.pop("iterations")
        r.update(iterations=clean.iterations, before=clean.before, after=clean.after,
                 wall_ms_less_deposit=r["wall_ms"] - out["residual_call_with_deposit_wall_ms"])  # (a clean deposits once)
        out.setdefault("clean_from_zero_field_" + solver, []).append(r)
    ctx.close()
    return out


def es_case(n, ppc, steps):
    dx, dt, v0, vth = 0.125, 0.05, 0.2, 1e-3  # tools/es_time.py
    ctx = X.Context("es", (n, n, n), (dx,) * 3, dt, device=0)
    nodes = n ** 3
    for b, sgn in enumerate((+1.0, -1.0)):
        s = ctx.add_sort(ppc, 0.5, -1.0, 1.0, capacity=int(ppc * nodes * 1.2) + 1024)
        ctx.load_synthetic(s, ppc, vth, seed=11 + b, profile="regular", drift=(sgn * v0, 0.0, 0.0))
    bw = ctx.probe_copy_bandwidth(1 << 30, 10)
    out = {"grid": f"{n}^3", "beams": 2, "ppc_per_beam": ppc, "copy_GBps": bw / 1e9,
           "tolerances": {"rtol": X.ES_RTOL, "atol": X.ES_ATOL, "maxit": X.ES_MAXIT}}

    def step():
        return timed(ctx, nodes, bw, ctx.step)
    out["cold_step_cg"] = step()
    out["warm_steps_cg"] = [step() for _ in range(steps)]
    ctx.set_poisson_solver("direct")
    out["warm_steps_direct"] = [step() for _ in range(steps + 1)]  # (the first builds the tables)
    ctx.set_poisson_solver("cg")
    out["warm_steps_cg_again"] = [step() for _ in range(steps)]
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[128, 256])
    ap.add_argument("--ppc", type=int, nargs="+", default=[64, 8], help="one value, or one per size")
    ap.add_argument("--rtol", type=float, default=1e-10)
    ap.add_argument("--es-n", type=int, default=128, help="0: no es case")
    ap.add_argument("--es-ppc", type=int, default=16)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poisson_time.json"))
    a = ap.parse_args()
    ppc = a.ppc * len(a.sizes) if len(a.ppc) == 1 else a.ppc
    assert len(ppc) == len(a.sizes), "--ppc takes one value or one per size"
    argv = sys.argv[1:]
    if "--out" in argv:  # (where the file went is no parameter of the measurement)
        del argv[argv.index("--out"):argv.index("--out") + 2]
    out = {"argv": argv, "clean": [clean_case(n, p, a.rtol) for n, p in zip(a.sizes, ppc)]}
    if a.es_n:
        out["es"] = es_case(a.es_n, a.es_ppc, a.steps)
    text = json.dumps(out, indent=1)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
