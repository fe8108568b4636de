#!/usr/bin/env python3
"""Times the electrostatic scheme (include/xpic_es.h) at BASELINE configs[1]'s own size: 128^3 cells, two electron beams
(+-0.2 c along x) of 16 particles per cell each on the regular lattice of the synthetic loader, fp64, dx = 0.125, dt = 0.05.

Device times are the context's profile sections (event pairs around the launches), per launch = per sort:
  es_push         k_es_push: gather, kick, full move and the fused charge deposit
  charge_density  k_charge_density on the same particles -- with `move` (k_move) the parent commit's kernels for that work
  basic_push      k_esirkepov_push<0> of a `basic` context on the same load (the round table's kernel is inside the section)
and the solve's kernels (gauss_*).  Steps: the first from E = 0 (cold: the whole potential is solved for), then warm ones
(E^n is the start); iterations from xpic_step, wall time by time.perf_counter around the call (re-binning, reductions' round
trips and the host loop in it).  The in-process copy rate (xpic_probe_copy_bandwidth) stands beside them, and per particle
kernel the bytes a particle's record makes it move at least (96 B: r, v read and written) over that rate.
Prints one JSON object (profiles/es_time.json).
usage: es_time.py [--n 128] [--ppc 16] [--steps 10]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import xpic_amd as X  # noqa: E402

DX, DT, V0, VTH = 0.125, 0.05, 0.2, 1e-3
GAUSS = ("gauss_residual", "gauss_lap_dot", "gauss_update", "gauss_dir", "gauss_correct")


def beams(ctx, n, ppc):
    ids = []
    for b, sgn in enumerate((+1.0, -1.0)):
        s = ctx.add_sort(ppc, 0.5, -1.0, 1.0, capacity=int(ppc * n ** 3 * 1.2) + 1024)
        ctx.load_synthetic(s, ppc, VTH, seed=11 + b, profile="regular", drift=(sgn * V0, 0.0, 0.0))
        ids.append(s)
    return ids


def section(ctx, name):
    launches, ms = ctx.profile_get(name)
    return {"launches": launches, "ms_per_launch": ms / launches if launches else None}


def timed_step(ctx):
    ctx.synchronize()
    ctx.profile_enable(True)
    ctx.profile_reset()
    t0 = time.perf_counter()
    its = ctx.step()
    ctx.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    out = {"cg_iterations": its, "wall_ms": wall, "es_push": section(ctx, "es_push")}
    solve = 0.0
    for name in GAUSS:
        launches, ms = ctx.profile_get(name)
        solve += ms
        out[name] = section(ctx, name)
    out["solve_kernels_ms"] = solve
    ctx.profile_enable(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--ppc", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    n = a.n
    ctx = X.Context("es", (n, n, n), (DX,) * 3, DT, device=0)
    ids = beams(ctx, n, a.ppc)
    per_sort = ctx.count(ids[0])
    bw = ctx.probe_copy_bandwidth(1 << 30, 10)
    record_ms = 96.0 * per_sort / bw * 1e3
    out = {"argv": sys.argv[1:], "grid": f"{n}^3", "beams": 2, "ppc_per_beam": a.ppc, "particles_per_sort": per_sort,
           "dx": DX, "dt": DT, "copy_GBps": bw / 1e9, "record_copy_ms_per_sort": record_ms,
           "tolerances": {"rtol": X.ES_RTOL, "atol": X.ES_ATOL, "maxit": X.ES_MAXIT}}
    out["cold_step_from_zero_field"] = timed_step(ctx)
    warm = [timed_step(ctx) for _ in range(a.steps)]
    out["warm_steps"] = warm
    out["warm_mean"] = {"cg_iterations": sum(w["cg_iterations"] for w in warm) / len(warm),
                        "wall_ms": sum(w["wall_ms"] for w in warm) / len(warm),
                        "es_push_ms_per_sort": sum(w["es_push"]["ms_per_launch"] for w in warm) / len(warm),
                        "solve_kernels_ms": sum(w["solve_kernels_ms"] for w in warm) / len(warm)}
    # the parent commit's kernels for the push's move and deposit, on the same particles
    ctx.profile_enable(True)
    ctx.profile_reset()
    for _ in range(3):
        for s in ids:
            ctx.charge_density(s)
    out["charge_density"] = section(ctx, "charge_density")
    ctx.profile_reset()
    for s in ids:
        ctx.ecsim_first_push(s)  # k_move by dt
    out["move"] = section(ctx, "move")
    ctx.profile_enable(False)
    ctx.close()
    # the basic scheme's push on the same load
    b = X.Context("basic", (n, n, n), (DX,) * 3, DT, device=0)
    bid = beams(b, n, a.ppc)
    for s in bid:
        b.basic_push(s)  # (warm-up: the round table)
        b.update_cells(s)
    b.profile_enable(True)
    b.profile_reset()
    for _ in range(3):
        for s in bid:
            b.basic_push(s)
            b.update_cells(s)
    out["basic_push"] = section(b, "basic_push")
    b.close()
    es = out["warm_mean"]["es_push_ms_per_sort"]
    out["ratios"] = {"es_push_over_charge_density": es / out["charge_density"]["ms_per_launch"],
                     "es_push_over_charge_density_plus_move": es / (out["charge_density"]["ms_per_launch"] + out["move"]["ms_per_launch"]),
                     "es_push_over_basic_push": es / out["basic_push"]["ms_per_launch"],
                     "es_push_over_record_copy": es / record_ms}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
