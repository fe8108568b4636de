#!/usr/bin/env python3
"""Times the Gauss-law cleaner (include/xpic_gauss.h) on ecsim contexts of n^3 nodes with one electron sort in the `blob`
profile: the residual pass, one CG iteration split by kernel, a whole clean from E = 0 (the electrostatic start), and a whole
clean of the error one ecsim step leaves behind a clean field, twice (the first step still carries the start's transient).

Device times are the context's profile sections (event pairs around the launches): gauss_residual, gauss_lap_dot,
gauss_update, gauss_dir, gauss_correct, summed over a clean and divided by the launches.  Each stands beside the time a
copy of the same number of scalar vectors takes at the copy rate measured in the same process (xpic_probe_copy_bandwidth:
bytes read plus bytes written per second), and k_lap_dot beside k_cg_apply_dot, the kernel xpic_solve's CG on matM runs
for the same access pattern on 3-vectors (section matM_apply, which also holds that call's second-stage reduction and
its 8-byte copy back: the comparison flatters k_lap_dot by that much).  wall: time.perf_counter around the call, with the
charge deposit, the reductions' round trips and the halo-free host loop in it.
Prints one JSON object (profiles/gauss_clean_time.json).
usage: gauss_clean_time.py [--sizes 128 256] [--ppc 64 | --ppc 64 64] [--rtol 1e-10]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import xpic_amd as X  # noqa: E402

# scalar vectors a launch moves (read + written)
VECTORS = {"gauss_residual": 5, "gauss_lap_dot": 2, "gauss_update": 6, "gauss_dir": 3, "gauss_correct": 7}


def sections(ctx, nodes, bw):
    out = {}
    for name, v in VECTORS.items():
        launches, ms = ctx.profile_get(name)
        if launches:
            per = ms / launches
            copy = v * 8.0 * nodes / bw * 1e3
            out[name] = {"launches": launches, "ms_per_launch": per, "scalar_vectors": v, "copy_ms": copy,
                         "fraction_of_copy_rate": copy / per}
    return out


def timed_clean(ctx, nodes, bw, rtol):
    ctx.synchronize()
    ctx.profile_enable(True)
    ctx.profile_reset()
    t0 = time.perf_counter()
    r = ctx.gauss_clean(X.E, rtol=rtol, maxit=100000)
    ctx.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    sec = sections(ctx, nodes, bw)
    ctx.profile_enable(False)
    it_ms = sum(sec[k]["ms_per_launch"] for k in ("gauss_lap_dot", "gauss_update", "gauss_dir") if k in sec)
    return {"iterations": r.iterations, "before": r.before, "after": r.after, "wall_ms": wall, "kernels": sec,
            "iteration_kernels_ms": it_ms, "iteration_copy_ms": 11 * 8.0 * nodes / bw * 1e3,
            "wall_ms_per_iteration": wall / max(r.iterations, 1)}


def size(n, ppc, rtol):
    d = 0.5
    ctx = X.Context("ecsim", (n, n, n), (d,) * 3, 0.5, device=0)
    nodes = n ** 3
    s = ctx.add_sort(ppc, 1.0, -1.0, 1.0, capacity=int(ppc * nodes * 1.3) + 1024)
    ctx.load_synthetic(s, ppc, 0.05, seed=3, profile="blob", param=(0.5, n / 8.0))
    bw = ctx.probe_copy_bandwidth(1 << 30, 10)
    out = {"grid": f"{n}^3", "ppc": ppc, "particles": ctx.count(s), "copy_GBps": bw / 1e9, "rtol": rtol}
    ctx.gauss_residual()  # (allocates the solve's vectors, warms the kernels up)
    ctx.profile_enable(True)
    ctx.profile_reset()
    t0 = time.perf_counter()
    for _ in range(5):
        ctx.gauss_residual()
    ctx.synchronize()
    out["residual"] = {"wall_ms_with_deposit": (time.perf_counter() - t0) * 1e3 / 5, **sections(ctx, nodes, bw)["gauss_residual"]}
    ctx.profile_enable(False)
    out["clean_from_zero_field"] = timed_clean(ctx, nodes, bw, rtol)
    ctx.set_tolerances(1e-7, 1e-7, 200)
    ctx.step()
    out["clean_after_one_ecsim_step"] = timed_clean(ctx, nodes, bw, rtol)
    # the case `every = 1` meets: the error ONE step leaves behind a field that was clean when the step began
    ctx.step()
    out["clean_after_one_step_from_clean"] = timed_clean(ctx, nodes, bw, rtol)
    # k_cg_apply_dot on the same grid: a few iterations of xpic_solve's CG on matM
    ctx.set_field(X.W0, np.random.default_rng(1).normal(size=ctx.fshape()))
    ctx.profile_enable(True)
    ctx.profile_reset()
    its = ctx.solve(X.OP_MATM_CG, X.W0, X.W1, rtol=1e-6, atol=1e-50, maxit=200)[0]
    launches, ms = ctx.profile_get("matM_apply")
    ctx.profile_enable(False)
    per = ms / launches
    lap = out["clean_from_zero_field"]["kernels"]["gauss_lap_dot"]["ms_per_launch"]
    out["cg_apply_dot"] = {"iterations": its, "launches": launches, "ms_per_launch": per, "scalar_vectors": 6,
                           "ns_per_byte": per * 1e6 / (6 * 8.0 * nodes), "fraction_of_copy_rate": 6 * 8.0 * nodes / bw * 1e3 / per}
    out["lap_dot_ns_per_byte"] = lap * 1e6 / (2 * 8.0 * nodes)
    out["lap_dot_rate_over_cg_apply_dot_rate"] = out["cg_apply_dot"]["ns_per_byte"] / out["lap_dot_ns_per_byte"]
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--ppc", type=int, nargs="+", default=[64], help="one value, or one per size")
    ap.add_argument("--rtol", type=float, default=1e-10)
    args = ap.parse_args()
    ppc = args.ppc * len(args.sizes) if len(args.ppc) == 1 else args.ppc
    assert len(ppc) == len(args.sizes), "--ppc takes one value or one per size"
    print(json.dumps({"argv": sys.argv[1:], "sizes": [size(n, p, args.rtol) for n, p in zip(args.sizes, ppc)]}, indent=1))


if __name__ == "__main__":
    main()
