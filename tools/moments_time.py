#!/usr/bin/env python3
"""Times the particle diagnostics (xpic_moment, xpic_velocity_distribution) on the headline state: ECSIM, 256^3 x 64 per cell from load_synthetic, after one step (the records in the step's own order).

Kernel time only, from the context's named profile sections ("moment", "velocity_distribution"); the
copy-out to the host is not counted.  Each time is also given as a multiple of the floor = the bytes of one read of the
records (24 B per particle for the density: r; 48 B for the other moments: r and v; 24 B for vx_vy: v) at the measured
device copy rate.  Prints
one JSON object.  Run it under `rocprofv3 --kernel-trace --stats -- python tools/moments_time.py` for the kernel table.
usage: moments_time.py [--n 256] [--ppc 64] [--reps 3]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import xpic_amd as X  # noqa: E402

MOMENTS = ("density", "current", "momentum_flux", "momentum_flux_diag", "momentum_flux_cyl", "momentum_flux_diag_cyl")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--ppc", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--vth", type=float, default=0.014)  # bench.py's default
    args = ap.parse_args()
    n = args.n
    ctx = X.Context("ecsim", (n, n, n), (0.5,) * 3, 1.0, device=0)
    Np, dens, q, m = args.ppc, 1.0, -1.0, 1.0
    s = ctx.add_sort(Np, dens, q, m, capacity=int(Np * ctx.N * 1.02) + 1024)
    ctx.load_synthetic(s, Np, args.vth, seed=1234)
    B = np.zeros(ctx.fshape())
    B[..., 2] = 0.2
    ctx.set_field(X.B, B)
    ctx.set_field(X.B0, B)
    del B
    ctx.step()
    npart = ctx.count(s)
    res = {"grid": f"{n}^3", "ppc": args.ppc, "particles": npart, "reps": args.reps}
    try:  # the headroom the diagnostics have next to the context (hipMemGetInfo of the device the context uses)
        import ctypes

        hip = ctypes.CDLL("libamdhip64.so")
        free, total = ctypes.c_size_t(), ctypes.c_size_t()
        assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
        res["hbm_free_GB"], res["hbm_total_GB"] = free.value / 1e9, total.value / 1e9
    except Exception as e:  # noqa: BLE001 -- informative only
        res["hbm_free_GB"] = repr(e)
    bw = ctx.probe_copy_bandwidth(1 << 30, 10)
    res["copy_GBps"] = bw / 1e9

    def timed(section, call, nbytes):
        call()  # warm-up (and the LDS attribute of the first launch)
        ctx.synchronize()
        ctx.profile_enable(True)
        ctx.profile_reset()
        for _ in range(args.reps):
            call()
        ctx.synchronize()
        launches, ms = ctx.profile_get(section)
        ctx.profile_enable(False)
        per = ms / max(launches, 1)
        floor = nbytes / bw * 1e3
        return {"ms": per, "launches_per_call": launches / args.reps, "floor_ms": floor, "x_floor": per / floor}

    out = {}
    for name in MOMENTS:
        out[name] = timed("moment", lambda: ctx.moment(s, name), npart * (24 if name == "density" else 48))
    box = {"name": "box", "min": (0.0, 0.0, 0.0), "max": (n * 0.5,) * 3}
    v = 4 * args.vth
    for label, dv in (("vx_vy, LDS path", v / 20), ("vx_vy, global path", v / 200)):
        sz = int(round(2 * v / dv)) ** 2
        out[f"{label} ({sz} bins)"] = timed("velocity_distribution",
                                            lambda: ctx.velocity_distribution(s, "vx_vy", box, (-v, -v), (v, v), (dv, dv)),
                                            npart * 24)  # vx_vy reads the velocities only
    res["times"] = out
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
