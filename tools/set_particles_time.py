#!/usr/bin/env python3
"""Times a uniform box load with a Maxwellian momentum through xpic_set_particles at 64^3 x 64 and 128^3 x 64 per cell,
against two baselines: xpic_sort_load_synthetic on the same counts (the same job with its own generator: the yardstick of
the per-record cost), and, at 64^3 only, the host executable's mt19937 path (draw + xpic_sort_add_particles), taken as the
wall time of xpic_hip.out on a one-step config with the SetParticles preset on the host against the same config with
"device": true.

Every figure is the median of `--runs` alternating runs (device load, synthetic load, device load, ...) with the spread
(min, max).  wall: time.perf_counter around the call and a synchronize, i.e. kernels plus host; device: the context's
profile sections "cmd_set_particles" (the whole call), "cmd_set_count" and "cmd_set_write" (its two passes, summed over the
chunks).  bytes_per_record: the 48 B of a record written once, and the time that takes at the measured device copy rate.
Prints one JSON object (profiles/set_particles_time.json).
usage: set_particles_time.py [--sizes 64 128] [--ppc 64] [--runs 5] [--no-host]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import xpic_amd as X  # noqa: E402


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": len(v)}


def device_size(n, ppc, runs):
    d = 0.5
    L = (n * d,) * 3
    ctx = X.Context("ecsim", (n, n, n), (d,) * 3, 1.0, device=0)
    s = ctx.add_sort(ppc, 1.0, -1.0, 1.0, capacity=int(ppc * ctx.N * 1.25) + 1024)
    box = {"name": "CoordinateInBox", "min": (0.0, 0.0, 0.0), "max": L}
    mom = {"name": "MaxwellianMomentum", "T": (0.1, 0.1, 0.1), "tov": True}
    count = ctx.particles_number(s, box)
    bw = ctx.probe_copy_bandwidth(1 << 30, 10)
    vth = (0.1 / 511.0) ** 0.5
    wall = {"set_particles": [], "load_synthetic": []}
    dev = {"cmd_set_particles": [], "cmd_set_count": [], "cmd_set_write": []}
    for run in range(runs + 1):  # (run 0 warms both up and is dropped)
        for name in ("set_particles", "load_synthetic"):
            ctx.clear(s)
            ctx.synchronize()
            ctx.profile_enable(True)
            ctx.profile_reset()
            t0 = time.perf_counter()
            if name == "set_particles":
                added, _ = ctx.set_particles(s, count, box, mom, seed=run)
            else:
                ctx.load_synthetic(s, ppc, vth, seed=run + 1)
            ctx.synchronize()
            t1 = time.perf_counter()
            if name == "set_particles":
                assert added == count == ctx.count(s)
                sections = {k: ctx.profile_get(k)[1] for k in dev}
            ctx.profile_enable(False)
            if run:
                wall[name].append((t1 - t0) * 1e3)
                if name == "set_particles":
                    for k in dev:
                        dev[k].append(sections[k])
    records = ctx.count(s)
    out = {"grid": f"{n}^3", "ppc": ppc, "particles": count, "synthetic_records": records, "copy_GBps": bw / 1e9,
           "wall_ms": {k: stats(v) for k, v in wall.items()}, "device_ms": {k: stats(v) for k, v in dev.items()}}
    sp, ls = out["wall_ms"]["set_particles"]["median"], out["wall_ms"]["load_synthetic"]["median"]
    out["ns_per_record"] = {"set_particles": sp * 1e6 / count, "load_synthetic": ls * 1e6 / records}
    out["x_load_synthetic_per_record"] = out["ns_per_record"]["set_particles"] / out["ns_per_record"]["load_synthetic"]
    floor = 48 * count / bw * 1e3
    out["bytes_per_record"] = 48
    out["write_floor_ms"] = floor
    out["x_write_floor"] = sp / floor
    ctx.close()
    return out


def host_path(n, ppc, runs):
    """wall time of the host executable on one ECSIM step of n^3 x ppc: the preset drawn on the host, and on the device"""
    exe = os.path.join(ROOT, "xpic_amd", "host", "xpic_hip.out")
    L = n * 0.5
    wall = {"host": [], "device": []}
    with tempfile.TemporaryDirectory() as tmp:
        for name in wall:
            cfg = {"Simulation": "ecsim", "OutputDirectory": os.path.join(tmp, name),
                   "Geometry": {"x": L, "y": L, "z": L, "t": 1.0, "dx": 0.5, "dy": 0.5, "dz": 0.5, "dt": 1.0, "diagnose_period": 1.0,
                                "da_boundary_x": "DM_BOUNDARY_PERIODIC", "da_boundary_y": "DM_BOUNDARY_PERIODIC",
                                "da_boundary_z": "DM_BOUNDARY_PERIODIC"},
                   "Particles": [{"sort_name": "electrons", "Np": ppc, "n": 1.0, "q": -1.0, "m": 1.0, "T": 0.1}],
                   "Presets": [{"command": "SetParticles", "particles": "electrons", "coordinate": {"name": "CoordinateInBox"},
                                "momentum": {"name": "MaxwellianMomentum", "tov": True}, "device": name == "device"}],
                   "Diagnostics": []}
            with open(os.path.join(tmp, name + ".json"), "w") as f:
                json.dump(cfg, f)
        for run in range(runs):
            for name in wall:
                t0 = time.perf_counter()
                subprocess.run([exe, os.path.join(tmp, name + ".json")], check=True, capture_output=True, timeout=600)
                wall[name].append((time.perf_counter() - t0) * 1e3)
    out = {"grid": f"{n}^3", "ppc": ppc, "executable_wall_ms": {k: stats(v) for k, v in wall.items()}}
    out["host_minus_device_ms"] = out["executable_wall_ms"]["host"]["median"] - out["executable_wall_ms"]["device"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--ppc", type=int, default=64)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    res = {"runs": args.runs, "sizes": [device_size(n, args.ppc, args.runs) for n in args.sizes]}
    if not args.no_host:
        res["host_path_64"] = host_path(64, args.ppc, args.runs)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
