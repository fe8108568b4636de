#!/usr/bin/env python3
"""Times the moments of a tracer set (include/xpic_tracer_moments.h): a full-orbit set of --tracers
particles (default 2^20) in a 64^3 box, density and momentum flux, uniform over the box and bunched into 4^3 cells.

(a) the map's deposit per step: kernel time from the context's profile sections "tracer_moment" (direct path) and
    "tracer_moment_lds", over --steps due steps of an advance, per deposit.  The whole box is 64^3 cells: its region does
    not fit the LDS budget and takes the direct path; the bunched ensemble is also timed with the 6^3-cell region around it,
    which fits and takes the LDS path.
(b) what the parent commit has: xpic_tracers_get (the 6 n doubles to the host, wall time, synchronised) plus a numpy deposit
    of the density (np.add.at over the 8 corners); and the same particles loaded into a sort and run through xpic_moment
    (wall time of the load and of the moment, and the moment's kernel time from the profile section "moment").
Every figure is repeated --reps times; the spread is (max - min) / median.  Prints one JSON object and writes it to --out
(default profiles/tracer_moments_time.json)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import xpic_amd as X  # noqa: E402

N, D = 64, 0.5
Q, M = -1.0, 1.0
NOWHERE = {"name": "box", "min": (-9.0, -9.0, -9.0), "max": (-8.0, -8.0, -8.0)}


def stats(v):
    med = float(np.median(v))
    return {"values": [float(x) for x in v], "median": med, "spread": float((max(v) - min(v)) / med) if med else 0.0}


def ensemble(kind, count, rng):
    if kind == "uniform":
        r = rng.random((count, 3)) * N * D
    else:  # within the 4^3 cells 30 .. 33 of every axis
        r = (30.0 + 4.0 * rng.random((count, 3))) * D
    return np.column_stack([r, rng.normal(0.0, 1e-3, (count, 3))])  # (slow: nobody leaves its cells during the run)


def host_density(pts):
    """the density deposit in numpy, whole box"""
    pr = pts[:, :3] / D
    st = np.where(pr - 1.0 >= 0, np.floor(pr - 1.0 + 0.5), np.ceil(pr - 1.0 - 0.5)).astype(np.int64)
    out = np.zeros((N, N, N))
    w = [np.clip(1.0 - np.abs(pr - (st + t + 0.5)), 0.0, None) for t in range(2)]
    for i in range(8):
        ix, iy, iz = i & 1, (i >> 1) & 1, i >> 2
        t = (st + (ix, iy, iz)) % N
        np.add.at(out, (t[:, 2], t[:, 1], t[:, 0]), w[ix][:, 0] * w[iy][:, 1] * w[iz][:, 2])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracers", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracer_moments_time.json"))
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    ctx = X.Context("basic", (N, N, N), (D, D, D), 0.1, device=0)
    ctx.set_field(X.B, np.zeros(ctx.fshape()) + np.array([0.0, 0.0, 0.3]))
    result = {"box": [N, N, N], "tracers": args.tracers, "due_steps_per_repetition": args.steps, "repetitions": args.reps,
              "unit": "ms", "cases": {}}
    around = (29, 29, 29, 6, 6, 6)
    for kind in ("uniform", "bunched"):
        pts = ensemble(kind, args.tracers, rng)
        s = ctx.tracers("full_orbit", pts, "B1B", Q / M, 0.1)
        case = {}
        for name in ("density", "momentum_flux"):
            for label, region in (("whole_box", None), ("region_6x6x6", around)):
                if kind == "uniform" and region is not None:
                    continue
                m = s.map(name, Q, M, region=region)
                s.advance(1)  # warm-up
                per = []
                for _ in range(args.reps):
                    ctx.profile_enable(True)
                    ctx.profile_reset()
                    s.advance(args.steps)
                    ctx.synchronize()
                    a, b = ctx.profile_get("tracer_moment"), ctx.profile_get("tracer_moment_lds")
                    ctx.profile_enable(False)
                    assert a[0] + b[0] == args.steps
                    per.append((a[1] + b[1]) / args.steps)
                path = "lds" if b[0] else "direct"
                _, deposits, counted, _ = m.get()
                # (the set is not folded into the box: the few that drift across its faces stop counting)
                assert 0.99 * deposits * args.tracers <= counted <= deposits * args.tracers, (counted, deposits)
                case["map_deposit_%s_%s" % (name, label)] = dict(stats(per), path=path)
                m.close()
        # the parent commit's ways
        get, dep = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            st = s.get()
            t1 = time.perf_counter()
            host_density(st.state)
            t2 = time.perf_counter()
            get.append(1e3 * (t1 - t0))
            dep.append(1e3 * (t2 - t1))
        case["tracers_get"] = stats(get)
        case["numpy_density_deposit"] = stats(dep)
        state = s.get().state
        s.close()
        sort = ctx.add_sort(1, 1.0, Q, M, capacity=args.tracers + 1024)
        load, wall, kern = [], {"density": [], "momentum_flux": []}, {"density": [], "momentum_flux": []}
        for _ in range(args.reps):
            ctx.remove_particles(sort, NOWHERE)  # (empties the sort: no cell's corner lies in it)
            t0 = time.perf_counter()
            ctx.add_particles(sort, state)
            ctx.synchronize()
            load.append(1e3 * (time.perf_counter() - t0))
            for name in wall:
                ctx.profile_enable(True)
                ctx.profile_reset()
                t0 = time.perf_counter()
                ctx.moment(sort, name)
                wall[name].append(1e3 * (time.perf_counter() - t0))
                kern[name].append(ctx.profile_get("moment")[1])
                ctx.profile_enable(False)
        case["sort_load"] = stats(load)
        for name in wall:
            case["xpic_moment_wall_" + name] = stats(wall[name])
            case["xpic_moment_kernel_" + name] = stats(kern[name])
        ctx.remove_particles(sort, NOWHERE)
        result["cases"][kind] = case
    ctx.close()
    print(json.dumps(result))
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
