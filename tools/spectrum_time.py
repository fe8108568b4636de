#!/usr/bin/env python3
"""Times the field spectra (include/xpic_spectrum.h) beside the host way they replace, on one context per size:

  spectrum   Context.spectrum(E, 0, dk, nshell): three passes, the fused combine, the small reductions, one download of
             nx + ny + nz + 2 (nshell + 1) numbers
  probe      a probe of 8 modes of E_x with every = 1 on an ecsim context whose step is not the subject: the probe's own
             launches (the passes and the gather) from the profile sections, and the wall time of a step with and without it
  host       get_field(E) and numpy.fft.fftn of one component, |F|^2 summed along the axes: the round trip of 3 N doubles
             and the host transform

Device times are the context's profile sections (event pairs around the launches): poisson_pass_x / _y / _z,
spectrum_combine, spectrum_reduce, spectrum_modes.  wall: time.perf_counter around the call, every host round trip in it.
Writes one JSON object (profiles/spectrum_time.json).
usage: spectrum_time.py [--sizes 128 256] [--ppc 8 1] [--nshell 64] [--reps 5] [--steps 3] [--out profiles/spectrum_time.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import xpic_amd as X  # noqa: E402

SECTIONS = ("poisson_pass_x", "poisson_pass_y", "poisson_pass_z", "spectrum_combine", "spectrum_reduce", "spectrum_modes")


def timed(ctx, call):
    ctx.synchronize()
    ctx.profile_enable(True)
    ctx.profile_reset()
    t0 = time.perf_counter()
    call()
    ctx.synchronize()
    out = {"wall_ms": (time.perf_counter() - t0) * 1e3}
    device = 0.0
    for name in SECTIONS:
        launches, ms = ctx.profile_get(name)
        if launches:
            out[name] = {"launches": launches, "ms": ms}
            device += ms
    out["spectrum_kernels_ms"] = device
    ctx.profile_enable(False)
    return out


def case(n, ppc, nshell, reps, steps):
    ctx = X.Context("ecsim", (n, n, n), (0.5,) * 3, 0.5, device=0)
    nodes = n ** 3
    s = ctx.add_sort(ppc, 1.0, -1.0, 1.0, capacity=int(ppc * nodes * 1.3) + 1024)
    ctx.load_synthetic(s, ppc, 0.05, seed=3)
    ctx.set_field(X.E, np.random.default_rng(1).normal(0.0, 1.0, (n, n, n, 3)))
    dk = np.pi / 0.5 * np.sqrt(3.0) / nshell
    out = {"grid": f"{n}^3", "ppc": ppc, "nshell": nshell}
    ctx.spectrum(X.E, 0, dk=dk, nshell=nshell)  # (builds the tables, sizes the partial sums, warms the kernels up)
    out["spectrum"] = [timed(ctx, lambda: ctx.spectrum(X.E, 0, dk=dk, nshell=nshell)) for _ in range(reps)]
    out["spectrum_power"] = [timed(ctx, lambda: ctx.spectrum_power(X.E, 0)) for _ in range(reps)]

    def host():
        f = np.fft.fftn(ctx.get_field(X.E)[..., 0]) / np.sqrt(nodes)
        p = f.real ** 2 + f.imag ** 2
        return p.sum(axis=(0, 1)), p.sum(axis=(0, 2)), p.sum(axis=(1, 2))
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        e = ctx.get_field(X.E)
        t1 = time.perf_counter()
        host()
        t.append({"get_field_wall_ms": (t1 - t0) * 1e3, "get_field_fftn_axis_sums_wall_ms": (time.perf_counter() - t1) * 1e3})
    del e
    out["host"] = t
    modes = [(m, 0, 0) for m in range(1, 9)]
    ctx.step()  # (warm)
    out["steps_without_probe"] = [timed(ctx, ctx.step) for _ in range(steps)]
    probe = ctx.spectrum_probe(X.E, modes, comp=0, every=1, capacity=steps + 1)
    ctx.step()
    out["steps_with_probe"] = [timed(ctx, ctx.step) for _ in range(steps)]
    rec, _, dropped = probe.get()
    out["probe_rows"], out["probe_dropped"] = int(rec.size), int(dropped)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[128, 256])
    ap.add_argument("--ppc", type=int, nargs="+", default=[8, 1], help="one value, or one per size")
    ap.add_argument("--nshell", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectrum_time.json"))
    a = ap.parse_args()
    ppc = a.ppc * len(a.sizes) if len(a.ppc) == 1 else a.ppc
    assert len(ppc) == len(a.sizes), "--ppc takes one value or one per size"
    argv = sys.argv[1:]
    if "--out" in argv:  # (where the file went is no parameter of the measurement)
        del argv[argv.index("--out"):argv.index("--out") + 2]
    out = {"argv": argv, "cases": [case(n, p, a.nshell, a.reps, a.steps) for n, p in zip(a.sizes, ppc)]}
    text = json.dumps(out, indent=1)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
