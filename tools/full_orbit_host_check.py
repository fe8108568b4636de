#!/usr/bin/env python3
"""Builds tools/full_orbit_host.cpp (the device functions of xpic_amd/csrc/full_orbit_step.h compiled for the host) and
runs it once against the numpy restatement tests/full_orbit_ref.py at the inputs of tests/test_gpu_full_orbit.py: both
gathers, one step of each of the 17 Chin ids, Crank-Nicolson with the iteration count pinned (maxit = 1, 2, 5 at
atol = rtol = 0) and with the default tolerances, and 70 steps of EB2B.  Prints the largest difference of each and of
all.  No GPU is used.  --sanitize builds the program with the host's address and undefined-behaviour sanitizers.
usage: full_orbit_host_check.py [--sanitize] [--keep DIR]"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import full_orbit_ref as R  # noqa: E402


def soa(F):
    return np.ascontiguousarray(np.moveaxis(F, 3, 0))  # [nz][ny][nx][3] -> [3][nz][ny][nx]


def run(exe, tmp, E, B, pts, mode, steps=1, atol=R.CN_ATOL, rtol=R.CN_RTOL, maxit=R.CN_MAXIT, dt=R.DT):
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        np.array([R.N[0], R.N[1], R.N[2], pts.shape[0], mode, maxit, steps, 0], dtype=np.int32).tofile(f)
        np.array(list(R.D) + [R.QM, dt, atol, rtol], dtype=np.float64).tofile(f)
        soa(E).tofile(f)
        soa(B).tofile(f)
        np.ascontiguousarray(pts, dtype=np.float64).tofile(f)
    subprocess.check_call([exe, fin, fout])
    out = np.fromfile(fout, dtype=np.float64).reshape(-1, 7)
    return out[:, :6], out[:, 6].astype(int)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sanitize", action="store_true")
    ap.add_argument("--keep", default=None, help="directory for the program and its files (default: a temporary one)")
    args = ap.parse_args()
    tmp = args.keep or tempfile.mkdtemp(prefix="fo_host_")
    os.makedirs(tmp, exist_ok=True)
    exe = os.path.join(tmp, "full_orbit_host")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "hip", "--offload-host-only", "-O2", "-std=c++17", "-DXPIC_FO_HOST",
           "-Wno-unused-function", os.path.join(ROOT, "tools", "full_orbit_host.cpp"), "-o", exe]
    if args.sanitize:
        cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"]
    subprocess.check_call(cmd)

    E, B = R.case_fields()
    p = R.case_particles()
    worst = {}

    def note(name, got, ref, scale):
        worst[name] = np.abs(got - ref).max() / scale
        print("%-28s max |host - restatement| / scale = %.3e" % (name, worst[name]))

    got, _ = run(exe, tmp, E, B, p, -1)
    Ep, Bp = R.gather(E, B, R.D, p[:, :3])
    note("gather E", got[:, :3], Ep, np.abs(E).max())
    note("gather B", got[:, 3:], Bp, np.abs(B).max())
    seg = np.column_stack([p[:, :3] + 0.7 * p[:, 3:], p[:, :3]])
    got, _ = run(exe, tmp, E, B, seg, -2)
    Ep, Bp = R.gather_segment(E, B, R.D, seg[:, :3], seg[:, 3:])
    note("segment gather E", got[:, :3], Ep, np.abs(E).max())
    note("segment gather B", got[:, 3:], Bp, np.abs(B).max())
    for k, sid in enumerate(R.SCHEMES):
        got, _ = run(exe, tmp, E, B, p, k)
        note("step " + sid, got, R.step(sid, E, B, R.D, p, R.QM, R.DT), np.abs(p).max())
    for k in (1, 2, 5):
        got, its = run(exe, tmp, E, B, p, 17, atol=0.0, rtol=0.0, maxit=k)
        ref, its_ref = R.cn_step(E, B, R.D, p, R.QM, R.DT, atol=0.0, rtol=0.0, maxit=k)
        assert (its == k).all() and (its_ref == k).all()
        note("CN maxit=%d" % k, got, ref, np.abs(p).max())
    got, its = run(exe, tmp, E, B, p, 17)
    ref, its_ref = R.cn_step(E, B, R.D, p, R.QM, R.DT)
    print("CN default tolerances: iterations host %d..%d, restatement %d..%d, largest difference of counts %d" % (
        its.min(), its.max(), its_ref.min(), its_ref.max(), np.abs(its - its_ref).max()))
    note("CN default tolerances", got, ref, np.abs(p).max())
    # a zero-field patch: the magnetic ids keep v, nothing is NaN
    B0 = B.copy()
    B0[2:6, 2:6, 2:6, :] = 0.0
    pz = p[:8].copy()
    pz[:, :3] = 4.0
    for k, sid in enumerate(R.MAGNETIC):
        got, _ = run(exe, tmp, E, B0, pz, k)
        assert np.isfinite(got).all() and np.array_equal(got[:, 3:], pz[:, 3:]), sid
    print("zero-B patch: v unchanged, all finite, in the 13 magnetic ids")
    steps = 70
    got, _ = run(exe, tmp, E, B, p, 16, steps=steps)
    ref = p
    for _ in range(steps):
        ref = R.step("EB2B", E, B, R.D, ref, R.QM, R.DT)
    note("EB2B %d steps" % steps, got, ref, np.abs(ref).max())
    print("largest of all: %.3e" % max(worst.values()))


if __name__ == "__main__":
    main()
