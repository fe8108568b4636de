"""xpic_amd/csrc/field_line_step.h on the CPU (no GPU): tools/field_line_host.cpp compiles the header's own text with the
host compiler, without contraction, and runs it as a stand-alone program on an analytic field; every lane must equal the
numpy restatement (tests/field_lines_ref.py) bit for bit -- sqrt and the division are correctly rounded on both sides and
the field is a few exact-order operations -- for every stop code and for launches of any length."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import field_lines_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("field_line_host") / "field_line_host")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tools", "field_line_host.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    return exe


def field(r):
    return np.column_stack([-(r[:, 1] - 2.0), r[:, 0] - 2.0, 0.3 + 0.1 * r[:, 2]])


def run(program, seeds, h, max_steps, f_floor, close_tol, zmax, launch_steps):
    args = [repr(float(v)) for v in (h,)] + [str(max_steps)] + [repr(float(v)) for v in (f_floor, close_tol, zmax)] + [str(launch_steps)]
    out = subprocess.run([program] + args + [repr(float(v)) for v in seeds.ravel()], check=True, capture_output=True, text=True)
    rows = [line.split() for line in out.stdout.splitlines()]
    assert len(rows) == 2 * len(seeds)
    vals = np.array([[float.fromhex(w) for w in row[:8]] for row in rows]).reshape(len(seeds), 2, 8)
    steps = np.array([int(row[8]) for row in rows]).reshape(len(seeds), 2)
    code = np.array([int(row[9]) for row in rows]).reshape(len(seeds), 2)
    return vals, steps, code


@pytest.mark.parametrize("launch_steps", [1, 7, 256])
def test_header_equals_restatement(program, launch_steps):
    rng = np.random.default_rng(17)
    seeds = np.column_stack([2.0 + 1.5 * (rng.random((24, 2)) - 0.5), -2.0 + 3.0 * rng.random(24)])
    seeds[0] = (2.0, 2.0, -3.0)   # F = (0, 0, 0) exactly: NULL at the seed
    seeds[1] = (2.4, 2.0, -3.0)   # F_z = 0: a circle in the plane z = -3, CLOSED
    seeds[2, 2] = 1.7             # outside the region at the start: LEFT with no step
    seeds[3] = (2.005, 2.0, -2.7)  # runs down the axis to where |F| < f_floor: NULL after some steps
    h, S, floor, tol, zmax = 0.04, 90, 0.02, 0.04, 1.5
    vals, steps, code = run(program, seeds, h, S, floor, tol, zmax, launch_steps)
    ref = R.lines(R.function_source(field), seeds, h, S, keep=lambda r: r[:, 2] < zmax, f_floor=floor, close_tol=tol)
    assert {R.MAXSTEPS, R.LEFT, R.NULL, R.CLOSED} == set(np.unique(ref.code))
    assert ref.code[0, 0] == R.NULL and ref.steps[0, 0] == 0 and ref.code[0, 1] == R.CLOSED and ref.code[0, 2] == R.LEFT
    assert ((ref.code == R.NULL) & (ref.steps > 0)).any()  # lines that run down to where |F| < f_floor
    assert np.array_equal(steps, ref.steps.T) and np.array_equal(code, ref.code.T)
    want = np.concatenate([ref.end, np.stack([ref.length, ref.volume, ref.fmin, ref.smin, ref.fmax], axis=-1)], axis=-1)
    assert vals.tobytes() == np.ascontiguousarray(want.transpose(1, 0, 2)).tobytes()
