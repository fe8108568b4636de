"""CPU checks of tests/analytic_trace_ref.py, the model the GPU kernels of xpic_amd/csrc/model_trace.hip are tested
against.  Four ways: the reference's own PetscChecks of drift_kinetic_push_ex1 .. ex3, its recorded Crank-Nicolson tables
(tests/golden/crank_nicolson_push_ex1, ex2), agreement with the grid restatement on a uniform model, and the loss-cone
split that tests/test_gpu_model_trace.py repeats on the device."""
import os

import numpy as np
import pytest

import analytic_trace_ref as A
import full_orbit_ref as FO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
PETSC_SMALL = FO.PETSC_SMALL
OMEGA_DT = 0.1  # tests/drift_kinetic_push/CMakeLists.txt: set(omega_dt 0.1)
Q, M = -1.0, 1.0


def run_dk(field, B0, v0, dt, nt):
    """the loop of drift_kinetic_push_ex1 .. ex3: t = 0 .. geom_nt inclusive, from PointByField(point_init, B0, 1, q / m)"""
    p = A.point_by_field(np.array([0.0, 0.0, 0.0] + list(v0)), B0, 1.0, Q / M)[None]
    start = p.copy()
    for _ in range(nt + 1):
        p, its = A.dk_push(field, p, Q / M, M, dt)
        assert its[0] < 30
    return start[0], p[0]


def test_drift_kinetic_ex1_checks():
    """drift_kinetic_push_ex1.cpp: the guiding centre stays (1e-10) and the energy is conserved (PETSC_SMALL) in a uniform
    B over 1000 steps"""
    B0 = (0.0, 0.0, 2.0)
    start, end = run_dk(A.model("uniform", B0=B0), B0, (0.0, 1.0, 0.0), OMEGA_DT / 2.0, 1000)
    assert np.abs(end[:3] - start[:3]).max() < 1e-10
    assert abs((end[3] ** 2 + end[4] ** 2) - (start[3] ** 2 + start[4] ** 2)) < PETSC_SMALL


def test_drift_kinetic_ex2_checks():
    """drift_kinetic_push_ex2.cpp: p_parallel = q E t, z = q E t^2 / 2 and the E x B drift, each to 1e-4, 1000 steps"""
    E0, B0 = np.array([0.0, 1.0, 1.0]), np.array([0.0, 0.0, 1.0])
    dt, nt = OMEGA_DT / 1.0, 1000
    start, end = run_dk(A.model("uniform", E0=E0, B0=B0), B0, (0.0, 1.0, 0.0), dt, nt)
    T = dt * (nt + 1)
    q = (Q / M) * M
    assert abs(end[3] - q * E0[2] * T) < 1e-4
    z_theory = 0.5 * q * E0[2] * T * T
    assert abs(end[2] - z_theory) < 1e-4
    r_theory = start[:3] + np.cross(E0, B0) / B0.dot(B0) * T + np.array([0.0, 0.0, z_theory])
    assert np.abs(end[:3] - r_theory).max() < 1e-4


def test_drift_kinetic_ex3_checks():
    """drift_kinetic_push_ex3.cpp: the grad-B drift to 1e-8 over 100 steps"""
    B0, g, v0 = np.array([0.0, 0.0, 2.0]), np.array([1.0, 0.0, 0.0]), np.array([1.0, 0.0, 1.0])
    dt, nt = OMEGA_DT / 2.0, 100
    start, end = run_dk(A.model("linear", B0=B0, r0=(0, 0, 0), g=g), B0, v0, dt, nt)
    B = 2.0
    V = np.array([0.0, 0.0, v0[2]]) + M * v0[2] ** 2 / (Q * B ** 3) * np.cross(B0, g) + end[5] / (Q * B ** 2) * np.cross(B0, g)
    assert np.abs(end[:3] - (start[:3] + V * dt * (nt + 1))).max() < 1e-8


# Ten times the 1e-2 PETSC_SMALL = 1e-12 that full_orbit_ref.table_floor allows between two evaluations of one trajectory:
# the largest floor that function can return.  The entries of these tables are 1e-2 .. 1e3 (half a unit of the seventh
# digit is >= 5e-9), or exactly 0.
TABLE_FLOOR = 1e-11
EX1_ROWS = 13  # the row of t = 0 and 12 more: 9756 of the 100 000 steps every omega_dt of ex1 runs (geom_nt, ex1.cpp:28)


def read(ex, omega_dt):
    return np.loadtxt(os.path.join(GOLD, "crank_nicolson_push_ex%d" % ex, "omega_dt_%.1f.txt" % omega_dt), skiprows=1)


def cn_table(field, dt, steps, every):
    """PointTrace's rows {t, r, v} before step 0 and after every `every`-th step, one table per entry of dt"""
    dt = np.atleast_1d(np.asarray(dt, dtype=np.float64))
    p = np.zeros((len(dt), 6)) + np.array([0.5, 0.0, 0.0, 0.0, 1.0, 0.0])
    rows = []
    for t in range(steps + 1):
        if t % every == 0:
            rows.append(np.column_stack([t * dt, p]))
        if t < steps:
            p, its = A.cn_step(field, p, -1.0, dt)
            assert its.max() < FO.CN_MAXIT
    return np.stack(rows, axis=1)  # [table][row][7]


def test_crank_nicolson_ex1_tables():
    """crank_nicolson_push_ex1.cpp (B0 = (0, 0, 2), qm = -1): every omega_dt runs 100 000 steps, over the 20 000 this suite
    spends on a table, so the leading 13 rows of all five tables are compared, the five runs side by side"""
    omega = (0.1, 1.0, 10.0, 100.0, 1000.0)
    every = 100000 // 123
    mine = cn_table(A.model("uniform", B0=(0.0, 0.0, 2.0)), np.array(omega) / 2.0, (EX1_ROWS - 1) * every, every)
    for k, w in enumerate(omega):
        gold = read(1, w)[:EX1_ROWS]
        err = np.abs(mine[k] - gold)
        print("omega_dt", w, "max |restatement - table|", err.max())
        assert (err <= FO.table_bound(gold, TABLE_FLOOR)).all(), w


@pytest.mark.parametrize("omega_dt", [100.0, 1000.0])
def test_crank_nicolson_ex2_tables(omega_dt):
    """crank_nicolson_push_ex2.cpp (E0 = (0, 0, 1), B0 = (20, 0, 0)): geom_nt = ROUND_STEP(1e5 2 pi / 20, dt) is 6283 steps
    at omega_dt = 100 and 628 at 1000 (62 832 and more below: not run), the whole tables"""
    dt = omega_dt / 20.0
    nt = int(np.floor(100000 * (2.0 * np.pi / 20.0) / dt + 0.5))
    assert nt < 20000
    gold = read(2, omega_dt)
    every = nt // 123
    mine = cn_table(A.model("uniform", E0=(0.0, 0.0, 1.0), B0=(20.0, 0.0, 0.0)), dt, nt, every)[0]
    assert mine.shape == gold.shape
    err = np.abs(mine - gold)
    print("omega_dt", omega_dt, "steps", nt, "max |restatement - table|", err.max())
    assert (err <= FO.table_bound(gold, TABLE_FLOOR)).all()


@pytest.mark.parametrize("sid", ["EB2B", "M1A", "BLF", "C2A", "CN"])
def test_uniform_model_agrees_with_the_grid_restatement(sid):
    """the restated steps around a uniform model against full_orbit_ref.step / cn_step on uniform_fields, 200 steps of
    full_orbit_ref's batch: within 1e-2 PETSC_SMALL, what full_orbit_ref.table_floor allows between its two evaluations
    (the grid one sums 64 weighted copies of the constant)"""
    E0, B0 = (0.0, 0.1, -0.1), (0.2, 0.3, 1.0)
    E, B = FO.uniform_fields(E0, B0)
    field = A.model("uniform", E0=E0, B0=B0)
    a = b = FO.case_particles(n=64)
    for _ in range(200):
        if sid == "CN":
            a, ia = A.cn_step(field, a, FO.QM, FO.DT)
            b, ib = FO.cn_step(E, B, FO.D, b, FO.QM, FO.DT)
            assert np.array_equal(ia, ib)
        else:
            a, b = A.chin_step(sid, field, a, FO.QM, FO.DT), FO.step(sid, E, B, FO.D, b, FO.QM, FO.DT)
    diff = np.abs(a - b).max()
    print(sid, "max |analytic - grid| after 200 steps", diff)
    assert diff < 1e-2 * PETSC_SMALL


def test_loss_cone_split():
    """64 guiding centres at drift_kinetic_push_ex9's start in the Gaussian mirror, Omega dt = 1: the half at 0.8 of the
    critical pitch angle leaves through a throat, the half at 1.2 is still there after two transits"""
    p, dt = A.cone_batch()
    steps = A.cone_steps(dt)
    field = A.model("gaussian_mirror", **A.GAUSSIAN)
    out = A.trace(A.pusher("dk", field, A.QM, A.MP, dt), p, steps, A.cone_region(), A.CONE_D)
    h = A.CONE_N // 2
    print("steps", steps, "exit steps of the first half", np.unique(out.exit_step[:h]), "iterations_max", out.iterations_max.max())
    assert out.iterations_max.max() < 30
    assert (out.exit_step[:h] >= 0).all() and (out.exit_step[h:] < 0).all()
    assert out.removed == h
