"""CPU checks of tests/full_orbit_ref.py, the model the GPU full-orbit kernels are tested against: the reference's own
trajectory tables for the two examples whose fields are uniform and therefore exactly representable on a grid
(tests/golden/boris_push_ex1, boris_push_ex4), and the assertions of its crank_nicolson_push_ex2."""
import ctypes
import os
import re

import numpy as np
import pytest

import full_orbit_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
PETSC_SMALL = R.PETSC_SMALL
FO_SYMBOLS = ("xpic_full_orbit_push", "xpic_full_orbit_trace")

EX1_ROWS = 6    # the row of t = 0 and 5 more: 2715 of the table's 100 000 steps (0.26 ms a step here: the whole table
                # would take half a minute per id)
EX4_ROWS = 157  # the whole table: 5000 steps


@pytest.mark.parametrize("sid", R.MAGNETIC)
def test_ex1_table(oracle, sid):
    """boris_push_ex1 (B0 = (0, 0, 2), qm = -1, dt = pi / 4, r0 = (0.5, 0, 0), v0 = (0, 1, 0)) on an 8^3 grid, d = 1,
    filled with the constant: the first 6 rows (2715 steps) of every magnetic id against the committed table.  Measured
    largest |restatement - analytic-field trajectory| over these steps: 1.4e-13 (CLF; 1.2e-14 for M2A), so the floors are
    1.2e-13 .. 1.4e-12."""
    mine = R.run_example(R.EX1, sid, EX1_ROWS)
    gold = R.read_table(GOLD, R.EX1, sid, EX1_ROWS)
    diff, floor = R.table_floor(oracle, R.EX1, sid, mine)
    err = np.abs(mine - gold)
    print(sid, "restatement - analytic", diff, "max |restatement - table|", err.max())
    assert (err <= R.table_bound(gold, floor)).all()


@pytest.mark.parametrize("sid", R.SCHEMES[13:])
def test_ex4_table(oracle, sid):
    """boris_push_ex4 (E0 = (0, 0, 1), B0 = (250, 0, 0), dt = 0.1975, v0 = (0.1, 0, 0.4)): the whole table, 5000 steps.
    Measured largest |restatement - analytic-field trajectory|: 3.1e-14 (EB1A), so the floors are up to 3.1e-13."""
    mine = R.run_example(R.EX4, sid, EX4_ROWS)
    gold = R.read_table(GOLD, R.EX4, sid)
    assert gold.shape[0] == EX4_ROWS
    diff, floor = R.table_floor(oracle, R.EX4, sid, mine)
    err = np.abs(mine - gold)
    print(sid, "restatement - analytic", diff, "max |restatement - table|", err.max())
    assert (err <= R.table_bound(gold, floor)).all()


def whole_turns(phi, most):
    """the step count in (most / 2, most] after which a rotation by phi a step is closest to whole turns, and what is
    left of the last turn"""
    N = np.arange(most // 2 + 1, most + 1)
    left = np.abs((N * phi + np.pi) % (2 * np.pi) - np.pi)
    k = int(np.argmin(left))
    return int(N[k]), float(left[k])


@pytest.mark.parametrize("omega_dt,most", [(0.1, 4000), (10.0, 4000)])
def test_crank_nicolson_ex2(omega_dt, most):
    """crank_nicolson_push_ex2.cpp: E0 = (0, 0, 1), B0 = (20, 0, 0), qm = -1, r0 = (0.5, 0, 0), v0 = (0, 1, 0),
    dt = omega_dt / |B0|, tolerances at the defaults of crank_nicolson_push.h.

    Energy: 0.5 (pn^2 - p0^2) + 0.5 (pn + p0) . E0 dt is 0 to PETSC_SMALL at every step (the reference sums it and
    divides by the step count; each term is checked here, and their mean).

    Drift: the mean over the steps of 0.5 (pn + p0) transverse to B0 is E0 x B0 / B0^2 to 1e-4.  In uniform fields the
    scheme's vh is the drift plus a vector of length |v0 - drift| <= 1.05 that turns by phi = 2 atan(omega_dt / 2) a
    step, so the mean over N steps misses the drift by at most 1.05 |sin(N phi / 2)| / (N sin(phi / 2)).  The reference
    makes that small with 100 000 gyro-periods (6.3e6 steps at omega_dt = 0.1); this test has a few seconds, so it stops
    where the turns are closest to whole ones within its budget of 4000 steps: 2704 steps = 43 gyro-periods at omega_dt = 0.1,
    3191 steps = 5079 gyro-periods at omega_dt = 10 (2 pi / |B0| each).  The bound above, from the inputs alone, is asserted to be under
    a quarter of the 1e-4 first."""
    E0, B0 = np.array([0.0, 0.0, 1.0]), np.array([20.0, 0.0, 0.0])
    qm = -1.0
    omega = np.sqrt(B0.dot(B0))
    dt = omega_dt / omega
    phi = 2 * np.arctan(omega_dt / 2)
    N, left = whole_turns(phi, most)
    v_ExB = np.cross(E0, B0) / B0.dot(B0)
    miss = 1.05 * abs(np.sin(left / 2)) / (N * np.sin(phi / 2))
    print("omega_dt", omega_dt, "steps", N, "gyro-periods", N * dt * omega / (2 * np.pi), "mean's bound", miss)
    assert miss < 0.25e-4
    E, B = R.uniform_fields(E0, B0)
    p = np.array([[0.5, 0.0, 0.0, 0.0, 1.0, 0.0]])
    energy, drift, worst = 0.0, np.zeros(3), 0.0
    for _ in range(N):
        p0 = p
        p, its = R.cn_step(E, B, R.D, p0, qm, dt)
        assert its[0] < R.CN_MAXIT
        vn, v0 = p[0, 3:], p0[0, 3:]
        term = 0.5 * (vn.dot(vn) - v0.dot(v0)) + 0.5 * (vn + v0).dot(E0) * dt
        worst = max(worst, abs(term))
        energy += term / N
        vh = 0.5 * (vn + v0)
        drift += (vh - vh.dot(B0) * B0 / B0.dot(B0)) / N
    print("energy: worst step", worst, "mean", energy, "drift", drift, "theory", v_ExB)
    assert worst < PETSC_SMALL and abs(energy) < PETSC_SMALL
    assert np.abs(drift - v_ExB).max() < 1e-4


def test_zero_field_keeps_v_and_pinned_iterations_count():
    """the two conventions of include/xpic_hip.h that are not the reference's: |B_p| = 0 leaves v alone in the magnetic
    ids, and a Crank-Nicolson particle that runs out of iterations returns maxit"""
    E, B = R.uniform_fields((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    p = R.case_particles(n=8)
    for sid in R.MAGNETIC:
        out = R.step(sid, E, B, R.D, p, R.QM, R.DT)
        assert np.isfinite(out).all() and np.array_equal(out[:, 3:], p[:, 3:])
    E, B = R.case_fields()
    for k in (1, 2, 5):
        _, its = R.cn_step(E, B, R.D, p, R.QM, R.DT, atol=0.0, rtol=0.0, maxit=k)
        assert (its == k).all()
    pn, its = R.cn_step(E, B, R.D, p, R.QM, R.DT)
    assert its.max() < R.CN_MAXIT and np.isfinite(pn).all()


def test_gathers_return_constants_and_the_seam_is_periodic():
    E, B = R.uniform_fields((0.3, -1.1, 0.7), (-0.2, 0.5, 0.9))
    p = R.case_particles()
    r = p[:, :3]
    assert ((r < 0) | (r > 8)).any(axis=0).all()  # every axis has particles outside the box
    Ep, Bp = R.gather(E, B, R.D, r)
    assert np.abs(Ep - np.array([0.3, -1.1, 0.7])).max() < 1e-13 and np.abs(Bp - np.array([-0.2, 0.5, 0.9])).max() < 1e-13
    rn = r + 0.4 * p[:, 3:]
    Ep, Bp = R.gather_segment(E, B, R.D, rn, r)
    assert np.abs(Ep - np.array([0.3, -1.1, 0.7])).max() < 1e-13 and np.abs(Bp - np.array([-0.2, 0.5, 0.9])).max() < 1e-13
    # a shift by whole box lengths changes nothing but rounding
    E, B = R.case_fields()
    L = np.array(R.N) * np.array(R.D)
    for a, b in zip(R.gather(E, B, R.D, r), R.gather(E, B, R.D, r + 2 * L)):
        assert np.abs(a - b).max() < 1e-12
    for a, b in zip(R.gather_segment(E, B, R.D, rn, r), R.gather_segment(E, B, R.D, rn - L, r - L)):
        assert np.abs(a - b).max() < 1e-12


@pytest.mark.parametrize("qm", [-1.0, 1.0])
def test_orbit_centre_is_the_centre_of_the_boris_circle(qm):
    """B = (0, 0, 1), E = 0, one gyro-period of EB2B at dt = 0.1: every position is one Larmor radius from
    guiding_centre(..., orbit_centre=True), to the (omega dt)^2 = 1e-2 of a second-order scheme, for either sign of the
    charge.  The default, PointByField's constructor, is the mirror image of that point about the particle, so the
    orbit's distance from it ranges up to three radii."""
    import xpic_amd as X

    B0 = np.array([0.0, 0.0, 1.0])
    E, B = R.uniform_fields((0.0, 0.0, 0.0), B0)
    p = np.array([[3.0, 4.0, 2.0, 0.3, -0.4, 0.2], [5.0, 1.0, 6.0, 0.0, 0.7, 0.0]])
    rho = np.sqrt((p[:, 3:5] ** 2).sum(axis=1)) / abs(qm)
    centre = X.guiding_centre(p, B0, 1.0, qm, orbit_centre=True)
    mirror = X.guiding_centre(p, B0, 1.0, qm)
    assert np.array_equal(mirror[:, 3:], centre[:, 3:])
    assert np.abs(mirror[:, :3] + centre[:, :3] - 2 * p[:, :3]).max() < 1e-15 * 8
    near, far, s = [], [], p
    for _ in range(63):
        s = R.step("EB2B", E, B, R.D, s, qm, 0.1)
        near.append(np.sqrt(((s[:, :2] - centre[:, :2]) ** 2).sum(axis=1)) / rho)
        far.append(np.sqrt(((s[:, :2] - mirror[:, :2]) ** 2).sum(axis=1)) / rho)
    assert np.abs(np.array(near) - 1).max() < 1e-2
    assert np.array(far).max() > 2.9


def test_binding_header_and_library_agree():
    import xpic_amd

    hdr = open(os.path.join(ROOT, "include", "xpic_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in FO_SYMBOLS:
        assert name in xpic_amd.SYMBOLS
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert int(re.search(r"#define XPIC_FO_LAUNCH_STEPS (\d+)", hdr).group(1)) == xpic_amd.FO_LAUNCH_STEPS
    assert int(re.search(r"#define XPIC_FO_MAXIT (\d+)", hdr).group(1)) == xpic_amd.FO_MAXIT
    assert int(re.search(r"#define XPIC_VERSION (\d+)", hdr).group(1)) >= 6
    # enum xpic_fo_scheme and FO_SCHEMES name the same numbers, in the order of full_orbit_ref.SCHEMES + CN
    for name, k in xpic_amd.FO_SCHEMES.items():
        assert re.search(r"\bXPIC_FO_%s = %d\b" % (name, k), code), name
    assert [xpic_amd.FO_SCHEMES[s] for s in R.SCHEMES + ["CN"]] == list(range(18))
    if not os.path.exists(xpic_amd.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    lib = ctypes.CDLL(xpic_amd.LIB_PATH)
    for name in FO_SYMBOLS:
        assert hasattr(lib, name), name
    assert ctypes.sizeof(xpic_amd.FoParams) == 40  # four doubles and two int32
    for f in ("Context.full_orbit_push", "Context.full_orbit_trace"):
        obj = xpic_amd
        for part in f.split("."):
            obj = getattr(obj, part)
        assert callable(obj)
