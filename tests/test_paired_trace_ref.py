"""Pins tests/paired_trace_ref.py, the numpy restatement of the reference's guiding-centre / full-orbit comparison, to the
reference's own example tests/drift_kinetic_push/drift_kinetic_grid_boris_ex1.cpp: uniform E0 = (0, 1, -1), B0 = (0, 0, 1),
q / m = -1, r0 = (2, 2, 2), v0 = (0, 0.1, 0), the Boris member stepped as boris_step composes it (update_r(dt / 2),
update_vEB(dt), update_r(dt / 2): the Chin id EB2B).  The fields are uniform, so the small periodic grid of
full_orbit_ref (8^3 cells of 1) stands for the example's 20 x 5 x 100 one: wrapping is harmless.  No GPU."""
import numpy as np
import pytest

import drift_kinetic_ref as DK
import full_orbit_ref as FO
import paired_trace_ref as P

EPS = np.finfo(float).eps
E0, B0 = np.array([0.0, 1.0, -1.0]), np.array([0.0, 0.0, 1.0])
Q, M = -1.0, 1.0          # drift_kinetic_push.h:12-13
OMEGA_DT = 0.1            # the example's -omega_dt; dt = omega_dt / |B0| (ex1.cpp:29)
STEPS = 40                # T = 4: p_parallel reaches 4, 0.4 cells a step, inside the segment shape's one cell
R0, V0 = np.array([2.0, 2.0, 2.0]), np.array([0.0, 0.1, 0.0])


def point_by_field(point, Bp, mp, qm):
    """PointByField(point, Bp, mp, qm), src/interfaces/point.h:52-58"""
    r, p = point[:3], point[3:]
    lB = np.sqrt(Bp.dot(Bp))
    par = p.dot(Bp) * Bp / Bp.dot(Bp)
    perp = np.sqrt(((p - par) ** 2).sum())
    return np.concatenate([r - np.cross(p, Bp / lB) / (qm * lB), [np.sqrt(par.dot(par)), perp, mp * perp * perp / (2.0 * lB)]])


@pytest.fixture(scope="module")
def run():
    E, B = FO.uniform_fields(E0, B0)
    dt = OMEGA_DT / np.sqrt(B0.dot(B0))
    fo0 = np.concatenate([R0, V0])[None, :]
    gc0 = point_by_field(fo0[0], B0, M, Q / M)[None, :]
    fo, gc, stats, curve, errors = P.paired_trace(E, B, None, FO.D, fo0, gc0, STEPS, "EB2B", Q / M, M, dt, sample_every=1)
    return dict(E=E, B=B, dt=dt, fo0=fo0, gc0=gc0, fo=fo, gc=gc, stats=stats, curve=curve, errors=errors)


def test_the_examples_checks(run):
    """the PetscChecks of ex1.cpp:105-126 for the grid member, at the example's tolerance"""
    T = run["dt"] * STEPS
    q, E_par = Q / M, E0[2]
    gc = run["gc"][0]
    p_par_theory = q * E_par * T                                    # :103
    assert abs(gc[3] - p_par_theory) <= 1e-4                        # :108
    z_theory = 0.5 * q * E_par * T * T                              # :111
    assert abs(gc[2] - (z_theory + R0[2])) <= 1e-4                  # :116
    V_drift = np.cross(E0, B0) / (np.sqrt(B0.dot(B0)) ** 2)         # :119
    r_theory = run["gc0"][0, :3] + V_drift * T + np.array([0.0, 0.0, z_theory])
    assert np.abs(gc[:3] - r_theory).max() <= 1e-4                  # :125


def test_errors_equal_a_direct_evaluation(run):
    """The two trajectories stepped on their own, and err_mu / err_energy (and err_z) written out for B = B0 = (0, 0, 1):
    mu of the orbit is 0.5 m (px^2 + py^2) / 1.  The restatement takes B from the grid gather, whose 64 weights sum to 1
    and whose parallel_to divides two sums of three products: a dozen roundings, each relative to the operands of the
    final subtraction, hence 32 eps of the larger operand."""
    E, B, dt = run["E"], run["B"], run["dt"]
    fo, gc = run["fo0"], run["gc0"]
    m = np.zeros(4)
    for k in range(STEPS):
        gc, its = DK.push(E, B, None, FO.D, gc, Q / M, M, dt)
        assert its[0] < 30
        fo = FO.step("EB2B", E, B, FO.D, fo, Q / M, dt)
        px, py, pz = fo[0, 3:]
        mu_a, mu_b = gc[0, 5], 0.5 * M * (px * px + py * py)
        en_a, en_b = 0.5 * (gc[0, 4] ** 2 + gc[0, 3] ** 2), 0.5 * (px * px + py * py + pz * pz)
        par_a, par_b = gc[0, 3], abs(pz)
        direct = np.array([abs(gc[0, 2] - fo[0, 2]), abs(par_a - par_b), abs(mu_a - mu_b), abs(en_a - en_b)])
        scale = np.array([max(abs(gc[0, 2]), abs(fo[0, 2])), max(par_a, par_b), max(mu_a, mu_b), max(en_a, en_b)])
        got = run["errors"][k, 0]
        assert (np.abs(got - direct) <= 32 * EPS * scale).all(), (k, got, direct)
        m = np.maximum(m, got)
    assert np.array_equal(run["fo"], fo) and np.array_equal(run["gc"], gc)
    assert np.array_equal(run["stats"][0], m)
    assert np.array_equal(run["curve"], run["errors"][:, 0, :])  # one pair: the curve is its errors
    # the guiding centre conserves mu_p exactly and the orbit's p_perp^2 only gains the E x B drift's: the example's
    # statistics are small but not zero, and z of the pair agrees to the drift model's order
    assert run["stats"][0, 2] > 0 and run["stats"][0, 3] > 0


def test_accumulation_rule():
    """std::max(m, e) = (m < e) ? e : m: a NaN error leaves the maximum alone, an infinite one is kept, and a maximum that
    is a NaN stays one"""
    nan, inf = np.nan, np.inf
    m = np.array([1.0, 1.0, 1.0, nan, 0.0, inf])
    e = np.array([2.0, nan, inf, 5.0, 0.0, 3.0])
    out = P.accumulate(m, e)
    assert out[0] == 2.0 and out[1] == 1.0 and out[2] == inf and np.isnan(out[3]) and out[4] == 0.0 and out[5] == inf
    # compare_step with |Bg| = 0 follows the arithmetic: 0 / 0 in parallel_to, so every error but err_z and err_energy is
    # a NaN, and the accumulation skips it
    gc = np.array([[0.0, 0.0, 1.0, 0.5, 0.2, 0.1]])
    fo = np.array([[0.0, 0.0, 3.0, 0.1, 0.2, 0.3]])
    e = P.compare_step(gc, fo, np.zeros((1, 3)), 1.0)
    assert e[0, 0] == 2.0 and np.isnan(e[0, 1]) and np.isnan(e[0, 2]) and np.isfinite(e[0, 3])
    assert np.array_equal(P.accumulate(np.full((1, 4), 0.25), e), [[2.0, 0.25, 0.25, max(0.25, e[0, 3])]])
