"""Pins tests/triplet_trace_ref.py, the numpy restatement of the reference's three-way comparison (analytic guiding centre,
grid guiding centre, Boris orbit), to the reference's own examples tests/drift_kinetic_push/drift_kinetic_grid_boris_ex2.cpp
(the grad-B drift on a linear field, 20^3 cells of 1, both PetscChecks at 1e-8) and ex1.cpp (uniform E and B, its checks at
1e-4), and to a direct evaluation of the seven statistics from three separately stepped trajectories.  No GPU."""
import numpy as np
import pytest

import analytic_trace_ref as A
import drift_kinetic_ref as DK
import full_orbit_ref as FO
import paired_trace_ref as P
import triplet_trace_ref as T

EPS = np.finfo(float).eps
Q, M = -1.0, 1.0   # drift_kinetic_push.h:12-13
OMEGA_DT = 0.1     # tests/drift_kinetic_push/CMakeLists.txt:17, the examples' -omega_dt


def start(r0, v0, B0):
    fo = np.concatenate([r0, v0])[None, :]
    gc = A.point_by_field(fo[0], B0, M, Q / M)[None, :]
    return fo, gc


def test_ex2_grad_B_drift():
    """ex2.cpp: B = B0 + ((r - r0) . gradB0) gradB0 / |gradB0|, 101 steps (t = 0 .. geom_nt = 100) of dt = omega_dt / |B0|;
    both guiding centres end at start_r + V_gradB T within 1e-8 (:102-116)"""
    r0, v0 = np.array([2.0, 2.0, 2.0]), np.array([0.1, 0.0, 0.1])
    B0, g0 = np.array([0.0, 0.0, 2.0]), np.array([1.0, 0.0, 0.0])
    n, d, steps = (20, 20, 20), (1.0, 1.0, 1.0), 101
    dt = OMEGA_DT / np.sqrt(B0.dot(B0))
    field = A.model("linear", E0=(0, 0, 0), B0=B0, r0=r0, g=g0)
    grid = T.grid_from_model(field, n, d)
    fo, gc = start(r0, v0, B0)
    out = T.triplet_trace(field, grid, d, fo, gc, gc, steps, "EB2B", Q / M, M, dt)
    assert out.dm_max[0] < 30 and out.dg_max[0] < 30
    B = np.sqrt(B0.dot(B0))
    V = np.array([0.0, 0.0, v0[2]])                                          # :105
    V = V + M * v0[2] ** 2 / (Q * B ** 3) * np.cross(B0, g0)                 # :106
    V = V + gc[0, 5] / (Q * B ** 2) * np.cross(B0, g0)                       # :107
    r_theory = gc[0, :3] + V * (dt * (steps))                                # :109-110, T = dt (geom_nt + 1)
    print("analytic", out.gm[0, :3] - r_theory, "grid", out.gg[0, :3] - r_theory, "stats", out.stats[0])
    assert np.abs(out.gm[0, :3] - r_theory).max() <= 1e-8                    # :112
    assert np.abs(out.gg[0, :3] - r_theory).max() <= 1e-8                    # :115
    # a linear field on a grid of its own nodes is interpolated to rounding: B, grad B and the two centres agree
    assert out.stats[0, :3].max() <= 1e-12 and np.isfinite(out.stats).all() and (out.stats[0, 3:] > 0).all()


def test_ex1_uniform_fields():
    """ex1.cpp: E0 = (0, 1, -1), B0 = (0, 0, 1); the checks of :105-126 for both guiding centres at 1e-4.  40 steps, as
    tests/test_paired_trace_ref.py: p_parallel reaches 4, 0.4 cells a step, inside the segment shape's one cell"""
    E0, B0 = np.array([0.0, 1.0, -1.0]), np.array([0.0, 0.0, 1.0])
    r0, v0, steps = np.array([2.0, 2.0, 2.0]), np.array([0.0, 0.1, 0.0]), 40
    dt = OMEGA_DT / np.sqrt(B0.dot(B0))
    field = A.model("uniform", E0=E0, B0=B0)
    E, B = FO.uniform_fields(E0, B0)
    fo, gc = start(r0, v0, B0)
    out = T.triplet_trace(field, (E, B, None), FO.D, fo, gc, gc, steps, "EB2B", Q / M, M, dt)
    Tt, q, E_par = dt * steps, Q / M, E0[2]
    z_theory = 0.5 * q * E_par * Tt * Tt
    r_theory = gc[0, :3] + np.cross(E0, B0) / B0.dot(B0) * Tt + np.array([0.0, 0.0, z_theory])
    for member in (out.gm[0], out.gg[0]):
        assert abs(member[3] - q * E_par * Tt) <= 1e-4
        assert abs(member[2] - (z_theory + r0[2])) <= 1e-4
        assert np.abs(member[:3] - r_theory).max() <= 1e-4
    # uniform fields: the grid's 64 weights sum to 1 within rounding, so both centres agree to rounding and grad B is 0
    assert out.stats[0, 0] <= 8 * EPS and out.stats[0, 1] == 0.0 and out.stats[0, 2] <= 1e-12


MIRROR = dict(A.QUADRATIC)
N, D = (9, 8, 7), (0.5, 0.4, 0.3)
STEPS, DT = 12, 0.05


@pytest.fixture(scope="module")
def mirror():
    """four triplets around (2, 1.5, 1) of the quadratic mirror sampled on a coarse periodic grid (which does not resolve
    it: the grid statistics are large, which is what exercises them)"""
    field = A.model("quadratic_mirror", **MIRROR)
    grid = T.grid_from_model(field, N, D)
    rng = np.random.default_rng(3)
    r = np.array([2.0, 1.5, 1.0]) + 0.3 * (rng.random((4, 3)) - 0.5)
    v = 0.3 * rng.normal(size=(4, 3))
    fo = np.column_stack([r, v])
    gc = np.array([A.point_by_field(p, field(p[None, :3])[1][0], M, Q / M) for p in fo])
    out = T.triplet_trace(field, grid, D, fo, gc, gc, STEPS, "EB2B", Q / M, M, DT, sample_every=1)
    return dict(field=field, grid=grid, fo=fo, gc=gc, out=out)


def _norm(v):
    return np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def test_statistics_equal_a_direct_evaluation(mirror):
    """The three trajectories stepped on their own, one triplet at a time, and the seven errors written out with unit
    vectors instead of parallel_to / transverse_to.  Either side makes about a dozen roundings relative to the operands of
    the final subtraction: 32 eps of the larger operand, the bound of tests/test_paired_trace_ref.py."""
    field, (E, B, gB), out = mirror["field"], mirror["grid"], mirror["out"]
    for q in range(4):
        fo, gm, gg = mirror["fo"][q:q + 1], mirror["gc"][q:q + 1], mirror["gc"][q:q + 1]
        m = np.zeros(7)
        for k in range(STEPS):
            gm, _ = A.dk_push(field, gm, Q / M, M, DT)
            old = gg
            gg, _ = DK.push(E, B, gB, D, old, Q / M, M, DT)
            fo = A.chin_step("EB2B", field, fo, Q / M, DT)
            _, Ba, gBa = (a[0] for a in field(gm[:, :3]))
            _, Bg, gBg = (a[0] for a in DK.interpolate(E, B, gB, D, gg[:, :3], old[:, :3]))
            p, b = fo[0, 3:], Ba / _norm(Ba)
            ppar = p.dot(b)
            perp2 = _norm(p - ppar * b) ** 2
            a_ = np.array([gg[0, 2], gg[0, 3], gg[0, 5], 0.5 * (gg[0, 4] ** 2 + gg[0, 3] ** 2)])
            b_ = np.array([fo[0, 2], abs(ppar), 0.5 * M * perp2 / _norm(Ba), 0.5 * p.dot(p)])
            direct = np.concatenate([[_norm(Ba - Bg), _norm(gBa - gBg), _norm(gm[0, :3] - gg[0, :3])], np.abs(a_ - b_)])
            scale = np.concatenate([[max(_norm(Ba), _norm(Bg)), max(_norm(gBa), _norm(gBg)),
                                     max(_norm(gm[0, :3]), _norm(gg[0, :3]))], np.maximum(np.abs(a_), np.abs(b_))])
            got = out.errors[k, q]
            assert (np.abs(got - direct) <= 32 * EPS * scale).all(), (q, k, got, direct)
            m = np.maximum(m, got)
        assert np.array_equal(out.fo[q], fo[0]) and np.array_equal(out.gm[q], gm[0]) and np.array_equal(out.gg[q], gg[0])
        assert np.array_equal(out.stats[q], m)
    assert np.array_equal(out.curve, out.errors.max(axis=1))
    assert (out.stats > 0).all()  # the coarse grid differs from the model in B, in grad B and in where the centre goes


def test_the_projection_is_on_the_analytic_field(mirror):
    """statistics 4 and 5 use B_analytical (drift_kinetic_push.h:314), where paired_trace_ref projects on B_grid: one
    step's errors on the triplet's own states are compare_step with Ba, and with Bg the magnetic moment, which |B|
    enters, comes out differently (this mirror's B is along z on either side, so the direction alone is the same), while z
    and the energy, which no field enters, are the same"""
    E, B, gB = mirror["grid"]
    out = T.triplet_trace(mirror["field"], mirror["grid"], D, mirror["fo"], mirror["gc"], mirror["gc"], 1, "EB2B", Q / M, M, DT)
    _, Bg, _ = DK.interpolate(E, B, gB, D, out.gg[:, :3], mirror["gc"][:, :3])
    Ba = mirror["field"](out.gm[:, :3])[1]
    assert np.array_equal(out.stats[:, 3:], P.compare_step(out.gg, out.fo, Ba, M))
    on_grid = P.compare_step(out.gg, out.fo, Bg, M)
    assert np.array_equal(out.stats[:, 3], on_grid[:, 0]) and np.array_equal(out.stats[:, 6], on_grid[:, 3])
    assert (out.stats[:, 5] != on_grid[:, 2]).all()


def test_accumulation_rule(mirror):
    """an infinite maximum is kept and a preloaded one is only raised; a NaN triplet leaves its maxima alone and the curve
    is that of the healthy triplets (without the grid member: drift_kinetic_ref's gather takes no NaN position)"""
    errors = mirror["out"].errors
    given = np.zeros((4, 7))
    given[1] = 1e-3
    given[2] = np.inf
    out = T.triplet_trace(mirror["field"], mirror["grid"], D, mirror["fo"], mirror["gc"], mirror["gc"], 3, "EB2B", Q / M, M,
                          DT, stats=given)
    assert np.isinf(out.stats[2]).all()
    assert np.array_equal(out.stats[1], np.maximum(1e-3, errors[:3, 1].max(axis=0)))
    assert np.array_equal(out.stats[[0, 3]], errors[:3, [0, 3]].max(axis=0))
    fo, gm = mirror["fo"].copy(), mirror["gc"].copy()
    fo[1, :3] = np.nan
    gm[1, :3] = np.nan
    given = np.zeros((4, 7))
    given[1] = np.arange(1.0, 8.0)
    with np.errstate(invalid="ignore"):
        out = T.triplet_trace(mirror["field"], None, D, fo, gm, None, 3, "EB2B", Q / M, M, DT, sample_every=1, stats=given,
                              dk_maxit=3)
    assert np.array_equal(out.stats[1], given[1]) and np.isnan(out.errors[:, 1, 3:]).all()
    assert np.isfinite(out.curve).all() and (out.curve[:, 3:] > 0).all()
    assert np.array_equal(out.curve[:, 3:], out.errors[:, [0, 2, 3], 3:].max(axis=1))
    assert out.dm_max[1] == 3  # a NaN residual meets no tolerance


def test_without_the_grid_member(mirror):
    """the grid-less pair: statistics 0 .. 2 come back as they went in, 3 .. 6 are paired_trace_ref.compare_step of the
    analytic centre and the orbit with B at the analytic centre, and both states are those of the triplet's members"""
    field = mirror["field"]
    given = np.zeros((4, 7))
    given[:, :3] = [[7.0, np.nan, -1.0]]
    out = T.triplet_trace(field, None, D, mirror["fo"], mirror["gc"], None, STEPS, "EB2B", Q / M, M, DT, sample_every=2,
                          stats=given)
    assert out.gg is None and not out.dg_total.any()
    assert out.stats[:, :3].tobytes() == given[:, :3].tobytes() and not out.curve[:, :3].any()
    assert np.array_equal(out.fo, mirror["out"].fo) and np.array_equal(out.gm, mirror["out"].gm)
    fo, gm, m = mirror["fo"], mirror["gc"], np.zeros((4, 4))
    for k in range(STEPS):
        gm, _ = A.dk_push(field, gm, Q / M, M, DT)
        fo = A.chin_step("EB2B", field, fo, Q / M, DT)
        e = P.compare_step(gm, fo, field(gm[:, :3])[1], M)
        assert np.array_equal(out.errors[k, :, 3:], e)
        m = np.maximum(m, e)
    assert np.array_equal(out.stats[:, 3:], m)
    assert np.array_equal(out.curve[:, 3:], out.errors[1::2, :, 3:].max(axis=1))
