"""CPU checks of tests/commands_ref.py, the model the GPU commands are tested against: hand-computed values of the damping
profiles as the reference writes them, the corner rule of RemoveParticles, the coils quadrature against the field of a
loop on its axis, the builders' arithmetic and the counter-based stream."""
import math

import numpy as np
import pytest

import commands_ref as R

L = (10.0, 10.0, 10.0)
BOX = {"name": "box", "min": (2.0, 0.0, 0.0), "max": (8.0, 10.0, 10.0)}
CYL = {"name": "cylinder", "center": (5.0, 5.0, 5.0), "radius": 3.0, "height": 6.0}


def _bx(x):
    return float(R.damp_box(np.array([x, 5.0, 5.0]), BOX, 0.5, L))


def test_box_damping_as_written():
    # lower side: width = min - 0, delta = x - 0: 1 - c at the WALL, 1 at the interface
    assert _bx(0.0) == 0.5
    assert _bx(1.0) == 1.0 - 0.5 * 0.25
    assert abs(_bx(2.0 - 1e-12) - 1.0) < 1e-12
    # upper side: width = L - max, delta = x - max: 1 - c at the INTERFACE, 1 at the wall
    assert abs(_bx(8.0 + 1e-12) - 0.5) < 1e-12
    assert _bx(9.0) == 1.0 - 0.5 * 0.25
    assert _bx(10.0) == 1.0
    # x == max is outside the half-open box but on neither side: factor 1
    assert _bx(8.0) == 1.0
    assert not R.within(BOX, 8.0, 5.0, 5.0) and R.within(BOX, 2.0, 5.0, 5.0)
    # the factors of the axes multiply
    r = np.array([1.0, 5.0, 5.0])
    box3 = {"name": "box", "min": (2.0, 2.0, 2.0), "max": (8.0, 8.0, 8.0)}
    r[1] = 9.0
    assert float(R.damp_box(r, box3, 0.5, L)) == (1.0 - 0.5 * 0.25) ** 2


def _cy(rr):
    return float(R.damp_cylinder(np.array([5.0 + rr, 5.0, 5.0]), CYL, 0.25))


def test_cylinder_damping_as_written():
    # width = center x - radius = 2, delta0 = width (1 + 1/sqrt(c)) = 6
    assert _cy(2.9) == 1.0
    assert _cy(3.0) == 1.0 - 0.25
    assert _cy(5.0) == 1.0
    assert _cy(8.9) == pytest.approx(1.0 - 0.25 * (5.9 / 2 - 1) ** 2, rel=1e-14)
    assert _cy(9.0) == 0.0 and _cy(12.0) == 0.0  # zero from delta0 outwards
    # the cylinder test is strict in z, inclusive in r
    assert R.within(CYL, 8.0, 5.0, 5.0) and not R.within(CYL, 5.0, 5.0, 8.0) and R.within(CYL, 5.0, 5.0, 7.999)


def test_damping_energy_and_b0():
    n, d = (10, 10, 10), (1.0, 1.0, 1.0)
    rng = np.random.default_rng(0)
    E, B, B0 = rng.normal(size=(3, 10, 10, 10, 3))
    E2, B2, e = R.damping(E, B, B0, BOX, 0.5, n, d)
    inside = np.zeros((10, 10, 10), bool)
    inside[:, :, 2:8] = True  # centres 2.5 .. 7.5
    assert np.array_equal(E2[inside], E[inside])
    fac = np.array([R.damp_box(np.array([x + 0.5, 0, 0]), BOX, 0.5, L) for x in range(10)])
    assert np.allclose(E2, E * fac[None, None, :, None], rtol=1e-15, atol=0)
    assert np.allclose(B2 - B0, (B - B0) * fac[None, None, :, None], rtol=1e-14, atol=1e-15)
    k = (1 - fac ** 2)[None, None, :]
    ref = (0.5 * (E ** 2).sum(-1) * k).sum() + (0.5 * ((B - B0) ** 2).sum(-1) * k).sum()
    assert e == pytest.approx(ref, rel=1e-13)


def test_removal_tests_the_corner_not_the_centre():
    n, d = (4, 4, 4), (1.0, 1.0, 1.0)
    box = {"name": "box", "min": (0.2, 0.0, 0.0), "max": (4.0, 4.0, 4.0)}
    cells = np.array([0, 1])  # cells (0,0,0) and (1,0,0)
    assert not R.within(box, *R.cell_corner(cells[:1], n, d))[0]  # corner (0,0,0) fails
    assert R.within(box, *R.cell_centre(cells[:1], n, d))[0]      # the centre (0.5,..) would pass
    pts = np.zeros((3, 6))
    pts[:, 3:] = [[0.1, 0.0, 0.0], [0.0, 0.2, 0.0], [0.3, 0.0, 0.0]]
    keep, k, e = R.remove(pts, np.array([0, 0, 1]), box, n, d, 2.0, 0.5)
    assert list(keep) == [False, False, True] and k == 2
    assert e == pytest.approx(0.5 * 2.0 * (0.01 + 0.04) * 0.5, rel=1e-15)


def test_coils_on_axis_match_the_loop_field():
    """Bz of one loop on its axis, B_z = I R^2 2 pi / (R^2 + z^2)^(3/2) in the reference's units (the quadrature of a
    constant integrand: exact to rounding); Br vanishes there"""
    Rc, I, z0 = 2.5, 1.7, 3.0
    for z in (0.0, 1.0, 3.0, 7.25):
        bz = float(R.coils_Bz(np.array(z), np.array(0.0), [(z0, Rc, I)]))
        ref = I * Rc ** 2 * 2 * math.pi / (Rc ** 2 + (z - z0) ** 2) ** 1.5
        assert bz == pytest.approx(ref, rel=1e-13)
        assert abs(float(R.coils_Br(np.array(z), np.array(0.0), [(z0, Rc, I)]))) < 1e-12 * abs(ref)
    # a node on the axis: odd nx, ny put the Bz nodes on it; even nx with odd ny a Bx node (0 / 0 there, as in the reference)
    f = R.coils_field((5, 5, 4), (1.0, 1.0, 1.0), [(2.0, 1.5, 1.0)])
    assert np.isfinite(f[..., 2]).all()
    ref = 1.5 ** 2 * 2 * math.pi / (1.5 ** 2 + (np.arange(4) - 2.0) ** 2) ** 1.5
    assert np.allclose(f[:, 2, 2, 2], ref, rtol=1e-13)
    g = R.coils_field((4, 5, 2), (1.0, 1.0, 1.0), [(1.0, 1.5, 1.0)])
    assert np.isnan(g[:, 2, 2, 0]).all() and np.isfinite(g[..., 2]).all()


def test_coils_off_axis_against_elliptic_integrals():
    """the quadrature against the closed form of a loop's field (complete elliptic integrals by the AGM), far from the
    wire: the periodic trapezoid rule converges geometrically"""
    def ellipk_e(m):
        a, b, p = 1.0, math.sqrt(1 - m), 1.0
        s = 0.5 * m
        for _ in range(30):  # (quadratic convergence: a handful of rounds reach rounding)
            a, b, c = 0.5 * (a + b), math.sqrt(a * b), 0.5 * (a - b)
            p *= 2
            s += 0.5 * p * c * c
        K = math.pi / (2 * a)
        return K, K * (1 - s)

    Rc, I = 2.0, 1.0
    for (z, r) in ((0.5, 1.0), (1.5, 3.0), (-2.0, 0.7)):
        m = 4 * Rc * r / ((Rc + r) ** 2 + z ** 2)
        K, Ek = ellipk_e(m)
        q = math.sqrt((Rc + r) ** 2 + z ** 2)
        # loop field with mu0 I / (4 pi) -> I (the quadrature's normalisation: Bz(0, 0) = 2 pi I / R)
        bz = 2 * I / q * (K + (Rc ** 2 - r ** 2 - z ** 2) / ((Rc - r) ** 2 + z ** 2) * Ek)
        br = 2 * I * z / (r * q) * (-K + (Rc ** 2 + r ** 2 + z ** 2) / ((Rc - r) ** 2 + z ** 2) * Ek)
        assert float(R.coils_Bz(np.array(z), np.array(r), [(0.0, Rc, I)])) == pytest.approx(bz, rel=1e-9)
        assert float(R.coils_Br(np.array(z), np.array(r), [(0.0, Rc, I)])) == pytest.approx(br, rel=1e-9)


def test_inject_builder_arithmetic():
    d, dt, Lg = (0.5, 0.5, 0.5), 0.25, (10.0, 10.0, 10.0)
    box = {"name": "CoordinateInBox", "min": (0.0, 0.0, 0.0), "max": (1.0, 2.0, 1.5)}
    # number = volume * Np / (dx dy dz) = 3 * 10 / 0.125 = 240; default window [0, 1]: tau = 1
    assert R.particles_number(box, 10, d, Lg) == 240
    assert R.inject_schedule({"coordinate": box}, 10, d, dt, Lg, 40) == (0, 1, 240)
    # injection_end in time units -> ROUND_STEP(end, dt); tau from the window, integer division
    assert R.inject_schedule({"coordinate": box, "injection_start": 0.5, "injection_end": 2.6}, 10, d, dt, Lg, 40) == (2, 10, 30)
    assert R.inject_schedule({"coordinate": box, "injection_end": "geom_t", "tau": 1.75}, 10, d, dt, Lg, 40) == (0, 40, 34)
    assert R.inject_schedule({"coordinate": box, "per_step_particles_num": 7}, 10, d, dt, Lg, 40)[2] == 7
    cyl = {"name": "CoordinateInCylinder", "radius": 1.0, "height": 2.0}
    assert R.particles_number(cyl, 4, d, Lg) == int(math.pi * 2.0 * 32)
    assert R.particles_number({"name": "PreciseCoordinate", "value": (1, 1, 1)}, 9, d, Lg) == 9
    with pytest.raises(ZeroDivisionError):
        R.inject_schedule({"coordinate": box, "tau": 0.05}, 10, d, dt, Lg, 40)
    assert [t for t in range(6) if R.injects_at(t, 1, 3)] == [1, 2, 3]
    assert R.round_step(0.375, 0.25) == 2 and R.round_step(-0.375, 0.25) == -2


def test_stream_is_splitmix():
    """the numpy stream equals a scalar restatement of splitmix64 keyed as commands.hip keys it"""
    key = R.stream_key(5, 3)
    S = R._Stream(key, 4)
    a = S.u01()
    for p in range(4):
        st = (key + p * 0x2545F4914F6CDD1D) & R.M64
        st, z = R._splitmix_int(st)
        assert a[p] == ((z >> 11) + 0.5) / 2.0 ** 53
    assert 0.0 < a.min() and a.max() < 1.0
    r, pi, pe = R.inject_draws(20000, 2, 9, {"name": "CoordinateInCylinder", "center": (5, 5, 5), "radius": 2.0,
                                            "height": 4.0}, {"name": "MaxwellianMomentum", "T": (1.0, 2.0, 3.0)},
                               {"name": "PreciseMomentum", "value": (0.1, 0.2, 0.3)}, 1.0, 2.0)
    rr2 = (r[:, 0] - 5) ** 2 + (r[:, 1] - 5) ** 2
    assert rr2.max() <= 4.0 and abs(r[:, 2] - 5).max() <= 2.0
    assert abs(rr2.mean() - 2.0) < 6 * math.sqrt(4.0 / 12 * 4 / 20000) * 2
    assert np.allclose(pi.var(axis=0), np.array([1.0, 2.0, 3.0]) / 511.0, rtol=0.1)
    assert (pe == [0.1, 0.2, 0.3]).all()
