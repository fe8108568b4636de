"""tests/set_particles_ref.py against closed forms (no GPU): the moments of the three generators it adds, composition
through particle0, and that it tells three deliberate mistakes from the definition."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import set_particles_ref as S  # noqa: E402

N = 1 << 16
M = 7.5
ANN = {"name": "CoordinateOnAnnulus", "center": (3.0, 2.0, 1.0), "inner_r": 0.5, "outer_r": 1.75, "height": 1.5}
BOX = {"name": "CoordinateInBox", "min": (0.0, 0.0, 0.0), "max": (6.0, 4.0, 2.0)}
COS = {"name": "MaxwellCosinePerturbation", "T": (1.0, 2.0, 0.5), "amplitude": (0.5, 0.25, 0.0), "wave_number": (2.0, 1.0, 3.0),
       "min": (0.0, 0.0, 0.0), "max": (6.0, 4.0, 2.0)}
ANG = {"name": "AngularMomentum", "T": (1.0, 4.0, 0.25), "drift": (0.0, 0.0, 0.0), "center": (3.0, 2.0, 0.0)}


def within6(x, mean, var):
    return abs(x.mean() - mean) <= 6 * math.sqrt(var / len(x))


def annulus_r2_is_uniform(bug=None):
    r, _ = S.draws(N, 3, 17, ANN, {"name": "PreciseMomentum", "value": (0.0, 0.0, 0.0)}, M, bug=bug)
    r2 = (r[:, 0] - ANN["center"][0]) ** 2 + (r[:, 1] - ANN["center"][1]) ** 2
    a, b = ANN["inner_r"] ** 2, ANN["outer_r"] ** 2
    assert r2.min() >= a * (1 - 1e-12) and r2.max() <= b * (1 + 1e-12)
    return within6(r2, 0.5 * (a + b), (b - a) ** 2 / 12) and within6(r2 * r2, (a * a + a * b + b * b) / 3,
                                                                      (b ** 5 - a ** 5) / (5 * (b - a)))


def test_annulus_moments():
    assert annulus_r2_is_uniform()
    r, _ = S.draws(N, 3, 17, ANN, {"name": "PreciseMomentum", "value": (0.0, 0.0, 0.0)}, M)
    h = ANN["height"]
    assert within6(r[:, 2], ANN["center"][2], h * h / 12)
    phi = np.arctan2(r[:, 1] - ANN["center"][1], r[:, 0] - ANN["center"][0])
    assert within6(np.cos(phi), 0.0, 0.5) and within6(np.sin(phi), 0.0, 0.5)


def test_angular_momentum_moments():
    r, p = S.draws(N, 0, 5, ANN, ANG, M)
    assert (p >= 0.0).all()  # no phase factor: the thermal part is a modulus
    for a in range(3):
        s2 = ANG["T"][a] * M / S.MEC2  # p^2 = -2 s2 ln u: mean 2 s2, variance 4 s2^2
        assert within6(p[:, a] ** 2, 2 * s2, 4 * s2 * s2)
    # without temperature: (-px y / r, +py x / r, pz), perpendicular to the radius when px == py
    cold = dict(ANG, T=(0.0, 0.0, 0.0), drift=(0.3, 0.3, -0.1))
    r, p = S.draws(1000, 0, 5, ANN, cold, M)
    x, y = r[:, 0] - 3.0, r[:, 1] - 2.0
    assert np.abs(p[:, 0] * x + p[:, 1] * y).max() <= 1e-15 * 4 and np.allclose(np.hypot(p[:, 0], p[:, 1]), 0.3, rtol=1e-14)
    assert (p[:, 2] == -0.1).all() and (p[:, 0] * y <= 0).all()
    # on the axis 1 / r is infinite: (0, 0, pz) plus the thermal part
    axis = {"name": "PreciseCoordinate", "value": (3.0, 2.0, 1.0)}
    _, p = S.draws(8, 0, 5, axis, cold, M)
    assert np.array_equal(p, np.tile([0.0, 0.0, -0.1], (8, 1)))


def test_cosine_perturbation_bin_means():
    r, p = S.draws(N, 2, 9, BOX, COS, M)
    L = [COS["max"][a] - COS["min"][a] for a in range(3)]
    for a in range(3):
        v0 = COS["amplitude"][a] * math.sqrt(COS["T"][a] / (M * S.MEC2))
        thermal = p[:, a] - v0 * np.cos(2 * np.pi * COS["wave_number"][a] * r[:, a] / L[a])
        # the thermal part is symmetric about 0 and at most |p| / m, <p^2> = T m / mec2
        bound = COS["T"][a] * M / S.MEC2 / (M * M)
        bins = np.minimum((r[:, a] / L[a] * 16).astype(int), 15)
        for b in range(16):
            assert within6(thermal[bins == b], 0.0, bound), (a, b)
        # (<p^2 / den^2> <= <p^2> / m^2, and the variance of p^2 is 2 <p^2>^2)
        assert 0.5 * bound < (thermal ** 2).mean() <= bound * (1 + 6 * math.sqrt(2 / N))
    # always divided by sqrt(m^2 + p^2), whatever tov says
    _, q = S.draws(N, 2, 9, BOX, dict(COS, tov=False, amplitude=(0.0, 0.0, 0.0)), M)
    _, mx = S.draws(N, 2, 9, BOX, {"name": "MaxwellianMomentum", "T": COS["T"], "tov": True}, M)
    assert np.array_equal(q, mx)


def test_composition_through_particle0():
    for coord, mom in ((ANN, ANG), (BOX, COS)):
        r, p = S.draws(257, 4, 21, coord, mom, M)
        r1, p1 = S.draws(100, 4, 21, coord, mom, M)
        r2, p2 = S.draws(157, 4, 21, coord, mom, M, particle0=100)
        assert np.array_equal(r, np.concatenate([r1, r2])) and np.array_equal(p, np.concatenate([p1, p2]))
    n, d = (12, 10, 8), (0.5, 0.4, 0.25)
    whole = S.set_particles(257, 4, 21, BOX, COS, M, 0.125, n, d)
    a = S.set_particles(100, 4, 21, BOX, COS, M, 0.125, n, d)
    b = S.set_particles(157, 4, 21, BOX, COS, M, 0.125, n, d, particle0=100)
    assert whole[2] == a[2] + b[2] and abs(whole[3] - (a[3] + b[3])) <= 1e-14 * whole[3]
    # slabs: every record lies in exactly one
    parts = [S.set_particles(257, 4, 21, BOX, COS, M, 0.125, (12, 10, 9), d, z0=3 * k, nzl=3) for k in range(3)]
    one = S.set_particles(257, 4, 21, BOX, COS, M, 0.125, (12, 10, 9), d)
    assert sum(q[2] for q in parts) == one[2]


def test_the_restatement_sees_the_amplitude_drawn_before_the_phase():
    _, p = S.draws(1000, 2, 9, BOX, COS, M)
    _, q = S.draws(1000, 2, 9, BOX, COS, M, bug="amplitude_first")
    assert (np.abs(p - q).max(axis=1) > 1e-6).mean() > 0.99


def test_the_restatement_sees_a_radius_linear_in_u():
    assert annulus_r2_is_uniform() and not annulus_r2_is_uniform(bug="linear_radius")


def test_the_count_is_truncated_not_rounded():
    d, L = (0.5, 0.4, 0.25), (6.0, 4.0, 2.0)
    box = {"name": "CoordinateInBox", "min": (0.0, 0.0, 0.0), "max": (0.625, 0.4, 0.25)}  # 1.25 cells, Np 7: 8.75
    assert S.particles_number(box, 7, d, L) == 8 and S.particles_number(box, 7, d, L, bug="rounded_count") == 9
    # the annulus: pi (outer^2 - inner^2) h Np / (dx dy dz)
    v = math.pi * (1.75 ** 2 - 0.5 ** 2) * 1.5 * (7 / 0.05)
    assert v - int(v) > 0.5 and S.particles_number(ANN, 7, d, L) == int(v) == 1855
    assert S.particles_number(ANN, 7, d, L, bug="rounded_count") == 1856
    assert S.particles_number({"name": "PreciseCoordinate", "value": (1, 1, 1)}, 7, d, L) == 7
    cyl = {"name": "CoordinateInCylinder", "center": (3, 2, 1), "radius": 1.0, "height": 2.0}
    assert S.particles_number(cyl, 7, d, L) == int(math.pi * 1.0 * 2.0 * (7 / (0.5 * 0.4 * 0.25)))
