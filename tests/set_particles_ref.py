"""numpy float64 restatement of SetParticles on the device (include/xpic_set_particles.h; xpic_amd/csrc/commands.hip): the
reference's generators (src/utils/particles_load.cpp:6-125) on this build's counter-based stream.  The stream, the three
coordinate and two momentum generators InjectParticles has, the cell test, the energy and the builder's count come from
tests/commands_ref.py; CoordinateOnAnnulus, MaxwellCosinePerturbation, AngularMomentum and the annulus count are added here.

Generators are dicts as Context.set_particles takes them.  `bug` switches one deliberate mistake on (the tests show that
the restatement tells them apart): "amplitude_first", "linear_radius", "rounded_count".
"""
import math

import numpy as np

from commands_ref import (MEC2, _coordinate, _momentum, _Stream, kinetic, local_cells,  # noqa: F401
                          particles_number as _particles_number, stream_key)


def coordinate(S, gen, n, bug=None):
    if gen["name"] != "CoordinateOnAnnulus":
        return _coordinate(S, gen, n)
    c, ri, ro, h = gen["center"], gen["inner_r"], gen["outer_r"], gen["height"]
    u = S.u01()
    rr = ri + (ro - ri) * u if bug == "linear_radius" else np.sqrt(ri * ri + (ro * ro - ri * ri) * u)
    phi = 2.0 * np.pi * S.u01()
    z = c[2] + h * (S.u01() - 0.5)
    return np.stack([c[0] + rr * np.cos(phi), c[1] + rr * np.sin(phi), z], axis=1)


def _thermal(S, T, m):
    """temperature_momentum (:52-55)"""
    return np.sqrt(-2.0 * (T * m / MEC2) * np.log(S.u01()))


def momentum(S, gen, m, r, bug=None):
    n = len(r)
    name = gen["name"]
    T = gen.get("T", (0.0, 0.0, 0.0))
    if name == "MaxwellCosinePerturbation":
        p = np.empty((n, 3))
        for a in range(3):
            if bug == "amplitude_first":
                amp = _thermal(S, T[a], m)
                ph = np.sin(2.0 * np.pi * S.u01())
            else:
                ph = np.sin(2.0 * np.pi * S.u01())
                amp = _thermal(S, T[a], m)
            p[:, a] = ph * amp
        den = np.sqrt(m * m + (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1] + p[:, 2] * p[:, 2]))
        p = p / den[:, None]
        for a in range(3):
            v0 = gen["amplitude"][a] * math.sqrt(T[a] / (m * MEC2))
            L = gen["max"][a] - gen["min"][a]
            p[:, a] = p[:, a] + v0 * np.cos(2.0 * np.pi * gen["wave_number"][a] * r[:, a] / L)
        return p
    if name == "AngularMomentum":
        drift, c = gen.get("drift", (0.0, 0.0, 0.0)), gen["center"]
        x, y = r[:, 0] - c[0], r[:, 1] - c[1]
        rr = np.hypot(x, y)
        t = [_thermal(S, T[a], m) for a in range(3)]
        with np.errstate(divide="ignore", invalid="ignore"):
            axis = np.isinf(1.0 / rr)
            px = np.where(axis, 0.0, -drift[0] * (y / rr)) + t[0]
            py = np.where(axis, 0.0, +drift[1] * (x / rr)) + t[1]
        return np.stack([px, py, drift[2] + t[2]], axis=1)
    return _momentum(S, gen, m, n)


def draws(n, step, seed, coord, mom, m, particle0=0, bug=None):
    """the coordinates and momenta of the particles particle0 .. particle0 + n - 1, in the draw order of commands.hip"""
    S = _Stream(stream_key(seed, step), particle0 + n)
    S.st = S.st[particle0:]
    r = coordinate(S, coord, n, bug)
    return r, momentum(S, mom, m, r, bug)


def set_particles(n, step, seed, coord, mom, m, mpw, grid_n, grid_d, particle0=0, z0=0, nzl=None, bug=None):
    """-> (records (added, 6), their local cells, added, energy) of one slab"""
    r, p = draws(n, step, seed, coord, mom, m, particle0, bug)
    cells = local_cells(r, grid_n, grid_d, z0, nzl)
    ok = cells >= 0
    return np.concatenate([r[ok], p[ok]], axis=1), cells[ok], int(ok.sum()), float(kinetic(p[ok], m, mpw).sum())


def face_distance(r, grid_d):
    """the smallest distance of a coordinate from a cell face, in cell widths"""
    if len(r) == 0:
        return np.inf
    s = r / np.asarray(grid_d, dtype=np.float64)
    return float(np.abs(s - np.round(s)).min())


def particles_number(coord, Np, d, L, bug=None):
    """ParticlesBuilder::load_coordinate's count, truncated; the annulus (an extension): pi (outer^2 - inner^2) h frac"""
    if coord["name"] != "CoordinateOnAnnulus":
        if bug == "rounded_count" and coord["name"] == "CoordinateInBox":
            lo, hi = coord["min"], coord["max"]
            return int(round((hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2]) * (Np / (d[0] * d[1] * d[2]))))
        return _particles_number(coord, Np, d, L)
    frac = Np / (d[0] * d[1] * d[2])
    v = math.pi * (coord["outer_r"] * coord["outer_r"] - coord["inner_r"] * coord["inner_r"]) * coord["height"] * frac
    return int(round(v)) if bug == "rounded_count" else int(v)
