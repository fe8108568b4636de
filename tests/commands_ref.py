"""numpy restatement of the reference's per-step commands (src/commands/), the model the HIP path (xpic_amd/csrc/commands.hip)
is tested against: the geometry tests (src/utils/geometries.cpp:3-19), RemoveParticles (remove_particles.cpp:11-40),
FieldsDamping with both profiles as written (fields_damping.cpp:15-111), the SetCoilsField quadrature
(set_magnetic_field.cpp:38-150), InjectParticles' generators (src/utils/particles_load.cpp:6-76) on this build's
counter-based stream, and the builders' arithmetic (inject_particles_builder.cpp:11-71, particles_builder.cpp:10-38).

Geometries are dicts: {"name": "box", "min": xyz, "max": xyz} or {"name": "cylinder", "center": xyz, "radius": r,
"height": h}.  Fields are (nz, ny, nx, 3) arrays, positions in the reference's units.
"""
import math

import numpy as np

MEC2 = 511.0  # src/constants.h:30
COIL_N = 2000  # SetCoilsField::N
COIL_TOL = 1e-10  # SetCoilsField::denominator_tolerance
M64 = (1 << 64) - 1


def _kind(geometry):
    return {"box": 0, "BoxGeometry": 0, "cylinder": 1, "CylinderGeometry": 1}[geometry["name"]]


def within(geometry, x, y, z):
    """WithinBox (half-open) / WithinCylinder (strict |z| < h/2, r^2 <= R^2) of arrays of points"""
    x, y, z = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64), np.asarray(z, dtype=np.float64)
    if _kind(geometry) == 0:
        lo, hi = geometry["min"], geometry["max"]
        return (lo[0] <= x) & (x < hi[0]) & (lo[1] <= y) & (y < hi[1]) & (lo[2] <= z) & (z < hi[2])
    c, R, h = geometry["center"], geometry["radius"], geometry["height"]
    px, py, pz = x - c[0], y - c[1], z - c[2]
    return (np.abs(pz) < 0.5 * h) & ((px * px + py * py) <= R * R)


def cell_corner(cells, n, d, z0=0):
    """(start + g) d of local cell indices g -- the point RemoveParticles tests"""
    cells = np.asarray(cells, dtype=np.int64)
    x, y, z = cells % n[0], (cells // n[0]) % n[1], cells // (n[0] * n[1]) + z0
    return x * d[0], y * d[1], z * d[2]


def cell_centre(cells, n, d, z0=0):
    """(start + g + 1/2) d -- the point VelocityDistribution and FieldsDamping test"""
    cells = np.asarray(cells, dtype=np.int64)
    x, y, z = cells % n[0], (cells // n[0]) % n[1], cells // (n[0] * n[1]) + z0
    return (x + 0.5) * d[0], (y + 0.5) * d[1], (z + 0.5) * d[2]


def kinetic(v, m, mpw):
    """Energy::get_kinetic (energy.cpp:188-191) of each row of v"""
    v = np.asarray(v, dtype=np.float64)
    return 0.5 * (m * (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])) * mpw


def remove(pts, cells, geometry, n, d, m, mpw, z0=0):
    """RemoveParticles on records in storage order with their local cells -> (kept mask, removed count, removed energy)"""
    keep = within(geometry, *cell_corner(cells, n, d, z0))
    gone = ~keep
    return keep, int(gone.sum()), float(kinetic(pts[gone, 3:], m, mpw).sum())


def damp_box(r, geometry, coef, L):
    """DampForBox (fields_damping.cpp:71-94) as written, r: (..., 3)"""
    r = np.asarray(r, dtype=np.float64)
    lo, hi = geometry["min"], geometry["max"]
    damping = np.ones(r.shape[:-1])
    for i in range(3):
        g = r[..., i]
        up, down = g > hi[i], g < lo[i]
        width = np.where(up, L[i] - hi[i], np.where(down, lo[i] - 0.0, 1.0))
        delta = np.where(up, g - hi[i], np.where(down, g - 0.0, 0.0))
        q = delta / width - 1.0
        damping = np.where(up | down, damping * (1.0 - coef * (q * q)), damping)
    return damping


def damp_cylinder(r, geometry, coef):
    """DampForCylinder (fields_damping.cpp:96-111) as written: width = center x - radius, 0 from delta0 outwards"""
    r = np.asarray(r, dtype=np.float64)
    c, R = geometry["center"], geometry["radius"]
    rr = np.hypot(r[..., 0] - c[0], r[..., 1] - c[1])
    width = c[0] - R
    delta = rr - R
    delta0 = width * (1.0 + 1.0 / math.sqrt(coef))
    q = delta / width - 1.0
    damping = np.where(delta < delta0, 1.0 - coef * (q * q), 0.0)
    return np.where(rr < R, 1.0, damping)


def damp_factor(r, geometry, coef, L):
    return damp_box(r, geometry, coef, L) if _kind(geometry) == 0 else damp_cylinder(r, geometry, coef)


def damping(E, B, B0, geometry, coef, n, d, z0=0):
    """FieldsDamping::execute on one slab -> (E', B', energy): E and B - B0 scaled outside the geometry at the cell centres,
    B = (B - B0) + B0 everywhere, energy = sum 0.5 |f|^2 (1 - damping^2)"""
    nz = E.shape[0]
    z, y, x = np.meshgrid(np.arange(nz) + z0, np.arange(n[1]), np.arange(n[0]), indexing="ij")
    r = np.stack([(x + 0.5) * d[0], (y + 0.5) * d[1], (z + 0.5) * d[2]], axis=-1)
    L = [n[i] * d[i] for i in range(3)]
    inside = within(geometry, r[..., 0], r[..., 1], r[..., 2])
    fac = np.where(inside, 1.0, damp_factor(r, geometry, coef, L))
    fe = E.copy()
    fb = B + (-1.0 * B0)
    k = np.where(inside, 0.0, 1.0 - fac * fac)
    energy = float(((0.5 * (fe[..., 0] * fe[..., 0] + fe[..., 1] * fe[..., 1] + fe[..., 2] * fe[..., 2])) * k).sum()
                   + ((0.5 * (fb[..., 0] * fb[..., 0] + fb[..., 1] * fb[..., 1] + fb[..., 2] * fb[..., 2])) * k).sum())
    f3 = np.where(inside, 1.0, fac)[..., None]
    fe = np.where(inside[..., None], fe, fe * f3)
    fb = np.where(inside[..., None], fb, fb * f3)
    return fe, fb + 1.0 * B0, energy


# ---- SetCoilsField
def _coil_cos():
    hp = 2 * math.pi / COIL_N
    return hp, [math.cos(i * hp) for i in range(COIL_N)]


def coil_integral(z, r, R, radial):
    """get_integ_r / get_integ_z (set_magnetic_field.cpp:118-150), summed over i in order"""
    hp, cs = _coil_cos()
    z, r = np.asarray(z, dtype=np.float64), np.asarray(r, dtype=np.float64)
    integral = np.zeros(np.broadcast(z, r).shape)
    for c in cs:
        den = z * z + R * R + r * r - 2.0 * R * r * c
        den = np.where(np.abs(den) < COIL_TOL, COIL_TOL, den)
        integral = integral + (c if radial else (R - r * c)) / (den * np.sqrt(den))
    return hp * integral


def coils_Br(z, r, coils):
    Br = 0.0
    for z0, R, I in coils:
        zc = z - z0
        Br = Br + I * R * zc * coil_integral(zc, r, R, True)
    return Br


def coils_Bz(z, r, coils):
    Bz = 0.0
    for z0, R, I in coils:
        zc = z - z0
        Bz = Bz + I * R * coil_integral(zc, r, R, False)
    return Bz


def coils_field(n, d, coils, nz=None, z0=0):
    """SetCoilsField's contribution at every node of a slab, (nz, ny, nx, 3), at the staggered positions it writes; a Bx or
    By node on the axis is 0 / 0 (NaN) as there"""
    nz = n[2] if nz is None else nz
    z, y, x = np.meshgrid(np.arange(nz) + z0, np.arange(n[1]), np.arange(n[0]), indexing="ij")
    cx, cy = 0.5 * n[0] * d[0], 0.5 * n[1] * d[1]
    out = np.zeros((nz, n[1], n[0], 3))
    with np.errstate(invalid="ignore", divide="ignore"):
        sx, sy, sz = x * d[0] - cx, (y + 0.5) * d[1] - cy, (z + 0.5) * d[2]
        r = np.hypot(sx, sy)
        out[..., 0] = coils_Br(sz, r, coils) * sx / r
        sy, sx, sz = y * d[1] - cy, (x + 0.5) * d[0] - cx, (z + 0.5) * d[2]
        r = np.hypot(sx, sy)
        out[..., 1] = coils_Br(sz, r, coils) * sy / r
        sz, sx, sy = z * d[2], (x + 0.5) * d[0] - cx, (y + 0.5) * d[1] - cy
        r = np.hypot(sx, sy)
        out[..., 2] = coils_Bz(sz, r, coils)
    return out


# ---- InjectParticles on this build's stream (xpic_amd/csrc/device_common.h: splitmix / u01; commands.hip: pair_stream)
def _splitmix_int(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return x, z ^ (z >> 31)


def stream_key(seed, step):
    k, _ = _splitmix_int(seed & M64)
    k ^= (step * 0xD1342543DE82EF95) & M64
    _, out = _splitmix_int(k)
    return out


class _Stream:
    """the per-pair states key + p * C; each draw advances every state by one splitmix step"""

    def __init__(self, key, pairs):
        with np.errstate(over="ignore"):
            self.st = np.uint64(key) + np.arange(pairs, dtype=np.uint64) * np.uint64(0x2545F4914F6CDD1D)

    def u01(self):
        with np.errstate(over="ignore"):
            self.st = self.st + np.uint64(0x9E3779B97F4A7C15)
            z = self.st.copy()
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            z = z ^ (z >> np.uint64(31))
        return ((z >> np.uint64(11)).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


def _coordinate(S, coordinate, pairs):
    name = coordinate["name"]
    if name == "CoordinateInBox":
        lo, hi = coordinate["min"], coordinate["max"]
        return np.stack([lo[a] + S.u01() * (hi[a] - lo[a]) for a in range(3)], axis=1)
    if name == "CoordinateInCylinder":
        c, R, h = coordinate["center"], coordinate["radius"], coordinate["height"]
        rr = R * np.sqrt(S.u01())
        phi = 2.0 * np.pi * S.u01()
        z = c[2] + h * (S.u01() - 0.5)
        return np.stack([c[0] + rr * np.cos(phi), c[1] + rr * np.sin(phi), z], axis=1)
    return np.tile(np.asarray(coordinate["value"], dtype=np.float64), (pairs, 1))


def _momentum(S, mom, m, pairs):
    if mom["name"] == "MaxwellianMomentum":
        T, drift = mom.get("T", (0.0, 0.0, 0.0)), mom.get("drift", (0.0, 0.0, 0.0))
        p = np.empty((pairs, 3))
        for a in range(3):
            ph = np.sin(2.0 * np.pi * S.u01())
            amp = np.sqrt(-2.0 * (T[a] * m / MEC2) * np.log(S.u01()))
            p[:, a] = drift[a] + ph * amp
        if mom.get("tov", False):
            den = np.sqrt(m * m + (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1] + p[:, 2] * p[:, 2]))
            p = p / den[:, None]
        return p
    return np.tile(np.asarray(mom["value"], dtype=np.float64), (pairs, 1))


def inject_draws(pairs, step, seed, coordinate, momentum_i, momentum_e, m_i, m_e):
    """every pair's shared coordinate and the two momenta, in the draw order of commands.hip"""
    S = _Stream(stream_key(seed, step), pairs)
    r = _coordinate(S, coordinate, pairs)
    pi = _momentum(S, momentum_i, m_i, pairs)
    pe = _momentum(S, momentum_e, m_e, pairs)
    return r, pi, pe


def local_cells(r, n, d, z0=0, nzl=None):
    """add_particle's FLOOR_STEP test (src/interfaces/particles.cpp:47-67): local cell of each point, -1 outside the slab"""
    nzl = n[2] if nzl is None else nzl
    c = [np.floor(r[:, a] / d[a]).astype(np.int64) for a in range(3)]
    c[2] = c[2] - z0
    ok = (c[0] >= 0) & (c[0] < n[0]) & (c[1] >= 0) & (c[1] < n[1]) & (c[2] >= 0) & (c[2] < nzl)
    return np.where(ok, (c[2] * n[1] + c[1]) * n[0] + c[0], -1)


# ---- builders
def round_step(s, ds):
    """ROUND_STEP (src/utils/utils.h:73): std::round, half away from zero"""
    v = s / ds
    return int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


def particles_number(coordinate, Np, d, L):
    """ParticlesBuilder::load_coordinate's number_of_particles (particles_builder.cpp:10-38), truncated to PetscInt"""
    frac = Np / (d[0] * d[1] * d[2])
    name = coordinate["name"]
    if name == "PreciseCoordinate":
        return int(Np)
    if name == "CoordinateInBox":
        lo, hi = coordinate.get("min", (0.0, 0.0, 0.0)), coordinate.get("max", L)
        return int((hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2]) * frac)
    R = coordinate.get("radius", 0.5 * min(L[0], L[1]))
    h = coordinate.get("height", L[2])
    return int(math.pi * (R * R) * h * frac)


def inject_schedule(info, Np, d, dt, L, geom_nt):
    """InjectParticlesBuilder::build (inject_particles_builder.cpp:11-71) -> (start, end, per-step pairs)"""
    start, end = 0, 1
    if "injection_start" in info:
        start = round_step(info["injection_start"], dt)
    if "injection_end" in info:
        v = info["injection_end"]
        if isinstance(v, str):
            if v == "geom_t":
                end = geom_nt
        else:
            end = round_step(v, dt)
    number = particles_number(info["coordinate"], Np, d, L)
    tau = end - start
    if "tau" in info:
        tau = round_step(info["tau"], dt)
    if tau == 0:
        raise ZeroDivisionError("InjectParticles: tau == 0")
    per_step = abs(number) // abs(tau) * (1 if (number >= 0) == (tau > 0) else -1)  # PetscInt division: toward zero
    if "per_step_particles_num" in info:
        per_step = int(info["per_step_particles_num"])
    return start, end, per_step


def injects_at(t, start, end):
    """InjectParticles::execute's window (inject_particles.cpp:32-33)"""
    return start <= t <= end
