"""numpy restatement of the open-trap traces (include/xpic_hip.h: xpic_trace_region) and the inputs of their tests:

  mirror_field(...)   SetApproximateMirrorField::operator() (src/commands/set_magnetic_field.cpp:142-191), vectorised
  keep(...)           RemoveParticles' rule (src/commands/remove_particles.cpp:22-38) for single particles: the corner of
                      the particle's cell, FLOOR_STEP of the unfolded position, tested with commands_ref.within
  trace_open(...)     the step loop of an open trace around any one-step pusher: tests/test_open_trace_ref.py runs it around
                      the numpy pushers (full_orbit_ref.step / cn_step, drift_kinetic_ref.push), tests/test_gpu_open_trace.py
                      around the device's one-step calls, whose bits the device's open trace must then return
  fields(), particles(...), REGION, ...   the inputs of those tests
"""
import collections

import numpy as np

import commands_ref as C
import drift_kinetic_ref as DK
import full_orbit_ref as FO

OpenRef = collections.namedtuple("OpenRef", "state samples exit_step alive removed iterations_sum iterations_max")


def mirror_field(n, d, D, R, I):
    """the (nz, ny, nx, 3) array the setter adds: both transverse terms in the X component at (z + 1/2) dz, B0 in the Z
    component at z dz, nothing in Y"""
    z, y, x = np.meshgrid(np.arange(n[2], dtype=np.float64), np.arange(n[1], dtype=np.float64),
                          np.arange(n[0], dtype=np.float64), indexing="ij")

    def B0(z, sign):
        return 0.5 * I * (R * R) / np.power(R * R + (z + 0.5 * sign * D) ** 2, 1.5)

    def B1(z, sign):
        return (z + 0.5 * sign * D) / (R * R + (z + 0.5 * sign * D) ** 2)

    out = np.zeros((n[2], n[1], n[0], 3))
    sz = (z + 0.5) * d[2]
    for sm in (1.5 * (x * d[0] - 0.5 * (n[0] * d[0])), 1.5 * (y * d[1] - 0.5 * (n[1] * d[1]))):
        out[..., 0] += B0(sz, +1.0) * sm * B1(sz, +1.0)
        out[..., 0] += B0(sz, -1.0) * sm * B1(sz, -1.0)
    sz = z * d[2]
    out[..., 2] += B0(sz, +1.0)
    out[..., 2] += B0(sz, -1.0)
    return out


def corner(r, d):
    """(floor(x / dx) dx, floor(y / dy) dy, floor(z / dz) dz) of positions [n][3]"""
    d = np.asarray(d, dtype=np.float64)
    return np.floor(np.asarray(r, dtype=np.float64) / d) * d


def keep(geometry, r, d):
    c = corner(r, d)
    return C.within(geometry, c[:, 0], c[:, 1], c[:, 2])


def trace_open(push, p, steps, geometry, d, sample_every=0, exit_step=None, step0=0):
    """push(records of the particles that are alive) -> (their new records, their iteration counts).  At the top of every
    step the alive particles whose cell corner fails `geometry` are removed (exit_step = step0 + steps completed, state
    kept); sample k is the whole batch after step (k + 1) sample_every, alive[k] the particles alive then."""
    p = np.array(p, dtype=np.float64).reshape(-1, 6)
    n = p.shape[0]
    ex = np.full(n, -1, dtype=np.int64) if exit_step is None else np.array(exit_step, dtype=np.int64)
    nsamp = steps // sample_every if sample_every else 0
    samples = np.zeros((nsamp, n, 6)) if sample_every else None
    alive = np.zeros(nsamp, dtype=np.int64) if sample_every else None
    tot, mx = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32)
    removed = 0
    for k in range(steps):
        a = np.flatnonzero(ex < 0)
        out = a[~keep(geometry, p[a, :3], d)]
        ex[out] = step0 + k
        removed += len(out)
        a = np.flatnonzero(ex < 0)
        if len(a):
            pn, its = push(p[a])
            p[a] = pn
            tot[a] += its
            mx[a] = np.maximum(mx[a], its)
        if sample_every and (k + 1) % sample_every == 0:
            samples[(k + 1) // sample_every - 1] = p
            alive[(k + 1) // sample_every - 1] = (ex < 0).sum()
    return OpenRef(p, samples, ex, alive, removed, tot, mx)


def compactions(exit_step, steps, policy, launch_steps=64):
    """how often a call that ended with exit_step (everybody alive at its start, step0 = 0) rebuilt its list: after a
    launch that is not the last, while somebody is alive, by enum xpic_trace_compact (0: fewer than half of the listed
    entries alive, 1: never, 2: any entry not alive)"""
    ex = np.asarray(exit_step)
    listed, count = len(ex), 0
    for first in range(0, steps, launch_steps):
        end = min(steps, first + launch_steps)
        live = int(((ex < 0) | (ex >= end)).sum())  # (removed at the top of step c + 1 <= end: c < end)
        if live == 0:
            break
        if end < steps and policy != 1 and live < listed and (policy == 2 or 2 * live < listed):
            count += 1
            listed = live
    return count


# ---- the inputs of tests/test_gpu_open_trace.py and tests/test_open_trace_ref.py
N, D = (8, 8, 8), (1.0, 1.0, 1.0)
NPART = 3 * 256 + 7          # three whole workgroups and a ragged one
STEPS, EVERY, SPLIT = 150, 7, 70  # two launch boundaries (64, 128), not a multiple of 64; 70 = 10 samples
QM, MP, DT = -1.0, 1.0, 0.05
# Crank-Nicolson with atol = rtol = 0: no residual is < 0, so every step makes exactly 3 iterations and the iteration
# counters of a particle say how many steps it took (with the default tolerances every count is 0)
CN_KW = dict(atol=0.0, rtol=0.0, maxit=3)
MIRROR = dict(D=8.0, R=3.0, I=2.0)  # coils at z = -4 and +4: |B| largest in the plane z = 4
B_UNIFORM = (0.0, 0.0, 1.0)         # the mirror part only adds to Bz: |B| >= 1 everywhere
E_UNIFORM = (0.0, 0.01, 0.0)
# ends one cell inside the domain in z: a particle is removed once its cell is the plane z = 0 or z = 7
REGION = {"name": "box", "min": (0.0, 0.0, 1.0), "max": (8.0, 8.0, 7.0)}
EVERYWHERE = {"name": "box", "min": (-1e6, -1e6, -1e6), "max": (1e6, 1e6, 1e6)}
# strict in z: corners z = 2 .. 6 pass; radius 3 about the axis (4, 4): the corner (7, 4) lies on it and passes (<=)
CYLINDER = {"name": "cylinder", "center": (4.0, 4.0, 4.0), "radius": 3.0, "height": 6.0}


def fields():
    """(E, B, gradB): uniform parts plus the mirror field; gradB = central differences of |B| on the nodes (the pusher
    does not ask it to be more than a vector)"""
    shape = (N[2], N[1], N[0], 3)
    E = np.zeros(shape) + np.array(E_UNIFORM)
    B = np.zeros(shape) + np.array(B_UNIFORM) + mirror_field(N, D, **MIRROR)
    return E, B, grad_abs(B)


def grad_abs(B):
    lB = np.sqrt((B * B).sum(axis=-1))
    g = np.zeros_like(B)
    for c, axis in enumerate((2, 1, 0)):
        g[..., c] = (np.roll(lB, -1, axis=axis) - np.roll(lB, 1, axis=axis)) / (2.0 * D[c])
    return g


def particles(kind, B, seed=41):
    """NPART records within half a cell of the box centre, 2.5 .. 3.5 cells from the planes that remove them, in three
    interleaved groups by the speed along z (either sign): 1.3 .. 2.0 reaches a plane within 64 steps of DT (3.2 time
    units x 1.3 > 3.5 cells), 0.5 .. 0.72 between step 64 and step 150 (3.2 x 0.72 < 2.5, 7.5 x 0.5 > 3.5), 0.1 .. 0.25
    never (7.5 x 0.25 < 2.5).  The field bends and mirrors these a little; tests/test_open_trace_ref.py counts what the
    groups really do.  kind "fo": Point records {r, v}; "dk": {r, p_parallel, p_perp, mu_p} of the same motion."""
    rng = np.random.default_rng(seed)
    n = NPART
    r = 4.0 + (rng.random((n, 3)) - 0.5)
    group = np.arange(n) % 3
    lo, hi = np.array([1.3, 0.5, 0.1])[group], np.array([2.0, 0.72, 0.25])[group]
    vz = (lo + (hi - lo) * rng.random(n)) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    vperp = 0.1 + 0.2 * rng.random(n)
    ang = 2 * np.pi * rng.random(n)
    if kind == "fo":
        return np.column_stack([r, vperp * np.cos(ang), vperp * np.sin(ang), vz])
    (Bp,) = DK.interpolate_B([B], D, r)
    return np.column_stack([r, vz, vperp, MP * vperp * vperp / (2.0 * DK._len(Bp))])


def with_cylinder_probes(p):
    """the first four records at rest in chosen cells: corner (7, 4, 4) on the radius, corner (7, 5, 4) beyond it, corner
    (4, 4, 1) on the lower lid (|z - 4| < 3 is strict), corner (1, 4, 6) on the radius on the other side"""
    p = p.copy()
    p[:4, :3] = [(7.5, 4.5, 4.5), (7.5, 5.5, 4.5), (4.5, 4.5, 1.5), (1.5, 4.5, 6.5)]
    p[:4, 3:] = 0.0
    return p


def numpy_push(kind, E, B, gradB):
    """the one-step pusher of `kind` ("EB2B" or another Chin id, "CN", "dk") from the numpy restatements"""
    if kind == "dk":
        return lambda p: DK.push(E, B, gradB, D, p, QM, MP, DT)
    if kind == "CN":
        return lambda p: FO.cn_step(E, B, D, p, QM, DT, **CN_KW)
    return lambda p: (FO.step(kind, E, B, D, p, QM, DT), np.zeros(len(p), dtype=np.int32))


def groups(exit_step):
    """(removed within the first launch, removed later, never removed) counts"""
    ex = np.asarray(exit_step)
    return int(((ex >= 0) & (ex < 64)).sum()), int((ex >= 64).sum()), int((ex < 0).sum())
