"""numpy restatement of the field-line tracer (include/xpic_field_lines.h, xpic_amd/csrc/field_line_step.h): the RK4 step of
dr/dl = s F / |F| at a fixed arc-length step, the stop rules and the accumulators, in the kernel's order of operations.
The reference has no field-line tracer: the yardstick is this statement, held against closed forms by
tests/test_field_lines_ref.py, and the device is held against it by tests/test_gpu_field_lines.py.

  grid_source(F, d, stagger)   r -> F(r): the gather of tests/full_orbit_ref.py (gather_B, and the electric products of
                               gather from the same pieces); a position that is not a number or further out than the
                               device forms an index from gives NaN, as fo_gather does
  trace(source, seeds, ...)    the lanes of one direction -> Lines
  lines(source, seeds, ...)    both directions, arrays [2][n] as the entry points return them
  bug=...                      one planted bug (BUGS), for tests/test_field_lines_ref.py: each must be visible

Everything is vectorised over the lanes and works in the dtype asked for: float64 states the kernel, np.longdouble measures
how far rounding alone moves a result (the tolerance of the device tests)."""
import collections

import numpy as np

import full_orbit_ref as FO
import open_trace_ref as O

MAXSTEPS, LEFT, NULL, CLOSED = 0, 1, 2, 3  # XPIC_LINE_*
STAGGER_B, STAGGER_E = 0, 1
BUGS = ("euler", "unnormalised", "no_half", "region_after")  # and the wrong stagger, which is the caller's to plant

Lines = collections.namedtuple("Lines", "end length volume fmin smin fmax steps code samples")


def grid_source(F, d, stagger=STAGGER_B):
    """the vector F [nz][ny][nx][3] with the magnetic products (STAGGER_B) or the electric ones (STAGGER_E)"""
    d = np.asarray(d, dtype=np.float64)

    def at(r):
        out = np.full(r.shape, np.nan, dtype=r.dtype)
        with np.errstate(invalid="ignore"):
            ok = (np.abs(r) <= 1e9 * d).all(axis=1)  # fo_in_range
        if ok.any():
            q = r[ok]
            if stagger == STAGGER_B:
                out[ok] = FO.gather_B(F, d, q)
            else:  # E_x: No_z No_y Sh_x, E_y: No_z Sh_y No_x, E_z: Sh_z No_y No_x (FO.gather's, without its cast of r)
                st, No, Sh = FO._point_shape(d, q)
                out[ok] = np.column_stack([FO._weighted(F, st, 0, No[2], No[1], Sh[0]), FO._weighted(F, st, 1, No[2], Sh[1], No[0]),
                                           FO._weighted(F, st, 2, Sh[2], No[1], No[0])])
        return out
    return at


def function_source(fn):
    """a field given as fn(r float64 [m][3]) -> [m][3] (a model evaluated elsewhere)"""
    return lambda r: np.asarray(fn(np.asarray(r, dtype=np.float64)), dtype=r.dtype)


def abs3(F):
    """sqrt((Fx Fx + Fy Fy) + Fz Fz)"""
    return np.sqrt((F[:, 0] * F[:, 0] + F[:, 1] * F[:, 1]) + F[:, 2] * F[:, 2])


def usable(f, f_floor):
    with np.errstate(invalid="ignore"):
        return (f >= f_floor) & (f > 0) & np.isfinite(f)


def region_keep(geometry, d):
    """the open traces' rule (open_trace_ref.keep) for positions of any dtype"""
    return lambda r: O.keep(geometry, np.asarray(r, dtype=np.float64), d)


def step(source, r, F0, f0, s, h, f_floor, bug=None):
    """one step of the lanes r, whose field is F0 with the usable |F0| = f0 -> (ok, r', F(r'), |F|(r')); the lanes that are
    not ok met an unusable |F| at a stage or at r' and take no step"""
    T = r.dtype.type
    hh, h6 = h / T(2), h / T(6)
    F, f = F0, f0
    ok = np.ones(len(r), dtype=bool)
    acc = rs = None
    stages = ((hh, 1), (hh, 2), (h, 2), (h6, 1)) if bug != "euler" else ((h, 1),)
    for k, (a, w) in enumerate(stages):
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            t = s * F if bug == "unnormalised" else s * (F / f[:, None])
            acc = t if k == 0 else acc + T(w) * t
            rs = r + a * (t if k < 3 else acc)
        rs = np.where(ok[:, None], rs, r)  # (a lane that is out takes no further part)
        F = source(rs)
        f = abs3(F)
        ok &= usable(f, f_floor)
    return ok, rs, F, f


def trace(source, seeds, h, max_steps, s=+1, keep=None, f_floor=0.0, close_tol=0.0, sample_every=0, bug=None,
          dtype=np.float64):
    """the lanes that follow s F from seeds [n][3] -> Lines (arrays [n]; samples [n][max_steps // sample_every][3] or None)"""
    T = np.dtype(dtype).type
    seed = np.array(seeds, dtype=dtype).reshape(-1, 3)
    n = len(seed)
    h, s, f_floor, close_tol = T(h), T(s), T(f_floor), T(close_tol)
    hh = h / T(2)
    r = seed.copy()
    length, volume, smin, fmax = (np.zeros(n, dtype=dtype) for _ in range(4))
    fmin = np.full(n, np.inf, dtype=dtype)
    steps, code = np.zeros(n, dtype=np.int64), np.full(n, -1, dtype=np.int32)
    nsamp = max_steps // sample_every if sample_every else 0
    samples = np.zeros((n, nsamp, 3), dtype=dtype) if sample_every else None

    def extrema(a, f):
        with np.errstate(invalid="ignore"):
            lo, hi = f < fmin[a], f > fmax[a]
        smin[a[lo]] = length[a[lo]]
        fmin[a[lo]] = f[lo]
        fmax[a[hi]] = f[hi]

    F0 = source(r)
    f0 = abs3(F0)
    extrema(np.arange(n), f0)
    while True:
        code[(code < 0) & (steps >= max_steps)] = MAXSTEPS
        if keep is not None and bug != "region_after":
            a = np.flatnonzero(code < 0)
            code[a[~keep(r[a])]] = LEFT
        code[(code < 0) & ~usable(f0, f_floor)] = NULL
        a = np.flatnonzero(code < 0)
        if not len(a):
            break
        closing = np.zeros(len(a), dtype=bool)
        if close_tol > 0:  # back at the seed: the step that passes it closes the line
            x = r[a] - seed[a]
            dist = np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2])
            closing = (steps[a] >= 2) & (dist <= close_tol)
        ok, rn, Fn, fn = step(source, r[a], F0[a], f0[a], s, h, f_floor, bug)
        code[a[~ok]] = NULL
        closing = closing[ok]
        b, rn, Fn, fn = a[ok], rn[ok], Fn[ok], fn[ok]
        r[b] = rn
        length[b] = length[b] + h
        volume[b] = volume[b] + (h if bug == "no_half" else hh) * (T(1) / f0[b] + T(1) / fn)
        steps[b] += 1
        F0[b], f0[b] = Fn, fn
        extrema(b, fn)
        if sample_every:
            m = b[(steps[b] % sample_every == 0) & (steps[b] // sample_every - 1 < nsamp)]
            samples[m, steps[m] // sample_every - 1] = r[m]
        code[b[closing]] = CLOSED
        if keep is not None and bug == "region_after":
            b = b[code[b] < 0]
            code[b[~keep(r[b])]] = LEFT
    if sample_every:
        for q in range(n):  # the rows behind a lane's last step repeat its last point
            samples[q, min(steps[q] // sample_every, nsamp):] = r[q]
    return Lines(r, length, volume, fmin, smin, fmax, steps, code, samples)


def lines(source, seeds, h, max_steps, directions=3, **kw):
    """both directions -> Lines of arrays [2][n] (direction major: row 0 follows +F, row 1 follows -F); a direction that
    was not asked for is zeros, with code -1, as the package returns it"""
    seeds = np.asarray(seeds).reshape(-1, 3)
    n = len(seeds)
    got = [trace(source, seeds, h, max_steps, s=sign, **kw) if directions & (1 << k) else None
           for k, sign in enumerate((+1, -1))]
    one = next(g for g in got if g is not None)
    out = []
    for f, x in zip(Lines._fields, one):
        if x is None:
            out.append(None)
            continue
        rows = [getattr(g, f) if g is not None else (np.full(n, -1, dtype=x.dtype) if f == "code" else np.zeros_like(x))
                for g in got]
        out.append(np.stack(rows))
    return Lines(*out)


# ---- the closed-form cases of tests/test_field_lines_ref.py and tests/test_gpu_field_lines.py
UNIFORM_N, UNIFORM_D, UNIFORM_F = (8, 8, 8), (1.0, 1.0, 1.0), (0.0, 0.0, 2.0)
CIRCLE_N, CIRCLE_D, CIRCLE_C = (16, 16, 4), (0.25, 0.25, 0.25), (2.0, 2.0)
CIRCLE_RADII = (0.4, 0.5, 0.6, 0.7, 0.8)
CIRCLE_H = 0.03  # 2 pi r / h is 83.8, 104.7, 125.7, 146.6, 167.6: no count at a tie


def uniform_field(n=UNIFORM_N, F=UNIFORM_F):
    return np.zeros((n[2], n[1], n[0], 3)) + np.asarray(F, dtype=np.float64)


def circle_field(stagger=STAGGER_B, n=CIRCLE_N, d=CIRCLE_D, c=CIRCLE_C):
    """F = (-(y - y_c), x - x_c, 0) sampled where the stagger keeps each component: B_x at (i, j + 1/2, k + 1/2) and
    B_y at (i + 1/2, j, k + 1/2); E_x at (i + 1/2, j, k) and E_y at (i, j + 1/2, k).  The second-order spline reproduces a
    linear function exactly, so away from the periodic seam the gather returns F itself, up to rounding."""
    z, y, x = np.meshgrid(np.arange(n[2], dtype=np.float64), np.arange(n[1], dtype=np.float64),
                          np.arange(n[0], dtype=np.float64), indexing="ij")
    half = 0.5 if stagger == STAGGER_B else 0.0
    F = np.zeros((n[2], n[1], n[0], 3))
    F[..., 0] = -((y + half) * d[1] - c[1])
    F[..., 1] = (x + half) * d[0] - c[0]
    return F


def circle_seeds(radii=CIRCLE_RADII, c=CIRCLE_C, z=0.55):
    """one seed per radius, at different angles"""
    ang = 0.3 + 1.1 * np.arange(len(radii))
    rad = np.asarray(radii, dtype=np.float64)
    return np.column_stack([c[0] + rad * np.cos(ang), c[1] + rad * np.sin(ang), np.full(len(rad), z)])


def circle_radius(r, c=CIRCLE_C):
    r = np.asarray(r, dtype=np.float64)
    return np.sqrt((r[..., 0] - c[0]) ** 2 + (r[..., 1] - c[1]) ** 2)
