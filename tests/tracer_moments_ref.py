"""numpy restatement of the moments of a tracer set (include/xpic_tracer_moments.h, xpic_amd/csrc/tracer_moments.hip), in
the kernel's order of operations.  The deposit is DistributionMoment's (tests/moments_ref.py states it for a cell-sorted
sort; tests/test_tracer_moments_ref.py holds this file to that one); what a set adds is stated here:

  storage_cells(r, d)   floor(r / d) per axis of the position as it is, not folded (the open traces' cell)
  counts(...)           the mask of the particles that count: live (exit_step < 0) and their cell in the region
  fo_values / dk_values the per-particle values of a full-orbit record and of a guiding centre (gyro-averaged)
  moment(...)           one deposit -> Deposit(out, counted, absum, contributions)
  map_sum(...)          a map: the sum of the moments at the due steps
  bug=...               one planted bug (BUGS), for tests/test_tracer_moments_ref.py: each must be visible

absum and contributions are, per node and component, the sum of |contribution| and the number of contributions: what the
project's deposit bound 2 eps * contributions * sum |contribution| is made of."""
import collections

import numpy as np

import field_lines_ref as FL
import moments_ref as M

BUGS = ("round_cell", "count_dead", "wrap_partial", "no_delta")
Deposit = collections.namedtuple("Deposit", "out counted absum contributions")
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))  # the six components of a symmetric tensor, in the reference's order


def storage_cells(r, d, bug=None):
    """-> float array [n][3] (a position that is not a number has none: NaN)"""
    s = np.asarray(r, dtype=np.float64) / np.asarray(d, dtype=np.float64)
    return M.cround(s) if bug == "round_cell" else np.floor(s)


def region_of(n, region):
    """-> (start, end, full) per axis"""
    n = np.array([int(v) for v in n])
    start = np.zeros(3, dtype=np.int64) if region is None else np.asarray(region, dtype=np.int64).reshape(6)[:3]
    size = n if region is None else np.asarray(region, dtype=np.int64).reshape(6)[3:]
    return start, start + size, (start == 0) & (size == n)


def counts(pts, exit_step, n, d, region=None, bug=None):
    """the particles that count: live, and floor(r / d) in the region (so inside the box, and a number)"""
    start, end, _ = region_of(n, region)
    c = storage_cells(np.asarray(pts)[:, :3], d, bug)
    with np.errstate(invalid="ignore"):
        inside = np.all((c >= start) & (c < end), axis=1)
    live = np.ones(len(c), dtype=bool) if bug == "count_dead" else np.asarray(exit_step) < 0
    return live & inside


def hypot_device(x, y):
    """hypot as the device's math library forms it (ROCm device libs, ocml hypotD): both arguments scaled by the power of
    two of the larger, sqrt(fma(a, a, b * b)), scaled back.  The scaling is exact, so this is sqrt of the once-rounded
    a a + round(b b); the fused sum is formed exactly in rationals.  libm's hypot is rounded differently in the last bit
    for some arguments, which the cylindrical values would carry into a node with a single contribution."""
    from fractions import Fraction

    out = np.empty(len(x))
    for k, (a, b) in enumerate(zip(np.abs(x).tolist(), np.abs(y).tolist())):
        out[k] = np.sqrt(float(Fraction(a) * Fraction(a) + Fraction(b * b)))
    return out


def v_cyl(pts, n, d):
    """moments_ref.v_cyl with the device's hypot"""
    x = pts[:, 0] - 0.5 * (n[0] * d[0])
    y = pts[:, 1] - 0.5 * (n[1] * d[1])
    r = hypot_device(x, y)
    v = pts[:, 3:6]
    with np.errstate(divide="ignore", invalid="ignore"):
        vr = (+x * v[:, 0] + y * v[:, 1]) / r
        va = (-y * v[:, 0] + x * v[:, 1]) / r
        axis = np.isinf(1.0 / r)
    return np.stack([np.where(axis, v[:, 0], vr), np.where(axis, v[:, 1], va), v[:, 2]], axis=1)


def fo_values(name, pts, q, m, n, d):
    """moments_ref.moment_values; the cylindrical kinds through v_cyl above"""
    if name.endswith("_cyl"):
        pts = np.hstack([pts[:, :3], v_cyl(pts, n, d)])
        name = name[:-4]
    return M.moment_values(name, pts, q, m, n, d)


def direction(B, d, r):
    """b = B(r) / |B(r)| per component, B the field-line tracer's gather; |B| == 0: the zero vector"""
    Bp = FL.grid_source(B, d, FL.STAGGER_B)(np.asarray(r, dtype=np.float64))
    f = FL.abs3(Bp)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where((f == 0)[:, None], 0.0, Bp / f[:, None])


def tensor_values(name, m, ppar, pperp, b, bug=None):
    """m (p_par^2 b_i b_j + p_perp^2 / 2 (delta_ij - b_i b_j)) for the unit vector b [n][3], six components or the diagonal"""
    par, perp = m * (ppar * ppar), m * (0.5 * (pperp * pperp))
    pairs = ((0, 0), (1, 1), (2, 2)) if name.startswith("momentum_flux_diag") else PAIRS
    cols = []
    for i, j in pairs:
        bb = b[:, i] * b[:, j]
        cols.append(par * bb if bug == "no_delta" else par * bb + perp * ((1.0 if i == j else 0.0) - bb))
    return np.stack(cols, axis=1)


def dk_values(name, pts, q, m, n, d, b, bug=None):
    """the values of guiding centres {r, p_parallel, p_perp, mu_p} whose field direction is b"""
    ppar, pperp = pts[:, 3], pts[:, 4]
    if name == "density":
        return np.ones((len(pts), 1))
    if name == "current":
        qp = q * ppar
        return np.stack([qp * b[:, 0], qp * b[:, 1], qp * b[:, 2]], axis=1)
    if name.endswith("_cyl"):  # b rotated as v_cyl rotates v
        b = v_cyl(np.hstack([pts[:, :3], b]), n, d)
    return tensor_values(name, m, ppar, pperp, b, bug)


def dk_scales(name, pts, q, m):
    """per component the size of what multiplies b in a guiding centre's value: an error db of b moves a component of the
    current by at most |q p_par| db and one of the tensor by at most m (p_par^2 + p_perp^2 / 2) 2 db (|b| <= 1)"""
    ppar, pperp = pts[:, 3], pts[:, 4]
    one = {"density": 0.0 * ppar, "current": np.abs(q * ppar)}.get(name, np.abs(m) * (ppar * ppar + 0.5 * (pperp * pperp)))
    return np.repeat(one[:, None], M.DOF[name], axis=1)


def deposit(values, r, weight, n, d, region=None, bug=None):
    """DistributionMoment's deposit of values [k][dof] at r [k][3], every particle counted -> (out, absum, contributions)"""
    n = tuple(int(v) for v in n)
    start, end, full = region_of(n, region)
    if bug == "wrap_partial":  # every axis wrapped, and what was wrapped kept wherever it lands
        full, start, end = np.ones(3, dtype=bool), np.zeros(3, dtype=np.int64), np.array(n)
    dof = values.shape[1]
    out, absum = np.zeros((n[2], n[1], n[0], dof)), np.zeros((n[2], n[1], n[0], dof))
    cnt = np.zeros((n[2], n[1], n[0], dof), dtype=np.int64)
    if len(r) == 0:
        return out, absum, cnt
    pr = r / np.array(d, dtype=np.float64)
    st = M.cround(pr - 1.0).astype(np.int64)
    w = []
    for t in range(2):
        dd = np.abs(pr - ((st + t).astype(np.float64) + 0.5))
        w.append(np.where(dd <= 1.0, 1.0 - dd, 0.0))
    for i in range(8):
        ix, iy, iz = i % 2, (i // 2) % 2, i // 4
        si = ((w[ix][:, 0] * w[iy][:, 1]) * w[iz][:, 2]) * weight
        tgt = st + np.array([ix, iy, iz])
        for a in range(3):
            if full[a]:  # one wrap
                tgt[:, a] = np.where(tgt[:, a] < 0, tgt[:, a] + n[a], np.where(tgt[:, a] >= n[a], tgt[:, a] - n[a], tgt[:, a]))
        ok = np.all((tgt >= start) & (tgt < end), axis=1) & (si != 0.0)
        where = (tgt[ok, 2], tgt[ok, 1], tgt[ok, 0])
        for j in range(dof):
            c = values[ok, j] * si[ok]
            np.add.at(out[..., j], where, c)
            np.add.at(absum[..., j], where, np.abs(c))
            np.add.at(cnt[..., j], where, 1)
    return out, absum, cnt


def moment(name, pts, exit_step, q, m, weight, n, d, region=None, kind="full_orbit", B=None, bug=None):
    """the moment `name` of a set whose records are pts [k][6] and exit_step [k] -> Deposit.  kind "drift_kinetic": B is the
    context's B [nz][ny][nx][3]"""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 6)
    keep = counts(pts, exit_step, n, d, region, bug)
    p = pts[keep]
    if kind == "full_orbit":
        vals = fo_values(name, p, q, m, n, d) if len(p) else np.zeros((0, M.DOF[name]))
    else:
        b = direction(B, d, p[:, :3]) if len(p) else np.zeros((0, 3))
        vals = dk_values(name, p, q, m, n, d, b, bug) if len(p) else np.zeros((0, M.DOF[name]))
    out, absum, cnt = deposit(vals, p[:, :3], weight, n, d, region, bug)
    return Deposit(out, int(keep.sum()), absum, cnt)


def map_sum(deposits):
    """a map: the sum of the Deposits made at its due steps -> (Deposit, deposits made)"""
    deposits = list(deposits)
    tot = Deposit(sum(x.out for x in deposits), sum(x.counted for x in deposits), sum(x.absum for x in deposits),
                  sum(x.contributions for x in deposits))
    return tot, len(deposits)


def bound(dep, extra=0.0):
    """the project's deposit bound per node and component: 2 eps * contributions * sum |contribution|, plus
    `extra` * sum |contribution| for what is not the deposit's (the rounding of b in a guiding centre's values)"""
    eps = np.finfo(np.float64).eps
    return 2.0 * eps * dep.contributions * dep.absum + extra * dep.absum
