"""Plain numpy restatement of the reference's drift-kinetic pusher on a periodic grid, the model the GPU kernels of
xpic_amd/csrc/drift_kinetic.hip are tested against (the role of tests/moments_ref.py and tests/commands_ref.py):

  interpolate(...)   DriftKineticEsirkepov::interpolate   src/algorithms/drift_kinetic_implicit.cpp:11-31
                     (ImplicitEsirkepov::Shape::setup / interpolate, implicit_esirkepov.cpp:11-90; Shape::setup(r),
                     src/utils/shape.cpp:31-80; SimpleInterpolation's magnetic products)
  push(...)          DriftKineticPush::process            src/algorithms/drift_kinetic_push.cpp:48-160
  residuals(...)     its get_residue_r / get_residue_v at a returned state

Fields are arrays [nz][ny][nx][3] (Context.fshape()); a particle is {x, y, z, p_parallel, p_perp, mu_p}.  Everything is
vectorised over the particles; a particle that has left the Picard loop is no longer written."""
import numpy as np


def _len(v):
    return np.sqrt((v * v).sum(axis=-1))


def _normalized(v):
    l = _len(v)[:, None]
    return np.divide(v, l, out=np.zeros_like(v), where=l > 0)


def spline2(s):
    """spline_of_2nd_order (src/interfaces/sort_parameters.cpp:21)"""
    s = np.abs(s)
    return np.where(s <= 0.5, 0.75 - s * s, np.where(s < 1.5, 0.5 * (1.5 - s) * (1.5 - s), 0.0))


def _sfunc_2(j, s):
    s = np.abs(s)
    return (0.75 - s * s) if j == 1 else 0.5 * (1.5 - s) * (1.5 - s)


def _at(F, gx, gy, gz, c):
    nz, ny, nx = F.shape[:3]
    return F[gz % nz, gy % ny, gx % nx, c]


def interpolate_E(E, d, rn, r0):
    """E_p of ImplicitEsirkepov::interpolate: the 54 weights of the segment r0 -> rn"""
    d = np.asarray(d, dtype=np.float64)
    prn, pr0 = rn / d, r0 / d
    prh = 0.5 * (prn + pr0)
    gc = np.round(prh)  # half away from zero is std::round; np.round differs only at exact .5, which no test hits
    gc = np.where(np.abs(prh - np.trunc(prh)) == 0.5, np.trunc(prh) + np.sign(prh), gc)
    start = gc.astype(np.int64) - 1
    gv = gc + 0.5
    Ep = np.zeros_like(rn)
    for cx in range(3):
        cy, cz = (cx + 1) % 3, (cx + 2) % 3
        for i in range(2):
            shx = (1.0 / 6.0) * (1.0 - np.abs(gv[:, cx] + (i - 1) - prh[:, cx]))
            for j in range(3):
                sny = _sfunc_2(j, gc[:, cy] + (j - 1) - prn[:, cy])
                s0y = _sfunc_2(j, gc[:, cy] + (j - 1) - pr0[:, cy])
                for k in range(3):
                    snz = _sfunc_2(k, gc[:, cz] + (k - 1) - prn[:, cz])
                    s0z = _sfunc_2(k, gc[:, cz] + (k - 1) - pr0[:, cz])
                    w = shx * (sny * (2 * snz + s0z) + s0y * (2 * s0z + snz))
                    o = [None, None, None]
                    o[cx], o[cy], o[cz] = i, j, k
                    Ep[:, cx] += _at(E, start[:, 0] + o[0], start[:, 1] + o[1], start[:, 2] + o[2], cx) * w
    return Ep


def interpolate_B(fields, d, r):
    """Shape::setup(r, 1.5, spline_of_2nd_order) + SimpleInterpolation::process({}, b_fields): every field of `fields`
    with the same weights (B_x: Sh_z Sh_y No_x, B_y: Sh_z No_y Sh_x, B_z: No_z Sh_y Sh_x)"""
    d = np.asarray(d, dtype=np.float64)
    pr = r / d
    rr = pr - 1.5
    st = np.where(np.abs(rr - np.trunc(rr)) == 0.5, np.trunc(rr) + np.sign(rr), np.round(rr)).astype(np.int64)
    sz = np.floor(pr + 1.5).astype(np.int64) + 1 - st
    assert sz.min() >= 3 and sz.max() <= 4
    No = [[spline2(pr[:, a] - (st[:, a] + t)) for t in range(4)] for a in range(3)]
    Sh = [[spline2(pr[:, a] - (st[:, a] + t + 0.5)) for t in range(4)] for a in range(3)]
    out = [np.zeros_like(r) for _ in fields]
    for kz in range(4):
        for jy in range(4):
            for ix in range(4):
                m = (kz < sz[:, 2]) & (jy < sz[:, 1]) & (ix < sz[:, 0])
                w = (Sh[2][kz] * Sh[1][jy] * No[0][ix], Sh[2][kz] * No[1][jy] * Sh[0][ix], No[2][kz] * Sh[1][jy] * Sh[0][ix])
                for F, o in zip(fields, out):
                    for c in range(3):
                        o[:, c] += np.where(m, _at(F, st[:, 0] + ix, st[:, 1] + jy, st[:, 2] + kz, c) * w[c], 0.0)
    return out


def interpolate(E, B, gradB, d, rn, r0):
    """-> (E_p, B_p, gradB_p); gradB None is the reference's gradB_g == nullptr: gradB_p = 0"""
    rn, r0 = np.asarray(rn, dtype=np.float64), np.asarray(r0, dtype=np.float64)
    Ep = interpolate_E(E, d, rn, r0)
    if gradB is None:
        (Bp,) = interpolate_B([B], d, rn)
        return Ep, Bp, np.zeros_like(Bp)
    Bp, gBp = interpolate_B([B, gradB], d, rn)
    return Ep, Bp, gBp


def _get_Vd(mu, qm, mp, h, Vh, Bh, gradBh, Eh):
    with np.errstate(divide="ignore", invalid="ignore"):
        Bh_ = Bh[:, None]
        v = np.cross(Eh, h) / Bh_ + (1.0 / qm * (Vh * Vh / Bh + mu / mp))[:, None] * np.cross(h, gradBh / Bh_)
    return np.where(Bh_ < 1e-12, 0.0, v)


def _v_terms(mu, qm, mp, dt, Vh, h, Vd, lenBp, lenB0, Eh):
    small = np.abs(Vh) < 1e-12
    with np.errstate(divide="ignore", invalid="ignore"):
        term = np.where(small, 0.0, (Eh * Vd).sum(axis=1) / Vh)
        mu_term = np.where(small, 0.0, (mu / mp) * ((lenBp - lenB0) / Vh))
    return dt * qm * ((Eh * h).sum(axis=1) + term), mu_term


def push(E, B, gradB, d, p0, qm, mp, dt, eps=1e-12, delta=1e-12, maxit=30):
    """DriftKineticPush::process of every particle from the initial guess pn = p0 -> (pn, iterations)"""
    p0 = np.asarray(p0, dtype=np.float64).reshape(-1, 6)
    n = p0.shape[0]
    pn = p0.copy()
    r0, par0, perp0, mu = p0[:, :3], p0[:, 3], p0[:, 4], p0[:, 5]
    Eh, Bp, gradBp = interpolate(E, B, gradB, d, pn[:, :3], r0)
    B0, Bh, gradB0, gradBh = Bp.copy(), Bp.copy(), gradBp.copy(), gradBp.copy()
    b0 = _normalized(Bp)
    h = b0.copy()
    lenB0 = _len(B0)
    lenBp = lenB0.copy()
    its = np.zeros(n, dtype=np.int32)
    active = np.ones(n, dtype=bool)
    for it in range(maxit):
        Vh = 0.5 * (pn[:, 3] + par0)
        Vd = _get_Vd(mu, qm, mp, h, Vh, _len(Bh), gradBh, Eh)
        step = dt * (Vh[:, None] * h + Vd)
        R1 = _len(pn[:, :3] - r0 - step)
        drive, mu_term = _v_terms(mu, qm, mp, dt, Vh, h, Vd, lenBp, lenB0, Eh)
        R2 = np.abs((pn[:, 3] - par0) - drive + mu_term)
        if it:
            active &= ~((R1 < eps) & (R2 < delta))
        if not active.any():
            break
        a = active
        pn[a, :3] = (r0 + step)[a]
        Eh_, Bp_, gradBp_ = interpolate(E, B, gradB, d, pn[:, :3], r0)
        Eh[a], Bp[a], gradBp[a] = Eh_[a], Bp_[a], gradBp_[a]
        Bh[a] = (0.5 * (Bp + B0))[a]
        gradBh[a] = (0.5 * (gradBp + gradB0))[a]
        h[a] = (0.5 * (_normalized(Bp) + b0))[a]
        lenBp[a] = _len(Bp)[a]
        with np.errstate(divide="ignore", invalid="ignore"):
            pn[a, 4] = (perp0 * np.sqrt(lenBp / lenB0))[a]
        drive, mu_term = _v_terms(mu, qm, mp, dt, Vh, h, Vd, lenBp, lenB0, Eh)
        pn[a, 3] = (par0 + drive - mu_term)[a]
        its[a] = it + 1
    return pn, its


def residuals(E, B, gradB, d, p0, pn, qm, mp, dt):
    """(R1, R2) as process() forms them at the top of an iteration whose state is (p0, pn): every quantity there is a
    function of the two states (Bh, gradBh, h from the fields at pn.r and p0.r, Eh over the segment)"""
    p0, pn = np.asarray(p0, dtype=np.float64), np.asarray(pn, dtype=np.float64)
    r0, mu = p0[:, :3], p0[:, 5]
    _, B0, gradB0 = interpolate(E, B, gradB, d, r0, r0)
    Eh, Bp, gradBp = interpolate(E, B, gradB, d, pn[:, :3], r0)
    Bh, gradBh = 0.5 * (Bp + B0), 0.5 * (gradBp + gradB0)
    h = 0.5 * (_normalized(Bp) + _normalized(B0))
    Vh = 0.5 * (pn[:, 3] + p0[:, 3])
    Vd = _get_Vd(mu, qm, mp, h, Vh, _len(Bh), gradBh, Eh)
    R1 = _len(pn[:, :3] - r0 - dt * (Vh[:, None] * h + Vd))
    drive, mu_term = _v_terms(mu, qm, mp, dt, Vh, h, Vd, _len(Bp), _len(B0), Eh)
    return R1, np.abs((pn[:, 3] - p0[:, 3]) - drive + mu_term)


def mirror_fields(N, D, amplitude=0.3):
    """B = (0, 0, 1 + amplitude cos(2 pi z / Lz)) and its analytic grad |B| on the nodes (z = k dz for the z components,
    the positions SimpleInterpolation's magnetic products weight them at), E = 0 -> (E, B, gradB)"""
    nz = N[2]
    Lz = N[2] * D[2]
    z = np.arange(nz) * D[2]
    shape = (N[2], N[1], N[0], 3)
    E, B, gB = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    B[..., 2] = (1.0 + amplitude * np.cos(2 * np.pi * z / Lz))[:, None, None]
    gB[..., 2] = (-amplitude * 2 * np.pi / Lz * np.sin(2 * np.pi * z / Lz))[:, None, None]
    return E, B, gB


# ---- the inputs of tests/test_gpu_drift_kinetic.py (here so that a CPU test can check them against the restatement)
N, D = (9, 8, 7), (0.5, 0.4, 0.3)  # the grid of tests/test_eccapfim_kernels.py
NPART = 1001                       # four workgroups of 256 with a ragged tail
QM, MP, DT = -1.0, 1.0, 0.05       # DT: every particle of case_particles converges (test_drift_kinetic_ref.py)


def smooth_field(rng, base, amplitude):
    """base + amplitude * (a few box-periodic modes with random phases), per component"""
    nz, ny, nx = N[2], N[1], N[0]
    z, y, x = np.meshgrid(np.arange(nz) / nz, np.arange(ny) / ny, np.arange(nx) / nx, indexing="ij")
    F = np.zeros((nz, ny, nx, 3))
    for c in range(3):
        F[..., c] = base[c]
        for _ in range(3):
            k = rng.integers(0, 2, 3)
            ph = rng.random() * 2 * np.pi
            F[..., c] += amplitude / 3 * np.cos(2 * np.pi * (k[0] * x + k[1] * y + k[2] * z) + ph)
    return F


def case_fields(seed=11):
    """random smooth E, B and grad B (three independent fields: the pusher does not ask grad B to be B's gradient)"""
    rng = np.random.default_rng(seed)
    return (smooth_field(rng, (0.0, 0.1, -0.1), 0.2), smooth_field(rng, (0.2, 0.3, 1.0), 0.3),
            smooth_field(rng, (0.0, 0.0, 0.0), 0.3))


def case_segments(seed=12, n=NPART, max_cells=1.4):
    """random segments of up to max_cells cells; the first half start within a cell of a box face (outside it as often
    as inside), so they cross the periodic seam"""
    rng = np.random.default_rng(seed)
    L, d = np.array(N) * np.array(D), np.array(D)
    r0 = rng.random((n, 3)) * L
    h = n // 2
    face = np.where(rng.random((h, 3)) < 0.5, 0.0, 1.0) * L
    r0[:h] = face + (rng.random((h, 3)) * 2 - 1) * d
    rn = r0 + (rng.random((n, 3)) * 2 - 1) * max_cells * d
    return rn, r0


def case_particles(B, seed=13, n=NPART, zero_par=50):
    """guiding centres all over the box (the first half near its faces), |p_parallel| in [0.2, 1] with either sign -- away
    from 0, where the pusher's 1 / Vh terms amplify rounding beyond any fixed relative bound -- except the first
    zero_par particles, which have p_parallel = 0 exactly (|Vh| under the guard in the first iteration).  Those start
    cold: their Vh stays ~ dt qm E_par / 2, and an update multiplies a perturbation of p_parallel by about
    (mu_p / mp) dt |Vd . grad B| / (2 Vh^2), which is 10 - 30 per iteration at the p_perp of the others (measured: a
    1e-16 difference between two roundings of |B| grew to 1.7e-11 in five iterations).  With a tenth of the p_perp, a
    hundredth of mu_p, the map contracts and a comparison of iterates is conditioned.  mu_p from p_perp and |B| at the
    particle as PointByField forms it"""
    rng = np.random.default_rng(seed)
    _, r = case_segments(seed + 100, n)
    par = (0.2 + 0.8 * rng.random(n)) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    par[:zero_par] = 0.0
    perp = 0.1 + 0.4 * rng.random(n)
    perp[:zero_par] *= 0.1
    (Bp,) = interpolate_B([B], D, r)
    lB = _len(Bp)
    mu = np.divide(MP * perp * perp, 2.0 * lB, out=np.zeros(n), where=lB > 0)
    return np.column_stack([r, par, perp, mu])
