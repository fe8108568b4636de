"""numpy restatement of the tracers on analytic field models (include/xpic_hip.h: xpic_field_model), the model the GPU
kernels of xpic_amd/csrc/model_trace.hip are tested against:

  model(kind, **params)     the four callbacks -> a function r [n][3] -> (E, B, gradB):
                            uniform            tests/drift_kinetic_push/drift_kinetic_push_ex1.cpp:9-13, ex2.cpp:11-16
                            linear             drift_kinetic_push_ex3.cpp:12-17
                            quadratic_mirror   tests/drift_kinetic_push/drift_kinetic_push.h:24-70, ex4.cpp:12-22
                            gaussian_mirror    drift_kinetic_push.h:72-157
  dk_push(field, ...)       DriftKineticPush::process (src/algorithms/drift_kinetic_push.cpp:48-160), callback at rn
  chin_step(sid, field, ..) process_<id> (tests/boris_push/boris_push.h:20-198), fields at the particle's r
  cn_step(field, ...)       CrankNicolsonPush::process (src/algorithms/crank_nicolson_push.cpp:31-71), callback at the
                            midpoint (r1 + r0) / 2 (drift_kinetic_push_ex9.cpp:75-78)
  pusher(...), trace(...)   open_trace_ref.trace_open around them

The step arithmetic is that of drift_kinetic_ref.py and full_orbit_ref.py (their helper functions are used as they are);
only where the fields come from differs.  Vectorised over the particles; dt may be one number or one per particle."""
import numpy as np

import drift_kinetic_ref as DK
import full_orbit_ref as FO
import open_trace_ref as OT

KINDS = ("uniform", "linear", "quadratic_mirror", "gaussian_mirror")
QUADRATIC = dict(B_min=1.0, B_max=4.0, W=20.0, D=40.0)  # drift_kinetic_push.h:26-29
GAUSSIAN = dict(B_min=1.0, B_max=4.0, L=5.0, W=1.0)     # drift_kinetic_push.h:74-77


def _col(n, v):
    return np.zeros((n, 3)) + np.asarray(v, dtype=np.float64)


def gaussian_Bz(z, B_min, B_max, L, W):
    """gaussian_magnetic_mirror::get_Bz (:87-90), z measured from the midplane"""
    S = W * W
    return B_min + (B_max - B_min) * (np.exp(-((z + L) * (z + L)) / S) + np.exp(-((z - L) * (z - L)) / S))


def model(kind, E0=(0, 0, 0), B0=(0, 0, 0), r0=(0, 0, 0), g=(0, 0, 0), B_min=0.0, B_max=0.0, W=0.0, D=0.0, L=0.0, E_phi=0.0,
          phi=0.0):
    if kind == "uniform":
        return lambda r: (_col(len(r), E0), _col(len(r), B0), np.zeros((len(r), 3)))
    if kind == "linear":
        g_ = np.asarray(g, dtype=np.float64)
        l = np.hypot(np.hypot(g_[0], g_[1]), g_[2])
        nrm = g_ / l if l > 0 else np.zeros(3)

        def linear(r):
            s = ((r - np.asarray(r0, dtype=np.float64)) * g_).sum(axis=1)
            return _col(len(r), E0), _col(len(r), B0) + s[:, None] * nrm, _col(len(r), g_)
        return linear
    if kind == "quadratic_mirror":
        Rc, Lh = W / 2, D / 2

        def quadratic(r):
            x, y, z = r[:, 0] - Rc, r[:, 1] - Rc, r[:, 2] - Lh
            rr = np.hypot(x, y)
            Bz = B_min + (B_max - B_min) * ((z / D) * (z / D))
            Bm = Bz * (1.0 + 0.5 * ((rr / W) * (rr / W)))
            dBz_dz = 2 * (B_max - B_min) * z / (D * D)
            dB_dz = dBz_dz * (1.0 + 0.5 * ((rr / D) * (rr / D)))
            dB_dr = Bz * rr / (D * D)
            far = rr > 1e-10
            safe = np.where(far, rr, 1.0)
            gB = np.column_stack([np.where(far, x / safe * dB_dr, 0.0), np.where(far, y / safe * dB_dr, 0.0), dB_dz])
            B = np.column_stack([np.zeros_like(Bm), np.zeros_like(Bm), Bm])
            if E_phi != 0.0 or phi != 0.0:
                E = np.column_stack([+E_phi * (r[:, 1] - Rc), -E_phi * (r[:, 0] - Rc),
                                     +phi * np.pi / D * np.sin(np.pi * (r[:, 2] - Lh) / D)])
            else:
                E = np.zeros_like(B)
            return E, B, gB
        return quadratic
    if kind == "gaussian_mirror":
        S, Rc, dB = W * W, L, B_max - B_min

        def gaussian(r):
            x, y, z = r[:, 0] - Rc, r[:, 1] - Rc, r[:, 2] - L
            r2 = x * x + y * y
            rr = np.sqrt(r2)
            t1, t2 = z + L, z - L
            e1, e2 = np.exp(-(t1 * t1) / S), np.exp(-(t2 * t2) / S)
            Bz = B_min + dB * (e1 + e2)
            d1 = dB * ((-2.0 * t1 / S * e1) + (-2.0 * t2 / S * e2))
            d2 = dB * ((-2.0 / S + 4.0 * ((t1 / S) * (t1 / S))) * e1 + (-2.0 / S + 4.0 * ((t2 / S) * (t2 / S))) * e2)
            d3 = dB * ((12.0 * t1 / (S * S) - 8.0 * ((t1 / S) * (t1 / S) * (t1 / S))) * e1 +
                       (12.0 * t2 / (S * S) - 8.0 * ((t2 / S) * (t2 / S) * (t2 / S))) * e2)
            B = np.column_stack([-0.5 * x * d1, -0.5 * y * d1, Bz - 0.25 * r2 * d2])
            dB_dr = -0.5 * rr * d2
            dB_dz = d1 - 0.25 * r2 * d3
            far = rr > 1e-12
            safe = np.where(far, rr, 1.0)
            gB = np.column_stack([np.where(far, x / safe * dB_dr, 0.0), np.where(far, y / safe * dB_dr, 0.0), dB_dz])
            return np.zeros_like(B), B, gB
        return gaussian
    raise KeyError(kind)


def _c(dt):
    """dt as a column when it is one value per particle"""
    return dt[:, None] if np.ndim(dt) else dt


# ---- DriftKineticPush::process around a field function: drift_kinetic_ref.push with interpolate -> field(rn)
def dk_push(field, p0, qm, mp, dt, eps=1e-12, delta=1e-12, maxit=30):
    p0 = np.asarray(p0, dtype=np.float64).reshape(-1, 6)
    n = p0.shape[0]
    pn = p0.copy()
    r0, par0, perp0, mu = p0[:, :3], p0[:, 3], p0[:, 4], p0[:, 5]
    Eh, Bp, gradBp = (a.copy() for a in field(pn[:, :3]))
    B0, Bh, gradB0, gradBh = Bp.copy(), Bp.copy(), gradBp.copy(), gradBp.copy()
    b0 = DK._normalized(Bp)
    h = b0.copy()
    lenB0 = DK._len(B0)
    lenBp = lenB0.copy()
    its = np.zeros(n, dtype=np.int32)
    active = np.ones(n, dtype=bool)
    for it in range(maxit):
        Vh = 0.5 * (pn[:, 3] + par0)
        Vd = DK._get_Vd(mu, qm, mp, h, Vh, DK._len(Bh), gradBh, Eh)
        step = _c(dt) * (Vh[:, None] * h + Vd)
        R1 = DK._len(pn[:, :3] - r0 - step)
        drive, mu_term = DK._v_terms(mu, qm, mp, dt, Vh, h, Vd, lenBp, lenB0, Eh)
        R2 = np.abs((pn[:, 3] - par0) - drive + mu_term)
        if it:
            active &= ~((R1 < eps) & (R2 < delta))
        if not active.any():
            break
        a = active
        pn[a, :3] = (r0 + step)[a]
        Eh_, Bp_, gradBp_ = field(pn[:, :3])
        Eh[a], Bp[a], gradBp[a] = Eh_[a], Bp_[a], gradBp_[a]
        Bh[a] = (0.5 * (Bp + B0))[a]
        gradBh[a] = (0.5 * (gradBp + gradB0))[a]
        h[a] = (0.5 * (DK._normalized(Bp) + b0))[a]
        lenBp[a] = DK._len(Bp)[a]
        with np.errstate(divide="ignore", invalid="ignore"):
            pn[a, 4] = (perp0 * np.sqrt(lenBp / lenB0))[a]
        drive, mu_term = DK._v_terms(mu, qm, mp, dt, Vh, h, Vd, lenBp, lenB0, Eh)
        pn[a, 3] = (par0 + drive - mu_term)[a]
        its[a] = it + 1
    return pn, its


# ---- process_<id> around a field function: full_orbit_ref.step with gather -> field(r)
def _kick(field, kind, h, qm, r, v):
    Ep, Bp, _ = field(r)
    return FO._update_vEB(_c(h), qm, Ep, Bp, v) if kind == "EB" else FO._update_v_magnetic(kind, h, qm, Bp, v)


def chin_step(scheme, field, p, qm, dt):
    p = np.asarray(p, dtype=np.float64).reshape(-1, 6)
    r, v = p[:, :3].copy(), p[:, 3:].copy()
    fam = "EB" if scheme.startswith("EB") else scheme[0]
    tail = scheme[len(fam):]
    kind = {"M": "M", "B": "B", "EB": "EB", "C": "C2" if tail == "2A" else "C1"}[fam]
    if tail == "1A":
        v = _kick(field, kind, dt, qm, r, v)
        r = r + v * _c(dt)
    elif tail in ("1B", "LF"):
        r = r + v * _c(dt)
        v = _kick(field, kind, dt, qm, r, v)
    elif tail == "2A":
        v = _kick(field, kind, dt / 2.0, qm, r, v)
        r = r + v * _c(dt)
        v = _kick(field, kind, dt / 2.0, qm, r, v)
    elif tail == "2B":
        r = r + v * _c(dt / 2.0)
        v = _kick(field, kind, dt, qm, r, v)
        r = r + v * _c(dt / 2.0)
    else:
        raise KeyError(scheme)
    return np.column_stack([r, v])


# ---- CrankNicolsonPush::process around a field function: full_orbit_ref.cn_step with gather_segment -> the midpoint
def _cn_res(dt, qm, pn_p, p0_p, vh, Ep, Bp):
    return DK._len((pn_p - p0_p) - _c(dt) * qm * (Ep + np.cross(vh, Bp)))


def cn_step(field, p0, qm, dt, atol=FO.CN_ATOL, rtol=FO.CN_RTOL, maxit=FO.CN_MAXIT):
    p0 = np.asarray(p0, dtype=np.float64).reshape(-1, 6)
    n = p0.shape[0]
    r0, v0 = p0[:, :3], p0[:, 3:]
    pn = p0.copy()
    vh = 0.5 * (pn[:, 3:] + v0)
    pn[:, :3] = r0 + _c(dt) * vh
    Ep, Bp, _ = (a.copy() for a in field((r0 + pn[:, :3]) / 2))
    res0 = _cn_res(dt, qm, pn[:, 3:], v0, vh, Ep, Bp)
    alpha = _c(0.5 * dt * qm)
    its = np.full(n, maxit, dtype=np.int32)
    active = np.ones(n, dtype=bool)
    for it in range(maxit):
        a, b = alpha * Ep, alpha * Bp
        w = v0 + a
        vh = (w + np.cross(w, b) + b * (w * b).sum(axis=1)[:, None]) / (1.0 + (b * b).sum(axis=1))[:, None]
        m = active
        pn[m, :3] = (r0 + _c(dt) * vh)[m]
        pn[m, 3:] = (2.0 * vh - v0)[m]
        rn = _cn_res(dt, qm, pn[:, 3:], v0, vh, Ep, Bp)
        done = active & (rn < atol + rtol * res0)
        its[done] = it
        active = active & ~done
        if not active.any():
            break
        Ep_, Bp_, _ = field((r0 + pn[:, :3]) / 2)
        Ep[active], Bp[active] = Ep_[active], Bp_[active]
    return pn, its


def pusher(kind, field, qm, mp, dt, **kw):
    """the one-step pusher of `kind` ("dk", "CN" or a Chin id) -> (records, iteration counts), as open_trace_ref's"""
    if kind == "dk":
        return lambda p: dk_push(field, p, qm, mp, dt, **kw)
    if kind == "CN":
        return lambda p: cn_step(field, p, qm, dt, **kw)
    return lambda p: (chin_step(kind, field, p, qm, dt), np.zeros(len(p), dtype=np.int32))


def trace(push, p, steps, geometry, d, sample_every=0, exit_step=None, step0=0):
    """open_trace_ref.trace_open; geometry None: no region (a box nothing finite leaves)"""
    return OT.trace_open(push, p, steps, OT.EVERYWHERE if geometry is None else geometry, d, sample_every, exit_step, step0)


def point_by_field(point, Bp, mp, qm):
    """PointByField(point, Bp, mp, qm) (src/interfaces/point.h:50-56) of one Point record -> {r, p_par, p_perp, mu_p}"""
    point, Bp = np.asarray(point, dtype=np.float64), np.asarray(Bp, dtype=np.float64)
    r, p = point[:3], point[3:]
    lB = np.sqrt(Bp.dot(Bp))
    par = p.dot(Bp) * Bp / Bp.dot(Bp)
    perp = np.sqrt(((p - par) ** 2).sum())
    return np.concatenate([r - np.cross(p, Bp / lB) / (qm * lB), [np.sqrt(par.dot(par)), perp, mp * perp * perp / (2.0 * lB)]])


# ---- the loss-cone batch of drift_kinetic_push_ex9.cpp, shared by the CPU and the GPU test
CONE_N = 64
CONE_OMEGA_DT = 1.0
CONE_FRACTIONS = (0.8, 1.2)  # of the critical pitch angle: the first half of the batch, the second half
CONE_D = (0.1, 0.1, 0.1)     # the spacing of drift_kinetic_grid_boris_ex4.cpp:25-29
QM, MP = -1.0, 1.0           # drift_kinetic_push.h:12-13


def cone_region(d=CONE_D, **g):
    """a box that ends half a cell beyond the mirror throats (z = 0 and z = 2 L) in z, wide open across"""
    g = g or GAUSSIAN
    return {"name": "box", "min": (-1e6, -1e6, -0.5 * d[2]), "max": (1e6, 1e6, 2 * g["L"] + 0.5 * d[2])}


def cone_batch(fractions=CONE_FRACTIONS, n=CONE_N, omega_dt=CONE_OMEGA_DT, **g):
    """ex9's start (ex9.cpp:29-47, :80): v_abs = 0.1, pitch = fraction asin(sqrt(Bz(0) / Bz(L))), r0 = (Rc + 0.1, Rc, L),
    the guiding centre PointByField({r0, v0}, {0, 0, get_Bz_corr(r0)}, 1, q / m); dt = omega_dt / get_Bz(0).
    -> (records [n][6], dt)"""
    g = g or GAUSSIAN
    L, Rc = g["L"], g["L"]
    mirror_R = gaussian_Bz(0.0, **g) / gaussian_Bz(L, **g)
    crit = np.arcsin(np.sqrt(mirror_R))
    field = model("gaussian_mirror", **g)
    r0 = np.array([Rc + 0.1, Rc, L])
    Bc = field(r0[None])[1][0, 2]  # get_Bz_corr(r0) is B_p's z component
    frac = np.repeat(np.asarray(fractions, dtype=np.float64), n // 2)
    recs = []
    for f in frac:
        pitch = f * crit
        v0 = (0.1 * np.sin(pitch), 0.0, 0.1 * np.cos(pitch))
        recs.append(point_by_field(np.concatenate([r0, v0]), (0.0, 0.0, Bc), MP, QM))
    dt = omega_dt / gaussian_Bz(0.0, **g)
    return np.array(recs), dt


def cone_steps(dt, **g):
    """two transits of the trap's length 2 L at the parallel speed of the shallower pitch angle"""
    g = g or GAUSSIAN
    crit = np.arcsin(np.sqrt(gaussian_Bz(0.0, **g) / gaussian_Bz(g["L"], **g)))
    return int(np.ceil(2 * (2 * g["L"]) / (0.1 * np.cos(max(CONE_FRACTIONS) * crit)) / dt))
