"""Plain numpy restatement of the electrostatic scheme (include/xpic_es.h, xpic_amd/csrc/es.hip and the "es" step of
api.hip), written from the header's step text with neither the oracle nor the library.  The field solve
is gauss_ref's (its operators D, G and its dense mean-free solve), or an FFT solve of the same 7-point operator for the
long runs; the gather is Shape::setup(r) + SimpleInterpolation (the statement of full_orbit_ref.gather, here in any
dtype so that np.longdouble can refine the float64 statement).

Fields are get_field's arrays [nz][ny][nx][3], scalars [nz][ny][nx]; n = (nx, ny, nz), d = (dx, dy, dz); a sort is a dict
with r [N][3], v [N][3], q, m, w (= n / Np, the weight of a macro-particle's charge: the deposit's value is q w).

    spline2(s)                    spline_of_2nd_order, the three-branch form
    gather(E, B, d, r)            (E_p, B_p), and with sums=True also sum |F w| per component (the rounding bound's scale)
    update_vEB(dt, qm, Ep, Bp, v) BorisPush::update_vEB
    deposit(r, d, n, value)       xpic_charge_density's rule -> (rho, contributions per node, sum |contribution| per node)
    fold(r, n, d)                 the re-bin's correct_coordinates: one fold per axis, s == L stays
    cells(r, n, d)                floor(r / d) -> the cell index (z ny + y) nx + x
    push(sort, E, B, d, dt)       phases 1 - 2 -> (r_new unfolded, v_new)
    step(sorts, E, B, n, d, dt)   one step -> (E_new, rho with background, phi); the sorts are advanced in place
    solve_fft(res, n, d)          phi of D G phi = res by the eigenvalues of the 7-point operator
    omega_leapfrog(n, d, dt, mode, axis)   the plasma frequency a cold uniform plasma oscillates at in this scheme

mutate (the planted bugs of tests/test_es_ref.py): "rho_old" deposits at the old position, "keep_mean" leaves the mean in,
"plus_grad" sets E + G phi, "gather_moved" gathers at r + dt v, "backward_grad" takes the backward-shift gradient."""
import numpy as np

import gauss_ref as G

EPS = np.finfo(np.float64).eps


def spline2(s):
    s = np.abs(s)
    return np.where(s <= 0.5, 0.75 - s * s, np.where(s < 1.5, 0.5 * (1.5 - s) * (1.5 - s), 0 * s))


def _round(x):
    """std::round: halves away from zero"""
    return np.where(np.abs(x - np.trunc(x)) == 0.5, np.trunc(x) + np.sign(x), np.round(x))


def gather(E, B, d, r, sums=False):
    """the 2nd-order shape at r: start round(r / d - 1.5), four nodes (the weight of a node the shape does not have is an
    exact 0), E_x: No_z No_y Sh_x, E_y: No_z Sh_y No_x, E_z: Sh_z No_y No_x; B_x: Sh_z Sh_y No_x, B_y: Sh_z No_y Sh_x,
    B_z: No_z Sh_y Sh_x"""
    r = np.asarray(r)
    dt_ = r.dtype
    nz, ny, nx = E.shape[:3]
    pr = r / np.asarray(d, dtype=dt_)
    st = _round(pr - dt_.type(1.5)).astype(np.int64)
    t = np.arange(4)
    g = st[:, :, None] + t                                   # [N][3][4]
    No = spline2(pr[:, :, None] - g.astype(dt_))
    Sh = spline2(pr[:, :, None] - (g.astype(dt_) + dt_.type(0.5)))
    gx, gy, gz = g[:, 0] % nx, g[:, 1] % ny, g[:, 2] % nz
    idx = (gz[:, :, None, None], gy[:, None, :, None], gx[:, None, None, :])

    def weighted(F, c, wz, wy, wx):
        w = (wz[:, :, None, None] * wy[:, None, :, None]) * wx[:, None, None, :]
        terms = (np.asarray(F, dtype=dt_)[idx + (c,)] * w).reshape(len(r), -1)
        return terms.sum(axis=1), np.abs(terms).sum(axis=1)

    parts = [weighted(E, 0, No[:, 2], No[:, 1], Sh[:, 0]), weighted(E, 1, No[:, 2], Sh[:, 1], No[:, 0]),
             weighted(E, 2, Sh[:, 2], No[:, 1], No[:, 0]), weighted(B, 0, Sh[:, 2], Sh[:, 1], No[:, 0]),
             weighted(B, 1, Sh[:, 2], No[:, 1], Sh[:, 0]), weighted(B, 2, No[:, 2], Sh[:, 1], Sh[:, 0])]
    Ep = np.column_stack([p[0] for p in parts[:3]])
    Bp = np.column_stack([p[0] for p in parts[3:]])
    if sums:
        return Ep, Bp, np.column_stack([p[1] for p in parts[:3]]), np.column_stack([p[1] for p in parts[3:]])
    return Ep, Bp


def update_vEB(dt, qm, Ep, Bp, v):
    """BorisPush::update_vEB (src/algorithms/boris_push.cpp:48-57)"""
    T = v.dtype.type
    alpha = T(dt) * T(qm)
    a, b = alpha * Ep, -alpha * Bp
    w = v + T(0.5) * a
    bw = np.cross(b, w)
    bbw = np.cross(b, bw)
    den = T(1) + T(0.25) * (b * b).sum(axis=1)
    return v + a + (bw + T(0.5) * bbw) / den[:, None]


def deposit(r, d, n, value, reverse=False):
    """reverse: the particles are summed in the opposite order (the same terms: what the summation order alone changes)"""
    r = np.asarray(r)[::-1] if reverse else np.asarray(r)
    T = r.dtype.type
    nx, ny, nz = n
    pr = r / np.asarray(d, dtype=r.dtype)
    st = np.ceil(pr - T(1.5)).astype(np.int64)
    t = np.arange(3)
    g = st[:, :, None] + t
    w = spline2(pr[:, :, None] - g.astype(r.dtype))          # [N][3][3]
    val = T(value) * ((w[:, 0][:, None, None, :] * w[:, 1][:, None, :, None]) * w[:, 2][:, :, None, None])  # [N][k][j][i]
    idx = ((g[:, 2] % nz)[:, :, None, None] + 0 * g[:, 1][:, None, :, None] + 0 * g[:, 0][:, None, None, :],
           0 * g[:, 2][:, :, None, None] + (g[:, 1] % ny)[:, None, :, None] + 0 * g[:, 0][:, None, None, :],
           0 * g[:, 2][:, :, None, None] + 0 * g[:, 1][:, None, :, None] + (g[:, 0] % nx)[:, None, None, :])
    rho = np.zeros((nz, ny, nx), dtype=r.dtype)
    count = np.zeros((nz, ny, nx))
    asum = np.zeros((nz, ny, nx))
    np.add.at(rho, idx, val)
    np.add.at(count, idx, (val != 0).astype(np.float64))
    np.add.at(asum, idx, np.abs(val).astype(np.float64))
    return rho, count, asum


def fold(r, n, d):
    """g_bound_periodic per axis: one fold, s == L is left as it is"""
    r = np.array(r)
    for a in range(3):
        L = r.dtype.type(n[a]) * r.dtype.type(d[a])
        s = r[:, a]
        r[:, a] = np.where(s < 0, L - (0 - s), np.where(s > L, 0 + (s - L), s))
    return r


def cells(r, n, d):
    c = np.floor(np.asarray(r, dtype=np.float64) / np.asarray(d)).astype(np.int64)
    return (c[:, 2] * n[1] + c[:, 1]) * n[0] + c[:, 0]


def push(sort, E, B, d, dt, mutate=None):
    r, v = sort["r"], sort["v"]
    T = r.dtype.type
    at = r + v * T(dt) if mutate == "gather_moved" else r
    Ep, Bp = gather(E, B, d, at)
    v1 = update_vEB(dt, sort["q"] / sort["m"], Ep, Bp, v)
    return r + v1 * T(dt), v1


def solve_fft(res, n, d):
    """phi with D G phi = res (res mean-free): the 7-point operator is diagonal in the discrete Fourier basis, its
    eigenvalues -sum 4 sin^2(pi k / n) / d^2; the constant mode is left at 0"""
    nx, ny, nz = n
    lam = 0
    for a, (m, shape) in enumerate(((nx, (1, 1, nx)), (ny, (1, ny, 1)), (nz, (nz, 1, 1)))):
        lam = lam - (4.0 * np.sin(np.pi * np.arange(m) / m) ** 2 / d[a] ** 2).reshape(shape)
    rk = np.fft.fftn(res)
    lam = lam + 0 * rk.real
    out = np.zeros_like(rk)
    nzr = lam != 0
    out[nzr] = rk[nzr] / lam[nzr]
    return np.fft.ifftn(out).real


def step(sorts, E, B, n, d, dt, background=None, mutate=None, dtype=np.float64, solver="dense", reverse=False):
    """one xpic_step of the scheme; sorts (r, v of the given dtype) are advanced in place.  -> (E_new, rho + background, phi)"""
    E = np.asarray(E, dtype=dtype)
    rho = np.zeros((n[2], n[1], n[0]), dtype=dtype)
    for s in sorts:
        r1, v1 = push(s, E, np.asarray(B, dtype=dtype), d, dt, mutate)
        rho = rho + deposit(s["r"] if mutate == "rho_old" else r1, d, n, s["q"] * s["w"], reverse)[0]
        s["r"], s["v"] = fold(r1, n, d), v1
    if background is not None:
        rho = rho + np.asarray(background, dtype=dtype)
    if solver == "fft":
        res, _ = G.residual(E, rho, d)
        phi = solve_fft(res, n, d)
        return E - G.grad(phi, d), rho, phi
    E1, phi, _, _ = G.clean(E, rho, d, backward=mutate == "backward_grad", remove_mean=mutate != "keep_mean",
                            sign=+1.0 if mutate == "plus_grad" else -1.0, dtype=dtype)
    return E1, rho, phi


def two_stream_energy(steps, reverse=False):
    """W_E = |E|^2 / 2 (xpic_energy's first number) of two_stream.beams() from E = 0 cleaned at the start: entry k is taken
    after step k + 1.  The FFT solve; tests/golden/es_two_stream/w_e.npy holds two_stream_energy(400)."""
    import two_stream as TS

    bm, n, d, _ = TS.beams()
    sorts = [dict(r=p[:, :3].copy(), v=p[:, 3:].copy(), q=-1.0, m=1.0, w=0.5 / TS.PPC_BEAM) for p in bm]
    E = np.zeros((n[2], n[1], n[0], 3))
    B = np.zeros_like(E)
    rho = sum(deposit(s["r"], d, n, s["q"] * s["w"], reverse)[0] for s in sorts)
    E = E - G.grad(solve_fft(G.residual(E, rho, d)[0], n, d), d)
    out = []
    for _ in range(steps):
        E = step(sorts, E, B, n, d, TS.DT, solver="fft", reverse=reverse)[0]
        out.append(0.5 * float((E ** 2).sum()))
    return np.array(out)


def omega_leapfrog(n, d, dt, mode, axis=0, wp=1.0):
    """A cold uniform plasma displaced by xi sin(k x): the frequency the scheme itself oscillates at.
    Grid: the deposit multiplies the charge perturbation by S(k) = (sin(k d / 2) / (k d / 2))^3, the 2nd-order spline's
    transform; the solve divides by K^2 = (2 sin(k d / 2) / d)^2 and the forward gradient on the edges returns
    E(x + d / 2) with the factor kappa = 2 sin(k d / 2) / d (the half-cell shift is where the edges are); the gather at
    the particle applies S(k) once more.  With rho_k = -i k n0 q xi S:  E_p = -wp^2 xi S^2 (k kappa / K^2) = -wp^2 xi S^2 (k d / 2) / sin(k d / 2)
    (a continuum of particles: what a particle lattice adds is bounded in tests/test_es_ref.py).  Time: leapfrog x'' = -W^2 x has sin(w dt / 2) = W dt / 2."""
    k = 2.0 * np.pi * mode / (n[axis] * d[axis])
    h = 0.5 * k * d[axis]
    S = (np.sin(h) / h) ** 3
    W = wp * S * np.sqrt(h / np.sin(h))
    return 2.0 / dt * np.arcsin(0.5 * W * dt)
