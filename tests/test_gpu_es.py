"""The electrostatic scheme on the device (include/xpic_es.h, xpic_amd/csrc/es.hip, the "es" step of api.hip) against
tests/es_ref.py's numpy statement: the push and its fused deposit, the deposit against the diagnostic, the slow path and
the periodic wrap, ten steps, the no-op and failing steps, the refusals, a self_ring slab, and the two-stream growth rate.

Bounds.  A gathered component carries K eps sum |F w| (F the field values, w the weights), and the push carries that into
    unit_v = eps (dt |q/m| (sum |E w| + |v| sum |B w|) + |v|),    unit_r = eps max |r| + dt unit_v
per particle (the largest component each).  K is twice the deviation of the float64 statement from the same statement in
np.longdouble on these very inputs, in those units (statement_rounding() below measures it; CPU only):
largest ratios 0.421 (v) and 0.481 (r), so K_PUSH_V = 0.85 and K_PUSH_R = 0.97.
A deposited node: 2 eps * contributions * sum |contribution| (tests/test_gpu_eccapfim.py's bound for deposits)."""
import os

import numpy as np
import pytest

import es_ref as R
import gauss_ref as G

pytestmark = pytest.mark.gpu
EPS = R.EPS
GRIDS = {"6x6x6": ((6, 6, 6), (0.5, 0.4, 0.25)), "7x6x9": ((7, 6, 9), (0.3, 0.5, 0.2))}
DT = 0.05
SORTS = ((5, -1.0, 1.0), (3, +1.0, 3.0))  # (ppc, q, m): opposite charge, different ppc
K_PUSH_V, K_PUSH_R = 0.85, 0.97
K_ROUNDING = 1553.0  # tests/test_gpu_gauss.py: the clean's rounding term K eps (|E| + |G phi|)
RTOL, ATOL, MAXIT = 1e-10, 1e-14, 10000  # the defaults of an "es" context (xpic_es.h)


def load(n, d, seed=7, big=300):
    """-> ([points6 per sort], E, B): one empty cell (cell 0), one cell (the last) with more particles than a round's 256
    lanes, uniform B != 0, random E + a uniform E0; no end point of the push within 1e-9 d of a cell face (asserted by
    the callers on the restatement)"""
    rng = np.random.default_rng(seed)
    nd = np.array(n) * np.array(d)
    pts = []
    for s, (ppc, q, m) in enumerate(SORTS):
        N = ppc * n[0] * n[1] * n[2]
        p = np.empty((N, 6))
        p[:, :3] = rng.random((N, 3)) * nd
        p[:, 3:] = rng.normal(0, 0.3, (N, 3))
        first = (p[:, :3] < np.array(d)).all(axis=1)  # cell 0 stays empty: its particles go to the far corner cell
        p[first, :3] += nd - np.array(d)
        if s == 0:
            extra = np.empty((big, 6))
            extra[:, :3] = nd - np.array(d) * rng.random((big, 3))
            extra[:, 3:] = rng.normal(0, 0.3, (big, 3))
            p = np.vstack([p, extra])
        pts.append(p)
    shape = (n[2], n[1], n[0])
    E = 0.1 * rng.normal(size=shape + (3,)) + np.array([0.02, -0.01, 0.03])
    B = np.zeros(shape + (3,)) + np.array([0.1, -0.2, 0.3])
    return pts, E, B


def context(X, n, d, pts, E, B, dt=DT, **kw):
    g = X.Context("es", n, d, dt, **kw)
    if kw.get("self_ring"):
        g.comm_init_callbacks(lambda down, up, nfu, nfd: (down, up), lambda a: None)
    for (ppc, q, m), p in zip(SORTS, pts):
        s = g.add_sort(ppc, 1.0, q, m, capacity=2 * len(p) + 1024)
        assert g.add_particles(s, p) == len(p)
    g.set_field(X.E, E)
    g.set_field(X.B, B)
    return g


def as_sort(p6, s):
    ppc, q, m = SORTS[s]
    return dict(r=p6[:, :3].copy(), v=p6[:, 3:].copy(), q=q, m=m, w=1.0 / ppc)


def push_units(sort, E, B, d, dt):
    """(unit_v, unit_r) [N] of the module docstring, and the restatement's (r1, v1)"""
    _, _, sE, sB = R.gather(E, B, d, sort["r"], sums=True)
    r1, v1 = R.push(sort, E, B, d, dt)
    vv = np.sqrt((sort["v"] ** 2).sum(axis=1)) + np.sqrt((v1 ** 2).sum(axis=1))
    uv = EPS * (dt * abs(sort["q"] / sort["m"]) * (sE.max(axis=1) + vv * sB.max(axis=1)) + vv)
    ur = EPS * np.maximum(np.abs(r1).max(axis=1), np.abs(sort["r"]).max(axis=1)) + dt * uv
    return uv, ur, r1, v1


def statement_rounding():
    """the measurement behind K_PUSH_* (CPU only; python -c "import test_gpu_es as T; print(T.statement_rounding())")"""
    worst = [0.0, 0.0]
    for n, d in GRIDS.values():
        pts, E, B = load(n, d)
        for s, p in enumerate(pts):
            so = as_sort(p, s)
            uv, ur, r1, v1 = push_units(so, E, B, d, DT)
            sx = dict(so, r=so["r"].astype(np.longdouble), v=so["v"].astype(np.longdouble))
            rx, vx = R.push(sx, E.astype(np.longdouble), B.astype(np.longdouble), d, DT)
            worst[0] = max(worst[0], float((np.abs(v1 - vx).max(axis=1) / uv).max()))
            worst[1] = max(worst[1], float((np.abs(r1 - rx).max(axis=1) / ur).max()))
    return worst


def off_faces(r, d, tol=1e-9):
    pr = r / np.array(d)
    return (np.abs(pr - np.round(pr)) > tol).all()


@pytest.fixture(scope="module")
def X():
    import xpic_amd

    return xpic_amd


def l2(a):
    return float(np.sqrt((np.asarray(a, dtype=np.float64) ** 2).sum()))


def check_push(g, n, d, pts, E, B, label):
    """sections 1 and 2 for every sort of a context: es_push against the restatement, rho against the bound, the cells of
    the re-bin, and the fused deposit against the diagnostic's deposit of the positions left behind"""
    for s in range(len(pts)):
        p0, _ = g.particles(s)  # the sort's own order: the push does not reorder
        so = as_sort(p0, s)
        uv, ur, r1, v1 = push_units(so, E, B, d, DT)
        assert off_faces(r1, d)
        rho = g.es_push(s)
        p1, _ = g.particles(s)
        ev = (np.abs(p1[:, 3:] - v1).max(axis=1) / uv).max()
        er = (np.abs(p1[:, :3] - r1).max(axis=1) / ur).max()
        ref, count, asum = R.deposit(r1, d, n, so["q"] * so["w"])
        bound = 2 * EPS * count * asum
        ed = (np.abs(rho - ref)[bound > 0] / bound[bound > 0]).max()
        print(label, "sort", s, "v err / unit", ev, "r err / unit", er, "rho err / bound", ed, "contributions <=", count.max())
        assert ev <= K_PUSH_V and er <= K_PUSH_R
        assert (np.abs(rho - ref) <= bound).all()
        assert g.update_cells(s) == len(p0)
        p2, c2 = g.particles(s)
        want = R.cells(R.fold(r1, n, d), n, d)
        assert np.array_equal(np.sort(c2), np.sort(want))
        assert np.array_equal(c2, R.cells(p2[:, :3], n, d)) and (np.diff(c2) >= 0).all()
        # 2. the diagnostic on the folded positions: independent of numpy but for the bound's counts
        diag = g.charge_density(s)
        _, count2, asum2 = R.deposit(p2[:, :3], d, n, so["q"] * so["w"])
        bound2 = 2 * EPS * count2 * asum2
        print(label, "sort", s, "fused vs diagnostic err / bound", (np.abs(rho - diag)[bound2 > 0] / bound2[bound2 > 0]).max())
        assert (np.abs(rho - diag) <= bound2).all()


# ---- 1, 2. the push, its deposit, the cells; the fused deposit against the diagnostic -----------------------------------------
@pytest.mark.parametrize("name", list(GRIDS))
def test_es_push_matches_the_statement(X, name):
    n, d = GRIDS[name]
    pts, E, B = load(n, d)
    g = context(X, n, d, pts, E, B)
    occ = np.bincount(R.cells(pts[0][:, :3], n, d), minlength=n[0] * n[1] * n[2])
    assert occ[0] == 0 and occ.max() > 256
    check_push(g, n, d, pts, E, B, name)
    g.close()


# ---- 3. slow path and wrap -----------------------------------------------------------------------------------------------------
def far_movers(n, d, dt):
    """positions and velocities with E = B = 0 (the kick is then exact and v dt the displacement): 1 to 3.5 cells in every
    direction, across each periodic face; a start exactly on a node, a start at L - ulp, an end exactly on a face (power-of-
    two spacings and dt: those products are exact)"""
    rng = np.random.default_rng(11)
    nd = np.array(n) * np.array(d)
    N = 600
    r = rng.random((N, 3)) * nd
    disp = rng.uniform(1.0, 3.5, (N, 3)) * rng.choice([-1.0, 1.0], (N, 3)) * np.array(d)
    for a in range(3):  # the first 60 of each axis start next to a face and cross it
        lo, hi = slice(120 * a, 120 * a + 60), slice(120 * a + 60, 120 * a + 120)
        r[lo, a] = rng.random(60) * d[a]
        disp[lo, a] = -np.abs(disp[lo, a])
        r[hi, a] = nd[a] - rng.random(60) * d[a]
        disp[hi, a] = np.abs(disp[hi, a])
    v = disp / dt
    special_r = np.array([[2 * d[0], 3 * d[1], 1 * d[2]],                               # exactly on a node
                          [np.nextafter(nd[0], 0), np.nextafter(nd[1], 0), np.nextafter(nd[2], 0)],  # L - ulp
                          [1.25 * d[0], 2.5 * d[1], 3.75 * d[2]]])                      # ends exactly on faces
    special_v = np.array([[2.5 * d[0], -1.5 * d[1], 3.0 * d[2]], [1.5 * d[0], 2.0 * d[1], 1.25 * d[2]],
                          [-2.25 * d[0], 1.5 * d[1], 3.25 * d[2]]]) / dt
    return np.hstack([np.vstack([r, special_r]), np.vstack([v, special_v])])


def test_slow_path_and_wrap(X):
    n, d, dt = (6, 6, 6), (0.5, 0.25, 0.125), 0.5
    p = far_movers(n, d, dt)
    Z = np.zeros((n[2], n[1], n[0], 3))
    g = context(X, n, d, [p], Z, Z, dt=dt)
    p0, _ = g.particles(0)
    so = as_sort(p0, 0)
    uv, ur, r1, v1 = push_units(so, Z, Z, d, dt)
    cells0 = np.floor(p0[:, :3] / np.array(d))
    moved = np.abs(np.floor(r1 / np.array(d)) - cells0).max(axis=1)
    assert (moved >= 1).all() and moved.max() >= 3 and (r1 < 0).any(axis=0).all() and (r1 > np.array(n) * np.array(d)).any(axis=0).all()
    rho = g.es_push(0)
    p1, _ = g.particles(0)
    assert np.array_equal(p1[:, 3:], v1)  # no field: the velocities are not touched
    assert (np.abs(p1[:, :3] - r1).max(axis=1) <= K_PUSH_R * ur).all()
    on_face = (r1 / np.array(d) == np.round(r1 / np.array(d))).all(axis=1)
    assert on_face.sum() >= 1 and np.array_equal(p1[on_face, :3], r1[on_face])
    ref, count, asum = R.deposit(r1, d, n, so["q"] * so["w"])
    bound = 2 * EPS * count * asum
    print("slow path: rho err / bound", (np.abs(rho - ref)[bound > 0] / bound[bound > 0]).max(), "cells moved <=", moved.max())
    assert (np.abs(rho - ref) <= bound).all()
    assert abs(rho.sum() - so["q"] * so["w"] * len(p0)) <= 2 * EPS * len(p0) * 27 * abs(so["q"] * so["w"]) * len(p0)
    assert g.update_cells(0) == len(p0) == g.count(0)  # the number of particles is conserved
    p2, c2 = g.particles(0)
    assert np.array_equal(np.sort(c2), np.sort(R.cells(R.fold(r1, n, d), n, d)))
    diag = g.charge_density(0)
    _, count2, asum2 = R.deposit(p2[:, :3], d, n, so["q"] * so["w"])
    b2 = 2 * EPS * count2 * asum2
    print("slow path: fused vs diagnostic err / bound", (np.abs(rho - diag)[b2 > 0] / b2[b2 > 0]).max())
    assert (np.abs(rho - diag) <= b2).all()
    g.close()


# ---- 4. ten steps --------------------------------------------------------------------------------------------------------------
def rot_plus(E, d):
    out = np.empty_like(E)
    dif = lambda c, a: (np.roll(E[..., c], -1, axis=2 - a) - E[..., c]) / d[a]  # noqa: E731
    out[..., 0] = dif(2, 1) - dif(1, 2)
    out[..., 1] = dif(0, 2) - dif(2, 0)
    out[..., 2] = dif(1, 0) - dif(0, 1)
    return out


def ten_step_deviation(name="6x6x6", steps=10):
    """the float64 statement against its np.longdouble refinement over the ten steps of section 4 (CPU only; printed by
    python -c "import test_gpu_es as T; print(T.ten_step_deviation())"): largest |dE|, |dr|, |dv| over the steps.
    Measured on 6x6x6: 1.91e-15, 1.28e-15, 4.74e-16."""
    n, d = GRIDS[name]
    pts, E, B = load(n, d, big=0)
    a = [as_sort(p, s) for s, p in enumerate(pts)]
    b = [dict(so, r=so["r"].astype(np.longdouble), v=so["v"].astype(np.longdouble)) for so in a]
    Ea, Eb = E, E.astype(np.longdouble)
    worst = [0.0, 0.0, 0.0]
    for _ in range(steps):
        Ea = R.step(a, Ea, B, n, d, DT)[0]
        Eb = R.step(b, Eb, B, n, d, DT, dtype=np.longdouble)[0]
        worst[0] = max(worst[0], float(np.abs(Ea - Eb).max()))
        worst[1] = max(worst[1], max(float(np.abs(x["r"] - y["r"]).max()) for x, y in zip(a, b)))
        worst[2] = max(worst[2], max(float(np.abs(x["v"] - y["v"]).max()) for x, y in zip(a, b)))
    return worst


DEV_E, DEV_R, DEV_V = 1.91e-15, 1.28e-15, 4.74e-16  # ten_step_deviation() on 6x6x6


def canon(p6, n, d):
    c = R.cells(p6[:, :3], n, d)
    return p6[np.lexsort((p6[:, 2], p6[:, 1], p6[:, 0], c))]


def test_ten_steps(X):
    """After each step: the law to the stopping rule + the clean's rounding term; rot(+) E and the sums of E within that term
    of their start; B bit-identical; E, r, v track the restatement.  The margin of the last is 2 DEV_* (the statement's own
    rounding over the ten steps) + what the stopping rule leaves in E: a residual |r| is an error |r| / sqrt(lambda_min) of
    E, which reaches v through dt q/m and r through dt again; the errors of earlier steps persist (E is the warm start),
    so they are summed over the steps so far."""
    name = "6x6x6"
    n, d = GRIDS[name]
    pts, E, B = load(n, d, big=0)
    g = context(X, n, d, pts, E, B)
    ref = [as_sort(g.particles(s)[0], s) for s in range(2)]
    Er = E
    lam = G.lambda_min(n, d)
    qm = max(abs(q / m) for _, q, m in SORTS)
    rot0, sum0 = rot_plus(E, d), E.sum(axis=(0, 1, 2))
    acc = 0.0
    for k in range(10):
        its = g.step()
        Er, rho, phi = R.step(ref, Er, B, n, d, DT)
        Eg = g.get_field(X.E)
        info = g.gauss_info()
        res = g.gauss_residual(X.E)
        tol = max(RTOL * res["rho_l2"], ATOL)
        term = K_ROUNDING * EPS * (l2(Eg) + l2(G.grad(phi, d)))
        assert its == info["last_iterations"] and its > 0
        assert res["l2"] <= tol + term / min(d), (k, res["l2"], tol)
        assert l2(rot_plus(Eg, d) - rot0) <= (k + 1) * term / min(d) * 2
        assert np.abs(Eg.sum(axis=(0, 1, 2)) - sum0).max() <= (k + 1) * term * np.sqrt(Eg.size)
        assert np.array_equal(g.get_field(X.B), B)
        acc += info["after"] / np.sqrt(lam)
        bE = 2 * DEV_E + acc + term
        dE = np.abs(Eg - Er).max()
        worst_r = worst_v = 0.0
        for s in range(2):
            pg = canon(g.particles(s)[0], n, d)
            pr = canon(np.hstack([ref[s]["r"], ref[s]["v"]]), n, d)
            worst_r = max(worst_r, np.abs(pg[:, :3] - pr[:, :3]).max())
            worst_v = max(worst_v, np.abs(pg[:, 3:] - pr[:, 3:]).max())
        bV = 2 * DEV_V + (k + 1) * DT * qm * bE
        bR = 2 * DEV_R + (k + 1) * DT * bV
        print("step", k, "its", its, "res", res["l2"], "tol", tol, "dE / bound", dE / bE, "dr / bound", worst_r / bR, "dv / bound", worst_v / bV)
        assert dE <= bE and worst_r <= bR and worst_v <= bV
    g.close()


# ---- 5. nothing to do costs nothing; a failing solve; a NaN ------------------------------------------------------------------
def test_noop_step_failed_solve_and_nan(X):
    n, d = GRIDS["6x6x6"]
    pts, E, B = load(n, d, big=0)
    Z = np.zeros_like(E)
    # a sort whose dt q/m is too small to change a position bit, at rest: a clean start stays clean (the fused deposit's
    # rho differs from the clean's by the order of its sums: 1e-16 of the charge, the rule allows 1e-10)
    g = X.Context("es", n, d, DT)
    s = g.add_sort(5, 1.0, -1.0, 1e300, capacity=len(pts[0]) + 16)
    p = pts[0].copy()
    p[:, 3:] = 0.0
    g.add_particles(s, p)
    g.set_field(X.E, Z)
    g.set_field(X.B, B)
    assert g.gauss_clean(rtol=1e-12).iterations > 0
    E0 = g.get_field(X.E)
    before = g.particles(s)[0]
    assert g.step() == 0
    after = g.particles(s)[0]  # (the re-bin may reorder the particles of a cell: compared as sets)
    key = lambda q: q[np.lexsort(q[:, :3].T[::-1])][:, :3]  # noqa: E731
    assert np.array_equal(g.get_field(X.E), E0) and np.array_equal(key(after), key(before))
    g.close()
    # maxit = 1 on a moving load: the step fails, E untouched
    g = context(X, n, d, pts, E, B)
    g.set_tolerances(RTOL, ATOL, 1)
    with pytest.raises(X.XpicError, match="did not converge"):
        g.step()
    assert np.array_equal(g.get_field(X.E), E)
    g.close()
    # a NaN velocity is an error, E untouched
    bad = [q.copy() for q in pts]
    bad[1][17, 4] = np.nan
    g = context(X, n, d, bad, E, B)
    with pytest.raises(X.XpicError, match="not finite"):
        g.step()
    assert np.array_equal(g.get_field(X.E), E)
    g.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals(X):
    n, d = GRIDS["6x6x6"]
    pts, E, B = load(n, d, big=0)
    g = context(X, n, d, pts, E, B)
    refused = lambda: pytest.raises(X.XpicError, match=r"xpic error [1-9]\d*: .+")  # noqa: E731
    with refused():
        g.set_gauss_clean(1)
    with refused():
        g.solve(X.OP_MATM_CG, X.W0, X.W1)
    for call in (g.ecsim_fill_current, lambda: g.ecsim_second_push(0), lambda: g.ecsimcorr_first_push(0),
                 lambda: g.ecsimcorr_second_push(0), lambda: g.ecsimcorr_final_update(0), lambda: g.basic_push(0),
                 lambda: g.sort_current(0, X.J), lambda: g.get_field(X.J), lambda: g.get_field(X.B0), g.matL):
        with refused():
            call()
    g.charge_collect()
    with refused():
        g.charge_columns()
    assert g.step() > 0  # (and the context still works)
    g.close()
    b = X.Context("basic", n, d, DT)
    sb = b.add_sort(1, 1.0, -1.0, 1.0, capacity=64)
    with refused():
        b.es_push(sb)
    b.close()
    for small in ((5, 6, 6), (6, 5, 6), (6, 6, 5)):
        with pytest.raises(X.XpicError, match=">= 6 cells"):
            X.Context("es", small, d, DT)
    with pytest.raises(X.XpicError, match="at least 6"):
        X.Context("es", (6, 6, 10), d, DT, nranks=2)


# ---- 7. a self_ring slab against the single context ---------------------------------------------------------------------------
def test_self_ring_slab_matches_the_single_context(X):
    """two z-slabs' machinery on one device (ghost planes, halo exchange of E and B, the deposit's ghost planes added to
    their owners, the all-reduces of the solve); distinct ranks stay unpinned"""
    n, d = (6, 6, 12), (0.5, 0.4, 0.25)
    pts, E, B = load(n, d, big=300)
    ring = context(X, n, d, pts, E, B, self_ring=True)
    check_push(ring, n, d, pts, E, B, "self_ring")
    ring.close()
    plain = context(X, n, d, pts, E, B)
    ring = context(X, n, d, pts, E, B, self_ring=True)
    ia, ib = plain.step(), ring.step()
    Ea, Eb = plain.get_field(X.E), ring.get_field(X.E)
    lam = G.lambda_min(n, d)
    fa, fb = plain.gauss_info(), ring.gauss_info()
    assert abs(ia - ib) <= 1
    assert l2(Ea - Eb) <= (fa["after"] + fb["after"]) / np.sqrt(lam) + 2 * K_ROUNDING * EPS * (l2(E) + l2(Ea - E))
    for s in range(2):
        (pa, ca), (pb, cb) = plain.particles(s), ring.particles(s)
        assert np.array_equal(ca, cb)
        assert np.abs(canon(pa, n, d) - canon(pb, n, d)).max() <= 64 * EPS
    plain.close()
    ring.close()


# ---- 8. two-stream -------------------------------------------------------------------------------------------------------------
# W_E of the restatement (es_ref.two_stream_energy(400): FFT solve, recorded once on the CPU -- 400 numpy steps of 73 728
# particles take minutes).  Tracking margin: ten times the largest relative difference between two restatement runs that
# differ only in the summation order of the deposit (reverse=True), over the 400 steps: 2.62e-10, TS_ORDER below.
TS_ORDER = 2.62e-10
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "es_two_stream", "w_e.npy")


def test_two_stream_growth_rate(X):
    import two_stream as TS

    bm, n, d, k = TS.beams()
    g = X.Context("es", n, d, TS.DT)
    for pts in bm:
        s = g.add_sort(TS.PPC_BEAM, 0.5, -1.0, 1.0, capacity=2 * pts.shape[0])
        assert g.add_particles(s, pts) == pts.shape[0]
    # E = 0, start clean.  (The beams' displacements cancel to first order: rho~ is 1e-4 of rho, and the clean's single-pass
    # mean leaves a constant sqrt(N) eps |rho| = 2e-14 in its residual: atol above that.  The first step's own solve, whose
    # mean is refined, then brings E to the step's rule.)
    g.gauss_clean(rtol=RTOL, atol=1e-12)
    t, w, its = [], [], []
    for it in range(700):
        its.append(g.step())
        t.append((it + 1) * TS.DT)
        w.append(g.energy()[0])
    w = np.array(w)
    rate, npts = TS.fit_growth(t, w, 1e-6, 1e-2)
    theory = TS.gamma_theory(k)
    print("two-stream: rate", rate, "theory", theory, "points", npts, "CG iterations per step: mean", np.mean(its), "max", max(its))
    assert w.max() > 1e8 * w[0] and npts >= 100
    assert abs(rate - theory) <= 0.10 * theory, (rate, theory)
    gold = np.load(GOLDEN)
    dev = np.abs(w[:400] / gold - 1.0).max()
    print("two-stream: W_E against the restatement, largest relative difference", dev, "margin", 10 * TS_ORDER)
    assert dev <= 10 * TS_ORDER
    assert g.count(0) == bm[0].shape[0] and g.count(1) == bm[1].shape[0]
    g.close()
