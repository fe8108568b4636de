"""CPU checks of tests/krylov_ref.py, the float64 restatement tests/test_gpu_krylov.py holds the field solve against: its
matrices against the oracle's operators on every shape of the GPU test, the oracle's solves against a direct solve, and --
for the bugs a Krylov driver can hide behind its own convergence -- that each of them, planted in a numpy copy of the
device's drivers (krylov.hip: classical Gram-Schmidt in one reduction, the multi-dot in groups of 8 with its w . w row,
the basis kept between solves), moves the assertion of the GPU test that is meant to catch it past its bound.  The last
test restates k_matA's decode of blockIdx.x and counts what a launch produces."""
import math

import numpy as np
import pytest

import krylov_ref as K
import precond_ref as P
from test_precond_ref import oracle_matL


@pytest.fixture(scope="module")
def systems(oracle):
    """name -> (n, d, dt, the oracle's context, matL, A = matM + matL, rhs): the solve grids of the GPU test"""
    out = {}
    for name, (n, d, dt, seed, B0) in K.SOLVE_CASES.items():
        sorts, B, rhs, _ = K.build_load(n, d, seed, B0=B0)
        o, matL = oracle_matL(oracle, n, d, dt, sorts, B, B0)
        A = K.matM_matrix(n, d, dt) + K.matL_matrix(matL, n)
        out[name] = (n, d, dt, o, matL, A.tocsr(), rhs)
    return out


# ---- the matrices ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K.SHAPES))
def test_matrices_reproduce_the_oracle(oracle, name):
    n, zs, _ = K.SHAPES[name]
    assert K.row_split(n[1], n[2]) == zs
    d, dt = K.D_GENERAL, K.DT
    sorts, B, x, _ = K.build_load(n, d, 200 + list(K.SHAPES).index(name), ppc=2 + list(K.SHAPES).index(name) % 3)
    o, matL = oracle_matL(oracle, n, d, dt, sorts, B, K.B0)
    Rp, Rm, M, L = K.rot_matrix(n, d, True), K.rot_matrix(n, d, False), K.matM_matrix(n, d, dt), K.matL_matrix(matL, n)
    for got, ref in ((K.apply(Rp, x), o.rot(+1, 1.0, x)), (K.apply(Rm, x), o.rot(-1, 1.0, x)), (K.apply(M, x), o.matM(x)),
                     (K.apply(L, x), o.matL_apply(x)), (K.apply(Rp, x), P.rot(x, d, True)), (K.apply(M, x), P.matM(x, d, dt))):
        assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()
    assert abs(Rm - Rp.T).max() == 0.0
    assert abs(M - M.T).max() <= 1e-13 * abs(M).max()
    N = M.shape[0]
    import scipy.sparse as sp

    assert abs(M - (2.0 * sp.identity(N) + 0.5 * dt * dt * (Rm @ Rp))).max() <= 1e-13 * abs(M).max()


@pytest.mark.parametrize("name", list(K.SOLVE_CASES))
def test_oracle_solves_agree_with_the_direct_solve(systems, name):
    n, d, dt, o, matL, A, rhs = systems[name]
    M = K.matM_matrix(n, d, dt)
    for op, mat in ((0, A), (1, M), (2, M)):
        xs = K.direct_solve(mat, rhs)
        xo, its, _ = o.solve(op, rhs, 1e-9, 1e-50, 300)
        assert its > 0
        assert np.linalg.norm(xo - xs) <= K.cond2(mat) * 1e-9 * np.linalg.norm(xs), (op, its)


def test_restated_methods_solve(systems):
    n, d, dt, o, matL, A, rhs = systems["6x5x4"]
    xs = K.direct_solve(A, rhs).ravel()
    bn = np.linalg.norm(rhs)
    x, its, hist = K.gmres(A, rhs, 1e-10, 0.0, 300)
    assert K.true_residual(A, x, rhs) <= 1.05e-10 * bn and len(hist) == its and np.linalg.norm(x - xs) <= 1e-8 * np.linalg.norm(xs)
    M = K.matM_matrix(n, d, dt)
    x, its, hist = K.cg(M, rhs, 1e-10, 0.0, 300)
    assert K.true_residual(M, x, rhs) <= 1.05e-10 * bn and len(hist) == its
    _, its_o, _ = o.solve(2, rhs, 1e-10, 1e-50, 300)
    assert abs(its - its_o) <= 1


def test_dot_bound_holds_for_other_summation_orders():
    rng = np.random.default_rng(5)
    x = np.where(np.arange(5001) % 2 == 0, 1e8, -1e8) + 1e-8 * rng.normal(size=5001)
    y = rng.normal(size=5001)
    ref, bound = K.dot_exact(x, y), K.dot_bound(x, y)
    for s in (x @ y, float(np.sum(x * y)), sum((x * y).tolist()), sum((x * y)[::-1].tolist())):
        assert abs(s - ref) <= bound
    assert abs(float(np.sum((x * y)[:-1])) - ref) > bound  # one term lost


# ---- the device's drivers in numpy, with the bugs to plant ---------------------------------------------------------------
class Workspace:
    """what a context keeps between its solves: the basis"""

    def __init__(self, N, fill=0.0):
        self.V = np.full((K.RESTART + 2, N), fill)


def device_gmres(A, b, rtol, atol, maxit, ws, x_in=None, plant=None):
    """krylov.hip: gmres without a preconditioner, line by line -> (x, its, reason, rnorm, reductions).
    plants: "drop8" the last column of a full group of 8 missing from the multi-dot; "wwrow" w . w read from row nv - 1;
    "stale" the driver does not stop at a breakdown (|h_j+1| at rounding level): V_j+1 is not written AND the iteration
    goes on with what the workspace held -- the stale vector alone is harmless, the loop ends there and the next solve
    rewrites the basis from V_0 on; what the eigenvector case guards is the stop; "recur" the restart keeps the recurrence's norm for b - A x; "dirty" x is not cleared; "pyth" the
    identity |w - sum h V|^2 = w.w - sum h^2 stays in use below 1e-6 |b|"""
    m = K.RESTART
    b = np.asarray(b, dtype=np.float64).ravel()
    V = ws.V
    x = np.zeros_like(b) if plant != "dirty" or x_in is None else np.array(x_in, dtype=np.float64).ravel()
    bnorm = math.sqrt(b @ b)
    nred = 1
    tol = max(rtol * bnorm, atol)
    rnorm, its = bnorm, 0
    if rnorm <= tol:
        return x, 0, 1, rnorm, nred
    r = b
    H = np.zeros((m + 1, m))
    cs, sn, gg, h = np.zeros(m), np.zeros(m), np.zeros(m + 1), np.zeros(m + 2)
    while its < maxit:
        V[0] = r / rnorm
        gg[:] = 0.0
        gg[0] = rnorm
        j = 0
        while j < m and its < maxit:
            w = A @ V[j]
            pyth = (tol >= 1e-8 * bnorm and rnorm > 1e-6 * bnorm) or plant == "pyth"
            nv = j + 1
            for j0 in range(0, nv, 8):
                g = min(8, nv - j0)
                h[j0:j0 + g] = V[j0:j0 + g] @ w
                if plant == "drop8" and g == 8:
                    h[j0 + 7] = 0.0
            ww = (h[nv - 1] if plant == "wwrow" else w @ w) if pyth else 0.0
            nred += 1
            hh = float(h[:nv] @ h[:nv])
            nrm2 = ww - hh if pyth else 0.0
            broke = False
            if not pyth or not nrm2 > 1e-4 * ww:
                w = w - h[:nv] @ V[:nv]
                nrm2 = w @ w
                nred += 1
                h[j + 1] = math.sqrt(nrm2)
                broke = plant == "stale" and h[j + 1] <= 1e-12 * abs(h[j])
                if h[j + 1] != 0.0 and not broke:
                    V[j + 1] = w / h[j + 1]
            else:
                h[j + 1] = math.sqrt(nrm2)
                V[j + 1] = (w - h[:nv] @ V[:nv]) / h[j + 1]
            for i in range(j):
                h[i], h[i + 1] = cs[i] * h[i] + sn[i] * h[i + 1], -sn[i] * h[i] + cs[i] * h[i + 1]
            den = math.hypot(h[j], h[j + 1])
            cs[j], sn[j] = (h[j] / den, h[j + 1] / den) if den != 0.0 else (1.0, 0.0)
            h[j] = den
            gg[j + 1], gg[j] = -sn[j] * gg[j], cs[j] * gg[j]
            H[:j + 1, j] = h[:j + 1]
            its += 1
            rnorm = abs(gg[j + 1])
            j += 1
            if rnorm <= tol and not broke:
                break
        y = np.zeros(j)
        for i in range(j - 1, -1, -1):
            t = gg[i] - H[i, i + 1:j] @ y[i + 1:]
            y[i] = t / H[i, i] if H[i, i] != 0.0 else 0.0
        x = x + y @ V[:j]
        if rnorm <= tol or its >= maxit:
            break
        w = b - A @ x
        nred += 1
        if plant != "recur":
            rnorm = math.sqrt(w @ w)
        V[m + 1] = w
        r = V[m + 1]
        if rnorm <= tol:
            break
    return x, its, (2 if rnorm <= tol else -3), rnorm, nred


def device_cg(A, b, rtol, atol, maxit, plant=None):
    """krylov.hip: cg.  plant "beta": the new r . r is stored before beta is formed from `the old one`"""
    b = np.asarray(b, dtype=np.float64).ravel()
    x, r, p = np.zeros_like(b), b.copy(), b.copy()
    rr = r @ r
    tol = max(rtol * math.sqrt(rr), atol)
    its = 0
    while math.sqrt(rr) > tol and its < maxit:
        Ap = A @ p
        alpha = rr / (p @ Ap)
        x += alpha * p
        r -= alpha * Ap
        rr1 = r @ r
        if plant == "beta":
            rr = rr1
        beta = rr1 / rr
        rr = rr1
        p = r + beta * p
        its += 1
    return x, its, (2 if math.sqrt(rr) <= tol else -3), math.sqrt(rr)


def figures(A, b, got, rtol, atol=1e-50, explicit=False, cgm=False):
    x, its, reason, rnorm = got[:4]
    if reason <= 0:
        return {"reason": (1, 0)}
    ref = (K.cg if cgm else K.gmres)(A, b, rtol, atol, 300)[1]
    return K.solve_figures(A, b, x, its, rnorm, rtol, atol, K.direct_solve(A, np.ravel(b)), K.cond2(A), ref, explicit)


def restart_system(systems):
    return systems["restart"][5], systems["restart"][6]


def test_the_unplanted_drivers_pass_every_check(systems):
    n, d, dt, o, matL, A, rhs = systems["8x8x6"]
    ws = Workspace(A.shape[0])
    for rtol in (1e-5, 1e-7, 1e-8, 1.01e-8, 0.99e-8, 1e-11):
        got = device_gmres(A, rhs, rtol, 1e-50, 300, ws)
        f = figures(A, rhs, got, rtol, explicit=rtol == 1e-11)
        print(rtol, got[1], got[4], f)
        assert not K.failed(f), (rtol, f)
        if rtol == 1e-5:
            assert got[4] <= got[1] + 3 + (got[1] - 1) // 30
    Ar, b = restart_system(systems)
    for rtol in (1e-9, 1e-7):  # every norm explicit; the one-reduction norm down to 1e-6 |b|
        got = device_gmres(Ar, b, rtol, 1e-50, 300, ws)
        f = figures(Ar, b, got, rtol)
        print("restart", rtol, got[1], f)
        assert 60 < got[1] < 120 and not K.failed(f), (rtol, got[1:], f)
    M = K.matM_matrix(n, d, dt)
    assert not K.failed(figures(M, rhs, device_cg(M, rhs, 1e-9, 1e-50, 300), 1e-9, cgm=True))


@pytest.mark.parametrize("plant", ["drop8", "wwrow", "stale", "recur", "dirty", "beta"])
def test_planted_bugs_move_their_assertion(systems, plant):
    """each plant against the case of the GPU test that is there for it"""
    n, d, dt, o, matL, A, rhs = systems["8x8x6"]
    ws = Workspace(A.shape[0])
    if plant == "drop8":  # more than 8 iterations: the ordinary solves
        for rtol in (1e-5, 1e-7):
            bad = K.failed(figures(A, rhs, device_gmres(A, rhs, rtol, 1e-50, 300, ws, plant=plant), rtol))
            assert bad, rtol
    elif plant == "wwrow":  # the norm falls back to a second reduction: visible in the count of reductions only
        x, its, reason, rn, nred = device_gmres(A, rhs, 1e-5, 1e-50, 300, ws, plant=plant)
        assert not K.failed(figures(A, rhs, (x, its, reason, rn), 1e-5))
        assert nred > its + 3 + (its - 1) // 30
    elif plant == "stale":  # a constant field on the empty context: A b = 2 b, one iteration
        M = K.matM_matrix(n, d, dt)
        b = np.zeros(rhs.shape) + np.array([0.5, -1.25, 2.0])
        x, its, reason, rn, _ = device_gmres(M, b, 1e-7, 1e-50, 300, Workspace(M.shape[0]))
        assert its == 1 and reason > 0 and np.abs(x - 0.5 * b.ravel()).max() <= 1e-15 * np.abs(b).max()
        device_gmres(M, rhs, 1e-7, 1e-50, 300, ws)  # an earlier solve leaves its basis behind
        x, its, reason, rn, _ = device_gmres(M, b, 1e-7, 1e-50, 300, ws, plant=plant)
        assert its != 1
    elif plant == "recur":  # two restarts at rtol 1e-7: above 1e-6 |b| the norms come from the one-reduction identity, the
        # recurrence drifts over a cycle, and only b - A x at the restart brings it back (at 1e-9 every norm is explicit
        # and the plant moves nothing: 1.4e-14 |b|)
        Ar, b = restart_system(systems)
        got = device_gmres(Ar, b, 1e-7, 1e-50, 300, ws, plant=plant)
        f = figures(Ar, b, got, 1e-7)
        print(got[1], f)
        assert {"residual", "rnorm", "iterations"} <= set(K.failed(f)), f
    elif plant == "dirty":  # b = 0 with x pre-filled, and an ordinary solve after it
        x, its, reason, rn, _ = device_gmres(A, np.zeros(rhs.shape), 1e-7, 1e-50, 300, ws, x_in=np.full(rhs.size, 7.0), plant=plant)
        assert its == 0 and np.any(x != 0.0)
        got = device_gmres(A, rhs, 1e-7, 1e-50, 300, ws, x_in=np.full(rhs.size, 7.0), plant=plant)
        assert "residual" in K.failed(figures(A, rhs, got, 1e-7))
    else:
        M = K.matM_matrix(n, d, dt)
        assert K.failed(figures(M, rhs, device_cg(M, rhs, 1e-9, 1e-50, 300, plant=plant), 1e-9, cgm=True))


def test_the_identity_kept_at_every_residual_stays_inside_the_bounds(systems):
    """One bug of the list does NOT move an assertion at these sizes, in this restatement: the one-reduction identity
    |w - sum h V|^2 = w.w - sum h^2 kept in use below 1e-6 |b| -- planted here at every residual and every tolerance
    ("pyth").  Its guard (the explicit norm whenever the difference keeps fewer than 4 digits) bounds what it can do, and
    the rest needs a basis that has lost orthogonality.  Measured at rtol 1e-11, 45 iterations: |rnorm - |b - A x|| =
    1.8e-15 against 6.7e-11, the count equal to the textbook method's."""
    n, d, dt, o, matL, A, rhs = systems["8x8x6"]
    ws = Workspace(A.shape[0])
    for rtol in (0.99e-8, 1e-11):
        assert not K.failed(figures(A, rhs, device_gmres(A, rhs, rtol, 1e-50, 300, ws, plant="pyth"), rtol, explicit=rtol == 1e-11))


# ---- k_matA's decode -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K.SHAPES))
def test_row_decode_produces_every_row_group_once(name):
    n, zs, _ = K.SHAPES[name]
    runs = [n[2]] + ([4, 2, 1] if name in ("two-bands", "eight-bands") else [])  # and the plane runs of a slab's split apply
    for nzr in runs:
        assert np.all(K.row_cover(n, nzr) == 1), nzr
    if name == "eight-bands":  # the one split no whole box of the GPU test takes: 1 run of planes x 8 groups of bands
        assert K.row_split(n[1], 1) == 1 and np.any(K.row_cover(n, 1, plant="Pb") != 1)
    if zs < 8 and K._bands(n[1])[1] > 1:  # more than one group of y-bands
        assert np.any(K.row_cover(n, n[2], plant="Pb") != 1)
    else:
        assert np.all(K.row_cover(n, n[2], plant="Pb") == 1)  # (one band, or one group: the plant cannot show)
