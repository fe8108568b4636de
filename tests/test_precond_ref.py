"""CPU checks of tests/precond_ref.py, the float64 restatement tests/test_gpu_precond.py holds the device against: its
stencil layout and matM against the oracle, its Chebyshev recurrence against the same polynomial of the dense matrix and
against the Chebyshev bound, and -- for every case of the GPU test -- that the bugs a polynomial preconditioner can hide
from the solver's own tests (a tap lost, a halo not wrapped, a stale window plane, a density ratio off by a node) move P r
by at least ten times the tolerance the GPU test grants."""
import ctypes as C

import numpy as np
import pytest

import precond_ref as P

SMALL = ((6, 5, 4), P.D_GENERAL, P.DT)


def oracle_matL(oracle, n, d, dt, sorts, B, B0=P.B0):
    o = oracle.OracleSim("ecsim", n, d, dt)
    for par, pts in sorts:
        s = o.add_sort(*par)
        assert o.add_particles(s, pts) == len(pts)
    o.set_field("B", B)
    o.set_field("B0", np.zeros_like(B) + np.array(B0))
    oracle.lib().orc_ecsim_fill_current(o.h)
    return o, o.matL()


def small_load(seed, B0=P.B0, ramp=False):
    n, d, dt = SMALL
    rng = np.random.default_rng(seed)
    npart = 32 * n[0] * n[1] * n[2]
    pts = np.empty((npart, 6))
    pts[:, :3] = rng.random((npart, 3)) * (np.array(n) * np.array(d))
    if ramp:
        pts[:, 0] = (6.0 - np.sqrt(36.0 - 35.0 * rng.random(npart))) / 5.0 * n[0] * d[0] * 0.999999
    pts[:, 3:] = rng.normal(0, 0.05, (npart, 3))
    shape = (n[2], n[1], n[0], 3)
    return [((32, 1.0, -1.0, 1.0), pts)], rng.normal(0, 0.02, shape) + np.array(B0), rng.normal(0, 1.0, shape)


def test_layout_and_matM_match_the_oracle(oracle):
    L = oracle.lib()
    for c1 in range(3):
        for k in range(P.LSTENCIL):
            c2, d3 = C.c_int(), (C.c_int * 3)()
            L.orc_lstencil_decode(c1, k, C.byref(c2), d3)
            assert (c2.value, tuple(d3)) == P.ldecode(c1, k)
            assert P.lencode(c1, c2.value, tuple(d3)) == k
    n, d, dt = SMALL
    o = oracle.OracleSim("ecsim", n, d, dt)
    x = np.random.default_rng(1).normal(0, 1, o.fshape())
    ref = o.matM(x)
    assert np.abs(P.matM(x, d, dt) - ref).max() <= 1e-13 * np.abs(ref).max()
    assert np.abs(P.stencil_apply(P.matM_stencil(d, dt), x, n) - ref).max() <= 1e-13 * np.abs(ref).max()
    # the surrogate's matL part against the oracle's matL applied to a vector that the translation average cannot tell from
    # matL itself: a constant one
    sorts, B, _ = small_load(2)
    o, matL = oracle_matL(oracle, n, d, dt, sorts, B)
    sur = P.Surrogate(matL, n, d, dt, 3)
    one = np.ones(o.fshape())
    full = P.stencil_apply(sur.abar[:, :P.LSTENCIL] - sur.mco, one, n)
    mean = o.matL_apply(one).mean(axis=(0, 1, 2))
    assert np.abs(full - mean).max() <= 1e-12 * np.abs(mean).max()
    # the kept taps carry their block's dropped ones: same row sums, block by block
    kept = P.stencil_apply(sur.lkept, one, n)
    assert np.abs(kept - mean).max() <= 1e-12 * np.abs(mean).max()
    assert np.count_nonzero(sur.lkept) == 3 * (27 + 12 + 12)


def dense_polynomial(A, lo, hi, degree, r):
    """z with r - A z = T_k((theta - A) / delta) r / T_k(theta / delta): the Chebyshev iteration's k-th iterate"""
    theta, delta = 0.5 * (hi + lo), 0.5 * (hi - lo)
    X = (theta * np.eye(A.shape[0]) - A) / delta
    s = theta / delta
    T0, T1, t0, t1 = np.eye(A.shape[0]), X, 1.0, s
    for _ in range(degree - 1):
        T0, T1 = T1, 2.0 * X @ T1 - T0
        t0, t1 = t1, 2.0 * s * t1 - t0
    return np.linalg.solve(A, r - T1 @ r / t1)


@pytest.mark.parametrize("kind", [3, 4])
def test_recurrence_is_the_polynomial_of_the_dense_matrix(oracle, kind):
    n, d, dt = SMALL
    sorts, B, r = small_load(3, ramp=kind == 4)
    _, matL = oracle_matL(oracle, n, d, dt, sorts, B)
    sur = P.Surrogate(matL, n, d, dt, kind)
    if kind == 4:
        A = P.dense_matrix(sur.lkept, n, rscale=sur.rscale, mco=sur.mco)
    else:
        A = P.dense_matrix(sur.ckept, n)
    assert np.abs(A @ r.ravel() - P.abar_apply(sur, r).ravel()).max() <= 1e-12 * np.abs(A).max() * np.abs(r).max()
    for degree in (2, 3, 5, sur.degree):
        z = P.cheb_abar(sur, r, degree)
        ref = dense_polynomial(A, sur.lo, sur.hi, degree, r.ravel())
        assert np.abs(z.ravel() - ref).max() <= 1e-12 * np.abs(ref).max(), degree
    # the polynomial in matM alone (kinds 1, 2)
    M = P.dense_matrix(sur.mco, n)
    lo, hi = P.matM_interval(d, dt)
    for degree in (2, 3, 5) + P.matM_degrees(d, dt):
        ref = dense_polynomial(M, lo, hi, degree, r.ravel())
        assert np.abs(P.cheb_matM(r, d, dt, degree).ravel() - ref).max() <= 1e-12 * np.abs(ref).max(), degree


def test_residual_stays_within_the_chebyshev_bound(oracle):
    """Without a magnetic field the translation average is symmetric: its eigenvalues are real, and where they lie in
    [lo, hi] the residual polynomial is bounded by 2 rho^k / (1 + rho^2k) in the 2-norm."""
    n, d, dt = SMALL
    sorts, B, r = small_load(4, B0=(0.0, 0.0, 0.0))
    _, matL = oracle_matL(oracle, n, d, dt, sorts, np.zeros_like(B), B0=(0.0, 0.0, 0.0))
    sur = P.Surrogate(matL, n, d, dt, 3)
    A = P.dense_matrix(sur.ckept, n)
    assert np.abs(A - A.T).max() <= 1e-12 * np.abs(A).max()
    ev = np.linalg.eigvalsh(0.5 * (A + A.T))
    assert sur.lo <= ev.min() and ev.max() <= sur.hi and sur.proven
    sk = np.sqrt(sur.hi / sur.lo)
    rho = (sk - 1.0) / (sk + 1.0)
    for k in (2, 5, 8):
        z = P.cheb_abar(sur, r, k)
        res = np.linalg.norm(r - P.abar_apply(sur, z)) / np.linalg.norm(r)
        assert res <= 2.0 * rho ** k / (1.0 + rho ** (2 * k)) * (1.0 + 1e-12), (k, res)


def drop_smallest_kept_tap(sur):
    nz = np.where(sur.ckept != 0.0, np.abs(sur.ckept), np.inf)
    i = np.unravel_index(np.argmin(nz), nz.shape)
    sur.ckept[i] = 0.0
    sur.lkept[i] = 0.0
    return sur


@pytest.mark.parametrize("name", list(P.CASES))
def test_mutations_are_visible(oracle, name):
    """Each listed bug, built into the float64 restatement, moves P r by >= 10 x the tolerance of the GPU test at this case
    (the plain rows for the first three, the scaled rows for all four; automatic degree, the one the solves run).
    Not every shape can show every bug: up to 8 planes are one z-chunk (no chunk boundary: 12x10x8, 16x10x8, 131x3x5,
    3x2x5), so the stale plane is checked where nz > 8."""
    n, d, dt, sorts, B, r = P.build_case(name)
    _, matL = oracle_matL(oracle, n, d, dt, sorts, B)
    # kind 5's choice cannot hang on rounding (threshold 0.2)
    spread = np.sqrt(P.Surrogate(matL, n, d, dt, 5).spread.max())
    assert not 0.15 <= spread <= 0.27, spread
    for kind in (3, 4):
        sur = P.Surrogate(matL, n, d, dt, kind)
        ref = P.cheb_abar(sur, r)
        tol = P.tolerance(ref, P.cheb_abar(sur, r, dtype=np.float32))
        assert tol <= 1e-5 * np.abs(ref).max()  # (fp32: a few 1e-6 of the result)
        moved = {"tap": P.cheb_abar(drop_smallest_kept_tap(P.Surrogate(matL, n, d, dt, kind)), r),
                 "halo": P.cheb_abar(sur, r, mutate="halo")}
        if P.first_chunk_boundary(n) is not None:
            moved["plane"] = P.cheb_abar(sur, r, mutate="plane")
        if kind == 4:
            moved["ratio"] = P.cheb_abar(sur, r, mutate="ratio")
        for what, z in moved.items():
            assert np.abs(z - ref).max() >= 10.0 * tol, (kind, what, np.abs(z - ref).max() / tol)
