"""The structure the Gauss-law cleaner rests on (no GPU): tests/gauss_ref.py's operators against each other, against the
dense 7-point matrix and against tests/krylov_ref.py's explicit rot(+) and rot(-); the clean's invariants; and the bugs
the GPU tests are there to catch, planted one by one, each seen by one of these checks."""
import numpy as np
import pytest

import gauss_ref as G
import krylov_ref as K

GRIDS = [((2, 3, 5), (0.5, 0.4, 0.25)), ((5, 4, 3), (0.3, 0.7, 0.45)), ((3, 3, 2), (0.6, 0.35, 0.8))]
IDS = ["2x3x5", "5x4x3", "3x3x2"]


def fields(n, seed=0):
    rng = np.random.default_rng(seed)
    shape = (n[2], n[1], n[0])
    return rng.normal(size=shape + (3,)), rng.normal(size=shape) + 0.7


@pytest.mark.parametrize("n,d", GRIDS, ids=IDS)
def test_div_grad_is_the_seven_point_laplacian(n, d):
    D, Gm = G.div_matrix(n, d), G.grad_matrix(n, d)
    L = G.laplacian_dense(n, d)
    DG = (D @ Gm).toarray()
    assert np.abs(DG - L).max() <= 8 * G.EPS * np.abs(L).max()
    assert (L == L.T).all() and np.abs(DG - DG.T).max() <= 8 * G.EPS * np.abs(L).max()
    w = np.linalg.eigvalsh(L)
    scale = np.abs(w).max()
    assert w.max() <= 64 * G.EPS * scale                       # negative semidefinite
    assert (np.abs(w) <= 64 * G.EPS * scale).sum() == 1        # one zero eigenvalue ...
    assert np.abs(L @ np.ones(L.shape[0])).max() <= 8 * G.EPS * scale  # ... and it is the constants'
    assert -w[-2] == pytest.approx(G.lambda_min(n, d), rel=1e-12)
    # the array statements are the matrices
    F, rho = fields(n)
    assert np.abs(G.div(F, d).ravel() - D @ F.ravel()).max() <= 16 * G.EPS * np.abs(D).dot(np.abs(F.ravel())).max()
    assert np.abs(G.grad(rho, d).ravel() - Gm @ rho.ravel()).max() <= 16 * G.EPS * np.abs(Gm).dot(np.abs(rho.ravel())).max()
    # the off-diagonal weight at an extent of 2 is 2 / d^2
    for c in range(3):
        if n[c] == 2:
            q1 = (1, n[0], n[0] * n[1])[c]
            assert L[0, q1] == pytest.approx(2.0 / d[c] ** 2, rel=1e-15)


@pytest.mark.parametrize("n,d", GRIDS, ids=IDS)
def test_curl_of_the_gradient_and_divergence_of_the_curl_vanish(n, d):
    Rp, Rm = K.rot_matrix(n, d, True), K.rot_matrix(n, d, False)
    D, Gm = G.div_matrix(n, d), G.grad_matrix(n, d)
    # in structure: every entry cancels to rounding of the products that make it up
    RG, DR = (Rp @ Gm).toarray(), (D @ Rm).toarray()
    assert np.abs(RG).max() <= 8 * G.EPS * (abs(Rp) @ abs(Gm)).toarray().max()
    assert np.abs(DR).max() <= 8 * G.EPS * (abs(D) @ abs(Rm)).toarray().max()
    # the planted bug: G with the backward shift is not annihilated by rot(+), and D G is then no longer symmetric
    Gb = G.grad_matrix(n, d, backward=True)
    assert np.abs((Rp @ Gb).toarray()).max() >= 0.5 / max(d) ** 2
    DGb = (D @ Gb).toarray()
    assert np.abs(DGb - DGb.T).max() >= 0.5 / max(d) ** 2 or max(n) <= 2


@pytest.mark.parametrize("n,d", GRIDS, ids=IDS)
def test_clean_restores_the_law_and_keeps_curl_and_means(n, d):
    F, rho = fields(n, 1)
    Rp = K.rot_matrix(n, d, True)
    F1, phi, res, mean = G.clean(F, rho, d)
    scale = np.abs(F).max() / min(d) + np.abs(rho).max()
    assert mean == rho.mean() and abs(phi.mean()) <= 64 * G.EPS * np.abs(phi).max()
    assert np.abs(G.residual(F1, rho, d)[0]).max() <= 1e3 * G.EPS * scale      # D F' = rho~ to solver precision
    assert np.abs(G.residual(F, rho, d)[0]).max() >= 1e-2 * scale               # (it was not so before)
    assert np.abs(Rp @ (F1 - F).ravel()).max() <= 1e3 * G.EPS * scale / min(d)  # rot F untouched
    assert np.abs((F1 - F).sum(axis=(0, 1, 2))).max() <= 1e3 * G.EPS * F.size * np.abs(F1 - F).max()  # the means too

    def after(**bug):
        F2 = G.clean(F, rho, d, **bug)[0]
        return (np.abs(G.residual(F2, rho, d)[0]).max(), np.abs(Rp @ (F2 - F).ravel()).max())

    # the planted bugs, each seen by the law or by the curl
    assert after(sign=+1.0)[0] >= 1e-2 * scale                                  # phi added instead of subtracted
    # the mean not removed: the right-hand side leaves the range of D G, no phi restores that law (sum D F = 0) and the
    # residual the buggy code would report never falls below the mean
    F2 = G.clean(F, rho, d, remove_mean=False)[0]
    assert np.sqrt((G.residual(F2, rho, d, remove_mean=False)[0] ** 2).mean()) >= 0.99 * abs(rho.mean())
    assert after(backward=True)[1] >= 1e-3 * scale                              # G with the backward shift: rot F changes
    if min(n) == 2:
        assert after(fold=False)[0] >= 1e-3 * scale                             # the unfolded stencil at extent 2
        Lu = G.laplacian_dense(n, d, fold=False)
        assert np.abs(Lu @ np.ones(Lu.shape[0])).max() >= 0.5 / max(d) ** 2     # (the constants left its null space)


def test_extended_precision_statement_agrees():
    """the float64 statement against the same statement refined in np.longdouble: the ratio K that the GPU test's bound
    K eps (|E| + |G phi|) takes twice over (tests/test_gpu_gauss.py: K_ROUNDING)"""
    worst = 0.0
    for n, d in GRIDS:
        F, rho = fields(n, 2)
        F64, phi64 = G.clean(F, rho, d)[:2]
        Fx, phix = G.clean(F, rho, d, dtype=np.longdouble)[:2]
        num = float(np.sqrt(((F64 - Fx) ** 2).sum()))
        den = G.EPS * float(np.sqrt((F ** 2).sum()) + np.sqrt((G.grad(phix, d) ** 2).sum()))
        worst = max(worst, num / den)
    assert worst <= 32.0, worst
