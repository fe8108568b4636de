"""Plain numpy restatement of Gauss's law on the periodic Yee grid (include/xpic_gauss.h, xpic_amd/csrc/gauss.hip; DESIGN.md
5za), written from the operators' definitions with neither the oracle nor the library.

Vectors are get_field's arrays [nz][ny][nx][3], scalars [nz][ny][nx]; n = (nx, ny, nz), d = (dx, dy, dz).

    div(F, d)                the negative-shift divergence D (src/utils/operators.cpp:275-333, fields.hip: k_div_neg_add)
    grad(phi, d)             G: the forward difference onto the edges where E lives (backward=True: the planted bug)
    laplacian_dense(n, d)    the 7-point matrix entry by entry, neighbours wrapped: at an extent of 2 both neighbours are
                             one node and the off-diagonal entry is 2 / d^2 (fold=False: the planted bug, one of them skipped)
    div_matrix, grad_matrix  D and G as sparse matrices on krylov_ref's interleaved unknowns ((z ny + y) nx + x) 3 + c
    solve_meanfree(L, b)     the minimum-norm least-squares solution: mean-free, the null space being the constants
    residual(F, rho, d)      (D F - (rho - mean rho), mean rho)
    clean(F, rho, d)         (F - G phi, phi, res, mean) with D G phi = res; dtype=np.longdouble refines the float64 solve
                             in extended precision (the yardstick of the float64 statement's own rounding)
    lambda_min(n, d)         smallest non-zero eigenvalue of -D G over the axes with n >= 2 (all of them)
"""
import numpy as np
import scipy.sparse as sp

import krylov_ref as K

EPS = K.EPS


def div(F, d):
    F = np.asarray(F)
    out = 0
    for c in range(3):
        i = F.dtype.type(1) / F.dtype.type(d[c])
        out = out + (i * F[..., c] - i * np.roll(F[..., c], 1, axis=2 - c))
    return out


def grad(phi, d, backward=False):
    phi = np.asarray(phi)
    out = np.empty(phi.shape + (3,), dtype=phi.dtype)
    for c in range(3):
        i = phi.dtype.type(1) / phi.dtype.type(d[c])
        out[..., c] = i * (phi - np.roll(phi, 1, axis=2 - c)) if backward else i * (np.roll(phi, -1, axis=2 - c) - phi)
    return out


def laplacian_dense(n, d, fold=True):
    nx, ny, nz = n
    N = nx * ny * nz
    L = np.zeros((N, N))
    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                q = (z * ny + y) * nx + x
                for c, (e, i) in enumerate(((nx, x), (ny, y), (nz, z))):
                    w = 1.0 / (d[c] * d[c])
                    L[q, q] -= 2.0 * w
                    for s in ((+1, -1) if fold or e > 2 else (+1,)):
                        j = [x, y, z]
                        j[c] = (i + s) % e
                        L[q, (j[2] * ny + j[1]) * nx + j[0]] += w
    return L


def _scalar_to_component(c, transpose=False):
    E = sp.coo_matrix(([1.0], ([c], [0])), shape=(3, 1))
    return E.T if transpose else E


def grad_matrix(n, d, backward=False):
    """(3N x N): phi -> the interleaved vector G phi"""
    return sum(sp.kron(K.diff_matrix(n, d, c, not backward), _scalar_to_component(c)) for c in range(3)).tocsr()


def div_matrix(n, d):
    """(N x 3N): the interleaved vector F -> D F (backward differences)"""
    return sum(sp.kron(K.diff_matrix(n, d, c, False), _scalar_to_component(c, True)) for c in range(3)).tocsr()


def solve_meanfree(L, b):
    return np.linalg.lstsq(np.asarray(L, dtype=np.float64), np.asarray(b, dtype=np.float64).ravel(), rcond=None)[0].reshape(np.shape(b))


def residual(F, rho, d, remove_mean=True):
    rho = np.asarray(rho)
    mean = rho.mean() if remove_mean else rho.dtype.type(0)
    return div(F, d) - (rho - mean), mean


def clean(F, rho, d, backward=False, remove_mean=True, fold=True, sign=-1.0, dtype=np.float64):
    F, rho = np.asarray(F, dtype=dtype), np.asarray(rho, dtype=dtype)
    n = (F.shape[2], F.shape[1], F.shape[0])
    res, mean = residual(F, rho, d, remove_mean)
    L = laplacian_dense(n, d, fold)
    phi = solve_meanfree(L, res).astype(dtype)
    if dtype != np.float64:
        Lx = L.astype(dtype)  # (its entries are sums of 1 / d^2 in float64: the same matrix in both precisions)
        for _ in range(4):
            r = res.ravel() - Lx @ phi.ravel()
            phi = phi + solve_meanfree(L, (r - r.mean()).astype(np.float64).reshape(res.shape)).astype(dtype)
        phi = phi - phi.mean()
    return F + dtype(sign) * grad(phi, d, backward), phi, res, mean


def lambda_min(n, d):
    return min(4.0 * np.sin(np.pi / n[c]) ** 2 / d[c] ** 2 for c in range(3) if n[c] >= 2)
