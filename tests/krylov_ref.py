"""Plain numpy / scipy float64 restatement of what the field solve rests on (xpic_amd/csrc/krylov.hip, fields.hip; DESIGN.md
section 4): the grid operators as explicit matrices, a direct solve on them, textbook Krylov methods for the iteration
counts an exact-arithmetic method needs, the forward error bound of a dot product, and the row kernel's share-out of its
workgroups.  Written from the operators' definitions, with neither the oracle nor the library.

Vectors are get_field's arrays [nz][ny][nx][3] flattened: unknown ((z ny + y) nx + x) 3 + c.  Matrices are scipy.sparse
CSR (a few thousand unknowns at the most); direct_solve and cond2 densify them.

    rot_matrix(n, d, forward)       rot+ / rot- from Kronecker products of periodic difference matrices
    matM_matrix(n, d, dt)           precond_ref.dense_matrix of precond_ref.matM_stencil: entry by entry, not as a product
    matL_matrix(matL, n)            a xpic_matL_get dump [node][c1][123] through precond_ref.ldecode
    direct_solve, cond2, true_residual
    gmres(A, b, rtol, atol, maxit)  restarted GMRES(30), MODIFIED Gram-Schmidt, explicit norms, x0 = 0
    cg(A, b, rtol, atol, maxit)     textbook CG, x0 = 0
    dot_bound(x, y)                 n eps sum |x_i y_i|: no summation order is further than this from math.fsum
    row_split, row_grid, row_decode fields.hip's cost rule, block count and decode of blockIdx.x in k_matA
    solve_figures(...)              the figures section c of tests/test_gpu_krylov.py asserts, each beside its bound
"""
import math

import numpy as np
import scipy.sparse as sp

import precond_ref as P

RESTART = 30                      # krylov.hip: kRestart
KROWX, KROWY, KBANDY = 64, 4, 4   # fields.hip: a workgroup's 64 lanes x 4 rows, y-chunks per band
BAND = KBANDY * KROWY             # rows of a y-band
KBLOCK, KREDBLOCKS = 256, 1024    # fields.hip / common.h: threads of a reduction block, cap of the partial sums
RED_CAP = KREDBLOCKS // 3         # red_grid: blocks per component
EPS = float(np.finfo(np.float64).eps)


# ---- the operators as matrices ---------------------------------------------------------------------------------------
def _shift(e, s):
    """(S f)[i] = f[(i + s) mod e]"""
    i = np.arange(e)
    return sp.coo_matrix((np.ones(e), (i, (i + s) % e)), shape=(e, e)).tocsr()


def diff_matrix(n, d, axis, forward):
    """the periodic forward / backward difference along axis (0 = x) on the nodes (z ny + y) nx + x"""
    e = n[axis]
    D = (_shift(e, 1) - sp.identity(e)) if forward else (sp.identity(e) - _shift(e, -1))
    mats = [sp.identity(n[2]), sp.identity(n[1]), sp.identity(n[0])]  # z, y, x
    mats[2 - axis] = D / d[axis]
    return sp.kron(mats[0], sp.kron(mats[1], mats[2])).tocsr()


def rot_matrix(n, d, forward):
    """(rot F)_x = D_y F_z - D_z F_y, (rot F)_y = D_z F_x - D_x F_z, (rot F)_z = D_x F_y - D_y F_x"""
    Dx, Dy, Dz = (diff_matrix(n, d, a, forward) for a in range(3))
    blocks = {(0, 2): Dy, (0, 1): -Dz, (1, 0): Dz, (1, 2): -Dx, (2, 1): Dx, (2, 0): -Dy}
    N = n[0] * n[1] * n[2]
    R = sp.csr_matrix((3 * N, 3 * N))
    for (c1, c2), D in blocks.items():
        E = sp.coo_matrix(([1.0], ([c1], [c2])), shape=(3, 3))
        R = R + sp.kron(D, E)
    return R.tocsr()


def matM_matrix(n, d, dt):
    return sp.csr_matrix(P.dense_matrix(P.matM_stencil(d, dt), n))


def matL_matrix(matL, n):
    """row (c1, node q) holds matL[q][c1][k] in column (c2, node q + d) of (c2, d) = ldecode(c1, k); taps that the
    periodic fold lays onto one column add up"""
    nx, ny, nz = n
    L = np.asarray(matL, dtype=np.float64).reshape(nz, ny, nx, 3, P.LSTENCIL)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    node = (z * ny + y) * nx + x
    rows, cols, vals = [], [], []
    for c1 in range(3):
        for k in range(P.LSTENCIL):
            c2, dd = P.ldecode(c1, k)
            col = (((z + dd[2]) % nz * ny + (y + dd[1]) % ny) * nx + (x + dd[0]) % nx) * 3 + c2
            rows.append((node * 3 + c1).ravel())
            cols.append(col.ravel())
            vals.append(L[..., c1, k].ravel())
    N = 3 * nx * ny * nz
    return sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(N, N)).tocsr()


def apply(A, F):
    return np.asarray(A @ F.ravel()).reshape(F.shape)


def _dense(A):
    return A.toarray() if sp.issparse(A) else np.asarray(A)


def direct_solve(A, b):
    return np.linalg.solve(_dense(A), np.asarray(b, dtype=np.float64).ravel()).reshape(np.shape(b))


def cond2(A):
    return float(np.linalg.cond(_dense(A), 2))


def true_residual(A, x, b):
    return float(np.linalg.norm(np.ravel(b) - A @ np.ravel(x)))


# ---- textbook Krylov methods: they only say how many iterations exact arithmetic needs -------------------------------------
def gmres(A, b, rtol, atol, maxit, restart=RESTART):
    """-> (x, iterations, [|r| of the recurrence after every iteration]).  Modified Gram-Schmidt, every norm explicit,
    the restart residual b - A x; stops on |r| <= max(rtol |b|, atol)"""
    b = np.asarray(b, dtype=np.float64).ravel()
    x = np.zeros_like(b)
    tol = max(rtol * np.linalg.norm(b), atol)
    r, hist, its = b.copy(), [], 0
    rnorm = np.linalg.norm(r)
    while rnorm > tol and its < maxit:
        V = [r / rnorm]
        H = np.zeros((restart + 1, restart))
        g = np.zeros(restart + 1)
        g[0] = rnorm
        cs, sn = np.zeros(restart), np.zeros(restart)
        j = 0
        while j < restart and its < maxit:
            w = A @ V[j]
            for i in range(j + 1):
                H[i, j] = w @ V[i]
                w = w - H[i, j] * V[i]
            H[j + 1, j] = np.linalg.norm(w)
            V.append(w / H[j + 1, j] if H[j + 1, j] != 0.0 else w)
            for i in range(j):
                H[i, j], H[i + 1, j] = cs[i] * H[i, j] + sn[i] * H[i + 1, j], -sn[i] * H[i, j] + cs[i] * H[i + 1, j]
            den = math.hypot(H[j, j], H[j + 1, j])
            cs[j], sn[j] = (H[j, j] / den, H[j + 1, j] / den) if den != 0.0 else (1.0, 0.0)
            H[j, j] = den
            g[j + 1], g[j] = -sn[j] * g[j], cs[j] * g[j]
            its, j = its + 1, j + 1
            rnorm = abs(g[j])
            hist.append(rnorm)
            if rnorm <= tol:
                break
        y = np.linalg.solve(np.triu(H[:j, :j]), g[:j])
        x = x + np.column_stack(V[:j]) @ y
        r = b - A @ x
        rnorm = np.linalg.norm(r)
    return x, its, hist


def cg(A, b, rtol, atol, maxit):
    """-> (x, iterations, [|r| of the recurrence after every iteration])"""
    b = np.asarray(b, dtype=np.float64).ravel()
    x, r, p = np.zeros_like(b), b.copy(), b.copy()
    rr = r @ r
    tol = max(rtol * math.sqrt(rr), atol)
    its, hist = 0, []
    while math.sqrt(rr) > tol and its < maxit:
        Ap = A @ p
        alpha = rr / (p @ Ap)
        x = x + alpha * p
        r = r - alpha * Ap
        rr1 = r @ r
        p = r + (rr1 / rr) * p
        rr = rr1
        its += 1
        hist.append(math.sqrt(rr))
    return x, its, hist


# ---- reductions -------------------------------------------------------------------------------------------------------
def dot_exact(x, y):
    """sum x_i y_i with the sum exact (math.fsum); the products are rounded once, which dot_bound's margin covers"""
    return math.fsum((np.ravel(x) * np.ravel(y)).tolist())


def dot_bound(x, y):
    """n eps sum |x_i y_i|: the forward error of a recursive sum of n terms in ANY order is below (n - 1) u sum |terms|
    (Higham, Accuracy and Stability, 4.2), a product rounded or contracted into the sum adds one u per term, and
    eps = 2 u leaves the factor two for the second-order terms"""
    x, y = np.ravel(x), np.ravel(y)
    return x.size * EPS * math.fsum(np.abs(x * y).tolist())


def red_blocks(nown):
    """fields.hip: red_grid's blocks per component"""
    return max(1, min(-(-nown // (KBLOCK * 4)), RED_CAP))


# ---- k_matA's share-out of the rows over the 8 XCDs ---------------------------------------------------------------------
def _bands(ny):
    nyc = -(-ny // KROWY)
    return nyc, -(-nyc // KBANDY)


def row_split(ny, nzr):
    """fields.hip: row_split.  zsplit runs of planes x 8 / zsplit groups of y-bands; the smallest largest share, ties to
    the larger zsplit"""
    _, nyt = _bands(ny)
    best, cost = 8, -1
    for zs in (8, 4, 2, 1):
        load = -(-nzr // zs) * -(-nyt // (8 // zs))
        if cost < 0 or load < cost:
            cost, best = load, zs
    return best


def row_grid(n, nzr, zsplit):
    """fields.hip: row_grid's number of workgroups"""
    nxc = -(-n[0] // KROWX)
    _, nyt = _bands(n[1])
    Pz, Pb = -(-nzr // zsplit), -(-nyt // (8 // zsplit))
    return 8 * Pb * Pz * KBANDY * nxc * 3


def row_decode(block, n, nzr, zsplit, plant=None):
    """k_matA: blockIdx.x -> (xcd, ytl, zr, c1, x0, y0), or None where the workgroup returns.  plant "Pb": the y-band of
    an XCD's group found with the number of bands in the place of the bands per group"""
    nxc = -(-n[0] // KROWX)
    _, nyt = _bands(n[1])
    ysplit = 8 // zsplit
    Pz, Pb = -(-nzr // zsplit), -(-nyt // ysplit)
    per_z = KBANDY * nxc * 3
    per_band = Pz * per_z
    xcd, q = block % 8, block // 8
    ytl = q // per_band
    yt = (xcd // zsplit) * (nyt if plant == "Pb" else Pb) + ytl
    rem = q % per_band
    zr = (xcd % zsplit) * Pz + rem // per_z
    rem2 = rem % per_z
    c1 = rem2 % 3
    x0 = ((rem2 // 3) % nxc) * KROWX
    y0 = (yt * KBANDY + rem2 // (3 * nxc)) * KROWY
    if ytl >= Pb or yt >= nyt or zr >= nzr:
        return None
    return xcd, ytl, zr, c1, x0, y0


def row_cover(n, nzr, plant=None):
    """how often the launch of row_grid(n, nzr, row_split) workgroups produces each (c1, x-chunk, y-row-group, z);
    workgroups whose rows all lie beyond the grid's edge (y0 >= ny) produce nothing"""
    zs = row_split(n[1], nzr)
    nxc, (nyc, _) = -(-n[0] // KROWX), _bands(n[1])
    count = np.zeros((3, nxc, nyc, nzr), dtype=np.int64)
    for blk in range(row_grid(n, nzr, zs)):
        t = row_decode(blk, n, nzr, zs, plant)
        if t is not None and t[5] < n[1]:
            count[t[3], t[4] // KROWX, t[5] // KROWY, t[2]] += 1
    return count


# ---- the shapes of the operator tests: (n, zsplit of the whole box, what the shape reaches) -----------------------------
SHAPES = {
    "2x2x2": ((2, 2, 2), 8, "every +-1 and +-2 neighbour is the node or its one neighbour"),
    "2x3x5": ((2, 3, 5), 8, "smallest mixed extents"),
    "5x2x3": ((5, 2, 3), 8, "smallest mixed extents"),
    "65x5x4": ((KROWX + 1, 5, 4), 8, "one full chunk and one lane"),
    "two-bands": ((3, 2 * BAND, 4), 4, "two y-bands, 4 planes"),
    "three-bands": ((3, 2 * BAND + 3, 4), 4, "three y-bands, the last short; a tie with 2 that the loop order keeps"),
    "eight-bands": ((2, 8 * BAND, 2), 2, "eight y-bands, 2 planes"),
    "band-edge": ((3, BAND + 1, 4), 4, "one row past a band: y-rows beyond the grid's edge"),
}


# ---- what a solve is held to (tests/test_gpu_krylov.py, section c; tests/test_krylov_ref.py plants bugs against it) ----
def solve_figures(A, b, x, its, rnorm, rtol, atol, xstar, kappa, its_ref=None, explicit=False):
    """{name: (figure, bound)} of one converged solve; every figure must be <= its bound.
    residual: |b - A x| by the explicit matrix against 1.05 max(rtol |b|, atol) (the margin the solver tests give the
    recurrence); rnorm: the reported norm against the true one, 1e-8 |b| for one-reduction Gram-Schmidt
    (test_preconditioner_with_the_mean_mass_matrix), 0.2 rnorm + 1e-14 where every norm is explicit
    (test_preconditioned_solve); error: |x - x*| against 2 cond2(A) tol / |b| |x*|; iterations: against the restated
    method's count, +- 1"""
    bn = float(np.linalg.norm(b))
    tol = max(rtol * bn, atol)
    res = true_residual(A, x, b)
    out = {"residual": (res, 1.05 * tol),
           "rnorm": (abs(rnorm - res), 0.2 * rnorm + 1e-14 if explicit else 1e-8 * bn),
           "error": (float(np.linalg.norm(np.ravel(x) - np.ravel(xstar))), 2.0 * kappa * tol / bn * float(np.linalg.norm(xstar)))}
    if its_ref is not None:
        out["iterations"] = (abs(its - its_ref), 1)
    return out


def failed(figures):
    return sorted(k for k, (v, bound) in figures.items() if not v <= bound)


# ---- the loads of the tests (shared by the CPU and the GPU file; the seeds are part of the tests) ------------------------
B0 = (0.3, -0.2, 0.9)
D_GENERAL, DT = (0.5, 0.4, 0.25), 0.7
RESTART_DT = 1.5  # the restart case (tests/test_gpu_krylov.py: test_solve_across_two_restarts has the count it gives)
# name: (n, d, dt, seed, B0) of the contexts the solves run on
SOLVE_CASES = {"6x5x4": ((6, 5, 4), D_GENERAL, DT, 300, B0), "8x8x6": ((8, 8, 6), D_GENERAL, DT, 301, B0),
               "restart": ((8, 8, 6), (0.25, 0.25, 0.25), RESTART_DT, 302, B0),
               "nonsymmetric": ((6, 5, 4), D_GENERAL, 1.0, 303, (0.5, -1.0, 2.0))}


def build_load(n, d, seed, ppc=3, B0=B0):
    """([(sort parameters, points6)] of two species of opposite charge with ppc particles per cell each, B, and two
    random fields [nz][ny][nx][3]) from the seed alone"""
    rng = np.random.default_rng(seed)
    N = n[0] * n[1] * n[2]
    L = np.array(n) * np.array(d)
    sorts = []
    for par in ((ppc, 1.0, -1.0, 1.0), (ppc, 1.0, 1.0, 100.0)):
        pts = np.empty((ppc * N, 6))
        pts[:, :3] = rng.random((ppc * N, 3)) * L
        pts[:, 3:] = rng.normal(0, 0.05, (ppc * N, 3))
        sorts.append((par, pts))
    shape = (n[2], n[1], n[0], 3)
    B = rng.normal(0, 0.02, shape) + np.array(B0)
    return sorts, B, rng.normal(0, 1.0, shape), rng.normal(0, 1.0, shape)
