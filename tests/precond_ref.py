"""Plain numpy float64 restatement of the Krylov preconditioners (xpic_amd/csrc/precond.hip, fields.hip: cheb_matM_inverse;
DESIGN.md, the preconditioner section), written from the kernels' code and not by calling the library.

Field vectors are arrays [nz][ny][nx][3] (xpic_field_get's layout); the assembled mass matrix is xpic_matL_get's
[node][c1][123] reshaped to [nz][ny][nx][3][123].  Every stencil is applied periodically with np.roll, so extents of 2 or 3
alias taps onto each other as the grid does.

    Surrogate(matL, n, d, dt, kind, lscale)   <matL> over the sampled rows, tap folding, matM's stencil, bounds, flags, degree
    cheb_abar(sur, r, degree, dtype)          P r of kinds 3 - 5
    cheb_matM(r, n, d, dt, degree, kind, dtype)   P r of kinds 1, 2

dtype = np.float32 repeats a recurrence with the device's number formats (coefficients rounded as the packed table is,
fp32 sums in the kernel's tap order; kind 1: fp64 arithmetic on fp32-stored vectors).  It only sizes tolerances: the
distance between the two restatements is what rounding alone does to P r.

The test loads (CASES, build_case) are shared by tests/test_precond_ref.py (CPU: the oracle's matL) and
tests/test_gpu_precond.py (device: the library's matL); their seeds are part of the tests.
"""
import math

import numpy as np

LSTENCIL = 123
KTX, KTY, KH, MIN_ZC = 128, 4, 2, 8  # k_cheb_bar: tile of 128 x 4 nodes, halo 2, z-chunks of at least 8 planes
AUTO_SPREAD = 0.2                    # kind 5 scales its rows where the relative spread of matL's diagonal is above this


# ---- lstencil.h -----------------------------------------------------------------------------------------------------
def lrange(c1, c2):
    lo, n = [-1, -1, -1], [3, 3, 3]
    if c1 != c2:
        lo[c1], n[c1] = -1, 4
        lo[c2], n[c2] = -2, 4
    return lo, n


def lblock_offset(c1, c2):
    return sum(27 if c == c1 else 48 for c in range(c2))


def lencode(c1, c2, d):
    lo, n = lrange(c1, c2)
    i = [d[a] - lo[a] for a in range(3)]
    if any(i[a] < 0 or i[a] >= n[a] for a in range(3)):
        return -1
    return lblock_offset(c1, c2) + (i[2] * n[1] + i[1]) * n[0] + i[0]


def ldecode(c1, k):
    for c2 in range(3):
        sz = 27 if c2 == c1 else 48
        if k < sz:
            lo, n = lrange(c1, c2)
            return c2, (lo[0] + k % n[0], lo[1] + (k // n[0]) % n[1], lo[2] + (k // n[0]) // n[1])
        k -= sz
    raise ValueError(k)


def tap_kept(c1, c2, d):
    """precond.hip: of a block between different components the polynomial keeps the 12 taps without a 1/48 overlap"""
    return c1 == c2 or (d[c1] in (0, 1) and d[c2] in (0, -1))


# TAPS[c1][k] = (c2, d, kept); ORDER: the kernel's order of accumulation (lines (c2, dz, dy), then dx, then c1)
TAPS = [[ldecode(c1, k) + (tap_kept(c1, *ldecode(c1, k)),) for k in range(LSTENCIL)] for c1 in range(3)]
ORDER = [(c2, (dx, dy, dz), [(c1, lencode(c1, c2, (dx, dy, dz))) for c1 in range(3) if lencode(c1, c2, (dx, dy, dz)) >= 0])
         for c2 in range(3) for dz in range(-2, 3) for dy in range(-2, 3) for dx in range(-2, 3)]
ORDER = [t for t in ORDER if t[2]]
KDIAG = [lencode(c, c, (0, 0, 0)) for c in range(3)]


# ---- matM = 2 I + 0.5 dt^2 rot- rot+ (fields.hip: rot_at / matM_at) ----------------------------------------------------
def _diff(f, axis, h, forward):
    # axis: 0 = x, 1 = y, 2 = z of an array [z][y][x]
    ax = 2 - axis
    return (np.roll(f, -1, ax) - f) / h if forward else (f - np.roll(f, 1, ax)) / h


def rot(F, d, forward):
    Dx, Dy, Dz = (lambda f, a=a: _diff(f, a, d[a], forward) for a in range(3))
    out = np.empty_like(F)
    out[..., 0] = Dy(F[..., 2]) - Dz(F[..., 1])
    out[..., 1] = -Dx(F[..., 2]) + Dz(F[..., 0])
    out[..., 2] = Dx(F[..., 1]) - Dy(F[..., 0])
    return out


def matM(F, d, dt):
    return 2.0 * F + (0.5 * dt * dt) * rot(rot(F, d, True), d, False)


def matM_stencil(d, dt):
    """matM's coefficients in the 123-pattern [3][123]: unit impulses on a 5^3 box (no aliasing: matM reaches one node)"""
    co = np.zeros((3, LSTENCIL))
    for c2 in range(3):
        F = np.zeros((5, 5, 5, 3))
        F[2, 2, 2, c2] = 1.0
        H = matM(F, d, dt)
        for c1 in range(3):
            for k in range(LSTENCIL):
                e2, dd, _ = TAPS[c1][k]
                if e2 == c2:  # row (c1, node q) couples to column (c2, node p = q + d)
                    co[c1, k] = H[2 - dd[2], 2 - dd[1], 2 - dd[0], c1]
    return co


def matM_interval(d, dt):
    return 2.0, 2.0 + 2.0 * dt * dt * sum(1.0 / (h * h) for h in d)


def matM_degrees(d, dt):
    """api.hip (xpic_create): the automatic degrees of the polynomial in matM, for the predict and for the correct solve"""
    kappa = 1.0 + dt * dt * sum(1.0 / (h * h) for h in d)
    rho = (math.sqrt(kappa) - 1.0) / (math.sqrt(kappa) + 1.0)
    k = math.ceil(math.log(0.04) / math.log(rho)) if rho > 0 else 2
    kM = math.ceil(math.log(0.00125) / math.log(rho)) if rho > 0 else 2
    return min(max(k, 2), 32), min(max(kM, 2), 48)


# ---- the surrogate Abar = matM + <matL> -----------------------------------------------------------------------------
def sample_stride(extent):
    return 8 if extent >= 64 else (4 if extent >= 16 else 1)


class Surrogate:
    """abar_update.  kind: 3 plain, 4 rows scaled by the local density, 5 chooses; lscale: the debug surrogate scale."""

    def __init__(self, matL, n, d, dt, kind, lscale=1.0, degree_user=0):
        nx, ny, nz = n
        self.n, self.d, self.dt, self.kind = tuple(n), tuple(d), dt, kind
        L = np.asarray(matL, dtype=np.float64).reshape(nz, ny, nx, 3, LSTENCIL)
        rows = L[::sample_stride(nz), ::sample_stride(ny)]  # k_lbar_rows: phase 0, every node of a sampled row
        self.mean = rows.mean(axis=(0, 1, 2))               # [3][123]
        dg = np.stack([rows[..., c, KDIAG[c]] for c in range(3)], axis=-1)
        self.d2 = (dg * dg).mean(axis=(0, 1, 2)) if kind == 5 else np.zeros(3)  # (only kind 5 sums the second moment)
        self.mco = matM_stencil(d, dt)
        lbar = self.mean * lscale
        self.abar = np.zeros((3, LSTENCIL + 1))
        self.abar[:, :LSTENCIL] = self.mco + lbar
        self.abar[:, LSTENCIL] = self.d2
        # k_abar: the kept taps of a block share the sum of its dropped ones in proportion
        self.lkept = np.zeros((3, LSTENCIL))
        for c1 in range(3):
            for c2 in range(3):
                ks = [k for k in range(LSTENCIL) if TAPS[c1][k][0] == c2]
                kept = [k for k in ks if TAPS[c1][k][2]]
                keep = 1.0
                if c1 != c2:
                    s_all, s_kept = self.mean[c1, ks].sum(), self.mean[c1, kept].sum()
                    if s_kept != 0.0 and abs(s_all) <= 4.0 * abs(s_kept):
                        keep = s_all / s_kept
                self.lkept[c1, kept] = keep * lbar[c1, kept]
        self.ckept = self.mco + self.lkept  # the packed table (matM has no dropped tap)
        # k_abar_bounds on the full pattern (Lbar read back as abar - matM, as the kernels read it)
        back = self.abar[:, :LSTENCIL] - self.mco
        sa = np.abs(back).sum(axis=1)
        diag = np.array([back[c, KDIAG[c]] for c in range(3)])
        self.rowsum, self.diag = sa, diag
        self.gersh = diag - (sa - np.abs(diag))
        with np.errstate(divide="ignore", invalid="ignore"):
            self.spread = np.where(diag > 0.0, self.d2 / (diag * diag) - 1.0, 0.0)
        cv2 = self.spread.max()
        self.scaled = kind == 4 or (kind == 5 and bool(np.isfinite(cv2)) and cv2 > AUTO_SPREAD * AUTO_SPREAD)
        # k_rscale: the row's own diagonal over the average's
        own = np.stack([L[..., c, KDIAG[c]] for c in range(3)], axis=-1)  # [nz][ny][nx][3]
        inv = np.where(diag > 0.0, 1.0 / np.where(diag > 0.0, diag, 1.0), 0.0)
        self.rscale = np.where(diag > 0.0, own * inv, 1.0)
        self.rscale32 = self.rscale.astype(np.float32)
        self.rmax = max(1.0, float(self.rscale32.max())) if self.scaled else 1.0
        rs, gl = sa.max(), self.gersh.min()
        self.lo, self.hi = 2.0, matM_interval(d, dt)[1] + self.rmax * rs
        self.gershgorin = 2.0 + gl
        self.valid = bool(np.isfinite(rs) and np.isfinite(self.rmax) and np.isfinite(gl))
        self.proven = self.valid and 2.0 + self.rmax * min(gl, 0.0) > 0.0 and lscale == 1.0
        self.degree = self.auto_degree(degree_user)

    def auto_degree(self, degree_user=0):
        """cheb_abar_degree: error bound 2 rho^k / (1 + rho^2k) of 2.5 % (0.25 % for the scaled rows)"""
        sk = math.sqrt(self.hi / self.lo)
        rh = (sk - 1.0) / (sk + 1.0)
        k = min(degree_user, 64) if degree_user > 0 else math.ceil(math.log(0.00125 if self.scaled else 0.0125) / math.log(rh))
        return min(max(k, 2), 64)


def first_chunk_boundary(n):
    """the first plane of the second z-chunk of k_cheb_bar at a test-sized box (chunks of MIN_ZC planes), or None"""
    return MIN_ZC if n[2] > MIN_ZC else None


def stencil_apply(co, z, n, mutate=None):
    """sum_k co[c1][k] z[c2(k)][node + d(k)], periodic; sums in the kernel's tap order and in z's dtype.
    mutate: "halo" -- the last x tile reads zero where its halo crosses the periodic edge; "plane" -- the window holds
    plane z - 1 in the place of plane z at the first z-chunk boundary"""
    nx = n[0]
    src = z
    if mutate == "plane":
        zb = first_chunk_boundary(n)
        src = z.copy()
        src[zb] = z[zb - 1]
    xs = np.arange(nx)
    last0 = ((nx + KTX - 1) // KTX - 1) * KTX
    out = np.zeros_like(z)
    for c2, dd, rows in ORDER:
        rows = [(c1, k) for c1, k in rows if co[c1, k] != 0.0]
        if not rows:
            continue
        v = np.roll(src[..., c2], (-dd[2], -dd[1], -dd[0]), axis=(0, 1, 2))
        if mutate == "halo" and dd[0] != 0:
            lost = (xs >= last0) & ((xs + dd[0] < 0) | (xs + dd[0] >= nx))
            v = np.where(lost, z.dtype.type(0), v)
        for c1, k in rows:
            out[..., c1] += co[c1, k] * v
    return out


def abar_apply(sur, z, mutate=None):
    """(matM + Lbar) z, or with scaled rows matM z + r o (Lbar z), on the kept taps"""
    F = z.dtype.type
    if not sur.scaled:
        return stencil_apply(sur.ckept.astype(F), z, sur.n, mutate)
    if F is np.float32:  # the kernel: both sums in fp32, (Lbar z) as their difference
        rs = sur.rscale32
        if mutate == "ratio":
            rs = np.roll(rs, -1, axis=2)
        acc = stencil_apply(sur.ckept.astype(F), z, sur.n, mutate)
        accM = stencil_apply(sur.mco.astype(F), z, sur.n, mutate)
        return accM + rs * (acc - accM)
    rs = sur.rscale
    if mutate == "ratio":  # the density ratio of the neighbouring node
        rs = np.roll(rs, -1, axis=2)
    return stencil_apply(sur.mco, z, sur.n, mutate) + rs * stencil_apply(sur.lkept, z, sur.n, mutate)


def cheb_coefficients(lo, hi, degree):
    """(theta, [(cd, cr)] of the degree - 1 steps) of the Chebyshev iteration on [lo, hi]"""
    theta, delta = 0.5 * (hi + lo), 0.5 * (hi - lo)
    sigma1 = theta / delta
    rho, steps = 1.0 / sigma1, []
    for _ in range(1, degree):
        rho_new = 1.0 / (2.0 * sigma1 - rho)
        steps.append((rho_new * rho, 2.0 * rho_new / delta))
        rho = rho_new
    return theta, steps


def cheb_abar(sur, r, degree=None, dtype=np.float64, mutate=None, apply=None):
    """cheb_abar_inverse: z_0 = d_0 = r / theta, then degree - 1 steps d = cd d + cr (r - Abar z), z += d"""
    F = np.dtype(dtype).type
    degree = sur.degree if degree is None else degree
    theta, steps = cheb_coefficients(sur.lo, sur.hi, degree)
    A = apply or (lambda v: abar_apply(sur, v, mutate))
    it = F(1.0 / theta)
    rv = np.asarray(r, dtype=np.float64).astype(F)
    z = rv * it
    d = z
    for i, (cd, cr) in enumerate(steps):
        m = A(rv) * it if i == 0 else A(z)  # first step: Abar z_0 = (Abar r) / theta
        d = F(cd) * d + F(cr) * (rv - m)
        z = z + d
    return z.astype(np.float64)


def cheb_matM(r, d, dt, degree, kind=2, dtype=np.float64):
    """cheb_matM_inverse.  kind 2: fp64.  kind 1 with dtype float32: fp64 arithmetic, the vectors r, d, z stored in fp32
    between the steps (k_cheb32); the last step's result is not rounded"""
    lo, hi = matM_interval(d, dt)
    theta, steps = cheb_coefficients(lo, hi, degree)
    r = np.asarray(r, dtype=np.float64)
    if degree <= 1:
        return r / theta
    narrow = kind != 2 and np.dtype(dtype) == np.float32
    store = (lambda a: a.astype(np.float32).astype(np.float64)) if narrow else (lambda a: a)
    it = 1.0 / theta
    rv, z, dv = r, None, None
    for i, (cd, cr) in enumerate(steps):
        first, last = i == 0, i == len(steps) - 1
        if first:
            z0 = rv * it
            dn = cd * z0 + cr * (rv - matM(rv, d, dt) * it)
            if not last:
                rv = store(rv)
        else:
            z0 = z
            dn = cd * dv + cr * (rv - matM(z, d, dt))
        if last:
            return z0 + dn
        dv, z = store(dn), store(z0 + dn)
    raise AssertionError


def dense_matrix(co, n, rscale=None, mco=None):
    """the dense periodic matrix of a constant stencil [3][123] on the box n (rows and columns ((z ny + y) nx + x) 3 + c);
    with rscale: matM + diag(r) L, co being L's stencil and mco matM's.  Built entry by entry, not through stencil_apply."""
    nx, ny, nz = n
    N = nx * ny * nz * 3
    A = np.zeros((N, N))
    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                for c1 in range(3):
                    row = ((z * ny + y) * nx + x) * 3 + c1
                    w = 1.0 if rscale is None else rscale[z, y, x, c1]
                    for k in range(LSTENCIL):
                        c2, dd, _ = TAPS[c1][k]
                        col = (((z + dd[2]) % nz * ny + (y + dd[1]) % ny) * nx + (x + dd[0]) % nx) * 3 + c2
                        A[row, col] += w * co[c1, k]
                        if mco is not None:
                            A[row, col] += mco[c1, k]
    return A


# ---- the loads of the tests ------------------------------------------------------------------------------------------
D_GENERAL, D_POW2, DT, B0 = (0.5, 0.4, 0.25), (0.5, 0.5, 0.25), 0.7, (0.3, -0.2, 0.9)
# name: (n, d, load, seed).  "two": two species of opposite charge, 8 per cell each; "dense": one species, 64 per cell;
# "ramp": one species, 48 per cell on average, density falling 6 : 1 along x
CASES = {
    "12x10x8": ((12, 10, 8), D_GENERAL, "two", 101),      # one tile wrapping onto itself, even nx
    "12x10x8-pow2": ((12, 10, 8), D_POW2, "two", 102),    # matL from the power-of-two spacing bodies of the assembly
    "12x10x8-dense": ((12, 10, 8), D_GENERAL, "dense", 103),  # kind 5 keeps the plain rows
    "16x10x8-ramp": ((16, 10, 8), D_GENERAL, "ramp", 104),    # kind 5 scales its rows
    "13x5x9": ((13, 5, 9), D_GENERAL, "two", 105),        # odd nx, a ragged y tile, chunks of 8 + 1 planes
    "130x6x17": ((130, 6, 17), D_GENERAL, "two", 106),    # second x tile two nodes wide, halo across the edge, chunks 8 + 8 + 1
    "131x3x5": ((131, 3, 5), D_GENERAL, "two", 107),      # odd nx over two tiles, ny below a tile, one short chunk
    "2x2x32": ((2, 2, 32), D_GENERAL, "two", 108),        # aliased taps: the reference's default geometry
    "3x2x5": ((3, 2, 5), D_GENERAL, "two", 109),          # aliased taps, odd
    "12x16x16": ((12, 16, 16), D_GENERAL, "two", 110),    # rows sampled at stride 4
    "4x64x16": ((4, 64, 16), D_GENERAL, "two", 111),      # rows sampled at strides 8 and 4
    "12x10x16": ((12, 10, 16), D_GENERAL, "two", 112),    # the box the z-slab case cuts in two
}
SORTS = {"two": [(8, 1.0, -1.0, 1.0), (8, 1.0, 1.0, 100.0)], "dense": [(64, 1.0, -1.0, 1.0)], "ramp": [(48, 1.0, -1.0, 1.0)]}


def build_case(name):
    """(n, d, dt, [(sort parameters, points6)], B[nz][ny][nx][3], r[nz][ny][nx][3]) of a case, from its seed alone"""
    n, d, load, seed = CASES[name]
    rng = np.random.default_rng(seed)
    N = n[0] * n[1] * n[2]
    L = np.array(n) * np.array(d)
    sorts = []
    for par in SORTS[load]:
        npart = par[0] * N
        pts = np.empty((npart, 6))
        pts[:, :3] = rng.random((npart, 3)) * L
        if load == "ramp":  # density ~ 6 - 5 x / Lx
            pts[:, 0] = (6.0 - np.sqrt(36.0 - 35.0 * rng.random(npart))) / 5.0 * L[0] * 0.999999
        pts[:, 3:] = rng.normal(0, 0.05, (npart, 3))
        sorts.append((par, pts))
    shape = (n[2], n[1], n[0], 3)
    B = rng.normal(0, 0.02, shape) + np.array(B0)
    r = rng.normal(0, 1.0, shape)
    return n, d, DT, sorts, B, r


def tolerance(ref64, ref32):
    """of a device result in fp32 against the fp64 restatement: four times what rounding does to the restatement itself (the
    factor covers the other summation order of up to 123 taps and FMA contraction), and never below the fp64 bound of
    1e-12 of the largest entry (a polynomial of degree 2 in matM runs without a single fp32 store)"""
    return max(4.0 * np.abs(ref32 - ref64).max(), 1e-12 * np.abs(ref64).max())
