"""Plain numpy restatement of the direct Poisson solve (include/xpic_poisson.h, xpic_amd/csrc/poisson.hip),
written from the header's formula with neither the oracle nor the library.

Scalars are [nz][ny][nx]; n = (nx, ny, nz), d = (dx, dy, dz).

    hartley(n)               H_n[k][j] = (cos(2 pi k j / n) + sin(2 pi k j / n)) / sqrt(n), in np.longdouble with k j reduced
                             modulo n in integers, rounded to float64 (minus=True: cos - sin, a planted bug)
    lam(n, d)                -4 sin^2(pi k / n) / d^2 (fold=False: the planted bug, the off-diagonal weight of an extent of
                             2 taken once: -2 sin^2(pi k / 2) / d^2)
    transform(f, tables)     Hz Hy Hx f, one axis after the other; tables = (Hx, Hy, Hz); back=True: Hx Hy Hz f, the order
                             of the library's three passes back
    apply(rhs, n, d)         one application: the mean-free phi with D G phi = rhs - mean(rhs).  mutate: "no_fold",
                             "keep_zero_mode" (the zero mode divided by the smallest |eigenvalue| instead of zeroed),
                             "minus_x" (cos - sin on the x axis of the forward transform only: in both directions it is
                             the same solve, H with k -> -k), "swap_xy" (the tables of x and y exchanged), "lam_high"
                             (lam[k] *= 1 + 1e-9 on the longest axis for the upper half of the wavenumbers,
                             min(k, n - k) >= n / 4: index k = n - 1 of a Hartley table is wavenumber 1, so the upper half
                             of the indices would hold the lowest mode too)
    solve(res, n, d, tol)    the refinement of gauss.hip's direct path -> (phi, applications, |r|_2).  mutate:
                             "store_second" (the second application overwrites phi instead of adding to it: the += epilogue
                             storing), or one of apply's
    gpu_inputs()             the right-hand sides tests/test_gpu_poisson.py gives xpic_poisson_apply: name -> (n, d, rhs)
    gpu_inputs(MORE)         those of the row-tile, block and extent-1024 shapes (seeds 5000 + i)
    refine_inputs()          those of REFINE: MORE's, and seed 5100 for 17x9x7

dtype=np.longdouble (hartley, lam, apply, lap, solve): the tables are kept in long double, not rounded to float64, and all of
the arithmetic is long double -- the high-precision side of the measurements behind the device tests' constants.
"""
import functools

import numpy as np

import gauss_ref as G

EPS = G.EPS

# the shapes of the device tests: the three small ones, each axis in turn on a tile edge with the others tiny, a general one
SMALL = {"2x3x5": ((2, 3, 5), (0.25, 0.5, 0.125)), "5x4x3": ((5, 4, 3), (0.5, 1.0, 0.25)), "6x7x9": ((6, 7, 9), (0.3, 0.45, 0.7))}
EDGES = {}
for _e in (15, 16, 17, 33):
    EDGES["%dx3x2" % _e] = ((_e, 3, 2), (0.5, 0.25, 1.0))
    EDGES["2x%dx3" % _e] = ((2, _e, 3), (0.25, 0.5, 0.125))
    EDGES["3x2x%d" % _e] = ((3, 2, _e), (1.0, 0.5, 0.25))
GENERAL = {"18x17x20": ((18, 17, 20), (0.3, 0.45, 0.7))}
SHAPES = dict(SMALL, **EDGES, **GENERAL)
# y and z in turn -- the axes along which the table is the kernel's left operand and the extent its count of rows -- on both
# sides of the 64-row tile and at two tiles and one row; every pass with two tiles in m and c and five in k, 67 products
# along y; the largest extent the library takes, on each axis
ROWS = {}
for _e in (63, 64, 65):
    ROWS["3x%dx2" % _e] = ((3, _e, 2), (0.5, 0.25, 1.0))
    ROWS["2x3x%d" % _e] = ((2, 3, _e), (0.25, 0.5, 0.125))
ROWS["2x129x3"] = ((2, 129, 3), (0.25, 0.5, 0.125))
ROWS["3x2x129"] = ((3, 2, 129), (1.0, 0.5, 0.25))
BLOCK = {"66x65x67": ((66, 65, 67), (0.3, 0.45, 0.7))}
LONG = {"1024x6x6": ((1024, 6, 6), (0.5, 0.25, 1.0)), "6x1024x6": ((6, 1024, 6), (0.5, 0.25, 1.0)),
        "6x6x1024": ((6, 6, 1024), (0.5, 0.25, 1.0))}
MORE = dict(ROWS, **BLOCK, **LONG)
# the shapes whose refinement the device tests pin: a small general one (test_gpu_gauss.py's), a ragged row tile along z, the
# block, and the long box on which float64 needs the second application
REFINE = {"17x9x7": ((17, 9, 7), (0.25, 0.125, 0.5)), "2x3x65": ROWS["2x3x65"], "66x65x67": BLOCK["66x65x67"],
          "6x6x1024": LONG["6x6x1024"]}


@functools.lru_cache(maxsize=None)
def _hartley(n, minus, dtype):
    k = np.arange(n, dtype=np.int64)
    kj = (k[:, None] * k[None, :]) % n
    pi = np.arctan(np.longdouble(1)) * 4
    a = 2 * pi * kj.astype(np.longdouble) / np.longdouble(n)
    h = (np.cos(a) - np.sin(a)) if minus else (np.cos(a) + np.sin(a))
    h = (h / np.sqrt(np.longdouble(n))).astype(dtype)
    h.setflags(write=False)
    return h


def hartley(n, minus=False, dtype=np.float64):
    """(read-only: one table per (n, minus, dtype), kept)"""
    return _hartley(int(n), bool(minus), np.dtype(dtype))


def lam(n, d, fold=True, dtype=np.float64):
    pi = np.arctan(np.longdouble(1)) * 4
    s = np.sin(pi * np.arange(n).astype(np.longdouble) / np.longdouble(n))
    w = 2 if (n == 2 and not fold) else 4
    return (-w * s * s / (np.longdouble(d) * np.longdouble(d))).astype(dtype)


def transform(f, tables, back=False):
    """the three passes in the library's order: x, y, z forward and z, y, x back (the same product either way; what
    rounding leaves in |rhs - D G phi| depends on the axis that goes last, by a factor 2.5 at 2x15x3)"""
    for a in ((2, 1, 0) if back else (0, 1, 2)):
        f = np.einsum(("zyj,aj->zya", "zjx,aj->zax", "jyx,aj->ayx")[a], f, tables[a])
    return f


def apply(rhs, n, d, mutate=None, dtype=np.float64):
    rhs = np.asarray(rhs, dtype=dtype)
    tables = [hartley(n[0], dtype=dtype), hartley(n[1], dtype=dtype), hartley(n[2], dtype=dtype)]
    lams = [lam(n[a], d[a], fold=mutate != "no_fold", dtype=dtype) for a in range(3)]
    if mutate == "lam_high":
        a = int(np.argmax(n))
        k = np.arange(n[a])
        lams[a][np.minimum(k, n[a] - k) >= (n[a] + 3) // 4] *= dtype(1) + dtype(1e-9)
    if mutate == "swap_xy":
        # (at unequal extents the wrong table is read as if it had the right shape, as a kernel given the wrong pointer would)
        tables[0], tables[1] = np.resize(tables[1], (n[0], n[0])), np.resize(tables[0], (n[1], n[1]))
        lams[0], lams[1] = np.resize(lams[1], n[0]), np.resize(lams[0], n[1])
    forward = [hartley(n[0], minus=True, dtype=dtype)] + tables[1:] if mutate == "minus_x" else tables
    f = transform(rhs - rhs.mean(), forward)
    den = lams[2][:, None, None] + lams[1][None, :, None] + lams[0][None, None, :]
    zero = den == 0
    out = np.where(zero, dtype(0), f / np.where(zero, dtype(1), den))
    if mutate == "keep_zero_mode":
        out[0, 0, 0] = f[0, 0, 0] / np.abs(den[~zero]).min() + 1.0
    return transform(out, tables, back=True)


def lap(phi, d):
    """D G phi in phi's own dtype"""
    return G.div(G.grad(phi, d), d)


def solve(res, n, d, tol, maxit=10, mutate=None, dtype=np.float64):
    res = np.asarray(res, dtype=dtype)
    phi, r, its = np.zeros_like(res), res.copy(), 0
    rn = float(np.sqrt((r ** 2).sum()))
    inner = None if mutate == "store_second" else mutate
    while its < maxit:
        dphi = apply(r, n, d, mutate=inner, dtype=dtype)
        phi = dphi if (mutate == "store_second" and its == 1) else phi + dphi
        its += 1
        r = res - lap(phi, d)
        rn1 = float(np.sqrt((r ** 2).sum()))
        halved, rn = rn1 <= 0.5 * rn, rn1
        if rn1 <= tol or not halved:
            break
    return phi, its, rn


def gauss_load(name, seed, field, background=True):
    """(E, rho, n, d) of tests/test_gpu_gauss.py's build(X, name, seed, background, field) without the library: the same
    generators in the same order, the sorts' charge by es_ref.deposit (xpic_charge_density's rule; the lattice particles'
    deposit is exact in float64, so this is the device's rho bit for bit)"""
    import es_ref as ES
    import test_gpu_gauss as T

    n, d, nsorts = T.GRIDS[name]
    rng = np.random.default_rng(1000 + seed)
    shape = (n[2], n[1], n[0])
    rho = np.zeros(shape)
    for s in range(nsorts):
        pts = T.lattice_particles(n, d, 10 * seed + s)
        rho = rho + ES.deposit(pts[:, :3], d, n, (-1.0, 1.0)[s % 2] * 1.0 / 4)[0]
    if background:
        rho = rho + rng.normal(0.3, 1.0, shape)
    E = rng.normal(0.0, 2.0, shape + (3,)) if field == "random" else np.zeros(shape + (3,))
    return E, rho, n, d


def gpu_inputs(shapes=None):
    out = {}
    base = 4000 if shapes is None else 5000
    for i, (name, (n, d)) in enumerate((SHAPES if shapes is None else shapes).items()):
        rng = np.random.default_rng(base + i)
        rhs = rng.normal(0.0, 1.0, (n[2], n[1], n[0]))
        out[name] = (n, d, rhs - rhs.mean())
    return out


def refine_inputs():
    more = gpu_inputs(MORE)
    out = {}
    for name, (n, d) in REFINE.items():
        if name in more:
            out[name] = more[name]
        else:
            rhs = np.random.default_rng(5100).normal(0.0, 1.0, (n[2], n[1], n[0]))
            out[name] = (n, d, rhs - rhs.mean())
    return out
