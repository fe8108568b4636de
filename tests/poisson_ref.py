"""Plain numpy restatement of the direct Poisson solve (include/xpic_poisson.h, xpic_amd/csrc/poisson.hip),
written from the header's formula with neither the oracle nor the library.

Scalars are [nz][ny][nx]; n = (nx, ny, nz), d = (dx, dy, dz).

    hartley(n)               H_n[k][j] = (cos(2 pi k j / n) + sin(2 pi k j / n)) / sqrt(n), in np.longdouble with k j reduced
                             modulo n in integers, rounded to float64 (minus=True: cos - sin, a planted bug)
    lam(n, d)                -4 sin^2(pi k / n) / d^2 (fold=False: the planted bug, the off-diagonal weight of an extent of
                             2 taken once: -2 sin^2(pi k / 2) / d^2)
    transform(f, tables)     Hz Hy Hx f, one axis after the other; tables = (Hx, Hy, Hz)
    apply(rhs, n, d)         one application: the mean-free phi with D G phi = rhs - mean(rhs).  mutate: "no_fold",
                             "keep_zero_mode" (the zero mode divided by the smallest |eigenvalue| instead of zeroed),
                             "minus_x" (cos - sin on the x axis of the forward transform only: in both directions it is
                             the same solve, H with k -> -k), "swap_xy" (the tables of x and y exchanged)
    solve(res, n, d, tol)    the refinement of gauss.hip's direct path -> (phi, applications, |r|_2)
    gpu_inputs()             the right-hand sides tests/test_gpu_poisson.py gives xpic_poisson_apply: name -> (n, d, rhs)
"""
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


def hartley(n, minus=False):
    k = np.arange(n, dtype=np.int64)
    kj = (k[:, None] * k[None, :]) % n
    pi = np.arctan(np.longdouble(1)) * 4
    a = 2 * pi * kj.astype(np.longdouble) / np.longdouble(n)
    h = (np.cos(a) - np.sin(a)) if minus else (np.cos(a) + np.sin(a))
    return (h / np.sqrt(np.longdouble(n))).astype(np.float64)


def lam(n, d, fold=True):
    pi = np.arctan(np.longdouble(1)) * 4
    s = np.sin(pi * np.arange(n).astype(np.longdouble) / np.longdouble(n))
    w = 2 if (n == 2 and not fold) else 4
    return (-w * s * s / (np.longdouble(d) * np.longdouble(d))).astype(np.float64)


def transform(f, tables):
    Hx, Hy, Hz = tables
    f = np.einsum("zyj,aj->zya", f, Hx)
    f = np.einsum("zjx,aj->zax", f, Hy)
    return np.einsum("jyx,aj->ayx", f, Hz)


def apply(rhs, n, d, mutate=None):
    rhs = np.asarray(rhs, dtype=np.float64)
    tables = [hartley(n[0]), hartley(n[1]), hartley(n[2])]
    lams = [lam(n[a], d[a], fold=mutate != "no_fold") for a in range(3)]
    if mutate == "swap_xy":
        # (at unequal extents the wrong table is read as if it had the right shape, as a kernel given the wrong pointer would)
        tables[0], tables[1] = np.resize(tables[1], (n[0], n[0])), np.resize(tables[0], (n[1], n[1]))
        lams[0], lams[1] = np.resize(lams[1], n[0]), np.resize(lams[0], n[1])
    forward = [hartley(n[0], minus=True)] + tables[1:] if mutate == "minus_x" else tables
    f = transform(rhs - rhs.mean(), forward)
    den = lams[2][:, None, None] + lams[1][None, :, None] + lams[0][None, None, :]
    zero = den == 0
    out = np.where(zero, 0.0, f / np.where(zero, 1.0, den))
    if mutate == "keep_zero_mode":
        out[0, 0, 0] = f[0, 0, 0] / np.abs(den[~zero]).min() + 1.0
    return transform(out, tables)


def lap(phi, d):
    return G.div(G.grad(phi, d), d)


def solve(res, n, d, tol, maxit=10):
    res = np.asarray(res, dtype=np.float64)
    phi, r, its = np.zeros_like(res), res.copy(), 0
    rn = float(np.sqrt((r ** 2).sum()))
    while its < maxit:
        phi = phi + apply(r, n, d)
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


def gpu_inputs():
    out = {}
    for i, (name, (n, d)) in enumerate(SHAPES.items()):
        rng = np.random.default_rng(4000 + i)
        rhs = rng.normal(0.0, 1.0, (n[2], n[1], n[0]))
        out[name] = (n, d, rhs - rhs.mean())
    return out
