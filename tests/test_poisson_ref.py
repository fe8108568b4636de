"""The numpy restatement of the direct Poisson solve (tests/poisson_ref.py) against what it restates (no GPU): the dense
mean-free solve of gauss_ref's Laplacian, es_ref's FFT solve, the Hartley matrix's own properties, the planted bugs, and
the count of applications the device tests' inputs need.

Bound on phi: K_ROUNDING_PHI eps kappa |phi|_2, kappa = lam_max / lambda_min -- the form and the constant
tests/test_gpu_gauss.py measured for the rounding of the dense float64 statement, which is one side of every comparison
here."""
import numpy as np
import pytest

import es_ref as ES
import gauss_ref as G
import poisson_ref as P

EPS = G.EPS
K_ROUNDING_PHI = 17.9  # tests/test_gpu_gauss.py

DENSE = {"2x3x5": ((2, 3, 5), (0.25, 0.5, 0.125)), "5x4x3": ((5, 4, 3), (0.5, 1.0, 0.25)), "3x3x2": ((3, 3, 2), (0.7, 0.3, 0.45)),
         "6x7x9": ((6, 7, 9), (0.3, 0.45, 0.7))}


def l2(a):
    return float(np.sqrt((np.asarray(a, dtype=np.float64) ** 2).sum()))


def kappa(n, d):
    return sum(4.0 / v ** 2 for v in d) / G.lambda_min(n, d)


def meanfree(n, seed):
    rhs = np.random.default_rng(seed).normal(0.0, 1.0, (n[2], n[1], n[0]))
    return rhs - rhs.mean()


@pytest.mark.parametrize("n", [1, 2, 3, 4, 7, 16, 17, 33, 64, 100])
def test_hartley_is_symmetric_and_its_own_inverse(n):
    """H = H^T exactly (k j mod n is symmetric).  (H H)[k][l]: n products of entries of size <= sqrt(2 / n), each entry
    rounded once (eps / 2 relative), each product and each partial sum rounded: 2 / n (n (3 eps / 2) + n (n - 1) eps / 4)
    <= (n + 5) eps / 2 ... taken as (n + 5) eps."""
    H = P.hartley(n)
    assert np.array_equal(H, H.T)
    err = np.abs(H @ H - np.eye(n)).max()
    print(n, "|H H - I| / bound", err / ((n + 5) * EPS))
    assert err <= (n + 5) * EPS
    assert np.array_equal(P.lam(n, 0.5)[:1], [0.0]) and (P.lam(n, 0.5)[1:] < 0).all()


@pytest.mark.parametrize("name", list(DENSE))
def test_apply_matches_the_dense_solve(name):
    n, d = DENSE[name]
    rhs = meanfree(n, 11)
    ref = G.solve_meanfree(G.laplacian_dense(n, d), rhs)
    phi = P.apply(rhs, n, d)
    bound = K_ROUNDING_PHI * EPS * kappa(n, d) * l2(ref)
    r = l2(rhs - P.lap(phi, d))
    print(name, "|dphi| / bound", l2(phi - ref) / bound, "|r| / |rhs|", r / l2(rhs), "mean / (N eps |phi|)",
          abs(phi.mean()) / (EPS * np.abs(phi).sum()))
    assert l2(phi - ref) <= bound
    assert abs(phi.mean()) * phi.size <= phi.size * EPS * np.abs(phi).sum()
    # a right-hand side with a mean: the mean is taken out, the same phi
    assert l2(P.apply(rhs + 3.0, n, d) - phi) <= bound


def test_apply_matches_the_fft_solve():
    n, d = P.GENERAL["18x17x20"]
    rhs = meanfree(n, 12)
    ref = ES.solve_fft(rhs, n, d)
    phi = P.apply(rhs, n, d)
    bound = K_ROUNDING_PHI * EPS * kappa(n, d) * l2(ref)
    print("18x17x20 |dphi| / bound", l2(phi - ref) / bound)
    assert l2(phi - ref) <= bound


@pytest.mark.parametrize("mutate, name", [("no_fold", "2x3x5"), ("no_fold", "3x3x2"), ("keep_zero_mode", "6x7x9"),
                                          ("minus_x", "6x7x9"), ("minus_x", "5x4x3"), ("swap_xy", "6x7x9"), ("swap_xy", "2x3x5")])
def test_planted_bugs_are_seen(mutate, name):
    n, d = DENSE[name]
    rhs = meanfree(n, 13)
    ref = G.solve_meanfree(G.laplacian_dense(n, d), rhs)
    bound = K_ROUNDING_PHI * EPS * kappa(n, d) * l2(ref)
    err = l2(P.apply(rhs, n, d, mutate=mutate) - ref)
    print(mutate, name, "|dphi| / bound", err / bound)
    assert err >= 1e6 * bound


def test_single_modes():
    """one Fourier mode per axis: an eigenvector, phi = rhs / lambda_k"""
    n, d = (7, 6, 8), (0.3, 0.45, 0.7)
    z, y, x = np.meshgrid(np.arange(n[2]), np.arange(n[1]), np.arange(n[0]), indexing="ij")
    for mode in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 1, 3)):
        rhs = np.cos(2 * np.pi * (mode[0] * x / n[0] + mode[1] * y / n[1] + mode[2] * z / n[2]) + 0.3)
        lam = -sum(4.0 * np.sin(np.pi * mode[c] / n[c]) ** 2 / d[c] ** 2 for c in range(3))
        want = (rhs - rhs.mean()) / lam
        assert l2(P.apply(rhs, n, d) - want) <= K_ROUNDING_PHI * EPS * kappa(n, d) * l2(want), mode
    assert not P.apply(np.full((n[2], n[1], n[0]), 2.5), n, d).any()  # a constant: phi = 0


def test_one_application_meets_the_device_tests_tolerance():
    """What `iterations <= 2` in tests/test_gpu_poisson.py rests on: with rtol = 1e-10 relative to the charge, one
    application is enough on every input those tests give a solve -- the right-hand sides of xpic_poisson_apply and the
    cleans of test_gpu_gauss.py's loads, from E = 0 and from a random E (seed 2, a background, as
    test_clean_matches_the_dense_solve builds them).  The device has a second one for what its own rounding adds."""
    import test_gpu_gauss as T

    for name, (n, d, rhs) in P.gpu_inputs().items():
        phi, its, rn = P.solve(rhs, n, d, 1e-10 * l2(rhs))
        print(name, "its", its, "|r| / |rhs|", rn / l2(rhs))
        assert its == 1 and rn <= 1e-10 * l2(rhs), name
    for name in T.GRIDS:
        for field in ("zero", "random"):
            E, rho, n, d = P.gauss_load(name, 2, field)
            res, mean = G.residual(E, rho, d)
            tol = 1e-10 * l2(rho - mean)
            phi, its, rn = P.solve(res, n, d, tol)
            print(name, field, "its", its, "|r| / tol", rn / tol, "|r| / (1e-12 |rho~|)", rn / (1e-12 * l2(rho - mean)))
            assert its == 1 and rn <= tol, (name, field)
            assert rn <= 1e-12 * l2(rho - mean), (name, field)  # (test_gpu_gauss.py's RTOL, which the device cleans are given)
