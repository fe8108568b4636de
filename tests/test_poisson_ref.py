"""The numpy restatement of the direct Poisson solve (tests/poisson_ref.py) against what it restates (no GPU): the dense
mean-free solve of gauss_ref's Laplacian, es_ref's FFT solve, the Hartley matrix's own properties, the planted bugs, the
count of applications the device tests' inputs need, and -- against the restatement in np.longdouble -- the constants and
the application counts that tests/test_gpu_poisson.py holds the row-tile, block and extent-1024 shapes and the refinement to.

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


@pytest.mark.parametrize("n", [1, 2, 3, 4, 7, 16, 17, 33, 64, 100, 129, 1024])
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


# ---- the shapes of poisson_ref.MORE and the refinement: the float64 restatement against itself in long double -----------------
LD = np.longdouble


def norm_dg(d):
    return sum(4.0 / v ** 2 for v in d)


@pytest.fixture(scope="module")
def more():
    """name -> (n, d, rhs, phi float64, phi long double) of one application on MORE's inputs: computed once"""
    out = {}
    for name, (n, d, rhs) in P.gpu_inputs(P.MORE).items():
        out[name] = (n, d, rhs, P.apply(rhs, n, d), P.apply(rhs, n, d, dtype=LD))
    return out


@pytest.fixture(scope="module")
def refine():
    """name -> (n, d, rhs, [(phi, its, rn) of solve(tol=0, maxit=k) for k = 1, 2, 10])"""
    return {name: (n, d, rhs, [P.solve(rhs, n, d, 0.0, maxit=k) for k in (1, 2, 10)]) for name, (n, d, rhs) in P.refine_inputs().items()}


def test_long_double_path_is_long_double():
    n, d = DENSE["6x7x9"]
    rhs = meanfree(n, 11)
    assert P.hartley(7, dtype=LD).dtype == LD and P.lam(7, 0.5, dtype=LD).dtype == LD
    assert np.array_equal(P.hartley(7, dtype=LD).astype(np.float64), P.hartley(7))  # float64's table is this one, rounded
    x = P.apply(rhs, n, d, dtype=LD)
    phi, its, rn = P.solve(rhs, n, d, 0.0, maxit=2, dtype=LD)
    assert x.dtype == LD and phi.dtype == LD and its == 2
    eps_ld = float(np.finfo(LD).eps)
    r = np.asarray(rhs, dtype=LD) - np.asarray(rhs, dtype=LD).mean() - P.lap(x, d)
    print("long double: |r| / |rhs| after one application", l2(r) / l2(rhs), "eps", eps_ld)
    assert l2(r) <= 100 * eps_ld * l2(rhs)  # (float64's own is 2 eps(float64) here: the arithmetic is long double throughout)
    assert l2(P.apply(rhs, n, d) - x) <= K_ROUNDING_PHI * EPS * kappa(n, d) * l2(x)


def test_the_phi_constant_holds_on_the_new_shapes(more):
    """K_ROUNDING_PHI = 17.9 was measured on grids of at most 65 nodes a side.  Twice the float64-vs-long-double deviation
    of one application on MORE's inputs, over eps kappa |phi|: 0.0187 at the most (3x63x2; 8.4e-6 at 6x6x1024, where kappa
    is 2.2e6) -- the constant carries over, and test_gpu_poisson.py keeps it for these shapes."""
    for name, (n, d, rhs, phi, x) in more.items():
        k = 2 * l2(phi - x) / (EPS * kappa(n, d) * l2(x))
        print(name, "kappa %.3g" % kappa(n, d), "2 |phi64 - phiLD| / (eps kappa |phi|) %.3g" % k)
        assert k <= K_ROUNDING_PHI, name


def test_the_refinement_takes_a_second_application_and_stops_at_the_third(more):
    """|r| / (eps |rhs|) after 1, 2 and 3 applications with tol = 0 on every new shape, measured here (float64):
        3x63x2 12.7 2.4 2.3     2x3x63 35 5.1 5.0      3x64x2 34 5.2 5.2      2x3x64 13 2.2 2.1      3x65x2 41 5.3 5.3
        2x3x65 16 5.5 5.3       2x129x3 793 154 156    3x2x129 67 13 14       66x65x67 9.5 1.65 1.64
        1024x6x6 8723 448 450   6x1024x6 841 74 74     6x6x1024 6179 2125 2127
    The first application is given |rhs| and halves it; the second halves what the first left; the third does not, and the
    loop stops there.  At 6x6x1024 the first leaves more than the cleaner's RTOL = 1e-12 of |rhs|: long boxes do take the
    second application."""
    for name, (n, d, rhs, phi, x) in more.items():
        r = [P.solve(rhs, n, d, 0.0, maxit=k) for k in (1, 2, 3)]
        full = P.solve(rhs, n, d, 0.0, maxit=10)
        rn = [v[2] for v in r]
        print(name, "|r| / (eps |rhs|) after 1, 2, 3:", [v / (EPS * l2(rhs)) for v in rn], "stops at", full[1])
        assert [v[1] for v in r] == [1, 2, 3] and full[1] == 3, name
        assert np.array_equal(r[0][0], phi) and np.array_equal(full[0], r[2][0]) and full[2] == rn[2]
        assert rn[0] <= 0.5 * l2(rhs) and rn[1] <= 0.5 * rn[0] and rn[2] > 0.5 * rn[1], name
        assert rn[0] <= 1e-10 * l2(rhs), name
    n, d, rhs = more["6x6x1024"][:3]
    assert P.solve(rhs, n, d, 1e-12 * l2(rhs))[1] == 2


def test_the_laplacian_constant(refine):
    """K_ROUNDING_LAP of tests/test_gpu_poisson.py: twice |lap(phi2) float64 - lap(phi2) long double|_2 over
    eps |D G| |phi2|, |D G| = sum 4 / d^2, on the refinement's inputs: 0.083 (17x9x7), 0.014 (2x3x65), 0.077 (66x65x67),
    7.3e-6 (6x6x1024: a smooth phi's differences are exact)."""
    import test_gpu_poisson as TP

    for name, (n, d, rhs, runs) in refine.items():
        phi2 = runs[1][0]
        c = 2 * l2(P.lap(phi2, d) - P.lap(phi2.astype(LD), d)) / (EPS * norm_dg(d) * l2(phi2))
        print(name, "2 |lap64 - lapLD| / (eps |D G| |phi2|) %.3g" % c)
        assert c <= TP.K_ROUNDING_LAP, name


def test_store_second_is_seen(refine):
    """the += epilogue storing: phi2 is then the second application's correction alone.  The phi bound the device tests hold
    phi2 to sees it by 1e8 and more, and |phi2 - phi1| is |phi1|, not the correction's 1e-11 |phi1|."""
    for name, (n, d, rhs, runs) in refine.items():
        (phi1, _, _), (phi2, its, _) = runs[0], runs[1]
        bad, bits, _ = P.solve(rhs, n, d, 0.0, maxit=2, mutate="store_second")
        bound = K_ROUNDING_PHI * EPS * kappa(n, d) * l2(phi2)
        print(name, "store_second: |dphi| / bound %.3g" % (l2(bad - phi2) / bound), "|phi2 - phi1| mutated / true %.3g" % (l2(bad - phi1) / l2(phi2 - phi1)))
        assert its == bits == 2
        assert l2(bad - phi2) >= 1e6 * bound, name
        assert l2(bad - phi1) >= 1e6 * 4 * l2(phi2 - phi1), name


@pytest.mark.parametrize("name", ["3x2x129", "6x6x1024"])
def test_lam_high_passes_the_phi_bound_and_fails_the_residual_bound(more, name):
    """A relative error of 1e-9 in lam over the upper half of the long axis' wavenumbers.  The phi bound is dominated by the
    low modes (kappa = 2.2e3 and 2.2e6) and passes it -- the reason the device tests assert the residual as well, which has
    no kappa in it: |rhs - D G phi| / |rhs| <= K_RES = twice the restatement's own float64 ratio on that input."""
    n, d, rhs, phi, x = more[name]
    bad = P.apply(rhs, n, d, mutate="lam_high")
    bound = K_ROUNDING_PHI * EPS * kappa(n, d) * l2(x)
    k_res = 2 * l2(rhs - P.lap(phi, d)) / l2(rhs)
    res = l2(rhs - P.lap(bad, d)) / l2(rhs)
    print(name, "lam_high: |dphi| / bound %.3g" % (l2(bad - x) / bound), "|r| / |rhs| over K_RES %.3g" % (res / k_res))
    assert l2(bad - x) > 10 * l2(phi - x)  # (it is there, well above the rounding ...)
    assert l2(bad - x) <= bound            # ... and the phi bound misses it
    assert res >= 10 * k_res               # the residual bound does not
