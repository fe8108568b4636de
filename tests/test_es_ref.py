"""The numpy restatement of the electrostatic scheme (tests/es_ref.py) against what the scheme must do, without a GPU:
Gauss's law to rounding after every step with rot E, the mean of E and B left alone; a cold plasma oscillating at the
leapfrog-and-grid-corrected plasma frequency; and each planted bug visible in it."""
import numpy as np
import pytest

import es_ref as R
import gauss_ref as G
import krylov_ref as K

N, D, DT = (6, 6, 6), (0.5, 0.4, 0.25), 0.05


def load(seed=3, dtype=np.float64):
    """two sorts of opposite and unequal charge (a net charge: the mean matters), random E + uniform E0, uniform B"""
    rng = np.random.default_rng(seed)
    L = np.array(N) * np.array(D)
    sorts = []
    for ppc, q, m, dens in ((3, -1.0, 1.0, 1.0), (2, +1.0, 4.0, 0.5)):
        n = ppc * N[0] * N[1] * N[2]
        sorts.append(dict(r=(rng.random((n, 3)) * L).astype(dtype), v=rng.normal(0, 0.3, (n, 3)).astype(dtype), q=q, m=m, w=dens / ppc))
    E = 0.1 * rng.normal(size=(N[2], N[1], N[0], 3)) + np.array([0.02, -0.01, 0.03])
    B = np.zeros((N[2], N[1], N[0], 3)) + np.array([0.1, -0.2, 0.3])
    return sorts, E, B


def total_charge(sorts):
    return sum(R.deposit(s["r"], D, N, s["q"] * s["w"])[0] for s in sorts)


def test_law_curl_means_and_B_after_every_step():
    sorts, E, B = load()
    B0 = B.copy()
    Rp = K.rot_matrix(N, D, True)
    scale = np.abs(E).max() / min(D) + 2.0
    for _ in range(3):
        E1, rho, phi = R.step(sorts, E, B, N, D, DT)
        assert np.abs(rho - total_charge(sorts)).max() <= 64 * R.EPS * np.abs(rho).max()  # the charge of the positions it leaves
        assert np.abs(G.residual(E1, rho, D)[0]).max() <= 1e3 * R.EPS * scale
        assert np.abs(Rp @ (E1 - E).ravel()).max() <= 1e3 * R.EPS * scale / min(D)
        assert np.abs((E1 - E).sum(axis=(0, 1, 2))).max() <= 1e3 * R.EPS * E.size * max(np.abs(E1 - E).max(), 1e-300)
        assert np.array_equal(B, B0)
        for s in sorts:  # folded into the box
            assert (s["r"] >= 0).all() and (s["r"] <= np.array(N) * np.array(D)).all()
        E = E1
    # the FFT solve of the long runs is the same solve
    sorts2, E2, _ = load()
    Ed = R.step(sorts2, E2, B, N, D, DT)[0]
    sorts3, E3, _ = load()
    Ef = R.step(sorts3, E3, B, N, D, DT, solver="fft")[0]
    assert np.abs(Ed - Ef).max() <= 1e4 * R.EPS * np.abs(Ed).max()


def test_cold_plasma_oscillates_at_the_corrected_plasma_frequency():
    """A uniform cold electron lattice (n0 = 1, q = -1, m = 1: w_p = 1; the mean taken out is the ion background),
    displaced by xi sin(k x), from E cleaned at the start.  The seeded mode's amplitude a(t) is a pure harmonic, so
    a(t + dt) + a(t - dt) = 2 cos(w dt) a(t): w from the least-squares fit of that recurrence.  Expected:
    es_ref.omega_leapfrog (derived there): W^2 = w_p^2 S(k)^2 (k d / 2) / sin(k d / 2) of the grid, S the spline's transform,
    then sin(w dt / 2) = W dt / 2 of the leapfrog.
    What the derivation neglects.  It takes the particles for a continuum; a lattice of P particles per cell along x adds
    the lattice's aliases to the deposited charge, relative sum_{m != 0} (h / (h + 2 pi P m))^2 <= 3.3 (h / (2 pi P))^2
    with h = k d / 2 (the charge perturbation is a derivative: its aliases fall off with the square, not the cube) =
    5.0e-5 of W^2 at P = 8, the gather's cubic aliases and the oscillation's nonlinearity (k xi)^2 = 6e-10 far below.  Half
    of that reaches w: 2.5e-5.  (At P = 2 the same sum is 1.6e-3, as large as the leapfrog's correction -- measured.)  The
    bound 1e-4 is four times what is neglected, 16 times below the leapfrog's correction (+0.16 %) and 160 times below the
    grid's (-1.6 %): either one missing from the scheme fails it."""
    n, d, dt, mode, xi = (16, 6, 6), (0.25, 0.25, 0.25), 0.2, 1, 1e-5
    per = (8, 1, 1)
    ax = [(np.arange(q * m) + 0.5) * (dd / q) for m, dd, q in zip(n, d, per)]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    k = 2 * np.pi * mode / (n[0] * d[0])
    r = np.column_stack([X.ravel() + xi * np.sin(k * X.ravel()), Y.ravel(), Z.ravel()])
    sorts = [dict(r=r, v=np.zeros_like(r), q=-1.0, m=1.0, w=1.0 / 8)]
    E = np.zeros((n[2], n[1], n[0], 3))
    B = np.zeros_like(E)
    rho = R.deposit(r, d, n, -1.0 / 8)[0]
    res = G.residual(E, rho, d)[0]
    E = E - G.grad(R.solve_fft(res, n, d), d)  # the clean at the start
    xe = (np.arange(n[0]) + 0.5) * d[0]       # E_x lives on the x edges
    a = []
    for _ in range(160):
        a.append((E[..., 0] * np.sin(k * xe)).sum())
        E = R.step(sorts, E, B, n, d, dt, solver="fft")[0]
    a = np.array(a)
    c = (a[1:-1] * (a[2:] + a[:-2])).sum() / (a[1:-1] ** 2).sum()
    w = np.arccos(0.5 * c) / dt
    expect = R.omega_leapfrog(n, d, dt, mode)
    print("omega", w, "expected", expect, "relative", w / expect - 1)
    assert abs(w / expect - 1) <= 1e-4
    assert abs(expect - 1.0) >= 1e-2 and abs(expect / (2 / dt * np.arcsin(0.5 * dt)) - 1) >= 1e-2  # (the corrections are visible)


@pytest.mark.parametrize("bug", ["rho_old", "keep_mean", "plus_grad", "gather_moved", "backward_grad"])
def test_planted_bugs_are_visible(bug):
    sorts, E, B = load()
    good, Eg, _ = load()
    Rp = K.rot_matrix(N, D, True)
    scale = np.abs(E).max() / min(D) + 2.0
    E1, rho, _ = R.step(sorts, E, B, N, D, DT, mutate=bug)
    Eg1 = R.step(good, Eg, B, N, D, DT)[0]
    now = total_charge(sorts)
    law = np.abs(G.residual(E1, now, D)[0]).max()
    curl = np.abs(Rp @ (E1 - E).ravel()).max()
    if bug == "rho_old":      # the law holds for the charge of the step's start, not for the charge it leaves
        assert law >= 1e-3 * scale
    elif bug == "keep_mean":  # no phi restores a law whose right-hand side has a mean: the residual it reports stays above it
        assert abs(now.mean()) > 0.1
        assert np.sqrt((G.residual(E1, now, D, remove_mean=False)[0] ** 2).mean()) >= 0.99 * abs(now.mean())
    elif bug == "plus_grad":
        assert law >= 1e-2 * scale
    elif bug == "gather_moved":  # the law still holds; the velocities are another scheme's
        dv = max(np.abs(a["v"] - b["v"]).max() for a, b in zip(sorts, good))
        assert law <= 1e3 * R.EPS * scale and dv >= 1e-5
    else:
        assert curl >= 1e-3 * scale
    if bug != "keep_mean":
        assert np.abs(E1 - Eg1).max() >= 1e-6


def test_extended_precision_statement_agrees():
    """the float64 statement of one push against the same statement in np.longdouble, in the units the GPU test's bounds
    are written in (tests/test_gpu_es.py: statement_rounding, K_PUSH)"""
    import test_gpu_es as T

    kv, kr = T.statement_rounding()
    assert 2 * kv <= T.K_PUSH_V <= 2.1 * kv and 2 * kr <= T.K_PUSH_R <= 2.1 * kr, (kv, kr)  # (the constants are twice these)
