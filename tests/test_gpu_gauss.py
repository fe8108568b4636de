"""Gauss's law on the device (include/xpic_gauss.h, xpic_amd/csrc/gauss.hip) against tests/gauss_ref.py's numpy statement:
the residual, the clean against a dense solve, its invariants, the stopping rule, one Fourier mode, a self_ring slab, the
clean that rides with the ecsim step, and what one clean at step 0 does for a basic run.

Grids: extents of 2 (the folded stencil), less than one workgroup, several workgroups with a ragged tail, and x extents
on both sides of 64 (the kernels have no tile or vector width in x; a wavefront's 64 lanes are the only width there is).
The particles of sections 1 - 6 sit on quarter points of power-of-two (unequal) spacings with a weight of 1 / 4: every
term of the charge deposit is then exact in float64 and the sum of its atomics does not depend on their order, so the
library's own deposit inside a call and the xpic_charge_density the numpy side reads are the same numbers, bit for bit.
The fields, the background and the spacings of the other sections are general."""
import numpy as np
import pytest

import gauss_ref as G

pytestmark = pytest.mark.gpu
EPS = G.EPS

# name: (n, d, sorts)
GRIDS = {
    "2x2x2": ((2, 2, 2), (0.5, 0.25, 1.0), 1),
    "2x3x5": ((2, 3, 5), (0.25, 0.5, 0.125), 1),
    "7x5x3": ((7, 5, 3), (0.5, 1.0, 0.25), 2),      # 105 nodes: less than one workgroup
    "17x9x7": ((17, 9, 7), (0.25, 0.125, 0.5), 2),  # 1071 nodes: several workgroups, a ragged tail
    "63x3x2": ((63, 3, 2), (0.5, 0.25, 1.0), 2),    # one lane short of a wavefront per x-row
    "65x3x2": ((65, 3, 2), (0.5, 0.25, 1.0), 2),    # one lane more
}
# Rounding of the numpy statement itself: |E'(float64) - E'(np.longdouble)|_2 / (eps (|E|_2 + |G phi|_2)) and the same for
# phi over eps kappa |phi|_2, measured on the grids above (E random and E = 0; tools-free: statement_rounding() below
# prints them): largest ratios 776.2 and 8.92, on the x-long grids from E = 0 (the dense matrix has its largest condition number
# there, and |E| adds nothing to the denominator).  The bounds take twice that.
K_ROUNDING = 1553.0
K_ROUNDING_PHI = 17.9
RTOL = 1e-12


def lattice_particles(n, d, seed, per_cell=3):
    rng = np.random.default_rng(seed)
    N = n[0] * n[1] * n[2] * per_cell
    cell = np.stack([rng.integers(0, n[c], N) for c in range(3)], axis=1)
    pts = np.zeros((N, 6))
    pts[:, :3] = (cell + rng.integers(0, 4, (N, 3)) / 4.0) * np.array(d)
    return pts


def build(X, name, seed=0, background=False, field="random", **kw):
    """-> (context, E, background or None); the sorts carry +-1/4 per particle"""
    n, d, nsorts = GRIDS[name]
    rng = np.random.default_rng(1000 + seed)
    g = X.Context("ecsim", n, d, 0.5, **kw)
    if kw.get("self_ring"):
        g.comm_init_callbacks(lambda down, up, nfu, nfd: (down, up), lambda a: None)  # its own neighbour on both sides
    for s in range(nsorts):
        pts = lattice_particles(n, d, 10 * seed + s)
        sid = g.add_sort(4, 1.0, (-1.0, 1.0)[s % 2], 1.0, capacity=2 * len(pts) + 1024)
        assert g.add_particles(sid, pts) == len(pts)
    shape = (n[2], n[1], n[0])
    bg = rng.normal(0.3, 1.0, shape) if background else None
    if background:
        g.gauss_background(bg)
    E = rng.normal(0.0, 2.0, shape + (3,)) if field == "random" else np.zeros(shape + (3,))
    g.set_field(X.E, E)
    return g, E, bg


def charge(g, bg):
    """the numpy side's rho: xpic_charge_density summed in creation order, then the background"""
    parts = [g.charge_density(s) for s in range(g.nsorts)]
    rho = np.zeros((g.n[2], g.n[1], g.n[0]))
    for p in parts:
        rho = rho + p
    if bg is not None:
        rho = rho + bg
        parts.append(bg)
    return rho, parts


def term_sum(E, parts, mean, d):
    """sum |terms| of a node's residual: six differences' operands, the charges and the mean"""
    t = sum(np.abs(p) for p in parts) + abs(mean) if parts else abs(mean)
    for c in range(3):
        t = t + (np.abs(E[..., c]) + np.abs(np.roll(E[..., c], 1, axis=2 - c))) / d[c]
    return t


def statement_rounding():
    """the measurement behind K_ROUNDING (CPU only; python -c "import test_gpu_gauss as T; print(T.statement_rounding())")"""
    worst = [0.0, 0.0]
    for name, (n, d, _) in GRIDS.items():
        rng = np.random.default_rng(5)
        shape = (n[2], n[1], n[0])
        for E in (rng.normal(0.0, 2.0, shape + (3,)), np.zeros(shape + (3,))):
            rho = rng.normal(0.3, 1.0, shape)
            F64, p64 = G.clean(E, rho, d)[:2]
            Fx, px = G.clean(E, rho, d, dtype=np.longdouble)[:2]
            gphi = float(np.sqrt((G.grad(px, d) ** 2).sum()))
            kappa = sum(4.0 / v ** 2 for v in d) / G.lambda_min(n, d)
            worst[0] = max(worst[0], float(np.sqrt(((F64 - Fx) ** 2).sum())) / (EPS * (np.sqrt((E ** 2).sum()) + gphi)))
            worst[1] = max(worst[1], float(np.sqrt(((p64 - px) ** 2).sum())) / (EPS * kappa * float(np.sqrt((px ** 2).sum()))))
    return worst


@pytest.fixture(scope="module")
def X():
    import xpic_amd

    return xpic_amd


def l2(a):
    return float(np.sqrt((np.asarray(a, dtype=np.float64) ** 2).sum()))


# ---- 1. the residual -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("background", [False, True], ids=["sorts", "background"])
@pytest.mark.parametrize("name", list(GRIDS))
def test_residual_matches_the_statement(X, name, background):
    n, d, _ = GRIDS[name]
    g, E, bg = build(X, name, 1, background)
    rho, parts = charge(g, bg)
    res, mean = G.residual(E, rho, d)
    got = g.gauss_residual(X.E, want_residual=True)
    N = rho.size
    bound = 8 * EPS * term_sum(E, parts, mean, d)
    print(name, "residual: worst node error / bound", (np.abs(got["residual"] - res) / bound).max())
    assert (np.abs(got["residual"] - res) <= bound).all()
    assert abs(got["mean"] - mean) <= N * EPS * np.abs(rho).mean()
    assert abs(got["l1"] - np.abs(res).sum()) <= N * EPS * np.abs(res).sum() + bound.sum()
    assert abs(got["l2"] ** 2 - (res ** 2).sum()) <= N * EPS * (res ** 2).sum() + 2 * (np.abs(res) * bound).sum()
    rt = rho - mean
    assert abs(got["rho_l2"] ** 2 - (rt ** 2).sum()) <= N * EPS * (rt ** 2).sum() + 2 * (np.abs(rt) * bound).sum()
    # a charge of non-zero mean: the mean comes back, the residual is that of the mean-free charge
    shift = 0.75 if bg is None else 0.0
    g.gauss_background((bg if bg is not None else 0.0) + shift + np.zeros_like(rho))
    got2 = g.gauss_residual(X.E, want_residual=True)
    rho2 = rho + shift if bg is None else rho
    assert abs(got2["mean"] - rho2.mean()) <= N * EPS * np.abs(rho2).mean()
    bound2 = 8 * EPS * term_sum(E, parts + [np.full_like(rho, shift)], rho2.mean(), d)
    assert (np.abs(got2["residual"] - res) <= bound + bound2).all()
    # no output pointer for the residual: the same numbers
    got3 = g.gauss_residual(X.E)
    assert "residual" not in got3 and got3["l2"] == got2["l2"] and got3["mean"] == got2["mean"]
    g.close()


# ---- 2. the clean against the dense solve ----------------------------------------------------------------------------------
def check_clean(g, X, E, bg, d, n, out, label):
    """the corrected field and phi against gauss_ref.clean on the same charge"""
    rho, parts = charge(g, bg)
    E1_ref, phi_ref, res, mean = G.clean(E, rho, d)
    E1 = g.get_field(X.E)
    lam = G.lambda_min(n, d)
    kappa = sum(4.0 / v ** 2 for v in d) / lam
    tol = max(RTOL * l2(rho - mean), 0.0)
    gphi = l2(G.grad(out.phi, d))
    bound_E = out.after / np.sqrt(lam) + K_ROUNDING * EPS * (l2(E) + gphi)
    bound_phi = out.after / lam + K_ROUNDING_PHI * EPS * kappa * l2(phi_ref)
    after_np = l2(G.residual(E1, rho, d)[0])
    print(label, "its", out.iterations, "before", out.before, "after", out.after, "tol", tol, "|dE| / bound", l2(E1 - E1_ref) / bound_E,
          "|dphi| / bound", l2(out.phi - phi_ref) / bound_phi, "after numpy", after_np)
    assert out.iterations > 0 and out.before == pytest.approx(l2(res), rel=1e-12) and out.mean == pytest.approx(mean, abs=1e-13)
    assert l2(E1 - E1_ref) <= bound_E
    assert l2(out.phi - phi_ref) <= bound_phi
    assert out.gphi == pytest.approx(gphi, rel=1e-12)
    # the "after" norm is the residual of the field that came back, and it meets the rule
    assert abs(out.after - after_np) <= 8 * EPS * l2(term_sum(E1, parts, mean, d))
    assert out.after <= tol
    return E1, phi_ref


@pytest.mark.parametrize("field", ["zero", "random"])
@pytest.mark.parametrize("name", list(GRIDS))
def test_clean_matches_the_dense_solve(X, name, field):
    n, d, _ = GRIDS[name]
    g, E, bg = build(X, name, 2, background=True, field=field)
    out = g.gauss_clean(X.E, rtol=RTOL, maxit=4000, want_phi=True)
    check_clean(g, X, E, bg, d, n, out, name + " " + field)
    info = g.gauss_info()
    assert info["cleans"] == 1 and info["iterations"] == info["last_iterations"] == out.iterations
    assert info["before"] == out.before and info["after"] == out.after and info["mean"] == out.mean
    g.close()


# ---- 3. invariants on the device -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2x2x2", "7x5x3", "17x9x7", "65x3x2"])
def test_clean_keeps_the_curl_the_sums_and_every_other_vector(X, name):
    """From E = 0 (the electrostatic start), where the issue's bounds in max |G phi| are the rounding of what is computed:
    E' = -G phi, a curl component is four products of a stored value (rounded once, relative to |G phi|) and 1 / d, each
    rounded, and three additions of partial sums of at most four such terms: 4 (1/2 + 1/2) + 3 . 4 / 2 = 10 eps."""
    n, d, _ = GRIDS[name]
    g, E, bg = build(X, name, 3, background=True, field="zero")
    rng = np.random.default_rng(7)
    others = [X.B, X.B0, X.J, X.EP, X.EC, X.CURRI, X.CURRJE, X.W0, X.W1]  # every id but the field and the scratch W2
    g.rot_apply(+1, 1.0, X.E, X.W0)
    rot0 = g.get_field(X.W0)
    assert not rot0.any()
    kept = {f: rng.normal(size=E.shape) for f in others}
    for f, v in kept.items():
        g.set_field(f, v)
    out = g.gauss_clean(X.E, rtol=RTOL, maxit=4000, want_phi=True)
    for f, v in kept.items():  # every vector but the field and the documented scratch XPIC_W2: bit for bit
        assert np.array_equal(g.get_field(f), v), f
    E1 = g.get_field(X.E)
    gmax = np.abs(G.grad(out.phi, d)).max()
    g.rot_apply(+1, 1.0, X.E, X.W0)
    rot1 = g.get_field(X.W0)
    print(name, "curl change / bound", np.abs(rot1 - rot0).max() / (10 * EPS * gmax / min(d)),
          "sum change / bound", np.abs(E1.sum(axis=(0, 1, 2))).max() / (E1[..., 0].size * EPS * gmax))
    assert np.abs(rot1 - rot0).max() <= 10 * EPS * gmax / min(d)
    assert np.abs(E1.sum(axis=(0, 1, 2)) - E.sum(axis=(0, 1, 2))).max() <= E1[..., 0].size * EPS * gmax
    # the same on a work vector filled like E, and on Ep
    for f in (X.W0, X.EP):
        g.set_field(f, E)
        o = g.gauss_clean(f, rtol=RTOL, maxit=4000)
        assert o.iterations == out.iterations and np.array_equal(g.get_field(f), E1)
    with pytest.raises(X.XpicError, match="XPIC_W2"):
        g.gauss_clean(X.W2)
    g.close()


@pytest.mark.parametrize("name", ["2x3x5", "17x9x7"])
def test_clean_keeps_an_existing_curl(X, name):
    """From a random E, whose curl is not zero: the two curls are each rounded relative to their own field (10 eps max |E| /
    min d, as above) and E' = E - G phi is rounded once more relative to |E'|, so the bound in max |G phi| alone cannot
    hold; it is widened by exactly those terms.  A correction kernel that disturbs an existing curl shows here."""
    n, d, _ = GRIDS[name]
    g, E, bg = build(X, name, 8, background=True, field="random")
    g.rot_apply(+1, 1.0, X.E, X.W0)
    rot0 = g.get_field(X.W0)
    out = g.gauss_clean(X.E, rtol=RTOL, maxit=4000, want_phi=True)
    E1 = g.get_field(X.E)
    g.rot_apply(+1, 1.0, X.E, X.W0)
    rot1 = g.get_field(X.W0)
    gmax = np.abs(G.grad(out.phi, d)).max()
    bound = 10 * EPS * (gmax + np.abs(E).max() + np.abs(E1).max()) / min(d)
    print(name, "random E: curl change / bound", np.abs(rot1 - rot0).max() / bound, "|rot|", np.abs(rot0).max())
    assert np.abs(rot0).max() > 1.0 and np.abs(rot1 - rot0).max() <= bound
    N = E1[..., 0].size
    assert np.abs(E1.sum(axis=(0, 1, 2)) - E.sum(axis=(0, 1, 2))).max() <= N * EPS * (gmax + np.abs(E).max() + np.abs(E1).max())
    g.close()


# ---- 4. nothing to do, and failure -----------------------------------------------------------------------------------------
def test_second_clean_does_nothing_and_failures_leave_the_field(X):
    name = "17x9x7"
    n, d, _ = GRIDS[name]
    g, E, bg = build(X, name, 4, background=True)
    with pytest.raises(X.XpicError, match="gauss clean did not converge: 1 iterations"):
        g.gauss_clean(X.E, rtol=RTOL, maxit=1)
    assert np.array_equal(g.get_field(X.E), E)
    assert g.gauss_info()["cleans"] == 0
    first = g.gauss_clean(X.E, rtol=RTOL, maxit=4000)
    E1 = g.get_field(X.E)
    again = g.gauss_clean(X.E, rtol=RTOL, maxit=4000, want_phi=True)
    assert first.iterations > 0 and again.iterations == 0 and again.gphi == 0.0 and not again.phi.any()
    assert again.before == again.after == first.after
    assert np.array_equal(g.get_field(X.E), E1)
    assert g.gauss_info()["cleans"] == 2 and g.gauss_info()["iterations"] == first.iterations
    bad = E1.copy()
    bad[3, 2, 5, 1] = np.nan
    g.set_field(X.E, bad)
    with pytest.raises(X.XpicError, match="not finite"):
        g.gauss_clean(X.E, rtol=RTOL, maxit=4000)
    with pytest.raises(X.XpicError, match="not finite"):
        g.gauss_residual(X.E)
    for kw in (dict(rtol=-1.0), dict(atol=float("nan")), dict(maxit=0)):
        with pytest.raises(X.XpicError, match="gauss: "):
            g.gauss_clean(X.E, **kw)
    g.close()


# ---- 5. one Fourier mode ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 1, 3)])
def test_single_mode_potential(X, mode):
    """rho = cos(k . x) through the background, no particles, E = 0: res = -rho is an eigenvector of D G and
    phi = res / lambda_k, lambda_k = -sum_c 4 sin^2(pi k_c / n_c) / d_c^2 -- a wrong d on one axis cannot average away"""
    n, d = (7, 6, 8), (0.3, 0.45, 0.7)
    g = X.Context("ecsim", n, d, 0.5)
    z, y, x = np.meshgrid(np.arange(n[2]), np.arange(n[1]), np.arange(n[0]), indexing="ij")
    rho = np.cos(2 * np.pi * (mode[0] * x / n[0] + mode[1] * y / n[1] + mode[2] * z / n[2]) + 0.3)
    g.gauss_background(rho)
    out = g.gauss_clean(X.E, rtol=RTOL, maxit=50, want_phi=True)
    lam = -sum(4.0 * np.sin(np.pi * mode[c] / n[c]) ** 2 / d[c] ** 2 for c in range(3))
    res = -(rho - rho.mean())
    kappa = sum(4.0 / v ** 2 for v in d) / G.lambda_min(n, d)
    bound = out.after / abs(lam) + K_ROUNDING_PHI * EPS * kappa * l2(res / lam)
    print(mode, "its", out.iterations, "|dphi| / bound", l2(out.phi - res / lam) / bound)
    assert 1 <= out.iterations <= 3  # an eigenvector: one step, and what rounding leaves
    assert l2(out.phi - res / lam) <= bound
    g.close()


# ---- 6. a slab with ghost planes -------------------------------------------------------------------------------------------
def test_self_ring_cleans_like_the_plain_context(X):
    name = "17x9x7"
    n, d, _ = GRIDS[name]
    plain, E, bg = build(X, name, 6, background=True)
    ring, _, _ = build(X, name, 6, background=True, self_ring=True)
    a = plain.gauss_clean(X.E, rtol=RTOL, maxit=4000, want_phi=True)
    b = ring.gauss_clean(X.E, rtol=RTOL, maxit=4000, want_phi=True)
    Ea, _ = check_clean(plain, X, E, bg, d, n, a, "plain")
    Eb, _ = check_clean(ring, X, E, bg, d, n, b, "self_ring")
    lam = G.lambda_min(n, d)
    assert l2(Ea - Eb) <= (a.after + b.after) / np.sqrt(lam) + 2 * K_ROUNDING * EPS * (l2(E) + a.gphi)
    assert abs(a.iterations - b.iterations) <= 1 and b.before == pytest.approx(a.before, rel=1e-13)
    plain.close()
    ring.close()


# ---- 7. riding with the ecsim step -----------------------------------------------------------------------------------------
RIDE_N, RIDE_D, RIDE_DT, RIDE_RTOL, RIDE_STEPS = (6, 5, 4), (0.5, 0.4, 0.6), 0.5, 1e-8, 10


def thermal_sorts(n, d, seed, ppc=4, vth=0.05):
    rng = np.random.default_rng(seed)
    out = []
    for q, m in ((-1.0, 1.0), (1.0, 16.0)):
        N = ppc * n[0] * n[1] * n[2]
        pts = np.empty((N, 6))
        pts[:, :3] = rng.random((N, 3)) * (np.array(n) * np.array(d))
        pts[:, 3:] = rng.normal(0.0, vth / np.sqrt(m), (N, 3))
        out.append(((ppc, 1.0, q, m), pts))
    return out


def ride_context(X, every):
    g = X.Context("ecsim", RIDE_N, RIDE_D, RIDE_DT)
    for par, pts in thermal_sorts(RIDE_N, RIDE_D, 77):
        s = g.add_sort(*par, capacity=4 * len(pts))
        g.add_particles(s, pts)
    g.set_tolerances(1e-12, 1e-50, 400)
    g.gauss_clean(X.E, rtol=RIDE_RTOL)  # started clean
    if every:
        g.set_gauss_clean(every, rtol=RIDE_RTOL)
    return g


def numpy_law(g, X):
    """(|res|_2, the rule's tolerance, the rounding of forming the residual twice from differently ordered deposits)"""
    rho, parts = charge(g, None)
    E = g.get_field(X.E)
    res, mean = G.residual(E, rho, g.d)
    return l2(res), RIDE_RTOL * l2(rho - mean), 64 * EPS * l2(term_sum(E, parts, mean, g.d))


def test_clean_rides_with_the_ecsim_step(X):
    """Without the clean the first-order ecsim deposit leaves a Gauss error that is carried for ever; the CPU oracle's ecsim
    steps on this load leave |res|_2 = 0.87 after 10 steps against the rule's 1.4e-8 (measured with the numpy residual
    before this test was relied on)."""
    off, on, third = ride_context(X, 0), ride_context(X, 1), ride_context(X, 3)
    r0, tol0, _ = numpy_law(off, X)
    assert r0 <= tol0
    its_sum, cleans3 = on.gauss_info()["iterations"], []
    for step in range(1, RIDE_STEPS + 1):
        off.step(); on.step(); third.step()
        r, tol, noise = numpy_law(on, X)
        assert r <= tol + noise, (step, r, tol)
        info = on.gauss_info()
        assert info["cleans"] == 1 + step and info["after"] <= tol
        its_sum += info["last_iterations"]
        assert info["iterations"] == its_sum
        cleans3.append(third.gauss_info()["cleans"])
    r, tol, _ = numpy_law(off, X)
    print("ecsim, %d steps: uncleaned |res| %.3e, tolerance %.3e, ratio %.1f" % (RIDE_STEPS, r, tol, r / tol))
    assert r >= 100 * tol                        # the number that shows the feature is needed
    assert off.gauss_info()["cleans"] == 1
    assert cleans3 == [1, 1, 2, 2, 2, 3, 3, 3, 4, 4]  # steps 3, 6, 9 only
    r3, tol3, noise3 = numpy_law(third, X)
    assert tol3 + noise3 < r3 < r                # one uncleaned step since step 9
    third.set_gauss_clean(0)
    third.step(); third.step()
    assert third.gauss_info()["cleans"] == 4     # (step 12 would have cleaned)
    for g in (off, on, third):
        g.close()


# ---- 8. conservation with basic --------------------------------------------------------------------------------------------
# |res(step 10) - res(step 0)|_2 of the CPU oracle's basic scheme on an equivalent load (electrons only, the same ppc, vth
# and 3 : 1 gradient, E = 0 at the start), with the numpy residual: the Esirkepov deposit conserves the Gauss error to this
BASIC_ORACLE_DRIFT = 8.8e-15  # (|res0|_2 = 4.39)
BASIC_N, BASIC_D, BASIC_DT = (8, 6, 6), (0.5, 0.4, 0.6), 0.2


def basic_context(X):
    g = X.Context("basic", BASIC_N, BASIC_D, BASIC_DT)
    s = g.add_sort(8, 1.0, -1.0, 1.0, capacity=1 << 14)
    g.load_synthetic(s, 8, 0.05, seed=5, profile="gradient", param=(3.0, 0.0))
    return g


def basic_law(g, X):
    rho, _ = charge(g, None)
    return G.residual(g.get_field(X.E), rho, g.d)[0], l2(rho - rho.mean())


def test_basic_conserves_what_the_start_leaves(X):
    raw, cleaned = basic_context(X), basic_context(X)
    first = cleaned.gauss_clean(X.E, rtol=RIDE_RTOL)
    res0, rho_l2 = basic_law(raw, X)
    bound = RIDE_RTOL * rho_l2 + 2 * BASIC_ORACLE_DRIFT
    assert first.before == pytest.approx(l2(res0), rel=1e-9) and l2(res0) >= 1e3 * bound  # E = 0 does not go with this load
    for _ in range(10):
        raw.step(); cleaned.step()
    res10, _ = basic_law(raw, X)
    resc, _ = basic_law(cleaned, X)
    print("basic, 10 steps: |res0| %.3e, |res10 - res0| %.3e, cleaned |res10| %.3e, bound %.3e" % (l2(res0), l2(res10 - res0), l2(resc), bound))
    assert l2(res10 - res0) <= bound             # carried for ever ...
    assert l2(resc) <= bound                     # ... or never there
    raw.close()
    cleaned.close()


# ---- 9. the host mirror ----------------------------------------------------------------------------------------------------
def test_host_mirror_gauss_law(X, tmp_path):
    """The reference's ecsim_ex1 set-up (10^3 cells, 100 electrons per cell, no ions) for 4 steps, with
    "GaussLaw": {"at_start": true, "every": 2} and without the key.  With it: temporal/gauss_law.txt holds a row per step,
    cleans at steps 0, 2 and 4 and the standing residual at 1 and 3, and the E of the last backup satisfies the law for the
    backup's particles.  Without it: the files of the parent -- no gauss_law.txt, and the tables' titles and step-0 rows
    equal the reference's golden ones in every printed character but the padding (later rows carry the last bits of the deposits' floating-point
    atomics and differ between any two runs of one executable, so bytes cannot pin them)."""
    import json
    import os
    import struct
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(X.__file__)))
    exe = os.path.join(root, "xpic_amd", "host", "xpic_hip.out")
    gold = os.path.join(root, "tests", "golden", "ecsim_ex1")
    rtol = 1e-10

    def run(name, extra):
        cfg = json.load(open(os.path.join(gold, "config.json")))
        dt = cfg["Geometry"]["dt"]
        cfg["Geometry"]["t"], cfg["Geometry"]["diagnose_period"] = 4 * dt, 2 * dt
        out_dir = tmp_path / name
        out_dir.mkdir()
        cfg["OutputDirectory"] = str(out_dir)
        cfg["SimulationBackup"] = {"diagnose_period": "2 [dt]"}
        cfg.update(extra)
        (out_dir / "config.json").write_text(json.dumps(cfg))
        out = subprocess.run([exe, str(out_dir / "config.json")], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        return out_dir, cfg

    with_key, cfg = run("with", {"GaussLaw": {"at_start": True, "every": 2, "rtol": rtol}})
    without, _ = run("without", {})
    assert sorted(os.listdir(without / "temporal")) == sorted(set(os.listdir(with_key / "temporal")) - {"gauss_law.txt"})
    assert "gauss_law.txt" in os.listdir(with_key / "temporal") and "gauss_law.txt" not in os.listdir(without / "temporal")
    assert sorted(set(os.listdir(with_key)) - {"config.json"}) == sorted(set(os.listdir(without)) - {"config.json"})
    for table in ("energy.txt", "energy_conservation.txt"):
        mine, ref = open(without / "temporal" / table).readlines(), open(os.path.join(gold, table)).readlines()
        assert len(mine) == 6 and [ln.split() for ln in mine[:2]] == [ln.split() for ln in ref[:2]], table
    # (the start clean changed E: the keyed run's step-0 field energy is not the golden one)
    assert open(with_key / "temporal" / "energy.txt").readlines()[1].split() != open(os.path.join(gold, "energy.txt")).readlines()[1].split()

    lines = open(with_key / "temporal" / "gauss_law.txt").readlines()
    assert lines[0].split() == ["Time", "Res_before", "Res_after", "Mean_rho", "Iterations"] and len(lines) == 6
    rows = np.array([[float(v) for v in ln.split()] for ln in lines[1:]])
    assert rows[:, 0].tolist() == [0, 1, 2, 3, 4]

    # the last backup: its particles and its E on a context of the same grid
    n, d = (10, 10, 10), (0.5, 0.5, 0.5)
    sort = cfg["Particles"][0]
    bdir = with_key / "simulation_backup" / "4"
    (count,) = struct.unpack(">i", open(bdir / "electrons.numparts", "rb").read())
    pts = np.fromfile(bdir / "electrons", dtype=">f8").astype(np.float64).reshape(count, 6)
    E = np.fromfile(bdir / "E", dtype=">f8", offset=8).astype(np.float64).reshape(n[2], n[1], n[0], 3)
    g = X.Context("ecsim", n, d, cfg["Geometry"]["dt"])
    s = g.add_sort(sort["Np"], sort["n"], sort["q"], sort["m"], capacity=2 * count)
    assert g.add_particles(s, pts) == count
    g.set_field(X.E, E)
    got = g.gauss_residual(X.E)
    rho, parts = charge(g, None)
    tol = rtol * got["rho_l2"]
    noise = 64 * EPS * l2(term_sum(E, parts, got["mean"], d))
    print("host mirror: final |res| %.3e, tolerance %.3e; table" % (got["l2"], tol), rows.tolist())
    assert got["l2"] <= tol + noise                      # the final E satisfies the law
    assert got["mean"] == pytest.approx(-1.0, rel=1e-10)  # electrons alone: the neutralising background is +1
    printed = 1 + 1e-6
    for t in (0, 2, 4):   # cleaned: iterations, and the rule met
        assert rows[t, 4] > 0 and rows[t, 2] <= tol * printed < rows[t, 1], rows[t]
    for t in (1, 3):      # not cleaned: the residual as it stands, above the rule
        assert rows[t, 4] == 0 and rows[t, 1] == rows[t, 2] > 100 * tol, rows[t]
    assert np.allclose(rows[:, 3], -1.0, rtol=1e-6)
    assert rows[4, 2] == pytest.approx(got["l2"], rel=1e-5, abs=noise)
    g.close()
