"""The direct Poisson solve on the device (include/xpic_poisson.h, xpic_amd/csrc/poisson.hip, the direct path of gauss.hip)
against tests/poisson_ref.py's numpy restatement and against what tests/test_gpu_gauss.py and tests/test_gpu_es.py hold the
CG solve to: one application of the transform solve alone, the clean with "direct", the choice of the solver, the clean that
rides with the ecsim step, the electrostatic step, and the host mirror's "solver" key.

Shapes of xpic_poisson_apply (poisson_ref.SHAPES): three small ones, each axis in turn at 15, 16, 17 and 33 nodes -- on both
sides of the 16-wide instruction tile, and of the 16-deep staging tile of the summed index -- with the other two tiny, and
18x17x20.  The x extents 63 and 65 and the several-workgroup grid come with test_gpu_gauss.py's loads in section 2.
`iterations <= 2` is a condition, not a measurement: tests/test_poisson_ref.py shows that one application meets the
tolerance on every input here; the second is for what the device's own rounding may add.

Further shapes (poisson_ref.MORE): y and z in turn at 63, 64, 65 and 129 -- along them the table is the kernel's left operand
and the extent its count of rows, so these are the first with a second row tile, a ragged last one and more than three tiles
of the summed index against a table; 66x65x67 -- two tiles in m and c and five in k in every pass, 67 products along y; and
1024x6x6, 6x1024x6, 6x6x1024 -- XPIC_POISSON_MAX_EXTENT on each axis, 64 tiles of accumulation, 16 row tiles.  Sections 7
and 8 pin the refinement (xpic_poisson_solve: the += epilogue, the explicit residual between applications, the "did not
halve" exit), on poisson_ref.REFINE.

Constants, all measured on the CPU against the restatement in np.longdouble (tests/test_poisson_ref.py asserts each):
  K_ROUNDING_PHI = 17.9 holds on the further shapes: twice the float64-vs-long-double deviation of one application there is
      at most 0.0187 eps kappa |phi| (3x63x2; 8.4e-6 at 6x6x1024), so no shape gets a constant of its own.
  K_ROUNDING_LAP = 0.083: twice |D G phi2 (float64) - D G phi2 (long double)|_2 over eps |D G| |phi2|, |D G| = sum 4 / d^2, on
      REFINE's inputs (0.083, 0.014, 0.077, 7.3e-6) -- what the library's explicit |r|_2 may differ by from numpy's.
  K_RES(input) = twice the restatement's own float64 |rhs - D G phi|_2 / |rhs|_2 on that input, computed here from P.apply:
      4 eps to 1.7e4 eps (1024x6x6).  The restatement makes its passes in the library's order (x, y, z forward, z, y, x back):
      the axis that goes last decides what rounding leaves, by a factor 2.5 at 2x15x3.  The kappa-free check: the phi bound is dominated by the low modes and passes a relative
      error of 1e-9 in the upper half of the spectrum at kappa >= 2e3 (test_lam_high_passes_the_phi_bound_...)."""
import numpy as np
import pytest

import es_ref as ES
import gauss_ref as G
import poisson_ref as P
import test_gpu_gauss as TG

pytestmark = pytest.mark.gpu
EPS = G.EPS
K_ROUNDING_PHI = TG.K_ROUNDING_PHI
K_ROUNDING_LAP = 0.083
RTOL = TG.RTOL
LD = np.longdouble


@pytest.fixture(scope="module")
def X():
    import xpic_amd

    return xpic_amd


@pytest.fixture(scope="module")
def inputs():
    """name -> (n, d, rhs, the restatement's phi): computed once, read by every test"""
    out = {}
    for name, (n, d, rhs) in dict(P.gpu_inputs(), **P.gpu_inputs(P.MORE)).items():
        phi = P.apply(rhs, n, d)
        rhs.setflags(write=False)
        phi.setflags(write=False)
        out[name] = (n, d, rhs, phi)
    return out


def l2(a):
    return float(np.sqrt((np.asarray(a, dtype=np.float64) ** 2).sum()))


def kappa(n, d):
    return sum(4.0 / v ** 2 for v in d) / G.lambda_min(n, d)


def norm_dg(d):
    return sum(4.0 / v ** 2 for v in d)


def check_apply(label, phi, rhs, ref, n, d):
    """phi against the restatement's ref by the phi bound, and by the residual bound: twice the restatement's own"""
    rhs = rhs - rhs.mean()
    bound = K_ROUNDING_PHI * EPS * kappa(n, d) * l2(ref)
    k_res = 2 * l2(rhs - P.lap(ref, d)) / l2(rhs)
    res = l2(rhs - P.lap(phi, d)) / l2(rhs)
    print(label, "|dphi| / bound", l2(phi - ref) / bound, "|r| / bound", res / k_res, "K_RES / eps", k_res / EPS)
    assert l2(phi - ref) <= bound
    assert res <= k_res
    return bound


# ---- 1. one application against the restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(P.SHAPES) + list(P.MORE))
def test_apply_matches_the_restatement(X, inputs, name):
    n, d, rhs, ref = inputs[name]
    g = X.Context("ecsim", n, d, 0.5)
    phi = g.poisson_apply(rhs)
    bound = check_apply(name, phi, rhs, ref, n, d)
    print(name, "mean / (N eps |phi|)", abs(phi.mean()) / (EPS * np.abs(phi).sum()))
    assert abs(phi.mean()) <= phi.size * EPS * np.abs(phi).mean()
    assert np.array_equal(g.poisson_apply(rhs), phi)  # the same bits
    # a mean in the right-hand side is taken out; a constant one gives phi = 0
    assert l2(g.poisson_apply(rhs + 3.0) - ref) <= bound
    assert not g.poisson_apply(np.full(rhs.shape, 2.5)).any()
    assert g.poisson_solver == "cg" and g.gauss_info()["cleans"] == 0  # the hook neither selects nor counts
    g.close()


@pytest.mark.parametrize("mode", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 1, 3)])
def test_single_mode(X, mode):
    """test_gpu_gauss.py's test_single_mode_potential on one application: an eigenvector of D G, phi = rhs / lambda_k"""
    n, d = (7, 6, 8), (0.3, 0.45, 0.7)
    g = X.Context("ecsim", n, d, 0.5)
    z, y, x = np.meshgrid(np.arange(n[2]), np.arange(n[1]), np.arange(n[0]), indexing="ij")
    rhs = np.cos(2 * np.pi * (mode[0] * x / n[0] + mode[1] * y / n[1] + mode[2] * z / n[2]) + 0.3)
    lam = -sum(4.0 * np.sin(np.pi * mode[c] / n[c]) ** 2 / d[c] ** 2 for c in range(3))
    want = (rhs - rhs.mean()) / lam
    phi = g.poisson_apply(rhs)
    bound = K_ROUNDING_PHI * EPS * kappa(n, d) * l2(want)
    print(mode, "|dphi| / bound", l2(phi - want) / bound)
    assert l2(phi - want) <= bound
    bad = rhs.copy()
    bad[3, 2, 5] = np.inf
    with pytest.raises(X.XpicError, match="not finite"):
        g.poisson_apply(bad)
    g.close()


@pytest.mark.parametrize("mode", [1, 64, 128])
@pytest.mark.parametrize("name, axis", [("2x129x3", 1), ("3x2x129", 2)])
def test_single_mode_through_two_ragged_row_tiles(X, name, axis, mode):
    """an eigenvector along the 129-node axis -- three row tiles, the last of one row -- at the lowest wavenumber from
    either end of the table (1, 128) and at the highest (64 = n // 2): phi = rhs / lam[mode]"""
    n, d = P.MORE[name]
    g = X.Context("ecsim", n, d, 0.5)
    j = np.arange(129).reshape([129 if a == 2 - axis else 1 for a in range(3)])
    rhs = np.cos(2 * np.pi * ((mode * j) % 129) / 129 + 0.3) + np.zeros((n[2], n[1], n[0]))
    lam = -4.0 * np.sin(np.pi * mode / 129) ** 2 / d[axis] ** 2
    want = (rhs - rhs.mean()) / lam
    phi = g.poisson_apply(rhs)
    bound = K_ROUNDING_PHI * EPS * kappa(n, d) * l2(want)
    print(name, mode, "|dphi| / bound against rhs / lam", l2(phi - want) / bound)
    assert l2(phi - want) <= bound
    check_apply("%s mode %d" % (name, mode), phi, rhs, P.apply(rhs, n, d), n, d)
    g.close()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_column_deltas_through_the_tile_seams(X, axis):
    """rhs = e_j - mean at 66x65x67, j = 0, 63, 64 and the last index along one axis (the other two indices at 5 and 37):
    the forward pass along that axis reads column j of its table alone, on both sides of the 64-wide seam"""
    n, d = P.BLOCK["66x65x67"]
    g = X.Context("ecsim", n, d, 0.5)
    for j in sorted({0, 63, 64, n[axis] - 1}):
        at = [5, 37, 5]
        at[2 - axis] = j
        rhs = np.zeros((n[2], n[1], n[0]))
        rhs[tuple(at)] = 1.0
        check_apply("delta axis %d j %d" % (axis, j), g.poisson_apply(rhs), rhs, P.apply(rhs, n, d), n, d)
    g.close()


def test_a_table_shared_by_x_and_z_then_a_fresh_context(X):
    """nx == nz != ny: one table for the axes 0 and 2, freed once; then a context whose tables differ from it"""
    for n, d, seed in (((65, 3, 65), (0.5, 0.25, 1.0), 5200), ((3, 65, 3), (0.25, 0.5, 0.125), 5201)):
        rhs = np.random.default_rng(seed).normal(0.0, 1.0, (n[2], n[1], n[0]))
        g = X.Context("ecsim", n, d, 0.5)
        phi = g.poisson_apply(rhs)
        check_apply("%dx%dx%d" % n, phi, rhs, P.apply(rhs, n, d), n, d)
        assert np.array_equal(g.poisson_apply(rhs), phi)
        g.close()


# ---- 2. the clean with "direct" ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", ["zero", "random"])
@pytest.mark.parametrize("name", list(TG.GRIDS))
def test_direct_clean_matches_the_dense_solve(X, name, field):
    n, d, _ = TG.GRIDS[name]
    g, E, bg = TG.build(X, name, 2, background=True, field=field)
    g.set_poisson_solver("direct")
    assert g.poisson_solver == "direct"
    out = g.gauss_clean(X.E, rtol=RTOL, maxit=4000, want_phi=True)
    TG.check_clean(g, X, E, bg, d, n, out, name + " " + field + " direct")  # (after <= tol and iterations > 0 are in there)
    assert out.iterations <= 2
    info = g.gauss_info()
    assert info["cleans"] == 1 and info["iterations"] == info["last_iterations"] == out.iterations
    # CG on the same context and load needs more
    g.set_field(X.E, E)
    g.set_poisson_solver("cg")
    cg = g.gauss_clean(X.E, rtol=RTOL, maxit=4000)
    print(name, field, "applications", out.iterations, "CG iterations", cg.iterations)
    assert cg.iterations > out.iterations
    g.close()


@pytest.mark.parametrize("name", ["2x2x2", "7x5x3", "17x9x7", "65x3x2"])
def test_direct_clean_keeps_the_curl_and_the_sums(X, name):
    """test_gpu_gauss.py's test_clean_keeps_the_curl_the_sums_and_every_other_vector with "direct", its bounds"""
    n, d, _ = TG.GRIDS[name]
    g, E, bg = TG.build(X, name, 3, background=True, field="zero")
    g.set_poisson_solver("direct")
    rng = np.random.default_rng(7)
    others = [X.B, X.B0, X.J, X.EP, X.EC, X.CURRI, X.CURRJE, X.W0, X.W1]
    kept = {f: rng.normal(size=E.shape) for f in others}
    for f, v in kept.items():
        g.set_field(f, v)
    out = g.gauss_clean(X.E, rtol=RTOL, maxit=4000, want_phi=True)
    for f, v in kept.items():
        assert np.array_equal(g.get_field(f), v), f
    E1 = g.get_field(X.E)
    gmax = np.abs(G.grad(out.phi, d)).max()
    g.rot_apply(+1, 1.0, X.E, X.W0)
    rot1 = g.get_field(X.W0)
    assert out.iterations <= 2
    assert np.abs(rot1).max() <= 10 * EPS * gmax / min(d)
    assert np.abs(E1.sum(axis=(0, 1, 2)) - E.sum(axis=(0, 1, 2))).max() <= E1[..., 0].size * EPS * gmax
    g.close()


def test_direct_second_clean_maxit_one_and_a_nan(X):
    name = "17x9x7"
    g, E, bg = TG.build(X, name, 4, background=True)
    g.set_poisson_solver("direct")
    first = g.gauss_clean(X.E, rtol=RTOL, maxit=1)  # one application is a whole solve
    assert first.iterations == 1 and first.after <= RTOL * g.gauss_residual(X.E)["rho_l2"]
    E1 = g.get_field(X.E)
    again = g.gauss_clean(X.E, rtol=RTOL, maxit=4000, want_phi=True)
    assert again.iterations == 0 and again.gphi == 0.0 and not again.phi.any()
    assert again.before == again.after == first.after
    assert np.array_equal(g.get_field(X.E), E1)
    assert g.gauss_info()["cleans"] == 2 and g.gauss_info()["iterations"] == 1
    bad = E.copy()
    bad[3, 2, 5, 1] = np.nan
    g.set_field(X.E, bad)
    with pytest.raises(X.XpicError, match="not finite"):
        g.gauss_clean(X.E, rtol=RTOL, maxit=4000)
    got = g.get_field(X.E)
    assert np.array_equal(np.isnan(got), np.isnan(bad)) and np.array_equal(got[~np.isnan(bad)], bad[~np.isnan(bad)])
    g.close()


# ---- 3. selection ------------------------------------------------------------------------------------------------------------
def test_selection(X):
    name = "17x9x7"
    fresh, E, bg = TG.build(X, name, 5, background=True)
    assert fresh.poisson_solver == "cg"  # the default
    a = fresh.gauss_clean(X.E, rtol=RTOL, maxit=4000, want_phi=True)
    g, _, _ = TG.build(X, name, 5, background=True)
    g.set_poisson_solver("direct")
    g.gauss_clean(X.E, rtol=RTOL, maxit=4000)
    g.set_field(X.E, E)
    g.set_poisson_solver("cg")
    b = g.gauss_clean(X.E, rtol=RTOL, maxit=4000, want_phi=True)
    assert a.iterations == b.iterations and a[1:5] == b[1:5] and np.array_equal(a.phi, b.phi)
    assert np.array_equal(fresh.get_field(X.E), g.get_field(X.E))  # CG after a switch and back: a fresh context's bits
    with pytest.raises(X.XpicError, match="unknown solver kind"):
        g.set_poisson_solver(7)
    assert g.poisson_solver == "cg"
    g.set_poisson_solver("direct")
    with pytest.raises(X.XpicError, match="unknown solver kind"):
        g.set_poisson_solver(-1)
    assert g.poisson_solver == "direct"
    ring, _, _ = TG.build(X, name, 5, background=True, self_ring=True)
    with pytest.raises(X.XpicError, match="single-slab"):
        ring.set_poisson_solver("direct")
    assert ring.poisson_solver == "cg"
    with pytest.raises(X.XpicError, match="single-slab"):
        ring.poisson_apply(np.zeros((ring.nzl, ring.n[1], ring.n[0])))
    long = X.Context("ecsim", (X.POISSON_MAX_EXTENT + 1, 2, 2), (0.5, 0.5, 0.5), 0.5)
    with pytest.raises(X.XpicError, match="extents up to 1024"):
        long.set_poisson_solver("direct")
    assert long.poisson_solver == "cg"
    # the refinement's hook with one application is xpic_poisson_apply, bit for bit; it has the hook's refusals, neither
    # selects nor counts, and a caller who asks for a count is not refused for not converging
    rhs = np.random.default_rng(9).normal(0.0, 1.0, (7, 9, 17))
    cleans = g.gauss_info()["cleans"]
    phi, its, rn = g.poisson_solve(rhs, maxit=1)
    assert its == 1 and rn > 0.0 and np.array_equal(phi, g.poisson_apply(rhs))
    assert np.array_equal(fresh.poisson_solve(rhs)[0], phi) and fresh.poisson_solver == "cg"
    assert g.poisson_solver == "direct" and g.gauss_info()["cleans"] == cleans and fresh.gauss_info()["cleans"] == 1
    with pytest.raises(X.XpicError, match="single-slab"):
        ring.poisson_solve(np.zeros((ring.nzl, ring.n[1], ring.n[0])))
    with pytest.raises(X.XpicError, match="extents up to 1024"):
        long.poisson_solve(np.zeros((2, 2, X.POISSON_MAX_EXTENT + 1)))
    bad = rhs.copy()
    bad[3, 2, 5] = np.nan
    with pytest.raises(X.XpicError, match="not finite"):
        g.poisson_solve(bad)
    for kw in (dict(tol=-1.0), dict(tol=float("nan")), dict(maxit=0)):
        with pytest.raises(X.XpicError, match="poisson: "):
            g.poisson_solve(rhs, **kw)
    for c in (fresh, g, ring, long):
        c.close()


# ---- 4. riding with the ecsim step -------------------------------------------------------------------------------------------
def test_direct_clean_rides_with_the_ecsim_step(X):
    """test_gpu_gauss.py's test_clean_rides_with_the_ecsim_step: its load, its tolerances, its law, the solver "direct" """
    g = X.Context("ecsim", TG.RIDE_N, TG.RIDE_D, TG.RIDE_DT)
    for par, pts in TG.thermal_sorts(TG.RIDE_N, TG.RIDE_D, 77):
        s = g.add_sort(*par, capacity=4 * len(pts))
        g.add_particles(s, pts)
    g.set_tolerances(1e-12, 1e-50, 400)
    g.set_poisson_solver("direct")
    assert g.gauss_clean(X.E, rtol=TG.RIDE_RTOL).iterations <= 2  # started clean
    g.set_gauss_clean(1, rtol=TG.RIDE_RTOL)
    its_sum = g.gauss_info()["iterations"]
    for step in range(1, TG.RIDE_STEPS + 1):
        g.step()
        r, tol, noise = TG.numpy_law(g, X)
        assert r <= tol + noise, (step, r, tol)
        info = g.gauss_info()
        assert info["cleans"] == 1 + step and info["after"] <= tol
        assert 1 <= info["last_iterations"] <= 2, (step, info)
        its_sum += info["last_iterations"]
        assert info["iterations"] == its_sum
    g.close()


# ---- 5. the electrostatic step -----------------------------------------------------------------------------------------------
ES_N, ES_D, ES_DT, ES_STEPS, ES_PPC = (8, 6, 6), (0.5, 0.4, 0.25), 0.05, 5, 4
ES_RTOL, ES_ATOL = 1e-10, 1e-14  # the defaults of an "es" context


def two_beams(seed=21, v0=0.4, vth=0.02):
    """two electron sorts drifting against each other along x (a neutralising background is the mean the solve takes out)"""
    rng = np.random.default_rng(seed)
    N = ES_PPC * ES_N[0] * ES_N[1] * ES_N[2]
    out = []
    for sign in (+1.0, -1.0):
        p = np.empty((N, 6))
        p[:, :3] = rng.random((N, 3)) * (np.array(ES_N) * np.array(ES_D))
        p[:, 3:] = rng.normal(0.0, vth, (N, 3)) + np.array([sign * v0, 0.0, 0.0])
        out.append(p)
    return out


def canon(p6):
    c = ES.cells(p6[:, :3], ES_N, ES_D)
    return p6[np.lexsort((p6[:, 2], p6[:, 1], p6[:, 0], c))]


def test_es_steps_with_the_direct_solve(X):
    """Five steps against es_ref.step(solver="fft") by the bounds of test_gpu_es.py's test_ten_steps: the law to the stopping
    rule + the clean's rounding term, and E, r, v within 2 DEV (the float64 statement's own rounding over these steps,
    measured here as the FFT statement against the np.longdouble dense one) + what the stopping rule leaves, summed over the
    steps so far."""
    K_ROUNDING = TG.K_ROUNDING
    n, d = ES_N, ES_D
    beams = two_beams()
    shape = (n[2], n[1], n[0])
    E0, B = np.zeros(shape + (3,)), np.zeros(shape + (3,))
    g = X.Context("es", n, d, ES_DT)
    for p in beams:
        s = g.add_sort(ES_PPC, 1.0, -1.0, 1.0, capacity=2 * len(p) + 1024)
        assert g.add_particles(s, p) == len(p)
    g.set_poisson_solver("direct")
    ref = [dict(r=g.particles(s)[0][:, :3].copy(), v=g.particles(s)[0][:, 3:].copy(), q=-1.0, m=1.0, w=1.0 / ES_PPC) for s in range(2)]
    fine = [dict(so, r=so["r"].astype(np.longdouble), v=so["v"].astype(np.longdouble)) for so in ref]
    Er, Ex = E0, E0.astype(np.longdouble)
    lam = G.lambda_min(n, d)
    dev = [0.0, 0.0, 0.0]
    acc = 0.0
    for k in range(ES_STEPS):
        its = g.step()
        Er, rho, phi = ES.step(ref, Er, B, n, d, ES_DT, solver="fft")
        Ex = ES.step(fine, Ex, B, n, d, ES_DT, dtype=np.longdouble)[0]
        dev[0] = max(dev[0], float(np.abs(Er - Ex).max()))
        dev[1] = max(dev[1], max(float(np.abs(a["r"] - b["r"]).max()) for a, b in zip(ref, fine)))
        dev[2] = max(dev[2], max(float(np.abs(a["v"] - b["v"]).max()) for a, b in zip(ref, fine)))
        Eg = g.get_field(X.E)
        info = g.gauss_info()
        res = g.gauss_residual(X.E)
        tol = max(ES_RTOL * res["rho_l2"], ES_ATOL)
        term = K_ROUNDING * EPS * (l2(Eg) + l2(G.grad(phi, d)))
        assert its == info["last_iterations"] and 1 <= its <= 2, (k, its)
        assert res["l2"] <= tol + term / min(d), (k, res["l2"], tol)
        acc += info["after"] / np.sqrt(lam)
        bE = 2 * dev[0] + acc + term
        bV = 2 * dev[2] + (k + 1) * ES_DT * bE
        bR = 2 * dev[1] + (k + 1) * ES_DT * bV
        dE = np.abs(Eg - Er).max()
        worst_r = worst_v = 0.0
        for s in range(2):
            pg = canon(g.particles(s)[0])
            pr = canon(np.hstack([ref[s]["r"], ref[s]["v"]]))
            worst_r = max(worst_r, np.abs(pg[:, :3] - pr[:, :3]).max())
            worst_v = max(worst_v, np.abs(pg[:, 3:] - pr[:, 3:]).max())
        print("step", k, "its", its, "res", res["l2"], "tol", tol, "dE / bound", dE / bE, "dr / bound", worst_r / bR, "dv / bound", worst_v / bV)
        assert dE <= bE and worst_r <= bR and worst_v <= bV
    g.close()


# ---- 6. the host mirror ------------------------------------------------------------------------------------------------------
def test_host_mirror_solver_key(X, tmp_path):
    """test_gpu_gauss.py's test_host_mirror_gauss_law set-up with "solver": "direct": every row of gauss_law.txt shows the law
    met with at most 2 iterations; a run without the key writes the parent's tables."""
    import json
    import os
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
        cfg.update(extra)
        (out_dir / "config.json").write_text(json.dumps(cfg))
        out = subprocess.run([exe, str(out_dir / "config.json")], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        return out_dir

    direct = run("direct", {"GaussLaw": {"at_start": True, "every": 1, "rtol": rtol, "solver": "direct"}})
    without = run("without", {})
    lines = open(direct / "temporal" / "gauss_law.txt").readlines()
    assert lines[0].split() == ["Time", "Res_before", "Res_after", "Mean_rho", "Iterations"] and len(lines) == 6
    rows = np.array([[float(v) for v in ln.split()] for ln in lines[1:]])
    print("host mirror, direct:", rows.tolist())
    # E = 0 at the start, so row 0's |res| before is |rho~| of the start; the later steps' |rho~| is the same thermal noise of
    # 1e5 particles, taken here as within a factor 2 of it (the library itself holds every clean to its own rho~: a clean that
    # misses the rule fails the step and the run)
    rho_l2 = rows[0, 1]
    for t in range(5):
        assert 1 <= rows[t, 4] <= 2, rows[t]
        assert rows[t, 2] <= 2.0 * rtol * rho_l2 < rows[t, 1], rows[t]
    assert np.allclose(rows[:, 3], -1.0, rtol=1e-6)
    assert "gauss_law.txt" not in os.listdir(without / "temporal")
    for table in ("energy.txt", "energy_conservation.txt"):
        mine, ref = open(without / "temporal" / table).readlines(), open(os.path.join(gold, table)).readlines()
        assert len(mine) == 6 and [ln.split() for ln in mine[:2]] == [ln.split() for ln in ref[:2]], table
    with pytest.raises(AssertionError):
        run("bad", {"GaussLaw": {"solver": "fft"}})


# ---- 7. the refinement: xpic_poisson_solve ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refine():
    """name -> (n, d, rhs, the restatement's phi after one application and after two): computed once, read by every test"""
    out = {}
    for name, (n, d, rhs) in P.refine_inputs().items():
        ref1, ref2 = P.apply(rhs, n, d), P.solve(rhs, n, d, 0.0, maxit=2)[0]
        for a in (rhs, ref1, ref2):
            a.setflags(write=False)
        out[name] = (n, d, rhs, ref1, ref2)
    return out


@pytest.mark.parametrize("name", list(P.REFINE))
def test_two_applications(X, refine, name):
    """tol = 0, maxit = 2: the second application runs k_hartley_pass<kAdd> on the explicit residual of the first.
    its == 2 is a condition: the first application is given |rhs| and leaves 1e-12 of it, so it halves, and nothing meets
    tol = 0.  |phi2 - phi1| within a factor 4 of the restatement's on both sides is a coarse band, no tolerance on rounding:
    a dropped correction gives 0 and a stored or doubled one |phi1|, which is 1e8 to 1e15 times the correction
    (tests/test_poisson_ref.py: test_store_second_is_seen)."""
    n, d, rhs, ref1, ref2 = refine[name]
    g = X.Context("ecsim", n, d, 0.5)
    phi1, its1, rn1 = g.poisson_solve(rhs, tol=0.0, maxit=1)
    phi2, its2, rn2 = g.poisson_solve(rhs, tol=0.0, maxit=2)
    rn_np = l2(rhs - P.lap(phi2, d))
    allowed = K_ROUNDING_LAP * EPS * norm_dg(d) * l2(phi2)
    bound = K_ROUNDING_PHI * EPS * kappa(n, d) * l2(ref2)
    step, step_ref = l2(phi2 - phi1), l2(ref2 - ref1)
    print(name, "rn1 / (eps |rhs|)", rn1 / (EPS * l2(rhs)), "rn2 / (eps |rhs|)", rn2 / (EPS * l2(rhs)), "|rn2 - numpy's| / allowed",
          abs(rn2 - rn_np) / allowed, "|dphi2| / bound", l2(phi2 - ref2) / bound, "|phi2 - phi1| / the restatement's", step / step_ref)
    assert its1 == 1 and its2 == 2
    assert np.array_equal(phi1, g.poisson_apply(rhs))
    assert abs(rn1 - l2(rhs - P.lap(phi1, d))) <= K_ROUNDING_LAP * EPS * norm_dg(d) * l2(phi1)
    assert abs(rn2 - rn_np) <= allowed
    assert l2(phi2 - ref2) <= bound
    assert step_ref / 4 <= step <= 4 * step_ref
    again = g.poisson_solve(rhs, tol=0.0, maxit=2)
    assert np.array_equal(again[0], phi2) and again[1:] == (its2, rn2)  # the same bits
    # tol = 0 and room: the loop ends by its own "did not halve" rule (the restatement: at 3; the cap is no measured count)
    phiN, itsN, rnN = g.poisson_solve(rhs, tol=0.0, maxit=10)
    print(name, "tol = 0, maxit = 10: applications", itsN, "rn / (eps |rhs|)", rnN / (EPS * l2(rhs)))
    assert 2 <= itsN <= 5 and np.isfinite(rnN) and rnN <= rn1
    # a tolerance the first application meets: one application, and converged or not the count is the caller's
    assert g.poisson_solve(rhs, tol=1e-6 * l2(rhs), maxit=10)[1] == 1
    assert g.poisson_solver == "cg" and g.gauss_info()["cleans"] == 0
    g.close()


def test_the_refinement_matters_on_the_long_box(X, refine):
    """6x6x1024, kappa = 2.2e6: the restatement's first application leaves 6.2e3 eps |rhs|, its second 2.1e3.  Against the
    long-double solve phi2 is no worse than phi1, and the second application halves the residual -- the loop's own rule
    (the restatement has a factor 2.9)."""
    n, d, rhs, ref1, ref2 = refine["6x6x1024"]
    x = P.solve(rhs, n, d, 0.0, maxit=2, dtype=LD)[0]
    g = X.Context("ecsim", n, d, 0.5)
    phi1, _, rn1 = g.poisson_solve(rhs, tol=0.0, maxit=1)
    phi2, _, rn2 = g.poisson_solve(rhs, tol=0.0, maxit=2)
    e1, e2 = l2(phi1 - x), l2(phi2 - x)
    print("6x6x1024: |phi1 - x|", e1, "|phi2 - x|", e2, "the restatement's", l2(ref1 - x), l2(ref2 - x), "rn2 / rn1", rn2 / rn1)
    assert e2 <= e1
    assert rn2 <= 0.5 * rn1
    g.close()


# ---- 8. a clean that needs the refinement -------------------------------------------------------------------------------------
def test_direct_clean_of_a_long_box(X):
    """test_gpu_gauss.py's build on 6x6x1024 (its generators in its order: two lattice sorts, a background, E = 0) cleaned with
    "direct" at RTOL = 1e-12.  check_clean's dense solve is out of reach at 36 864 nodes: phi and the corrected field are
    compared with the refinement in np.longdouble on the same residual instead, by check_clean's bounds; its dense-free
    checks are kept as they are.  `iterations` is printed, not held from below: whether the device's first residual lands
    above 1e-12 |rho~| is not known beforehand (the restatement's does: 2 applications); section 7 pins the second."""
    n, d = P.LONG["6x6x1024"]
    seed, shape = 2, (n[2], n[1], n[0])
    rng = np.random.default_rng(1000 + seed)
    g = X.Context("ecsim", n, d, 0.5)
    for s in range(2):
        pts = TG.lattice_particles(n, d, 10 * seed + s)
        sid = g.add_sort(4, 1.0, (-1.0, 1.0)[s % 2], 1.0, capacity=2 * len(pts) + 1024)
        assert g.add_particles(sid, pts) == len(pts)
    bg = rng.normal(0.3, 1.0, shape)
    g.gauss_background(bg)
    E = np.zeros(shape + (3,))
    g.set_field(X.E, E)
    g.set_poisson_solver("direct")
    out = g.gauss_clean(X.E, rtol=RTOL, maxit=4000, want_phi=True)
    rho, parts = TG.charge(g, bg)
    res, mean = G.residual(E, rho, d)
    phi_ref = P.solve(res, n, d, 0.0, maxit=3, dtype=LD)[0]
    E1_ref = (E - G.grad(phi_ref, d)).astype(np.float64)
    phi_ref = phi_ref.astype(np.float64)
    E1 = g.get_field(X.E)
    lam = G.lambda_min(n, d)
    tol = RTOL * l2(rho - mean)
    gphi = l2(G.grad(out.phi, d))
    bound_E = out.after / np.sqrt(lam) + TG.K_ROUNDING * EPS * (l2(E) + gphi)
    bound_phi = out.after / lam + K_ROUNDING_PHI * EPS * kappa(n, d) * l2(phi_ref)
    after_np = l2(G.residual(E1, rho, d)[0])
    print("6x6x1024 clean: applications", out.iterations, "before", out.before, "after", out.after, "tol", tol, "|dE| / bound",
          l2(E1 - E1_ref) / bound_E, "|dphi| / bound", l2(out.phi - phi_ref) / bound_phi, "after numpy", after_np)
    assert 0 < out.iterations <= 3
    assert out.before == pytest.approx(l2(res), rel=1e-12) and out.mean == pytest.approx(mean, abs=1e-13)
    assert l2(E1 - E1_ref) <= bound_E
    assert l2(out.phi - phi_ref) <= bound_phi
    assert out.gphi == pytest.approx(gphi, rel=1e-12)
    assert abs(out.after - after_np) <= 8 * EPS * l2(TG.term_sum(E1, parts, mean, d))
    assert out.after <= tol
    info = g.gauss_info()
    assert info["cleans"] == 1 and info["iterations"] == info["last_iterations"] == out.iterations
    g.close()
