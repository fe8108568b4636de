"""The direct Poisson solve on the device (include/xpic_poisson.h, xpic_amd/csrc/poisson.hip, the direct path of gauss.hip)
against tests/poisson_ref.py's numpy restatement and against what tests/test_gpu_gauss.py and tests/test_gpu_es.py hold the
CG solve to: one application of the transform solve alone, the clean with "direct", the choice of the solver, the clean that
rides with the ecsim step, the electrostatic step, and the host mirror's "solver" key.

Shapes of xpic_poisson_apply (poisson_ref.SHAPES): three small ones, each axis in turn at 15, 16, 17 and 33 nodes -- on both
sides of the 16-wide instruction tile, and of the 16-deep staging tile of the summed index -- with the other two tiny, and
18x17x20.  The x extents 63 and 65 and the several-workgroup grid come with test_gpu_gauss.py's loads in section 2.
`iterations <= 2` is a condition, not a measurement: tests/test_poisson_ref.py shows that one application meets the
tolerance on every input here; the second is for what the device's own rounding may add."""
import numpy as np
import pytest

import es_ref as ES
import gauss_ref as G
import poisson_ref as P
import test_gpu_gauss as TG

pytestmark = pytest.mark.gpu
EPS = G.EPS
K_ROUNDING_PHI = TG.K_ROUNDING_PHI
RTOL = TG.RTOL


@pytest.fixture(scope="module")
def X():
    import xpic_amd

    return xpic_amd


@pytest.fixture(scope="module")
def inputs():
    """name -> (n, d, rhs, the restatement's phi): computed once, read by every test"""
    out = {}
    for name, (n, d, rhs) in P.gpu_inputs().items():
        phi = P.apply(rhs, n, d)
        rhs.setflags(write=False)
        phi.setflags(write=False)
        out[name] = (n, d, rhs, phi)
    return out


def l2(a):
    return float(np.sqrt((np.asarray(a, dtype=np.float64) ** 2).sum()))


def kappa(n, d):
    return sum(4.0 / v ** 2 for v in d) / G.lambda_min(n, d)


# ---- 1. one application against the restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(P.SHAPES))
def test_apply_matches_the_restatement(X, inputs, name):
    n, d, rhs, ref = inputs[name]
    g = X.Context("ecsim", n, d, 0.5)
    phi = g.poisson_apply(rhs)
    bound = K_ROUNDING_PHI * EPS * kappa(n, d) * l2(ref)
    print(name, "|dphi| / bound", l2(phi - ref) / bound, "mean / (N eps |phi|)", abs(phi.mean()) / (EPS * np.abs(phi).sum()),
          "|rhs - D G phi| / |rhs|", l2(rhs - P.lap(phi, d)) / l2(rhs))
    assert l2(phi - ref) <= bound
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
