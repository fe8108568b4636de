"""xpic_moment (DistributionMoment, all six moments, the reference's region rule) and xpic_velocity_distribution
(VelocityDistribution) on the GPU against tests/moments_ref.py applied to the particles the context holds."""
import os
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import moments_ref as M  # noqa: E402

pytestmark = pytest.mark.gpu

SORTS = ((8, 1.0, -1.0, 1.0), (5, 0.6, 2.0, 7.5))  # Np, n, q, m: two sorts with different q, m and n/Np


def _ctx(scheme, n, d, dt, seed=0, ppc=None, rank=0, nranks=1):
    import xpic_amd as X

    rng = np.random.default_rng(seed)
    g = X.Context(scheme, n, d, dt, device=0, rank=rank, nranks=nranks)
    L = np.array(n) * np.array(d)
    pts_all = []
    for i, (Np, nn, q, m) in enumerate(SORTS):
        npart = (ppc or Np) * n[0] * n[1] * n[2]
        s = g.add_sort(Np, nn, q, m, capacity=2 * npart + 64)
        pts = np.empty((npart, 6))
        pts[:, :3] = rng.random((npart, 3)) * L
        pts[:, 3:] = rng.normal(0, 0.05 * (i + 1), (npart, 3))
        pts[0, :3] = [0.5 * L[0], 0.5 * L[1], 0.3 * L[2]]  # exactly on the cylinder axis
        g.add_particles(s, pts)
        pts_all.append(pts)
    if nranks == 1:
        B = np.zeros(g.fshape()) + np.array([0.05, 0.0, 0.3])  # B0 != 0
        for fid in (X.B, X.B0):
            g.set_field(fid, B)
    return g, pts_all


def _ref_moment(g, s, name, region=None):
    Np, nn, q, m = SORTS[s]
    pts, cells = g.particles(s)
    return M.moment(name, pts, cells, q, m, nn / Np, g.n, g.d, region)


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    scale = np.abs(b).max()
    assert scale > 0
    err = np.abs(a - b).max()
    assert err <= tol * scale, (err, scale)


def _regions(n):
    return [None,                                       # the whole box
            (2, 3, 1, n[0] - 5, n[1] - 4, n[2] - 3),    # an interior sub-box
            (0, 0, n[2] // 2, n[0], n[1], 1),           # a one-cell "2D" plane
            (0, 0, 2, n[0], n[1], n[2] // 2)]           # x and y in full, z in part


@pytest.mark.parametrize("scheme", ["basic", "ecsim"])
def test_all_moments_and_regions(scheme, oracle):
    n, d = (12, 10, 8), (0.5, 0.4, 0.25)
    g, pts = _ctx(scheme, n, d, 0.1 if scheme == "basic" else 1.0, seed=1)
    for t in range(2):
        if t:
            g.step()
            g.step()
        for s in range(2):
            for reg in _regions(n):
                for name in M.MOMENTS:
                    _close(g.moment(s, name, reg), _ref_moment(g, s, name, reg))
    # the region rule is exercised: a sub-region is not a crop of the whole box
    full = g.moment(0, "density")
    sub = g.moment(0, "density", _regions(n)[1])
    reg = _regions(n)[1]
    crop = np.zeros_like(full)
    sl = (slice(reg[2], reg[2] + reg[5]), slice(reg[1], reg[1] + reg[4]), slice(reg[0], reg[0] + reg[3]))
    crop[sl] = full[sl]
    assert np.abs(sub - crop).max() > 1e-3 * np.abs(full).max()
    plane = g.moment(1, "current", _regions(n)[2])
    assert np.abs(plane[n[2] // 2]).max() > 0 and np.abs(np.delete(plane, n[2] // 2, axis=0)).max() == 0


def test_density_agrees_with_moment_density_and_the_cpu_model(oracle):
    n, d = (12, 10, 8), (0.5, 0.4, 0.25)
    g, pts = _ctx("ecsim", n, d, 1.0, seed=2)
    o = oracle.OracleSim("ecsim", n, d, 1.0)
    for s, (Np, nn, q, m) in enumerate(SORTS):
        so = o.add_sort(Np, nn, q, m)
        assert o.add_particles(so, pts[s]) == g.count(s)
        mine = g.moment(s, "density")[..., 0]
        _close(mine, g.moment_density(s))
        _close(mine, o.moment_density(so))


def test_pencils_longer_than_a_tile():
    """x-pencils of 300 cells: five tiles of at most 64 cells, the last one ragged; 6 x 6 rows and planes"""
    n, d = (300, 6, 6), (0.5, 0.4, 0.25)
    g, _ = _ctx("ecsim", n, d, 1.0, seed=3, ppc=3)
    for s in range(2):
        for reg in (None, (61, 1, 0, 130, 4, 6), (0, 0, 5, 300, 6, 1)):
            for name in ("density", "current", "momentum_flux_cyl"):
                _close(g.moment(s, name, reg), _ref_moment(g, s, name, reg))


def test_sums_at_128_cubed():
    """128^3 x 16 per cell: the density sums to N n/Np, the current to q n/Np sum v (sum v from MomentumConservation's
    P = m/Np sum v, the 2nd-order shape's weights summing to 1)"""
    import xpic_amd as X

    n, d = (128, 128, 128), (0.5, 0.5, 0.5)
    g = X.Context("ecsim", n, d, 1.0, device=0)
    Np, nn, q, m = 16, 1.3, -1.0, 1.0
    s = g.add_sort(Np, nn, q, m, capacity=16 * 128 ** 3 + 1024)
    g.load_synthetic(s, 16, 0.05, seed=5, drift=(0.01, -0.02, 0.03))
    N = g.count(s)
    rho = g.moment(s, "density")
    assert abs(rho.sum() - N * nn / Np) <= 1e-10 * N * nn / Np
    j = g.moment(s, "current").sum(axis=(0, 1, 2))
    sv = g.momentum()[0, :3] * Np / m
    exp = q * nn / Np * sv
    assert np.all(np.abs(j - exp) <= 1e-9 * np.abs(exp).max()), (j, exp)


GEOMS = (("box", {"name": "box", "min": (0.5, 0.4, 0.25), "max": (5.0, 3.2, 1.5)}),
         ("cylinder", {"name": "cylinder", "center": (3.0, 2.0, 1.0), "radius": 1.7, "height": 1.2}))


@pytest.mark.parametrize("geom", [g[0] for g in GEOMS])
def test_velocity_distribution(geom):
    geometry = dict(GEOMS)[geom]
    n, d = (12, 10, 8), (0.5, 0.4, 0.25)
    g, _ = _ctx("ecsim", n, d, 1.0, seed=4)
    g.step()
    # bounds narrower than the spread (particles are dropped), dvx != dvy and vx_min != vy_min: the reference's sizes come
    # from the x axis alone; 20^2 bins take the LDS path, 190^2 the global one
    cases = (((-0.06, -0.02), (0.04, 0.09), (0.005, 0.007)), ((-0.095, -0.03), (0.095, 0.2), (0.001, 0.0013)),
             # ties of ROUND_STEP(vx_min, dvx): -2.5 and -0.5 round away from zero, to -3 and -1 (not to even)
             ((-1.0, -0.3), (1.0, 0.3), (0.4, 0.1)), ((-0.05, -0.2), (0.35, 0.2), (0.1, 0.03)))
    seen_lds = seen_global = False
    for s in range(2):
        Np, nn, q, m = SORTS[s]
        pts, cells = g.particles(s)
        for proj in ("vx_vy", "vz_vxy", "vr_vphi"):
            for vmin, vmax, dv in cases:
                h, v0 = g.velocity_distribution(s, proj, geometry, vmin, vmax, dv)
                r, rv0 = M.velocity_distribution(proj, geometry, pts, cells, nn / Np, n, d, vmin, vmax, dv)
                assert v0 == rv0 and h.shape == r.shape == (M.vsizes(vmin, vmax, dv)[1],) * 2
                if vmin[0] == -1.0:
                    assert v0 == (-3, -3) and h.shape == (5, 5)
                if vmin[0] == -0.05:
                    assert v0 == (-1, -1) and h.shape == (4, 4)
                _close(h, r)
                assert r.sum() < 0.999 * len(pts) * nn / Np  # some were dropped
                seen_lds |= h.size <= 8192
                seen_global |= h.size > 8192
    assert seen_lds and seen_global


def test_records_away_from_their_cells():
    """Positions moved by the phase entry point ecsim_first_push, cells not yet re-binned: a record counts by its STORAGE
    cell (distribution_moment.cpp:172-180) and deposits where it now is.  Records whose corners leave their block's tile
    take the second launch (profile section "moment_stray"); the storage cells are the ones the records had before the
    move (k_move keeps the order)."""
    n, d = (12, 10, 8), (0.5, 0.4, 0.25)
    g, _ = _ctx("ecsim", n, d, 2.0, seed=8)
    before = [g.particles(s) for s in range(2)]
    for s in range(2):
        g.ecsim_first_push(s)
    g.profile_enable(True)
    g.profile_reset()
    moved = 0
    for s in range(2):
        pts = g.particles(s)[0]
        cells = before[s][1]
        assert np.array_equal(pts[:, 3:], before[s][0][:, 3:])  # the same records in the same order
        now = np.floor(pts[:, :3] / np.array(d)).astype(np.int64)
        was = np.stack([cells % n[0], (cells // n[0]) % n[1], cells // (n[0] * n[1])], axis=1)
        moved += int(np.sum(np.abs(now - was).max(axis=1) >= 2))
        Np, nn, q, m = SORTS[s]
        for reg in _regions(n):
            for name in ("density", "current", "momentum_flux_cyl"):
                ref = M.moment(name, pts, cells, q, m, nn / Np, n, d, reg)
                _close(g.moment(s, name, reg), ref)
    assert moved > 0
    assert g.profile_get("moment_stray")[0] > 0


@pytest.mark.parametrize("nr", [2, 3])
def test_slabs_equal_one_rank(nr):
    from xpic_amd.parallel import ThreadRing

    n, d = (10, 8, 36), (0.5, 0.4, 0.25)
    regs = (None, (1, 2, 10, 6, 5, 9), (0, 0, 12, 10, 8, 1), (0, 0, 5, 10, 8, 20))
    geometry = dict(GEOMS)["cylinder"]
    vcase = ((-0.06, -0.02), (0.04, 0.09), (0.005, 0.007))

    def run(ctx):
        mom = {(s, name, i): ctx.moment(s, name, reg) for s in range(2) for name in M.MOMENTS for i, reg in enumerate(regs)}
        vd = [ctx.velocity_distribution(s, p, geometry, *vcase)[0] for s in range(2) for p in ("vx_vy", "vr_vphi")]
        return mom, vd

    ref, _ = _ctx("ecsim", n, d, 1.0, seed=6)
    rmom, rvd = run(ref)
    ring = ThreadRing(nr)
    res, errs = [None] * nr, []

    def rank_main(r):
        try:
            ctx, _ = _ctx("ecsim", n, d, 1.0, seed=6, rank=r, nranks=nr)
            ring.attach(ctx, r)
            res[r] = run(ctx)
            ctx.close()
        except BaseException as e:  # noqa: BLE001 -- release the other ranks, report below
            errs.append((r, repr(e)))
            ring.bar.abort()

    th = [threading.Thread(target=rank_main, args=(r,)) for r in range(nr)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not errs and all(x is not None for x in res), errs
    for k, v in rmom.items():
        _close(np.concatenate([x[0][k] for x in res], axis=0), v)
    for r in range(nr):
        for a, b in zip(res[r][1], rvd):
            _close(a, b)


def test_no_side_effects(oracle):
    """Every moment and histogram leaves E, B and the particles bit for bit as they were; the next step still agrees with
    the CPU model."""
    import xpic_amd as X

    n, d, dt = (12, 10, 8), (0.5, 0.4, 0.25), 1.0
    g, pts = _ctx("ecsim", n, d, dt, seed=7)
    o = oracle.OracleSim("ecsim", n, d, dt)
    for s, (Np, nn, q, m) in enumerate(SORTS):
        so = o.add_sort(Np, nn, q, m)
        o.add_particles(so, pts[s])
    B = np.zeros(g.fshape()) + np.array([0.05, 0.0, 0.3])
    o.set_field("B", B)
    o.set_field("B0", B)
    for sim in (o, g):
        sim.set_tolerances(1e-10, 1e-50, 200)
    assert o.step() > 0 and g.step() > 0

    def state():
        return [g.get_field(X.E), g.get_field(X.B)] + [a for s in range(2) for a in g.particles(s)]

    before = state()
    for s in range(2):
        for name in M.MOMENTS:
            for reg in _regions(n):
                g.moment(s, name, reg)
        for proj in ("vx_vy", "vz_vxy", "vr_vphi"):
            for geom in GEOMS:
                g.velocity_distribution(s, proj, geom[1], (-0.1, -0.1), (0.1, 0.1), (0.01, 0.02))
                g.velocity_distribution(s, proj, geom[1], (-0.1, -0.1), (0.1, 0.1), (0.001, 0.002))
    after = state()
    for a, b in zip(before, after):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert o.step() > 0 and g.step() > 0
    for name, fid in (("E", X.E), ("B", X.B)):
        a, b = o.get_field(name), g.get_field(fid)
        assert np.abs(a - b).max() <= 1e-6 * np.abs(a).max(), name
    for s in range(2):
        assert o.count(s) == g.count(s)
