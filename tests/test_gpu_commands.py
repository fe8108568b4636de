"""The per-step commands on the GPU (xpic_remove_particles, xpic_fields_damping, xpic_inject_particles, xpic_set_coils_field)
against tests/commands_ref.py on the same inputs, on one context and on three z-slabs, and inside a run of ECSIM steps
against the CPU oracle given the same edits."""
import math
import os
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import commands_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SORTS = ((8, 1.0, -1.0, 1.0), (5, 0.6, 2.0, 7.5))  # Np, n, q, m
GRID = ((12, 10, 8), (0.5, 0.4, 0.25))
GRID_P2 = ((12, 8, 8), (0.5, 0.5, 0.25))
BOTH = pytest.mark.parametrize("grid", [GRID, GRID_P2], ids=["general", "p2"])


def _L(n, d):
    return tuple(n[i] * d[i] for i in range(3))


def _ctx(n, d, seed=0, ppc=6, rank=0, nranks=1, capacity=None):
    import xpic_amd as X

    rng = np.random.default_rng(seed)
    g = X.Context("ecsim", n, d, 0.7, device=0, rank=rank, nranks=nranks)
    L = np.array(_L(n, d))
    for i, (Np, nn, q, m) in enumerate(SORTS):
        npart = ppc * n[0] * n[1] * n[2]
        s = g.add_sort(Np, nn, q, m, capacity=capacity or 4 * npart + 64)
        pts = np.empty((npart, 6))
        pts[:, :3] = rng.random((npart, 3)) * L
        pts[:, 3:] = rng.normal(0, 0.05 * (i + 1), (npart, 3))
        g.add_particles(s, pts)
    return g


def _shell(n, d, k=2):
    """a box k cells inside every face: removal empties a k-cell shell"""
    return {"name": "box", "min": tuple(k * d[i] for i in range(3)), "max": tuple((n[i] - k) * d[i] for i in range(3))}


def _cyl(n, d):
    L = _L(n, d)
    return {"name": "cylinder", "center": (0.5 * L[0], 0.5 * L[1], 0.5 * L[2]), "radius": 0.3 * min(L[0], L[1]),
            "height": 0.6 * L[2]}


def _rel(a, b, tol=1e-12):
    scale = max(abs(b), 1e-300)
    assert abs(a - b) <= tol * scale, (a, b)


@BOTH
@pytest.mark.parametrize("geom", ["shell", "cylinder"])
def test_remove_matches_ref(grid, geom):
    n, d = grid
    g = _ctx(n, d, seed=1)
    geometry = _shell(n, d) if geom == "shell" else _cyl(n, d)
    for s, (Np, nn, q, m) in enumerate(SORTS):
        pts, cells = g.particles(s)
        keep, k, e = R.remove(pts, cells, geometry, n, d, m, nn / Np)
        assert 0 < k < len(pts)
        removed, energy = g.remove_particles(s, geometry)
        assert removed == k
        _rel(energy, e)
        after, acells = g.particles(s)
        # the survivors, in their old order (cells in order, a cell's records as they were)
        assert np.array_equal(after, pts[keep]) and np.array_equal(acells, cells[keep])


def test_remove_nothing_touches_nothing():
    n, d = GRID
    g = _ctx(n, d, seed=2)
    whole = {"name": "box", "min": (0.0, 0.0, 0.0), "max": _L(n, d)}
    for s in range(2):
        pts, cells = g.particles(s)
        assert g.remove_particles(s, whole) == (0, 0.0)
        after, acells = g.particles(s)
        assert after.tobytes() == pts.tobytes() and acells.tobytes() == cells.tobytes()


@BOTH
@pytest.mark.parametrize("geom", ["box", "cylinder"])
def test_damping_matches_ref(grid, geom):
    import xpic_amd as X

    n, d = grid
    g = X.Context("ecsim", n, d, 0.7)
    rng = np.random.default_rng(3)
    E, B, B0 = (rng.normal(size=g.fshape()) for _ in range(3))
    for f, v in ((X.E, E), (X.B, B), (X.B0, B0)):
        g.set_field(f, v)
    L = _L(n, d)
    geometry = ({"name": "box", "min": (0.2 * L[0], 0.25 * L[1], 0.3 * L[2]), "max": (0.7 * L[0], 0.8 * L[1], 0.75 * L[2])}
                if geom == "box" else _cyl(n, d))
    e = g.fields_damping(geometry, 0.7)
    E2, B2, e_ref = R.damping(E, B, B0, geometry, 0.7, n, d)
    _rel(e, e_ref)
    for f, ref in ((X.E, E2), (X.B, B2)):
        got = g.get_field(f)
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.array_equal(g.get_field(X.B0), B0)
    assert not np.array_equal(E2, E)  # (something was damped)


def test_coils_matches_ref():
    import xpic_amd as X

    n, d = (9, 7, 6), (0.5, 0.4, 0.75)  # odd nx and ny: the Bz column (4, 3) lies on the axis, no Bx or By node does
    coils = [(1.0, 1.3, 2.0), (3.5, 0.9, -0.7)]
    g = X.Context("ecsim", n, d, 0.7)
    base = np.random.default_rng(4).normal(size=g.fshape())
    g.set_field(X.B0, base)
    g.set_coils_field(coils, X.B0)
    ref = base + R.coils_field(n, d, coils)
    got = g.get_field(X.B0)
    assert np.isfinite(ref).all()
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    # a Bx node on the axis (even nx, odd ny) is 0 / 0 as in the reference
    n2 = (8, 5, 4)
    g2 = X.Context("ecsim", n2, (0.5, 0.5, 0.5), 0.7)
    g2.set_coils_field([(1.0, 0.8, 1.0)], X.B0)
    f2, r2 = g2.get_field(X.B0), R.coils_field(n2, (0.5, 0.5, 0.5), [(1.0, 0.8, 1.0)])
    assert np.array_equal(np.isnan(f2), np.isnan(r2)) and np.isnan(f2[:, 2, 4, 0]).all()
    ok = np.isfinite(r2)
    assert np.abs(f2[ok] - r2[ok]).max() <= 1e-12 * np.abs(r2[ok]).max()


COORDS = {
    "box": lambda L: {"name": "CoordinateInBox", "min": (0.1 * L[0], 0.2 * L[1], 0.0), "max": (0.8 * L[0], 1.2 * L[1], 0.5 * L[2])},
    "cylinder": lambda L: {"name": "CoordinateInCylinder", "center": (0.5 * L[0], 0.5 * L[1], 0.5 * L[2]), "radius": 0.4 * L[0],
                           "height": 0.8 * L[2]},
    "point": lambda L: {"name": "PreciseCoordinate", "value": (0.3 * L[0], 0.6 * L[1], 0.45 * L[2])},
}
MOM_I = {"name": "MaxwellianMomentum", "T": (1.0, 2.0, 0.5), "drift": (0.01, 0.0, -0.02), "tov": True}
MOM_E = {"name": "MaxwellianMomentum", "T": (0.3, 0.3, 0.3)}


@BOTH
@pytest.mark.parametrize("coord", ["box", "cylinder", "point"])
def test_inject_matches_ref(grid, coord):
    n, d = grid
    g = _ctx(n, d, seed=5, ppc=3)
    L = _L(n, d)
    coordinate = COORDS[coord](L)
    mom_e = MOM_E if coord != "point" else {"name": "PreciseMomentum", "value": (0.1, -0.2, 0.05)}
    before = [g.particles(s) for s in range(2)]
    pairs, step, seed = 3000, 7, 11
    added, (ei, ee) = g.inject_particles(0, 1, pairs, step, coordinate, MOM_I, mom_e, seed=seed)
    r, pi, pe = R.inject_draws(pairs, step, seed, coordinate, MOM_I, mom_e, SORTS[0][3], SORTS[1][3])
    cells = R.local_cells(r, n, d)
    ok = cells >= 0
    assert added == int(ok.sum()) and 0 < added <= pairs and (coord != "box" or added < pairs)
    for s, p, e in ((0, pi, ei), (1, pe, ee)):
        Np, nn, q, m = SORTS[s]
        _rel(e, float(R.kinetic(p[ok], m, nn / Np).sum()))
        pts, pc = g.particles(s)
        assert len(pts) == len(before[s][0]) + added
        # cell by cell: the old records first, in their order, then the new ones
        ob, oc = before[s]
        new = np.concatenate([r[ok], p[ok]], axis=1)
        ncell = R.local_cells(new[:, :3], n, d)
        tails = []
        for c in np.unique(np.concatenate([oc, ncell])):
            got = pts[pc == c]
            old = ob[oc == c]
            assert np.array_equal(got[:len(old)], old)
            want = new[ncell == c]
            tail = got[len(old):]
            assert len(tail) == len(want)
            key = lambda a: a[np.lexsort(a.T[::-1])]  # noqa: E731
            assert np.abs(key(tail) - key(want)).max(initial=0) <= 1e-12
            tails.append(tail)
        _rel(e, float(R.kinetic(np.concatenate(tails)[:, 3:], m, nn / Np).sum()))  # the energy of the records read back


def test_inject_statistics():
    """a fixed seed, 2^18 pairs: the moments of the generators within 6 sigma; the two sorts share every coordinate"""
    n, d = (16, 16, 16), (0.5, 0.5, 0.5)
    import xpic_amd as X

    g = X.Context("ecsim", n, d, 0.7)
    for Np, nn, q, m in SORTS:
        g.add_sort(Np, nn, q, m, capacity=1 << 19)
    L = _L(n, d)
    c, Rr, h = (0.5 * L[0], 0.5 * L[1], 0.5 * L[2]), 3.0, 5.0
    coordinate = {"name": "CoordinateInCylinder", "center": c, "radius": Rr, "height": h}
    T = (1.0, 4.0, 0.25)
    N = 1 << 18
    added, _ = g.inject_particles(0, 1, N, 3, coordinate, {"name": "MaxwellianMomentum", "T": T}, MOM_E, seed=2024)
    assert added == N
    pi, _ = g.particles(0)
    pe, _ = g.particles(1)

    def within6(x, mean, var):
        assert abs(x.mean() - mean) <= 6 * math.sqrt(var / len(x)), (x.mean(), mean)

    m = SORTS[0][3]
    for a in range(3):
        s2 = T[a] * m / R.MEC2  # <p^2> of sin(2 pi u) sqrt(-2 s2 log u): s2; variance of p^2: 2 s2^2
        within6(pi[:, 3 + a], 0.0, s2)
        within6(pi[:, 3 + a] ** 2, s2, 2 * s2 * s2)
    r2 = (pi[:, 0] - c[0]) ** 2 + (pi[:, 1] - c[1]) ** 2
    within6(r2, Rr * Rr / 2, Rr ** 4 / 12)                  # r^2 uniform on [0, R^2]
    within6(pi[:, 2], c[2], h * h / 12)                      # z uniform over the height
    within6((pi[:, 2] - c[2]) ** 2, h * h / 12, h ** 4 / 180)
    key = lambda a: a[np.lexsort(a.T[::-1])]  # noqa: E731
    assert np.array_equal(key(pi[:, :3]), key(pe[:, :3]))  # the pairs share their coordinates


def test_capacity_overflow_raises():
    import xpic_amd as X

    n, d = GRID
    g = X.Context("ecsim", n, d, 0.7)
    for Np, nn, q, m in SORTS:
        g.add_sort(Np, nn, q, m, capacity=1000)
    L = _L(n, d)
    box = {"name": "CoordinateInBox", "min": tuple(0.1 * v for v in L), "max": tuple(0.9 * v for v in L)}
    assert g.inject_particles(0, 1, 900, 0, box, MOM_I, MOM_E)[0] == 900
    before = [g.particles(s)[0] for s in range(2)]
    with pytest.raises(X.XpicError, match="capacity"):
        g.inject_particles(0, 1, 200, 1, box, MOM_I, MOM_E)
    for s in range(2):
        assert np.array_equal(g.particles(s)[0], before[s])


def _commands(ctx, n, d):
    """remove, inject, damp on a context (or a slab of one) -> the returned values"""
    L = _L(n, d)
    out = [ctx.remove_particles(0, _shell(n, d, 1)), ctx.remove_particles(1, _cyl(n, d))]
    out.append(ctx.inject_particles(0, 1, 5000, 4, COORDS["cylinder"](L), MOM_I, MOM_E, seed=3))
    out.append(ctx.fields_damping(_cyl(n, d), 0.4))
    ctx.set_coils_field([(0.3 * L[2], 1.1, 1.0), (0.7 * L[2], 0.8, 2.0)])
    return out


def _fields(ctx, n, d, nranks=1, rank=0):
    import xpic_amd as X

    rng = np.random.default_rng(8)
    full = [rng.normal(size=(n[2], n[1], n[0], 3)) for _ in range(3)]
    nzl = n[2] // nranks
    for f, v in zip((X.E, X.B, X.B0), full):
        ctx.set_field(f, v[rank * nzl:(rank + 1) * nzl])


def test_slabs_equal_one_context():
    import xpic_amd as X
    from xpic_amd.parallel import ThreadRing

    n, d, nr = (8, 6, 24), (0.5, 0.4, 0.25), 3
    one = _ctx(n, d, seed=9)
    _fields(one, n, d)
    rvals = _commands(one, n, d)
    rparts = [one.particles(s)[0] for s in range(2)]
    rflds = [one.get_field(f) for f in (X.E, X.B, X.B0)]
    ring = ThreadRing(nr)
    res, errs = [None] * nr, []

    def rank_main(r):
        try:
            ctx = _ctx(n, d, seed=9, rank=r, nranks=nr)
            ring.attach(ctx, r)
            _fields(ctx, n, d, nr, r)
            vals = _commands(ctx, n, d)
            res[r] = (vals, [ctx.particles(s)[0] for s in range(2)], [ctx.get_field(f) for f in (X.E, X.B, X.B0)])
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
    for r in range(nr):
        vals = res[r][0]
        assert vals[0][0] == rvals[0][0] and vals[1][0] == rvals[1][0] and vals[2][0] == rvals[2][0]
        for a, b in ((vals[0][1], rvals[0][1]), (vals[1][1], rvals[1][1]), (vals[2][1][0], rvals[2][1][0]),
                     (vals[2][1][1], rvals[2][1][1]), (vals[3], rvals[3])):
            _rel(a, b)
    key = lambda a: a[np.lexsort(a.T[::-1])]  # noqa: E731
    for s in range(2):
        got = np.concatenate([res[r][1][s] for r in range(nr)])
        assert np.array_equal(key(got), key(rparts[s]))  # exactly the same records
    for i in range(3):
        got = np.concatenate([res[r][2][i] for r in range(nr)])
        assert np.abs(got - rflds[i]).max() <= 1e-13 * np.abs(rflds[i]).max()


def _canon(pts, cells):
    key = np.lexsort((pts[:, 5], pts[:, 4], pts[:, 3], pts[:, 2], pts[:, 1], pts[:, 0], cells))
    return pts[key], cells[key]


@pytest.mark.parametrize("fill_kernel", [0, 1])
@pytest.mark.parametrize("fused", [1, 0])
def test_step_state_after_commands(oracle, fill_kernel, fused):
    """ECSIM steps twice, then removal, an injection of exactly as many records as were removed, and damping; then two more
    steps.  The oracle is given the same edits (clear / add_particles / set_field).  A re-binning that took the second
    push's pre-binning of the old records for the new ones (same count) would send particles to wrong cells."""
    import xpic_amd as X

    n, d = GRID_P2
    dt = 0.7
    rng = np.random.default_rng(12)
    o = oracle.OracleSim("ecsim", n, d, dt)
    g = X.Context("ecsim", n, d, dt)
    g.set_preconditioner(0)
    g.set_fill_kernel(fill_kernel)
    g.set_fused_rebin(fused)
    Lv = np.array(_L(n, d))
    N = n[0] * n[1] * n[2]
    for (Np, nn, q, m) in ((8, 1.0, -1.0, 1.0), (8, 1.0, 1.0, 1836.0)):
        so, sg = o.add_sort(Np, nn, q, m), g.add_sort(Np, nn, q, m, capacity=24 * N)
        pts = np.empty((6 * N, 6))
        pts[:, :3] = rng.random((6 * N, 3)) * Lv
        pts[:, 3:] = rng.normal(0, 0.03, (6 * N, 3))
        assert o.add_particles(so, pts) == g.add_particles(sg, pts)
    for name, fid in (("E", X.E), ("B", X.B)):
        F = rng.normal(0, 0.05, o.fshape()) + (np.array([0.0, 0.0, 0.2]) if name == "B" else 0.0)
        o.set_field(name, F)
        g.set_field(fid, F)
    b0 = np.zeros(o.fshape()) + np.array([0.0, 0.0, 0.2])
    o.set_field("B0", b0)
    g.set_field(X.B0, b0)
    for s in (o, g):
        s.set_tolerances(1e-10, 1e-50, 300)
    for _ in range(2):
        o.step(), g.step()
    n0 = g.count(0)
    removed, _ = g.remove_particles(0, _shell(n, d, 1))
    assert removed > 0
    inner = {"name": "CoordinateInBox", "min": tuple(0.1 * Lv), "max": tuple(0.9 * Lv)}
    added, _ = g.inject_particles(0, 1, removed, 2, inner, {"name": "MaxwellianMomentum", "T": (0.4, 0.4, 0.4)},
                                  {"name": "MaxwellianMomentum", "T": (0.4, 0.4, 0.4)}, seed=5)
    assert added == removed and g.count(0) == n0  # sort 0: the same count, other records
    g.fields_damping({"name": "cylinder", "center": tuple(0.5 * Lv), "radius": 0.3 * Lv[0], "height": 0.8 * Lv[2]}, 0.5)
    for s in range(2):
        o.clear(s)
        assert o.add_particles(s, g.particles(s)[0]) == g.count(s)
    for name, fid in (("E", X.E), ("B", X.B)):
        o.set_field(name, g.get_field(fid))
    for _ in range(2):
        io, ig = o.step(), g.step()
        assert io > 0 and abs(io - ig) <= 1
        assert np.allclose(o.energy(), g.energy(), rtol=1e-7, atol=1e-14)
        for name, fid in (("E", X.E), ("B", X.B)):
            a, b = o.get_field(name), g.get_field(fid)
            assert np.abs(a - b).max() <= 1e-6 * np.abs(a).max()
    for s in range(2):
        assert o.count(s) == g.count(s)
        assert np.array_equal(_canon(*o.particles(s))[1], _canon(*g.particles(s))[1])
