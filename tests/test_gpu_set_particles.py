"""SetParticles on the GPU (xpic_set_particles, include/xpic_set_particles.h) against tests/set_particles_ref.py on the same
inputs: every coordinate generator with every momentum generator, the guarantees (a) - (f) of the header, three z-slabs,
the generators' statistics, and ECSIM steps after a device load.  Grids, sorts and the slab run are test_gpu_commands.py's."""
import ctypes as C
import math
import os
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import set_particles_ref as S  # noqa: E402
import test_gpu_commands as T  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 257, 3000)
COORDS = {
    "box": T.COORDS["box"],            # reaches beyond the domain in y: added < n
    "cylinder": T.COORDS["cylinder"],
    "annulus": lambda L: {"name": "CoordinateOnAnnulus", "center": (0.5 * L[0], 0.5 * L[1], 0.5 * L[2]), "inner_r": 0.2 * L[0],
                          "outer_r": 0.45 * L[1], "height": 0.8 * L[2]},
    "point": lambda L: {"name": "PreciseCoordinate", "value": (0.31 * L[0], 0.63 * L[1], 0.47 * L[2])},
}
MOMENTA = {
    "precise": lambda L: {"name": "PreciseMomentum", "value": (0.1, -0.2, 0.05)},
    "maxwell": lambda L: T.MOM_I,
    "cosine": lambda L: {"name": "MaxwellCosinePerturbation", "T": (1.0, 2.0, 0.5), "amplitude": (0.5, 0.25, 0.125),
                         "wave_number": (2.0, 1.0, 3.0), "min": (0.0, 0.0, 0.0), "max": tuple(L)},
    "angular": lambda L: {"name": "AngularMomentum", "T": (1.0, 2.0, 0.5), "drift": (0.3, 0.2, -0.1),
                          "center": (0.5 * L[0], 0.5 * L[1], 0.0)},
}


def key(a):
    return a[np.lexsort(a.T[::-1])]


def canon(pts, cells):
    k = np.lexsort((pts[:, 5], pts[:, 4], pts[:, 3], pts[:, 2], pts[:, 1], pts[:, 0], cells))
    return pts[k], cells[k]


def check_added(before, after, want, want_cells, tol):
    """cell by cell: the old records first and bit-equal, then the new ones as a sorted multiset within tol -> the tails"""
    (ob, oc), (pts, pc) = before, after
    assert len(pts) == len(ob) + len(want)
    tails = []
    for c in np.unique(np.concatenate([oc, want_cells])):
        got, old = pts[pc == c], ob[oc == c]
        assert got[:len(old)].tobytes() == old.tobytes()
        new, tail = want[want_cells == c], got[len(old):]
        assert len(tail) == len(new)
        assert np.abs(key(tail) - key(new)).max(initial=0) <= tol
        tails.append(tail)
    return np.concatenate(tails) if tails else np.zeros((0, 6))


@T.BOTH
@pytest.mark.parametrize("mom", list(MOMENTA))
@pytest.mark.parametrize("coord", list(COORDS))
def test_set_particles_matches_ref(grid, coord, mom):
    """every size of SIZES, one call after the other on a sort that holds records: (a), `added` exact, energy at 1e-12"""
    n, d = grid
    g = T._ctx(n, d, seed=5, ppc=3)
    L = T._L(n, d)
    cgen, mgen = COORDS[coord](L), MOMENTA[mom](L)
    sort = 1
    Np, nn, q, m = T.SORTS[sort]
    other = g.particles(0)[0]
    for step, num in enumerate(SIZES):
        seed = 11 + step
        r, _ = S.draws(num, step, seed, cgen, mgen, m)
        assert S.face_distance(r, d) > 1e-9  # (no coordinate that a rounding could move across a face)
        want, wcells, k, e = S.set_particles(num, step, seed, cgen, mgen, m, nn / Np, n, d)
        before = g.particles(sort)
        added, energy = g.set_particles(sort, num, cgen, mgen, step=step, seed=seed)
        assert added == k <= num and (num < 63 or 0 < added) and (coord != "box" or num < 63 or added < num)
        T._rel(energy, e)
        tail = check_added(before, g.particles(sort), want, wcells, 1e-12)
        T._rel(energy, float(S.kinetic(tail[:, 3:], m, nn / Np).sum()))  # the energy of the records read back
    assert g.particles(0)[0].tobytes() == other.tobytes()  # the other sort is left alone


@T.BOTH
def test_angular_momentum_on_the_axis(grid):
    """a precise coordinate on the axis: 1 / r is infinite, the momentum is (0, 0, pz) plus the thermal part"""
    n, d = grid
    g = T._ctx(n, d, seed=5, ppc=3)
    L = T._L(n, d)
    cgen = COORDS["point"](L)
    mgen = dict(MOMENTA["angular"](L), center=cgen["value"])
    Np, nn, q, m = T.SORTS[0]
    want, wcells, k, e = S.set_particles(65, 2, 3, cgen, mgen, m, nn / Np, n, d)
    assert k == 65 and (want[:, 3:5] >= 0).all() and np.isfinite(want).all()
    before = g.particles(0)
    added, energy = g.set_particles(0, 65, cgen, mgen, step=2, seed=3)
    assert added == 65
    T._rel(energy, e)
    tail = check_added(before, g.particles(0), want, wcells, 1e-12)
    assert np.isfinite(tail).all()
    # beside the axis the drift turns about it
    off = dict(cgen, value=(cgen["value"][0] + 0.01, cgen["value"][1], cgen["value"][2]))
    want, wcells, k, e = S.set_particles(3, 3, 3, off, dict(mgen, T=(0.0, 0.0, 0.0)), m, nn / Np, n, d)
    before = g.particles(0)
    g.set_particles(0, 3, off, dict(mgen, T=(0.0, 0.0, 0.0)), step=3, seed=3)
    tail = check_added(before, g.particles(0), want, wcells, 1e-12)
    assert np.abs(tail[:, 3:] - [0.0, 0.2, -0.1]).max() <= 1e-12


def test_calls_compose_and_chunk_changes_nothing():
    """(b) 257 = 100 + 157 through particle0, (c) chunk = 64 against the default: the same records in every cell"""
    n, d = T.GRID
    L = T._L(n, d)
    for coord, mom in (("annulus", "cosine"), ("box", "angular")):
        cgen, mgen = COORDS[coord](L), MOMENTA[mom](L)
        one, two, chunked = (T._ctx(n, d, seed=6, ppc=3) for _ in range(3))
        a, ea = one.set_particles(1, 257, cgen, mgen, step=4, seed=21)
        b1, e1 = two.set_particles(1, 100, cgen, mgen, step=4, seed=21)
        b2, e2 = two.set_particles(1, 157, cgen, mgen, step=4, seed=21, particle0=100)
        c, ec = chunked.set_particles(1, 257, cgen, mgen, step=4, seed=21, chunk=64)
        assert a == b1 + b2 == c and 0 < b1 < a
        T._rel(e1 + e2, ea)
        T._rel(ec, ea)
        ref = canon(*one.particles(1))
        for g in (two, chunked):
            got = canon(*g.particles(1))
            assert got[0].tobytes() == ref[0].tobytes() and np.array_equal(got[1], ref[1])


@pytest.mark.parametrize("coord", ["box", "cylinder", "point"])
def test_records_equal_injects_ionized_sort(coord):
    """(d) the generators inject_particles has: its ionized sort's records, bit for bit, as sorted multisets per cell"""
    n, d = T.GRID
    L = T._L(n, d)
    cgen = COORDS[coord](L)
    inj, dev = T._ctx(n, d, seed=7, ppc=3), T._ctx(n, d, seed=7, ppc=3)
    for step, mom in enumerate(("maxwell", "precise")):
        mgen = MOMENTA[mom](L)
        added, (ei, _) = inj.inject_particles(0, 1, 257, step, cgen, mgen, T.MOM_E, seed=13)
        got, e = dev.set_particles(0, 257, cgen, mgen, step=step, seed=13)
        assert got == added > 0
        T._rel(e, ei)
        a, b = canon(*inj.particles(0)), canon(*dev.particles(0))
        assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])


def _params(X, L, **over):
    p = X.SetParticlesParams()
    p.coordinate, p.momentum = X.COORDINATES["CoordinateOnAnnulus"], X.MOMENTA["MaxwellCosinePerturbation"]
    p.geom[:] = [0.5 * L[0], 0.5 * L[1], 0.5 * L[2], 0.5, 1.5, 1.0, 0.0]
    p.T[:] = [1.0, 1.0, 1.0]
    p.amplitude[:] = [0.1, 0.1, 0.1]
    p.wave_number[:] = [1.0, 1.0, 1.0]
    p.box6[:] = [0.0, 0.0, 0.0] + list(L)
    p.seed = 3
    for k, v in over.items():
        if isinstance(v, tuple):
            getattr(p, k)[v[0]] = v[1]
        else:
            setattr(p, k, v)
    return p


def _refused(g, sort, p, n=10, particle0=0, null=None):
    """the raw call -> the library's message; a refused call returns a non-zero code"""
    added, energy = C.c_int64(-7), C.c_double(-7.0)
    args = [g.h, sort, None if null == "params" else C.byref(p), n, particle0, 0,
            None if null == "added" else C.byref(added), None if null == "energy" else C.byref(energy)]
    rc = g.L.xpic_set_particles(*args)
    assert rc != 0, "the call was not refused"
    msg = g.L.xpic_last_error().decode()
    assert "xpic_set_particles" in msg, msg
    return msg


def test_refusals_change_nothing():
    """(e) every refusal names the entry point and leaves records and counts as they were"""
    import xpic_amd as X

    n, d = T.GRID
    L = T._L(n, d)
    npart = 3 * n[0] * n[1] * n[2]
    g = T._ctx(n, d, seed=8, ppc=3, capacity=npart + 100)
    bad = g.add_sort(4, 1.0, 1.0, float("nan"), capacity=64)  # (add_sort refuses m == 0 and Np <= 0; a NaN mass gets by)
    before = [g.particles(s) for s in range(2)]
    nan, inf = float("nan"), float("inf")
    cases = [
        dict(sort=2 + 1), dict(sort=-1), dict(null="params"), dict(null="added"), dict(null="energy"),
        dict(over=dict(coordinate=4)), dict(over=dict(coordinate=-1)), dict(over=dict(momentum=4)), dict(over=dict(momentum=-1)),
        dict(n=-1), dict(particle0=-1), dict(over=dict(chunk=-1)), dict(n=1 << 62, particle0=(1 << 63) - 1),
        dict(over=dict(geom=(4, 0.4))), dict(over=dict(geom=(3, -0.1))),  # outer_r < inner_r, a negative inner_r
        dict(over=dict(geom=(0, nan))), dict(over=dict(geom=(5, inf))), dict(over=dict(geom=(4, inf))),
        dict(over=dict(coordinate=2, geom=(3, -1.0))), dict(over=dict(T=(1, nan))), dict(over=dict(box6=(3, 0.0))),
        dict(over=dict(momentum=3, center=(0, nan))), dict(over=dict(momentum=1, value=(2, inf))),
        dict(sort=bad),
    ]
    for case in cases:
        p = _params(X, L, **case.get("over", {}))
        _refused(g, case.get("sort", 1), p, case.get("n", 10), case.get("particle0", 0), case.get("null"))
    # capacity: 100 free slots, 200 particles inside the domain, in chunks of 64 -- the overflow shows in the fourth chunk
    # only, and nothing may have been written by then
    msg = _refused(g, 1, _params(X, L, chunk=64), n=200)
    assert "capacity" in msg
    with pytest.raises(X.XpicError, match="xpic_set_particles.*capacity"):
        g.set_particles(1, 200, COORDS["annulus"](L), MOMENTA["cosine"](L), chunk=64)
    for s in range(2):
        pts, cells = g.particles(s)
        assert pts.tobytes() == before[s][0].tobytes() and cells.tobytes() == before[s][1].tobytes()
    assert g.count(bad) == 0
    # and the sort still takes what fits, after the refusals
    assert g.set_particles(1, 100, COORDS["annulus"](L), MOMENTA["cosine"](L), chunk=64)[0] == 100
    assert g.count(1) == npart + 100


def test_zero_particles_launch_nothing():
    """(f)"""
    n, d = T.GRID
    L = T._L(n, d)
    g = T._ctx(n, d, seed=9, ppc=3)
    before = g.particles(1)
    g.profile_enable()
    assert g.set_particles(1, 0, COORDS["box"](L), MOMENTA["maxwell"](L), seed=5, particle0=77) == (0, 0.0)
    assert g.profile_get("cmd_set_particles")[0] == 0
    after = g.particles(1)
    assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes()
    assert g.set_particles(1, 1, COORDS["point"](L), MOMENTA["maxwell"](L), seed=5)[0] == 1
    assert g.profile_get("cmd_set_particles")[0] == 1


def test_particles_number_is_the_builders():
    n, d = T.GRID
    L = T._L(n, d)
    g = T._ctx(n, d, seed=9, ppc=1)
    for sort, (Np, nn, q, m) in enumerate(T.SORTS):
        for coord in COORDS:
            cgen = COORDS[coord](L)
            assert g.particles_number(sort, cgen) == S.particles_number(cgen, Np, d, L), coord
    # truncated, not rounded: 1.55 cells of Np = 5 are 7.75 particles; an annulus whose count has a fraction above one half
    box = {"name": "CoordinateInBox", "min": (0.0, 0.0, 0.0), "max": (0.775, 0.4, 0.25)}
    assert g.particles_number(1, box) == 7 == S.particles_number(box, 5, d, L, bug="rounded_count") - 1
    for outer in np.arange(1.70, 1.80, 0.01):
        v = math.pi * (outer * outer - 0.5 * 0.5) * 1.5 * (5 / (d[0] * d[1] * d[2]))
        if 0.55 < v - int(v) < 0.95:
            break
    else:
        raise AssertionError("no annulus with such a count")
    ann = dict(COORDS["annulus"](L), inner_r=0.5, outer_r=float(outer), height=1.5)
    assert g.particles_number(1, ann) == int(v) == S.particles_number(ann, 5, d, L, bug="rounded_count") - 1


def _load(ctx, L):
    """two calls on a context (or a slab of one) -> what they returned"""
    out = [ctx.set_particles(0, 3000, COORDS["annulus"](L), MOMENTA["angular"](L), step=4, seed=3)]
    out.append(ctx.set_particles(1, 1000, COORDS["box"](L), MOMENTA["cosine"](L), step=5, seed=3, particle0=50, chunk=256))
    return out


def test_slabs_equal_one_context():
    """three z-slabs: the union of their new records is the single context's; `added` and the energy are the sums"""
    import xpic_amd as X
    from xpic_amd.parallel import ThreadRing

    n, d, nr = (8, 6, 24), (0.5, 0.4, 0.25), 3
    L = T._L(n, d)
    cap = 4 * 6 * n[0] * n[1] * n[2] + 64  # (_ctx's default capacity)
    one = T._ctx(n, d, seed=9)
    rvals = _load(one, L)
    rparts = [one.particles(s)[0] for s in range(2)]
    ring = ThreadRing(nr)
    res, errs = [None] * nr, []
    # a point in the middle slab: more particles than a sort holds overflow that slab alone, and every slab must refuse
    point = {"name": "PreciseCoordinate", "value": (0.31 * L[0], 0.63 * L[1], 0.47 * L[2])}

    def rank_main(r):
        try:
            ctx = T._ctx(n, d, seed=9, rank=r, nranks=nr, capacity=cap)
            ring.attach(ctx, r)
            vals = _load(ctx, L)
            parts = [ctx.particles(s)[0] for s in range(2)]
            refused = 0
            for kwargs in (dict(n=cap + 1), dict(n=-1)):
                try:
                    ctx.set_particles(1, kwargs["n"], point, MOMENTA["precise"](L))
                except X.XpicError as e:
                    refused += "xpic_set_particles" in str(e)
            same = all(ctx.particles(s)[0].tobytes() == parts[s].tobytes() for s in range(2))
            res[r] = (vals, parts, refused, same)
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
    local = [0, 0]
    for r in range(nr):
        vals, parts, refused, same = res[r]
        assert refused == 2 and same, r
        for k in range(2):
            assert vals[k][0] == rvals[k][0]
            T._rel(vals[k][1], rvals[k][1])
            local[k] += len(parts[k])
    for s in range(2):
        got = np.concatenate([res[r][1][s] for r in range(nr)])
        assert np.array_equal(key(got), key(rparts[s]))  # exactly the same records
        assert local[s] == len(rparts[s])
    assert 0 < rvals[1][0] < 1000 and rvals[0][0] == 3000


def test_statistics():
    """a fixed seed, 2^18 particles, within 6 sigma: the annulus, and the cosine perturbation's mean velocity in 16 x-bins"""
    import xpic_amd as X

    n, d = (16, 16, 16), (0.5, 0.5, 0.5)
    g = X.Context("ecsim", n, d, 0.7)
    Np, nn, q, m = T.SORTS[1]
    g.add_sort(Np, nn, q, m, capacity=1 << 18)
    L = T._L(n, d)
    c, ri, ro, h = (0.5 * L[0], 0.5 * L[1], 0.5 * L[2]), 1.0, 3.5, 5.0
    ann = {"name": "CoordinateOnAnnulus", "center": c, "inner_r": ri, "outer_r": ro, "height": h}
    Tk, amp, wn = (1.0, 4.0, 0.25), (0.5, 0.0, 0.0), (2.0, 0.0, 0.0)
    cos = {"name": "MaxwellCosinePerturbation", "T": Tk, "amplitude": amp, "wave_number": wn, "min": (0.0, 0.0, 0.0), "max": L}
    N = 1 << 18
    assert g.set_particles(0, N, ann, cos, step=3, seed=2024)[0] == N
    p, _ = g.particles(0)

    def within6(x, mean, var):
        assert abs(x.mean() - mean) <= 6 * math.sqrt(var / len(x)), (x.mean(), mean)

    a, b = ri * ri, ro * ro
    r2 = (p[:, 0] - c[0]) ** 2 + (p[:, 1] - c[1]) ** 2
    assert r2.min() >= a * (1 - 1e-12) and r2.max() <= b * (1 + 1e-12)
    within6(r2, 0.5 * (a + b), (b - a) ** 2 / 12)                   # r^2 uniform on [inner^2, outer^2]
    within6(r2 * r2, (a * a + a * b + b * b) / 3, (b ** 5 - a ** 5) / (5 * (b - a)))
    within6(p[:, 2], c[2], h * h / 12)                               # z uniform over the height
    phi = np.arctan2(p[:, 1] - c[1], p[:, 0] - c[0])
    within6(np.cos(phi), 0.0, 0.5)
    within6(np.sin(phi), 0.0, 0.5)
    # the thermal part is symmetric about 0 and at most |p| / m with <p^2> = T m / mec2: the bin's mean velocity is the mean
    # of v0 cos(2 pi m x / L) over its particles, within 6 sigma of that bound
    v0 = amp[0] * math.sqrt(Tk[0] / (m * S.MEC2))
    wave = v0 * np.cos(2 * np.pi * wn[0] * p[:, 0] / L[0])
    x0, x1 = c[0] - ro, c[0] + ro
    bins = np.minimum(((p[:, 0] - x0) / (x1 - x0) * 16).astype(int), 15)
    bound = Tk[0] * m / S.MEC2 / (m * m)
    for k in range(16):
        sel = bins == k
        assert sel.sum() > 1000
        within6(p[sel, 3] - wave[sel], 0.0, bound)
    assert wave.max() - wave.min() > 1.9 * v0 > 0  # (the bins see the whole wave)
    for axis in (1, 2):
        within6(p[:, 3 + axis], 0.0, Tk[axis] * m / S.MEC2 / (m * m))


def test_steps_after_a_device_load():
    """three ECSIM steps on a plasma loaded by xpic_set_particles: finite, and the energy is conserved"""
    import xpic_amd as X

    n, d = T.GRID_P2
    g = X.Context("ecsim", n, d, 0.7)
    g.set_preconditioner(0)
    L = T._L(n, d)
    N = n[0] * n[1] * n[2]
    box = {"name": "CoordinateInBox", "min": (0.0, 0.0, 0.0), "max": L}
    for s, (Np, nn, q, m) in enumerate(((8, 1.0, -1.0, 1.0), (8, 1.0, 1.0, 1836.0))):
        g.add_sort(Np, nn, q, m, capacity=12 * N)
        count = g.particles_number(s, box)
        assert count == 8 * N
        mom = {"name": "MaxwellianMomentum", "T": (0.4, 0.4, 0.4), "tov": True}
        assert g.set_particles(s, count, box, mom, seed=5 + s, chunk=4096)[0] == count
    b0 = np.zeros(g.fshape()) + np.array([0.0, 0.0, 0.2])
    g.set_field(X.B, b0)
    g.set_field(X.B0, b0)
    g.set_tolerances(1e-10, 1e-50, 300)
    e0 = g.energy()
    tot0 = e0[0] + e0[1] + e0[4] + e0[6]
    assert np.isfinite(e0).all() and e0[4] > 0 and e0[6] > 0
    for _ in range(3):
        assert g.step() > 0
        e = g.energy()
        assert np.isfinite(e).all()
        assert abs(e[0] + e[1] + e[4] + e[6] - tot0) <= 1e-7 * tot0
    for s in range(2):
        pts, cells = g.particles(s)
        assert len(pts) == 8 * N and np.isfinite(pts).all()
