"""The collisional grid traces and the background profiles on the device (xpic_full_orbit_trace_collisional,
xpic_drift_kinetic_trace_collisional, xpic_background_*; xpic_amd/csrc/collide_trace.hip, xpic_amd/csrc/background.hip)
against the numpy restatement tests/collisional_grid_trace_ref.py (pinned without a GPU by
tests/test_collisional_grid_trace_ref.py), and the guarantees (a) .. (f) of include/xpic_hip.h bit for bit.

The grid has three different extents, 6 x 5 x 4 cells with unequal spacings; the particles start up to two boxes outside
it on both sides of every axis, so every lookup folds, and the first one lies on a cell face of every axis.  The iterative
pushers run with pinned iteration counts where the device is held to the restatement step by step, as in
tests/test_gpu_collisional_trace.py."""
import ctypes as C

import numpy as np
import pytest

import collisional_grid_trace_ref as G
import collisional_trace_ref as CT
import test_gpu_collisions as GC
import test_gpu_drift_kinetic as TD
import test_gpu_full_orbit as TF
import test_gpu_model_trace as MT

pytestmark = pytest.mark.gpu

N, D = (6, 5, 4), (0.5, 0.4, 0.25)
SHAPE = (N[2], N[1], N[0])
NCELL = N[0] * N[1] * N[2]
L = np.array(N) * np.array(D)
QM, MP, DT = -1.0, 1.0, 0.05
KINDS = ["EB2B", "CN", "dk"]
PIN = MT.PIN
TOL_COLLISION = 1e-12  # of the largest |v|: tests/test_gpu_collisional_trace.py's bound, from tests/test_gpu_collisions.py
# one grid step against the restatement: the bound of tests/test_gpu_full_orbit.py and tests/test_gpu_drift_kinetic.py
TOL_PUSH = {"EB2B": TF._same.__defaults__[0], "CN": TF._same.__defaults__[0], "dk": TD._same.__defaults__[0]}
EPS = np.finfo(np.float64).eps
BACKGROUNDS = [dict(q=1.0, m=4.0, n=1.0, vth=0.5, drift=(0.1, 0.0, -0.2)), dict(q=-2.0, m=0.25, n=0.5, vth=2.0),
               dict(q=1.0, m=1836.0, n=3.0, vth=0.01), dict(q=1.0, m=1.0, n=0.7, vth=1.0, drift=(0.0, 0.3, 0.0))]
# open along z, where B points: the particles start within -2 .. 3 box lengths and leave one by one over 130 steps
REGION = {"name": "box", "min": (-2.5 * L[0], -2.5 * L[1], -3.0 * L[2]), "max": (3.5 * L[0], 3.5 * L[1], 8.0 * L[2])}
SORT = (8, 2.0, -1.0, 1.0)  # Np, n, q, m of the sort the profiles are made of


def grid_fields():
    """smooth periodic E, B and the central differences of |B| on the 6 x 5 x 4 nodes; |B| >= 0.6"""
    z, y, x = np.meshgrid(*[2 * np.pi * np.arange(m) / m for m in SHAPE], indexing="ij")
    E = 0.02 * np.stack([np.sin(y + z), np.cos(x - z), np.sin(x + y)], axis=-1)
    B = np.array([0.2, -0.1, 1.0]) + 0.15 * np.stack([np.cos(y), np.sin(z + x), np.cos(x + y)], axis=-1)
    lB = np.sqrt((B * B).sum(axis=-1))
    g = np.zeros_like(B)
    for c, axis in enumerate((2, 1, 0)):
        g[..., c] = (np.roll(lB, -1, axis=axis) - np.roll(lB, 1, axis=axis)) / (2.0 * D[c])
    return E, B, g


def graded(seed, empty_half=False):
    rng = np.random.default_rng(seed)
    n = 0.5 + rng.random(SHAPE)
    if empty_half:
        n[:, :, N[0] // 2:] = 0.0
    return G.profile(n, 0.2 + rng.random(SHAPE), 0.3 * rng.normal(size=SHAPE + (3,)))


SLOTS = {0: graded(21), 1: graded(22, empty_half=True), 3: graded(23)}


@pytest.fixture(scope="module")
def X():
    import xpic_amd

    return xpic_amd


@pytest.fixture(scope="module")
def ctx(X):
    g = X.Context("basic", N, D, 0.7)
    E, B, gB = grid_fields()
    g.set_field(X.E, E)
    g.set_field(X.B, B)
    g.set_field(X.W0, gB)
    for s, p in SLOTS.items():
        g.background_set(s, p["n"], p["vth"], p["drift"])
    return g


def ensemble(kind, n, seed=3):
    rng = np.random.default_rng(seed + n)
    r = (rng.random((n, 3)) * 5.0 - 2.0) * L
    r[0] = (3 * D[0], -2 * D[1], 5 * D[2] + L[2])  # on a cell face of every axis
    if kind != "dk":
        return np.column_stack([r, rng.normal(size=(n, 3))])
    # away from turning: the drift-kinetic push divides mu (|B_n| - |B_0|) by Vh = (p_par_n + p_par_0) / 2, so near
    # Vh = 0 one rounding of B moves the step by far more than the one-step bound (test_parity_per_step asserts the margin)
    perp = 0.5 * np.abs(rng.normal(size=n)) + 0.1
    par = (0.8 + np.abs(rng.normal(size=n))) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    return np.column_stack([r, par, perp, MP * perp * perp / 2.0])


def device(X, coll):
    return None if coll is None else X.trace_collisions(**coll)


def call(X, ctx, kind, p, steps, coll, prof=None, reg=None, pin=True, **kw):
    kw = dict(PIN.get(kind, {}) if pin else {}, **kw)
    if kind == "dk":
        return ctx.drift_kinetic_trace_collisional(p, steps, QM, MP, DT, device(X, coll), prof, reg, gradB_field=X.W0, **kw)
    return ctx.full_orbit_trace_collisional(p, steps, kind, QM, DT, device(X, coll), prof, reg, **kw)


def grid_trace(X, ctx, kind, p, steps, reg, pin=True, **kw):
    """the collisionless grid trace, open or (reg None) closed, as an OpenTrace"""
    kw = dict(PIN.get(kind, {}) if pin else {}, **kw)
    if reg is not None:
        if kind == "dk":
            return ctx.drift_kinetic_trace_open(p, steps, QM, MP, DT, reg, gradB_field=X.W0, **kw)
        return ctx.full_orbit_trace_open(p, steps, kind, QM, DT, reg, **kw)
    every = kw.get("sample_every", 0)
    if kind == "dk":
        s, sm, tot, mx = ctx.drift_kinetic_trace(p, steps, QM, MP, DT, X.W0, **kw)
    else:
        s, sm, tot, mx = ctx.full_orbit_trace(p, steps, kind, QM, DT, **kw)
    n = len(s)
    alive = np.full(steps // every, n, dtype=np.int64) if every else None
    return X.OpenTrace(s, sm, np.full(n, -1, dtype=np.int64), alive, 0, tot, mx)


# ---- one step at a time: each step starts from the device's previous state
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nbg,prof,every", [(1, [0], 1), (4, [3, -1, 1, 0], 3)])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_parity_per_step(X, ctx, n, nbg, prof, every, kind):
    """steps = 1 calls with step0 = 4 + k (not a multiple of `every`) against the restatement applied to the device's own
    state before that step.  Measured, largest error / bound over all cases: see DESIGN.md 5u"""
    fields = grid_fields()
    coll = CT.collisions(BACKGROUNDS[:nbg], strength=0.02, mass=2.0, every=every, seed=1234 + n, particle0=1000)
    p = ensemble(kind, n)
    worst = 0.0
    for k in range(4, 8):
        got = call(X, ctx, kind, p, 1, coll, prof, step0=k)
        ref, its, t = G.step(kind, fields, (N, D), p, QM, MP, DT, coll, prof, SLOTS, k + 1, 1000 + np.arange(n),
                             **PIN.get(kind, {}))
        scale = np.abs(ref[:, 3:]).max()  # the largest value of the column group, the scale of the pushers' own tests
        bound = TOL_COLLISION + TOL_PUSH[kind]
        if kind == "dk":  # the step is well conditioned: one rounding of every B moves the restatement's push by < bound / 10
            nudged = (fields[0], fields[1] * (1.0 + EPS * np.where(np.arange(fields[1].size).reshape(fields[1].shape) % 2, 1, -1)),
                      fields[2])
            a, b = G.push(kind, fields, D, p, QM, MP, DT, **PIN[kind])[0], G.push(kind, nudged, D, p, QM, MP, DT, **PIN[kind])[0]
            assert np.abs(a[:, 3:] - b[:, 3:]).max() / scale <= 0.1 * TOL_PUSH[kind]
        err = np.abs(got.state[:, 3:] - ref[:, 3:]).max() / scale
        errr = np.abs(got.state[:, :3] - ref[:, :3]).max() / np.abs(ref[:, :3]).max()
        worst = max(worst, err / bound, errr / TOL_PUSH[kind])
        print(kind, n, nbg, "step", k + 1, "velocity error / bound", err / bound, "position error / bound", errr / TOL_PUSH[kind])
        assert err <= bound, (k, err)
        assert errr <= TOL_PUSH[kind], (k, errr)
        assert np.array_equal(got.coll[[0, 1, 3]], t[[0, 1, 3]])
        assert abs(got.coll[2] - t[2]) <= 1e-12 * t[2]
        assert np.array_equal(got.iterations_max, its)
        if (k + 1) % every == 0:
            assert got.coll[0] > 0 or n < 4
        p = got.state
    print(kind, n, nbg, "largest error / bound:", worst)


# ---- the moments of xpic_background_from_sort
MOMENT_POPS = [0, 1, 2, 63, 64, 65, 130, 300]


def test_the_moments_of_a_sort(X):
    """n exact; u within (N + 2) eps sum |v_c| / N: a sum of N terms in any order is within (N - 1) eps sum |v_c| of the
    exact one to first order, the division adds one rounding of the quotient (eps / 2 |u| <= eps sum |v_c| / N), and two
    more eps of margin cover the second-order terms; the restatement's u (math.fsum, one division) is within eps / 2 |u|.
    vth^2 = S / (3 N), S = sum of t_i = |v_i - u|^2 >= 0: each t_i carries 3 subtractions, 3 products and 2 additions,
    every partial result non-negative after the squares, relative error <= 4 eps to first order with the subtraction's
    half eps on v_i - u counted twice by the square; the sum of N non-negative terms adds (N - 1) eps, the product 3 N and
    the quotient one eps: (N + 4) eps S / (3 N) in all.  A different u moves S: dS = -2 sum (v_i - u) . du + N |du|^2,
    and sum (v_i - u) vanishes only to rounding, so |dS| <= 2 sqrt(N S) |du| + N |du|^2 by Cauchy-Schwarz, with |du| the
    bound of u above, taken for both statements."""
    pops = np.zeros(NCELL, dtype=np.int64)
    pops[[0, 7, 19, 33, 34, 60, 77, 119]] = MOMENT_POPS  # the other cells are empty
    g = X.Context("ecsim", N, D, 0.7)
    rng = np.random.default_rng(5)
    pts = GC._points(pops, N, D, rng, 0.3)
    inside = pts[:, 0] >= 0
    pts[inside, 3:] += np.array([0.5, -1.0, 2.0])  # a drift that dwarfs the spread: two passes matter
    s = g.add_sort(*SORT, capacity=len(pts) + 64)
    g.add_particles(s, pts)
    rec, cells = g.particles(s)
    assert np.bincount(cells, minlength=NCELL).tolist() == pops.tolist()
    g.background_from_sort(2, s)
    n, vth, u = g.background_get(2)
    n, vth, u = n.reshape(-1), vth.reshape(-1), u.reshape(-1, 3)
    rn, rvth, ru = G.moments(rec[:, 3:], cells, NCELL, SORT[1] / SORT[0])
    assert n.tobytes() == rn.tobytes()
    worst_u = worst_v = 0.0
    for c in np.flatnonzero(pops):
        vc, Nc = rec[cells == c, 3:], float(pops[c])
        bu = (Nc + 2) * EPS * np.abs(vc).sum(axis=0) / Nc
        worst_u = max(worst_u, (np.abs(u[c] - ru[c]) / bu).max())
        assert (np.abs(u[c] - ru[c]) <= bu).all(), c
        S = 3.0 * Nc * rvth[c] ** 2
        du = 2.0 * np.sqrt((bu * bu).sum())
        bv = ((Nc + 4) * EPS * S + 2.0 * np.sqrt(Nc * S) * du + Nc * du * du) / (3.0 * Nc)
        err = abs(vth[c] ** 2 - rvth[c] ** 2)
        if pops[c] == 1:
            assert vth[c] == 0.0 and u[c].tobytes() == vc[0].tobytes()
        else:
            worst_v = max(worst_v, err / bv)
            assert err <= bv, (c, err, bv)
    # the comparison can fail: a spread divided by N - 1 misses the bound in every cell of two records or more
    _, slip, _ = G.moments(rec[:, 3:], cells, NCELL, SORT[1] / SORT[0], ddof=1)
    for c in np.flatnonzero(pops >= 2):
        Nc, S = float(pops[c]), 3.0 * float(pops[c]) * rvth[c] ** 2
        assert abs(slip[c] ** 2 - rvth[c] ** 2) > 100 * (Nc + 4) * EPS * S / (3.0 * Nc)
    print("cells whose vth^2 has the restatement's bits:", int((vth[pops >= 2] == rvth[pops >= 2]).sum()), "of", int((pops >= 2).sum()))
    empty = pops == 0
    assert not n[empty].any() and not vth[empty].any() and not u[empty].any()
    print("largest |u - restatement| / bound:", worst_u, "largest |vth^2 - restatement| / bound:", worst_v)
    # two calls give the same bits, into another slot too
    g.background_from_sort(0, s)
    assert [a.tobytes() for a in g.background_get(0)] == [a.tobytes() for a in g.background_get(2)]
    # set / get / clear
    g.background_set(1, SLOTS[0]["n"], SLOTS[0]["vth"])
    a = g.background_get(1)
    assert a[0].tobytes() == SLOTS[0]["n"].tobytes() and a[1].tobytes() == SLOTS[0]["vth"].tobytes() and not a[2].any()
    g.background_clear(1)
    with pytest.raises(X.XpicError, match="background_get"):
        g.background_get(1)


def test_the_sort_is_left_alone(X):
    """(f): the records before and after, and one xpic_collide call on two contexts, one of which made a profile.  (A step
    of the scheme is not compared between two contexts: the profile call does to the sort what reading its records does,
    and that is what the records' bytes above pin.)"""
    out = []
    for profiled in (False, True):
        g = GC._ctx(N, D, [np.full(NCELL, 9), np.full(NCELL, 5)], seed=2)
        before = [g.particles(s) for s in range(2)]
        if profiled:
            g.background_from_sort(0, 0)
            g.background_from_sort(3, 1)
            after = [g.particles(s) for s in range(2)]
            for (a, ca), (b, cb) in zip(before, after):
                assert a.tobytes() == b.tobytes() and ca.tobytes() == cb.tobytes()
        tally = g.collide(0, 1, GC.S, 3, seed=7)
        out.append((tally, [g.particles(s)[0].tobytes() for s in range(2)]))
    assert out[0] == out[1] and out[0][0]["pairs"] > 0


# ---- the guarantees on the traces
COLL = CT.collisions(BACKGROUNDS, strength=0.01, mass=1.0, every=3, seed=99, particle0=5)
PROF = [3, -1, 1, 0]
FIELDS = MT.FIELDS + ("coll",)


@pytest.mark.parametrize("kind", ["EB2B", "BLF", "CN", "dk"])
@pytest.mark.parametrize("open_", [True, False])
def test_no_collisions_is_the_grid_trace(X, ctx, kind, open_):
    """(a): collisions == NULL, nbg == 0 and strength == 0; 70 steps sampled every 7"""
    p, reg = ensemble(kind, 257), REGION if open_ else None
    ref = grid_trace(X, ctx, kind, p, 70, reg, sample_every=7)
    if open_:
        assert ref.removed > 0 and (ref.exit_step < 0).any()
    for coll, prof in ((None, None), (CT.collisions([], strength=0.01, mass=1.0), None), (dict(COLL, strength=0.0), PROF)):
        got = call(X, ctx, kind, p, 70, coll, prof, reg, sample_every=7)
        MT.same(got, ref, kind)
        assert not got.coll.any()
    if not open_:  # no region, but an exit_step: the collisional kernel with no background runs, and is the closed trace
        got = call(X, ctx, kind, p, 70, dict(COLL, strength=0.0), PROF, None, sample_every=7,
                   exit_step=np.full(257, -1, dtype=np.int64))
        MT.same(got, ref, kind)
        assert not got.coll.any()


@pytest.mark.parametrize("kind", KINDS)
def test_composition_split_and_compaction(X, ctx, kind):
    """(b) with (s1, s2) = (64, 1), (1, 64), (65, 65); (c) with 257 = 100 + 157; (d) the three policies"""
    p = ensemble(kind, 257)
    whole = {}
    for s1, s2 in ((64, 1), (1, 64), (65, 65)):
        steps = s1 + s2
        if steps not in whole:
            whole[steps] = call(X, ctx, kind, p, steps, COLL, PROF, REGION, sample_every=1)
        full = whole[steps]
        assert full.coll[0] > 0
        a = call(X, ctx, kind, p, s1, COLL, PROF, REGION, sample_every=1)
        b = call(X, ctx, kind, a.state, s2, COLL, PROF, REGION, sample_every=1, exit_step=a.exit_step, step0=s1)
        assert full.state.tobytes() == b.state.tobytes() and np.array_equal(full.exit_step, b.exit_step)
        assert full.samples.tobytes() == np.concatenate([a.samples, b.samples]).tobytes()
        assert np.array_equal(full.alive, np.concatenate([a.alive, b.alive]))
        assert full.removed == a.removed + b.removed
        assert np.array_equal(full.iterations_sum, a.iterations_sum + b.iterations_sum)
        assert np.array_equal(full.coll[[0, 1, 3]], a.coll[[0, 1, 3]] + b.coll[[0, 1, 3]])
        assert abs(full.coll[2] - a.coll[2] - b.coll[2]) <= 1e-12 * full.coll[2]
    full = whole[130]
    assert 0 < full.removed < 257
    for compact in ("auto", "never", "always"):
        MT.same(call(X, ctx, kind, p, 130, COLL, PROF, REGION, sample_every=1, compact=compact), full, compact, FIELDS)
    lo = call(X, ctx, kind, p[:100], 130, COLL, PROF, REGION, sample_every=1, compact="always")
    hi = call(X, ctx, kind, p[100:], 130, dict(COLL, particle0=COLL["particle0"] + 100), PROF, REGION, sample_every=1)
    for f in ("state", "exit_step", "iterations_sum", "iterations_max"):
        assert np.concatenate([getattr(lo, f), getattr(hi, f)]).tobytes() == getattr(full, f).tobytes(), f
    assert np.concatenate([lo.samples, hi.samples], axis=1).tobytes() == full.samples.tobytes()
    assert np.array_equal(lo.alive + hi.alive, full.alive) and lo.removed + hi.removed == full.removed
    assert np.array_equal((lo.coll + hi.coll)[[0, 1, 3]], full.coll[[0, 1, 3]])
    assert abs(lo.coll[2] + hi.coll[2] - full.coll[2]) <= 1e-12 * full.coll[2]
    # the closed form composes too (no region: exit_step travels, nobody leaves)
    a = call(X, ctx, kind, p, 64, COLL, PROF, None, sample_every=1)
    b = call(X, ctx, kind, a.state, 1, COLL, PROF, None, sample_every=1, step0=64)
    c = call(X, ctx, kind, p, 65, COLL, PROF, None, sample_every=1)
    assert c.state.tobytes() == b.state.tobytes() and c.removed == 0 and (c.alive == 257).all()
    assert c.samples.tobytes() == np.concatenate([a.samples, b.samples]).tobytes()


@pytest.mark.parametrize("kind", KINDS)
def test_a_constant_profile_is_the_uniform_background(X, ctx, kind):
    """(e): slot 2 holds background 2's n, vth and drift in every cell, slot 0 for a moment background 0's"""
    g = X.Context("basic", N, D, 0.7)
    for f, v in zip((X.E, X.B, X.W0), grid_fields()):
        g.set_field(f, v)
    for s, b in enumerate(BACKGROUNDS):
        g.background_set(s, b["n"], b["vth"], b.get("drift"))
    p = ensemble(kind, 257)
    ref = call(X, g, kind, p, 66, COLL, None, REGION, sample_every=5)
    assert ref.coll[0] > 0
    for prof in ([-1, -1, -1, -1], [0, 1, 2, 3], [0, -1, 2, -1]):
        MT.same(call(X, g, kind, p, 66, COLL, prof, REGION, sample_every=5), ref, str(prof), FIELDS)


def test_a_localised_profile(X, ctx):
    """slot 1 has n > 0 only in the cells with x < L / 2: the collisions made equal the restatement's count of (particle,
    step) visits to filled cells, exactly.  The ensemble is chosen so that no particle comes within 1e-9 d of a cell face
    at a collision step (asserted), so the count does not hang on a rounding"""
    coll = CT.collisions(BACKGROUNDS[1:2], strength=0.01, mass=1.0, every=2, seed=3, particle0=0)
    fields = grid_fields()
    p = ensemble("EB2B", 257)[1:]  # (without the particle on the faces)
    visits = []
    ref = G.trace("EB2B", fields, (N, D), p, 12, None, QM, MP, DT, coll, [1], SLOTS, visits=visits)
    count, margin = 0, np.inf
    for k, who, r in visits:
        if k % 2:
            continue
        s = r / np.array(D)
        margin = min(margin, np.abs(s - np.round(s)).min())
        count += int((SLOTS[1]["n"].reshape(-1)[G.cell_index(r, N, D)] > 0.0).sum())
    assert margin > 1e-9, margin
    assert count == ref.coll[0] and 0.2 * 6 * 256 < count < 0.8 * 6 * 256
    got = call(X, ctx, "EB2B", p, 12, coll, [1])
    assert got.coll[0] == count and got.coll[1] == 0
    assert np.abs(got.state - ref.state).max() <= 1e-10 * np.abs(ref.state).max()


def test_edges(X, ctx):
    for kind in KINDS:
        p = ensemble(kind, 5)
        out = call(X, ctx, kind, p[:0], 3, COLL, PROF, REGION, sample_every=1)
        assert out.state.shape == (0, 6) and out.removed == 0 and not out.coll.any()
        out = call(X, ctx, kind, p, 0, COLL, PROF, REGION)
        assert out.state.tobytes() == p.tobytes() and not out.coll.any() and not out.iterations_sum.any()
    # a particle that enters removed is returned untouched, with or without a region
    p = ensemble("EB2B", 70)
    ex = np.full(70, -1, dtype=np.int64)
    ex[::3] = 2
    for reg in (REGION, None):
        out = call(X, ctx, "EB2B", p, 5, COLL, PROF, reg, exit_step=ex, step0=9)
        assert out.state[::3].tobytes() == p[::3].tobytes() and np.array_equal(out.exit_step[::3], ex[::3])
        stepped = out.exit_step[1::3] != 9  # (not removed at the top of this call's first step)
        assert stepped.sum() > 5 and (out.state[1::3, :3] != p[1::3, :3])[stepped].all()


def test_refusals(X, ctx):
    """each refusal returns nonzero, names the entry point, and leaves the state, exit_step and the slots alone"""
    dp, i64, i32 = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    F, K = X.FoParams(QM, DT, 1e-7, 1e-7, X.FO_SCHEMES["EB2B"], 30), X.DkParams(QM, MP, DT, 1e-12, 1e-12, 30)
    good = dict(backgrounds=BACKGROUNDS[:2], strength=0.1, mass=1.0, every=1, seed=0, particle0=0)
    slots_before = [a.tobytes() for s in SLOTS for a in ctx.background_get(s)]

    def run(kind, coll, prof=None, geometry=0, compact=1, gradB=-1, steps=2):
        p = ensemble(kind, 3)
        s, out, ex = p.copy(), np.full(4, 7.0), np.full(3, -1, dtype=np.int64)
        tot, mx, removed = np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.int32), C.c_int64(0)
        reg = X.TraceRegion(geometry, compact, (C.c_double * 7)(-100, -100, -100, 100, 100, 100, 0), 0)
        pr = None if prof is None else (C.c_int32 * len(prof))(*prof)
        tail = [C.c_int64(steps), C.c_int64(0), s.ctypes.data_as(dp), None, tot.ctypes.data_as(i64),
                mx.ctypes.data_as(C.POINTER(C.c_int)), C.byref(reg), ex.ctypes.data_as(i64), None, C.byref(removed),
                None if coll is None else C.byref(coll), pr, out.ctypes.data_as(dp)]
        if kind == "dk":
            rc = ctx.L.xpic_drift_kinetic_trace_collisional(ctx.h, C.c_int64(3), C.byref(K), gradB, *tail)
        else:
            rc = ctx.L.xpic_full_orbit_trace_collisional(ctx.h, C.c_int64(3), C.byref(F), *tail)
        msg = ctx.L.xpic_last_error().decode() if rc else ""
        return rc, s.tobytes() == p.tobytes() and (ex == -1).all(), msg

    def bad(**change):
        c = X.trace_collisions(**good)
        for k, v in change.items():
            if k.startswith("bg_"):
                setattr(c.bg[1], k[3:], v)
            else:
                setattr(c, k, v)
        return c
    for kind, name in (("EB2B", "full_orbit_trace_collisional"), ("dk", "drift_kinetic_trace_collisional")):
        rc, same, _ = run(kind, bad(), [0, -1])
        assert rc == 0 and not same
        cases = [dict(coll=bad(**ch)) for ch in (
            dict(nbg=-1), dict(nbg=X.TRACE_BG_MAX + 1), dict(every=0), dict(particle0=-1), dict(strength=-1e-300),
            dict(strength=float("nan")), dict(mass=0.0), dict(bg_m=0.0), dict(bg_n=-1.0), dict(bg_vth=-0.5))]
        cases += [dict(coll=bad(), prof=[0, -2]), dict(coll=bad(), prof=[X.TRACE_BG_MAX, 0]), dict(coll=bad(), prof=[0, 2]),
                  dict(coll=bad(), geometry=5), dict(coll=bad(), compact=3)]
        # with the collisions off the grid trace itself refuses, under this entry point's name too: open, closed with an
        # exit_step, and a struct whose strength is 0
        cases += [dict(coll=None, steps=-1), dict(coll=None, steps=-1, geometry=X.GEOM_NONE), dict(coll=bad(strength=0.0), steps=-1)]
        if kind == "dk":
            cases.append(dict(coll=bad(), gradB=99))
        for case in cases:
            rc, same, msg = run(kind, **case)
            assert rc != 0 and same and name in msg, (kind, case, msg)
    assert [a.tobytes() for s in SLOTS for a in ctx.background_get(s)] == slots_before
    # the profiles' own refusals leave the slot as it was
    n, vth = SLOTS[0]["n"], SLOTS[0]["vth"]
    for args in ((-1, n, vth), (X.TRACE_BG_MAX, n, vth), (0, -n, vth), (0, n, np.where(vth > 1.0, np.inf, vth)),
                 (0, n, vth, np.full(SHAPE + (3,), np.nan))):
        with pytest.raises(X.XpicError, match="background_set"):
            ctx.background_set(*args)
    assert ctx.L.xpic_background_set(ctx.h, 0, None, vth.ctypes.data_as(dp), None) != 0
    with pytest.raises(X.XpicError, match="background_from_sort"):
        ctx.background_from_sort(0, 0)  # (this context has no sort)
    with pytest.raises(X.XpicError, match="background_get"):
        ctx.background_get(2)
    assert [a.tobytes() for s in SLOTS for a in ctx.background_get(s)] == slots_before
    # a context of several slabs has no profiles and no collisional grid trace
    ring = X.Context("basic", (4, 4, 8), (1.0, 1.0, 1.0), 0.7, self_ring=True)
    with pytest.raises(X.XpicError, match="background_set"):
        ring.background_set(0, 1.0, 1.0)
    with pytest.raises(X.XpicError, match="full_orbit_trace_collisional"):
        ring.full_orbit_trace_collisional(np.ones((2, 6)), 1, "EB2B", QM, DT, None)


# ---- physics, small: a trapped ensemble leaves an open mirror by collisions with the plasma of a sort.  The 8 x 8 x 8
# grid of tests/open_trace_ref.py with its uniform B plus xpic_set_mirror_field's field: |B| is largest in the plane
# z = 4 and, the box being periodic, in z = 12; unfolded positions between the two are a trap around z = 8 with the
# mirror ratio 1.2, so a particle of the midplane is trapped while |v_z| / v < 0.41.  MIRROR_N particles of speed 1 start
# within half a cell of (4, 4, 8) with |v_z| / v <= 0.2, every gyrophase; the region keeps the cells 4 <= z < 12.  The
# background is a sort of heavy cold ions (m = 1836), 24 records per cell about the midplane, thinning to none in the four
# planes next to the plugs: the profile made from it turns the velocity and changes next to nothing else.
MIRROR_N, MIRROR_STEPS, MIRROR_EVERY, MIRROR_SAMPLE, MIRROR_S = 256, 300, 10, 50, 0.008
MIRROR_REGION = {"name": "box", "min": (-100.0, -100.0, 4.0), "max": (100.0, 100.0, 12.0)}
MIRROR_SORT = (8, 1.0, 1.0, 1836.0)  # Np, n, q, m


def mirror_fields():
    import open_trace_ref as O

    shape = (O.N[2], O.N[1], O.N[0], 3)
    B = np.zeros(shape) + np.array(O.B_UNIFORM) + O.mirror_field(O.N, O.D, **O.MIRROR)
    return np.zeros(shape), B, None


def mirror_sort_points():
    """the records of the background sort, GC._points' padding included, and the populations per cell"""
    import open_trace_ref as O

    z, y, x = np.meshgrid(np.arange(O.N[2]), np.arange(O.N[1]), np.arange(O.N[0]), indexing="ij")
    per_plane = np.array([24, 12, 4, 0, 0, 4, 12, 24])  # dense about z = 0 = 8, the midplane of the trap
    pops = (per_plane[z] + np.where(per_plane[z] > 0, (x + y) % 3, 0)).reshape(-1)
    return GC._points(pops, O.N, O.D, np.random.default_rng(12), 0.01), pops


def mirror_ensemble(perturb=0.0):
    rng = np.random.default_rng(19)
    n = MIRROR_N
    r = np.array([4.0, 4.0, 8.0]) + (rng.random((n, 3)) - 0.5)
    mu, ang = 0.4 * rng.random(n) - 0.2, 2 * np.pi * rng.random(n)
    s = np.sqrt(1.0 - mu * mu)
    p = np.column_stack([r, s * np.cos(ang), s * np.sin(ang), mu])
    if perturb:
        p[:, 3:] *= 1.0 + perturb * np.random.default_rng(2).uniform(-1, 1, size=(n, 1))
    coll = CT.collisions([dict(q=MIRROR_SORT[2], m=MIRROR_SORT[3], n=0.0, vth=0.0)], strength=MIRROR_S, mass=1.0,
                         every=MIRROR_EVERY, seed=31)
    return p, coll


def mirror_restatement(prof, coll=True, perturb=0.0):
    import open_trace_ref as O

    p, c = mirror_ensemble(perturb)
    return G.trace("EB2B", mirror_fields(), (O.N, O.D), p, MIRROR_STEPS, MIRROR_REGION, O.QM, O.MP, O.DT, c if coll else None,
                   [0], {0: prof}, sample_every=MIRROR_SAMPLE)


def mirror_profile_restated():
    import open_trace_ref as O

    pts, pops = mirror_sort_points()
    inside = pts[pts[:, 0] >= 0]
    cells = G.cell_index(inside[:, :3], O.N, O.D)
    assert np.bincount(cells, minlength=len(pops)).tolist() == pops.tolist()
    shape = (O.N[2], O.N[1], O.N[0])
    return G.as_profile(*G.moments(inside[:, 3:], cells, len(pops), MIRROR_SORT[1] / MIRROR_SORT[0]), shape), pts


def test_a_trapped_ensemble_leaves_by_collisions_with_a_sort(X):
    """sort -> xpic_background_from_sort -> open grid trace -> alive curve.  Without collisions nobody leaves; with them the
    exit steps equal the restatement's exactly.  The ensemble is chosen on the CPU: the restatement's exits do not change
    when its initial velocities are perturbed by 1e-12 relative (asserted here, the condition of
    tests/test_gpu_collisional_trace.py::test_the_loss_cone_is_refilled), nor when it reads the restated profile
    instead of the device's."""
    import open_trace_ref as O

    g = X.Context("ecsim", O.N, O.D, 0.7)
    E, B, _ = mirror_fields()
    g.set_field(X.E, E)
    g.set_field(X.B, np.zeros_like(B) + np.array(O.B_UNIFORM))
    g.set_mirror_field(field=X.B, **O.MIRROR)
    assert np.abs(g.get_field(X.B) - B).max() <= 1e-13 * np.abs(B).max()
    restated, pts = mirror_profile_restated()
    s = g.add_sort(*MIRROR_SORT, capacity=len(pts) + 64)
    g.add_particles(s, pts)
    g.background_from_sort(0, s)
    n, vth, u = g.background_get(0)
    assert n.tobytes() == restated["n"].tobytes() and n.max() == 26 / 8 and (n[3:5] == 0).all()
    assert np.abs(vth - restated["vth"]).max() <= 1e-13 * vth.max() and np.abs(u - restated["drift"]).max() <= 1e-13 * vth.max()
    p, coll = mirror_ensemble()
    kw = dict(sample_every=MIRROR_SAMPLE, compact="auto")
    quiet = g.full_orbit_trace_open(p, MIRROR_STEPS, "EB2B", O.QM, O.DT, MIRROR_REGION, **kw)
    assert quiet.removed == 0 and (quiet.exit_step == -1).all() and (quiet.alive == MIRROR_N).all()
    got = g.full_orbit_trace_collisional(p, MIRROR_STEPS, "EB2B", O.QM, O.DT, X.trace_collisions(**coll), [0], MIRROR_REGION, **kw)
    ref = mirror_restatement(dict(n=n, vth=vth, drift=u))
    print("removed", got.removed, "of", MIRROR_N, "alive", got.alive, "restatement", ref.removed, ref.alive,
          "mean sigma^2", got.coll[2] / got.coll[0])
    assert 0.05 * MIRROR_N <= ref.removed <= 0.95 * MIRROR_N
    for other in (mirror_restatement(dict(n=n, vth=vth, drift=u), perturb=1e-12), mirror_restatement(restated)):
        assert np.array_equal(other.exit_step, ref.exit_step)
    assert mirror_restatement(restated, coll=False).removed == 0
    assert np.array_equal(got.exit_step, ref.exit_step) and got.removed == ref.removed
    assert np.array_equal(got.alive, ref.alive) and np.array_equal(got.coll[[0, 1, 3]], ref.coll[[0, 1, 3]])


if __name__ == "__main__":  # the restatement's figures for the mirror test, without a GPU
    import time

    t0 = time.time()
    prof_, _ = mirror_profile_restated()
    base, pert, none = mirror_restatement(prof_), mirror_restatement(prof_, perturb=1e-12), mirror_restatement(prof_, coll=False)
    print("removed", base.removed, "alive", base.alive, "mean sigma^2", base.coll[2] / base.coll[0], "changed exits",
          int((base.exit_step != pert.exit_step).sum()), "without collisions", none.removed, "seconds", time.time() - t0)
