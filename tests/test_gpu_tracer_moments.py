"""The moments of a tracer set on the device (include/xpic_tracer_moments.h) against their numpy restatement
(tests/tracer_moments_ref.py, pinned without a GPU by tests/test_tracer_moments_ref.py).

Bounds.  Full orbits: the per-particle values and the shape are the restatement's operations, compiled without
contraction, so what is left is the order of the sums: the project's deposit bound per node and component,
2 eps * contributions * sum |contribution|.  Guiding centres: that bound plus the rounding of b.  The gather of
B is the field-line tracer's, which the project pins to its restatement within K_B eps sum |B w| with K_B = 72 (64 nodes, each
a product of three spline weights and a field value, summed: DESIGN.md 8); the weights are non-negative and sum to 1, so
sum |B w| <= max |B_c| over the grid =: Bmax.  With f = |B| (two products, two sums, a root: 2.5 eps) and b_c = B_c / f
(one division),
    |db_c| <= (dB_c + |b_c| (|dB| + 2.5 eps f)) / f + eps <= (1 + sqrt 3) 72 eps Bmax / fmin + 4 eps =: db,
fmin the smallest |B| any counted particle sees.  The cylindrical kinds rotate b with |px / r|, |py / r| <= 1: two products,
a sum, a division, dc <= 2 db + 4 eps.  A component of the current is (q p_par) b_c and one of the tensor is
par c_i c_j + perp (delta_ij - c_i c_j) with |c| <= 1: it moves by at most scale * (2 dc + 4 eps) <= scale * (4 db + 12 eps),
scale = |q p_par| or m (p_par^2 + p_perp^2 / 2) (tracer_moments_ref.dk_scales), deposited with the particle's weights.
Nothing here is fitted to what the device returns."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import lattice_cases as LC
import moments_ref as M
import tracer_moments_ref as T

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
K_B = 72
GRIDS = {"6x5x4": ((6, 5, 4), (0.5, 0.4, 0.25)), "2x2x2": ((2, 2, 2), (0.5, 0.5, 0.25))}
REGIONS = {"6x5x4": (None, (1, 1, 0, 4, 3, 3), (0, 1, 1, 6, 3, 2)),  # the box, a partial region, one spanning x in full
           "2x2x2": (None, (1, 0, 1, 1, 1, 1), (0, 1, 0, 2, 1, 2))}
COUNTS = (0, 1, 65, 300)  # none, one lane, a wave and a lane, more than a workgroup
Q, MASS, WEIGHT, QM, MP, DT = -1.5, 2.0, 0.25, -1.0, 1.0, 0.3


@pytest.fixture(scope="module")
def X():
    import xpic_amd

    return xpic_amd


def bits(a):
    return np.ascontiguousarray(a).tobytes()


@functools.lru_cache(maxsize=None)
def field_B(grid):
    n, _ = GRIDS[grid]
    rng = np.random.default_rng(5)
    return np.array([0.3, 0.4, 1.0]) + 0.1 * rng.normal(size=(n[2], n[1], n[0], 3))


@functools.lru_cache(maxsize=None)
def records(grid, count, kind):
    """positions from the lattice families: cell faces (node_), cell centres, which are the exact .5 ties of
    round(r / d - 1) and where a spline weight is exactly 0 and floor and round part (half_), one ulp off them (near_), all
    three axes on planes at once (still); a sixth of them moved outside [0, L) by less and by more than one box"""
    n, d = GRIDS[grid]
    if count == 0:
        return np.zeros((0, 6))
    fam = LC.families(n, d, seed=3)
    pool = np.vstack([fam[k + a].u for k in ("half_", "node_", "near_") for a in "xyz"] + [fam["still"].u])
    rng = np.random.default_rng(count)
    u = pool[rng.choice(len(pool), count, replace=len(pool) < count)]
    if count == 1:
        u = fam["half_x"].u[:1]
    r = u * np.array(d)
    L = np.array(n) * np.array(d)
    for j in range(count // 6):
        a = j % 3
        r[j, a] = (-0.3 * L[a] * rng.random(), L[a] * (1 + 0.6 * rng.random()), 2.5 * L[a] + r[j, a], r[j, a] - 1.75 * L[a])[j % 4]
    if kind == "fo":
        return np.column_stack([r, rng.normal(0, 0.4, (count, 3))])
    return np.column_stack([r, rng.normal(0, 0.4, count), 0.1 + 0.3 * rng.random(count), 0.05 + 0.05 * rng.random(count)])


@functools.lru_cache(maxsize=None)
def reference(grid, count, kind, name, region):
    """the restatement, computed once for both kernel paths -> (Deposit, tolerance array)"""
    n, d = GRIDS[grid]
    p = records(grid, count, kind)
    ex = np.full(len(p), -1)
    return reference_of(grid, p, ex, kind, name, region)


def reference_of(grid, p, ex, kind, name, region):
    n, d = GRIDS[grid]
    if kind == "fo":
        dep = T.moment(name, p, ex, Q, MASS, WEIGHT, n, d, region)
        return dep, T.bound(dep)
    B = field_B(grid)
    dep = T.moment(name, p, ex, Q, MASS, WEIGHT, n, d, region, kind="drift_kinetic", B=B)
    keep = p[T.counts(p, ex, n, d, region)]
    if len(keep) == 0 or name == "density":
        return dep, T.bound(dep)
    fmin = T.FL.abs3(T.FL.grid_source(B, d)(keep[:, :3])).min()
    db = (1 + np.sqrt(3.0)) * K_B * EPS * np.abs(B).max() / fmin + 4 * EPS
    scale = T.deposit(T.dk_scales(name, keep, Q, MASS), keep[:, :3], WEIGHT, n, d, region)[0]
    return dep, T.bound(dep) + scale * (4 * db + 12 * EPS)


def context(X, grid):
    n, d = GRIDS[grid]
    g = X.Context("ecsim", n, d, DT)  # (the scheme that takes an extent of 2)
    rng = np.random.default_rng(6)
    g.set_field(X.B, field_B(grid))
    g.set_field(X.E, 0.05 * rng.normal(size=g.fshape()))
    return g


@pytest.fixture(scope="module", params=list(GRIDS))
def ctx(request, X):
    g = context(X, request.param)
    yield request.param, g
    g.close()


@pytest.fixture(scope="module")
def big(X):
    """the 6 x 5 x 4 context for the cases with a box region"""
    g = context(X, "6x5x4")
    yield "6x5x4", g
    g.close()


def make_set(g, kind, p, **kw):
    if kind == "fo":
        return g.tracers("full_orbit", p, "B1B", QM, DT, **kw)
    return g.tracers("drift_kinetic", p, QM, MP, DT, **kw)


def check(got, counted, dep, tol, what):
    assert counted == dep.counted, (what, counted, dep.counted)
    err = np.abs(got - dep.out)
    assert got.shape == dep.out.shape and np.all(err <= tol), (what, float((err - tol).max()), float(err.max()))
    assert np.all(got[dep.contributions == 0] == 0.0), what  # nothing where the restatement puts nothing


# ---- 1. the one-shot moment
@pytest.mark.parametrize("path", ["lds", "direct"])
@pytest.mark.parametrize("kind", ["fo", "dk"])
@pytest.mark.parametrize("count", COUNTS)
def test_moment_against_restatement(X, ctx, count, kind, path):
    """all six kinds and three regions; both kernel paths: these regions fit the LDS budget, and the knob of xpic_debug_set
    with 0 sends every deposit straight to memory"""
    grid, g = ctx
    p = records(grid, count, kind)
    g.debug_set(X.DEBUG_TRACER_MOMENT_LDS, 0 if path == "direct" else 9216)
    s = make_set(g, kind, p)
    before = s.get()
    some = 0
    for region in REGIONS[grid]:
        for name in M.MOMENTS:
            dep, tol = reference(grid, count, kind, name, region)
            got, counted = s.moment(name, Q, MASS, WEIGHT, region)
            check(got, counted, dep, tol, (grid, count, kind, path, name, region))
            some += dep.counted
    after = s.get()
    assert bits(before.state) == bits(after.state) == bits(p) and bits(before.exit_step) == bits(after.exit_step)
    assert after.steps == 0 and (some > 0) == (count > 0)
    if count >= 65:
        assert reference(grid, count, kind, "density", None)[0].counted < count  # the ones outside the box did not count
    s.close()
    g.debug_set(X.DEBUG_TRACER_MOMENT_LDS, 9216)


def test_a_zero_field_gives_the_isotropic_tensor(X):
    """|B| == 0: b is the zero vector, the tensor m p_perp^2 / 2 delta_ij and the current 0"""
    n, d = GRIDS["6x5x4"]
    g = X.Context("ecsim", n, d, DT)
    p = records("6x5x4", 65, "dk")
    s = make_set(g, "dk", p)
    B = np.zeros((n[2], n[1], n[0], 3))
    for name in ("current", "momentum_flux", "momentum_flux_diag_cyl"):
        dep = T.moment(name, p, np.full(65, -1), Q, MASS, WEIGHT, n, d, kind="drift_kinetic", B=B)
        got, counted = s.moment(name, Q, MASS, WEIGHT)
        check(got, counted, dep, T.bound(dep), name)
    assert np.all(s.moment("current", Q, MASS, WEIGHT)[0] == 0.0)
    g.close()


# ---- 2. dead particles
BOX = {"name": "box", "min": (0.5, 0.4, 0.25), "max": (2.5, 2.0, 0.75)}


def inside_box(count, seed):
    rng = np.random.default_rng(seed)
    lo, hi = np.array(BOX["min"]), np.array(BOX["max"])
    return np.column_stack([lo + (hi - lo) * rng.random((count, 3)), rng.normal(0, 0.5, (count, 3))])


def test_dead_particles_do_not_count(X, big):
    """a box region inside 6 x 5 x 4, fast particles: some leave at every step.  The moment is the restatement on
    exit_step < 0 as it stands.  The open traces test a particle at the top of a step: one retired at the top of a due step
    (exit_step = due - 1) does not count at that step; one whose exit_step will be the due step has made that step and
    counts there for the last time"""
    grid, g = big
    p = inside_box(300, 11)
    s, twin = make_set(g, "fo", p, region=BOX), make_set(g, "fo", p, region=BOX)
    m = s.map("current", Q, MASS, WEIGHT, every=2)
    deps, states = [], {}
    for k in range(1, 9):
        twin.advance(1)
        st = twin.get()
        states[k] = st
        for name in ("density", "momentum_flux"):
            dep, tol = reference_of(grid, st.state, st.exit_step, "fo", name, None)
            got, counted = twin.moment(name, Q, MASS, WEIGHT)
            check(got, counted, dep, tol, (k, name))
            assert counted <= (st.exit_step < 0).sum()
        if k % 2 == 0:
            deps.append(T.moment("current", st.state, st.exit_step, Q, MASS, WEIGHT, *GRIDS[grid]))
    final = states[8].exit_step
    assert 0 < (final >= 0).sum() < 300
    retired_at_due = np.isin(final, (1, 3, 5, 7))  # left the loop at the top of steps 2, 4, 6, 8
    last_at_due = np.isin(final, (2, 4, 6))        # made the due step, retired at the top of the next
    assert retired_at_due.any() and last_at_due.any()
    for k in (2, 4, 6, 8):
        assert np.all(states[k].exit_step[final == k - 1] == k - 1) and np.all(states[k].exit_step[final == k] == -1)
    s.advance(8)
    tot, made = T.map_sum(deps)
    got, deposits, counted, steps = m.get()
    assert (deposits, counted, steps) == (made, tot.counted, 8)
    check(got, counted, tot, T.bound(tot), "map over exits")
    s.close()
    twin.close()


# ---- 3. maps
@pytest.mark.parametrize("compact", ["never", "always"])
@pytest.mark.parametrize("kind", ["fo", "dk"])
def test_maps(X, big, kind, compact):
    grid, g = big
    n, d = GRIDS[grid]
    p = inside_box(300, 12)
    if kind == "dk":
        p[:, 4:] = np.abs(p[:, 4:]) * 0.2
    kw = dict(region=BOX, compact=compact, sample_every=2, sample_capacity=6)
    if kind == "dk":
        kw["gradB_field"] = "auto"
    s, twin = make_set(g, kind, p, **kw), make_set(g, kind, p, **kw)
    region = (1, 1, 0, 4, 3, 3)
    a = s.map("density", Q, MASS, WEIGHT, every=3)
    b = s.map("momentum_flux", Q, MASS, WEIGHT, region=region, every=2)
    s.advance(7)
    s.advance(5)
    one_a, one_b, ref_a, ref_b = [], [], [], []
    for k in range(1, 13):
        twin.advance(1)
        st = twin.get()
        if k % 3 == 0:
            one_a.append(twin.moment("density", Q, MASS, WEIGHT))
            ref_a.append(reference_of(grid, st.state, st.exit_step, kind, "density", None)[0])
        if k % 2 == 0:
            one_b.append(twin.moment("momentum_flux", Q, MASS, WEIGHT, region))
            ref_b.append(reference_of(grid, st.state, st.exit_step, kind, "momentum_flux", region)[0])
    # passive: the mapped set is the twin, bit for bit
    x, y = s.get(), twin.get()
    for f in ("state", "exit_step", "iterations_sum", "iterations_max"):
        assert bits(getattr(x, f)) == bits(getattr(y, f)), f
    assert (x.steps, x.removed, x.alive, x.held, x.dropped) == (y.steps, y.removed, y.alive, y.held, y.dropped)
    assert 0 < x.removed < 300
    xs, ys = s.samples(), twin.samples()
    assert bits(xs[0]) == bits(ys[0]) and bits(xs[1]) == bits(ys[1]) and len(xs[0]) == 6
    # the maps: the sums of the twin's one-shot moments, within the deposit bound with the contributions of all of them
    for m, ones, refs, every in ((a, one_a, ref_a, 3), (b, one_b, ref_b, 2)):
        tot, made = T.map_sum(refs)
        got, deposits, counted, steps = m.get()
        assert (deposits, counted, steps) == (12 // every, sum(c for _, c in ones), 12) and made == deposits
        assert counted == tot.counted
        err = np.abs(got - sum(o for o, _ in ones))
        assert np.all(err <= T.bound(tot)), (every, float(err.max()))
        assert np.all(got[tot.contributions == 0] == 0.0)
    # a map made after steps takes the later due steps only; reset zeroes
    late = s.map("density", Q, MASS, WEIGHT, every=5)
    s.advance(3)  # step 15
    twin.advance(3)
    want, wc = twin.moment("density", Q, MASS, WEIGHT)
    got, deposits, counted, steps = late.get(reset=True)
    st = twin.get()
    dep = reference_of(grid, st.state, st.exit_step, kind, "density", None)[0]
    assert (deposits, counted, steps) == (1, wc, 15) and np.all(np.abs(got - want) <= T.bound(dep))
    got, deposits, counted, steps = late.get()
    assert (deposits, counted, steps) == (0, 0, 15) and np.all(got == 0.0)
    assert a.get()[1] == 5 and b.get()[1] == 7  # (the other maps went on: steps 15 and 14)
    # limits: four maps, ids are not reused, a destroyed id is refused
    fourth = s.map("current", Q, MASS)
    with pytest.raises(X.XpicError, match="already has 4 maps"):
        s.map("current", Q, MASS)
    gone = fourth.id
    fourth.close()
    again = s.map("current", Q, MASS)
    assert again.id == gone + 1
    for call in (lambda: g.L.xpic_tracers_map_get(g.h, s.id, gone, None, None, 0),
                 lambda: g.L.xpic_tracers_map_destroy(g.h, s.id, gone),
                 lambda: g.L.xpic_tracers_map_get(g.h, 12345, 0, None, None, 0)):
        with pytest.raises(X.XpicError, match="does not exist"):
            g._ck(call())
    with pytest.raises(X.XpicError, match="every must be >= 1"):
        s.map("density", Q, MASS, every=0)
    with pytest.raises(X.XpicError, match="unknown moment kind"):
        g._ck(g.L.xpic_tracers_moment(g.h, s.id, 6, 1.0, 1.0, 1.0, None, np.zeros(120).ctypes.data_as(X.CTYPES["double*"]), None))
    with pytest.raises(X.XpicError, match="region"):
        s.moment("density", Q, MASS, region=(0, 0, 0, 7, 5, 4))
    s.close()  # (frees the maps that are left)
    twin.close()


def test_several_slabs_are_refused(X):
    for kw in (dict(self_ring=True), dict(rank=0, nranks=2)):
        h = X.Context("basic", (8, 8, 12), (0.5, 0.5, 0.5), 0.7, **kw)
        for call in (lambda: h.L.xpic_tracers_moment(h.h, 0, 0, 1.0, 1.0, 1.0, None, None, None),
                     lambda: h.L.xpic_tracers_map_get(h.h, 0, 0, None, None, 0)):
            with pytest.raises(X.XpicError, match="several z-slabs"):
                h._ck(call())
        h.close()


# ---- 4. riding
def riding_context(X):
    """6 x 6 x 6 ecsim, a coils field in B alone, so that rot B drives E and both fields change every step.  The sort is
    never loaded: with particles the step's own floating-point atomics make two runs differ in their last bits, and the
    comparison with the run without a set has to be bit for bit"""
    g = X.Context("ecsim", (6, 6, 6), (0.5, 0.5, 0.5), 0.5)
    sort = g.add_sort(1, 1.0, -1.0, 1.0, capacity=1 << 12)
    g.set_coils_field([(0.75, 1.0, 2.0), (2.25, 1.0, 2.0)], field=X.B)
    return g, sort


def test_a_map_rides_with_the_step(X):
    n, d = (6, 6, 6), (0.5, 0.5, 0.5)
    rng = np.random.default_rng(13)
    p = np.column_stack([0.5 + 2.0 * rng.random((300, 3)), rng.normal(0, 0.4, (300, 3))])
    g, sort = riding_context(X)
    s = g.tracers("full_orbit", p, "EB2B", QM, 0.3)
    s.attach()
    m = s.map("density", Q, MASS, WEIGHT)
    ones, refs = [], []
    for _ in range(4):
        g.step()
        ones.append(s.moment("density", Q, MASS, WEIGHT))
        st = s.get()
        refs.append(T.moment("density", st.state, st.exit_step, Q, MASS, WEIGHT, n, d))
    tot, made = T.map_sum(refs)
    got, deposits, counted, steps = m.get()
    assert (deposits, counted, steps) == (4, sum(c for _, c in ones), 4) and counted == tot.counted > 0
    assert np.all(np.abs(got - sum(o for o, _ in ones)) <= T.bound(tot))
    assert np.all(np.abs(got - tot.out) <= T.bound(tot))
    E, B, recs = g.get_field(X.E), g.get_field(X.B), g.particles(sort)
    g.close()
    h, sort = riding_context(X)
    B0 = h.get_field(X.B)
    for _ in range(4):
        h.step()
    assert bits(h.get_field(X.E)) == bits(E) and bits(h.get_field(X.B)) == bits(B) and not np.array_equal(B, B0)
    for x, y in zip(recs, h.particles(sort)):
        assert bits(x) == bits(y)
    h.close()


# ---- 5. the host mirror's "moments" key
def test_gpu_host_tracer_moments(X, tmp_path):
    exe = os.path.join(os.path.dirname(os.path.abspath(X.__file__)), "host", "xpic_hip.out")
    d, dt, nt, period = 0.5, 0.5, 6, 2
    rng = np.random.default_rng(21)
    r = 2.0 + (rng.random((5, 3)) - 0.5)
    fo = np.column_stack([r, rng.normal(0, 0.4, (5, 3))])
    points = [{"coordinate": {"name": "PreciseCoordinate", "value": list(map(float, q[:3]))},
               "momentum": {"name": "PreciseMomentum", "value": list(map(float, q[3:]))}} for q in fo]
    moments = [{"moment": "density", "q": -1.0, "m": 1.0},
               {"moment": "momentum_flux", "q": -1.0, "m": 1.0, "weight": 0.5, "every": 2,
                "region": {"start": [1.0, 0.5, 1.0], "size": [2.0, 3.0, 1.5]}}]
    listing = {}
    for key, extra in (("with", {"moments": moments}), ("without", {})):
        out = tmp_path / key
        out.mkdir()
        cfg = {
            "Simulation": "ecsim", "OutputDirectory": str(out),
            "Geometry": {"x": 4.0, "y": 4.0, "z": 4.0, "t": nt * dt, "dx": d, "dy": d, "dz": d, "dt": dt, "diagnose_period": period * dt,
                         "da_boundary_x": "DM_BOUNDARY_PERIODIC", "da_boundary_y": "DM_BOUNDARY_PERIODIC",
                         "da_boundary_z": "DM_BOUNDARY_PERIODIC"},
            "Particles": [{"sort_name": "electrons", "Np": 1, "n": 1.0, "q": -1.0, "m": 1.0, "T": 0.0}],
            "Presets": [{"command": "SetMagneticField", "field": "B", "setter": {"name": "SetCoilsField", "coils": [
                {"z0": 1.0, "R": 1.5, "I": 2.0}, {"z0": 3.0, "R": 1.5, "I": 2.0}]}}],
            "Diagnostics": [dict({"diagnostic": "TracedParticles", "name": "fo", "kind": "full_orbit", "scheme": "EB2B", "qm": -1.0,
                                  "dt": 0.3, "points": points}, **extra)],
        }
        (out / "config.json").write_text(json.dumps(cfg))
        run = subprocess.run([exe, str(out / "config.json")], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
        listing[key] = sorted(os.listdir(out / "traced_particles_fo"))
    assert listing["without"] == ["2", "4", "6"]  # what it is without the key: the sample rows alone
    assert listing["with"] == ["2", "4", "6", "density", "momentum_flux"]
    base = tmp_path / "with" / "traced_particles_fo"
    for t in ("2", "4", "6"):
        assert bits(np.fromfile(base / t)) == bits(np.fromfile(tmp_path / "without" / "traced_particles_fo" / t))
        dens = np.fromfile(base / "density" / t, dtype=np.float32)
        flux = np.fromfile(base / "momentum_flux" / t, dtype=np.float32)
        assert dens.shape == (8 * 8 * 8,) and flux.shape == (4 * 6 * 3 * 6,)  # the region: 2.0 / d, 3.0 / d, 1.5 / d cells
        # the sample rows of the period are the states the maps saw: density after both steps, the flux after the second
        rows = np.fromfile(base / t).reshape(period, 5, 6)
        grid = ((8, 8, 8), (d, d, d))
        alive = np.full(5, -1)
        want = sum(T.moment("density", r, alive, -1.0, 1.0, 1.0, *grid).out for r in rows) / period
        assert 0.0 < dens.sum() <= 5.0 * (1 + 1e-6) and np.allclose(dens.reshape(8, 8, 8), want[..., 0], rtol=1e-6, atol=1e-9)
        want = T.moment("momentum_flux", rows[-1], alive, -1.0, 1.0, 0.5, *grid, region=(2, 1, 2, 4, 6, 3)).out[2:5, 1:7, 2:6]
        assert np.allclose(flux.reshape(3, 6, 4, 6), want, rtol=1e-6, atol=1e-9) and np.abs(want).max() > 0.0
    assert sorted(os.listdir(base / "density")) == sorted(os.listdir(base / "momentum_flux")) == ["2", "4", "6"]
