"""Tracer sets and xpic_grad_abs_field on the device (include/xpic_tracers.h).  The gradient is compared bit for bit with
its numpy statement (tests/tracers_ref.py, pinned without a GPU by tests/test_tracers_ref.py); everything about the sets
is a comparison between device results, bit for bit: a set against the open trace of the same batch on the same fields, a
set advanced in parts against one advanced at once, a set that rides with xpic_step against a shadow batch advanced by
one-step open traces on the fields read back after every step.  The static inputs are open_trace_ref's: an 8 x 8 x 8 grid,
3 x 256 + 7 particles, 150 steps sampled every 7 (the launch boundaries 64 and 128 are crossed)."""
import numpy as np
import pytest

import open_trace_ref as O
import tracers_ref as T

pytestmark = pytest.mark.gpu
KINDS = ["B1B", "EB2B", "CN", "dk"]
REGIONS = {"box": O.REGION, "cylinder": O.CYLINDER}


@pytest.fixture(scope="module")
def X():
    import xpic_amd

    return xpic_amd


def static_context(X):
    g = X.Context("basic", O.N, O.D, 0.7)
    shape = g.fshape()
    g.set_field(X.E, np.zeros(shape) + np.array(O.E_UNIFORM))
    g.set_field(X.B, np.zeros(shape) + np.array(O.B_UNIFORM))
    g.set_mirror_field(field=X.B, **O.MIRROR)
    g.set_field(X.W0, O.grad_abs(g.get_field(X.B)))
    return g


@pytest.fixture(scope="module")
def ctx(X):
    return static_context(X)


def batch(X, ctx, kind, region):
    p = O.particles("dk" if kind == "dk" else "fo", ctx.get_field(X.B))
    return O.with_cylinder_probes(p) if region == "cylinder" else p


def open_trace(X, ctx, kind, p, steps, region, gradB=None, **kw):
    if kind == "dk":
        return ctx.drift_kinetic_trace_open(p, steps, O.QM, O.MP, O.DT, region, gradB_field=X.W0 if gradB is None else gradB, **kw)
    return ctx.full_orbit_trace_open(p, steps, kind, O.QM, O.DT, region, **(O.CN_KW if kind == "CN" else {}), **kw)


def make_set(X, ctx, kind, p, region, gradB=None, **kw):
    if kind == "dk":
        return ctx.tracers("drift_kinetic", p, O.QM, O.MP, O.DT, region=region, gradB_field=X.W0 if gradB is None else gradB, **kw)
    return ctx.tracers("full_orbit", p, kind, O.QM, O.DT, region=region, **(O.CN_KW if kind == "CN" else {}), **kw)


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def same_as_open(got, samples, alive, ref, what):
    """a set's TracerState and drained samples against an OpenTrace"""
    for f in ("state", "exit_step", "iterations_sum", "iterations_max"):
        x, y = getattr(got, f), getattr(ref, f)
        assert x.shape == y.shape and x.dtype == y.dtype and bits(x) == bits(y), (what, f)
    assert got.removed == ref.removed and got.alive == len(ref.state) - ref.removed, what
    if samples is not None:
        assert samples.shape == ref.samples.shape and bits(samples) == bits(ref.samples), (what, "samples")
        assert bits(alive) == bits(ref.alive), (what, "alive")


# ---- 1. the gradient
def grid_field(n, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n[2], n[1], n[0], 3)) + np.array([0.0, 0.0, 3.0])


@pytest.mark.parametrize("n,d", [((8, 6, 5), (0.5, 0.25, 2.0)), ((2, 2, 3), (0.5, 0.25, 2.0)), ((70, 19, 18), (1.0, 0.3, 0.7))])
def test_gradient_bit_for_bit(X, n, d):
    """8 x 6 x 5 with three spacings; 2 x 2 x 3, whose folded axes are exactly 0; and 70 x 19 x 18: more than one tile of
    the kernel along every axis, none of them whole"""
    g = X.Context("ecsim", n, d, 0.5)  # (the scheme that takes an extent of 2)
    B, F = grid_field(n, 3), grid_field(n, 4)
    for src, dst, field in ((X.B, X.W0, B), (X.W1, X.W2, F)):
        g.set_field(src, field)
        others = {f: g.get_field(f) for f in (X.E, X.B, X.B0, X.W0, X.W1, X.W2) if f != dst}
        g.grad_abs_field(src, dst)
        got, want = g.get_field(dst), T.grad_abs(field, d)
        assert got.shape == want.shape and bits(got) == bits(want), (n, src, np.abs(got - want).max())
        for f, before in others.items():
            assert bits(g.get_field(f)) == bits(before), f
    if n == (2, 2, 3):
        got = g.get_field(X.W0)
        assert np.all(got[..., :2] == 0.0) and np.abs(got[..., 2]).min() > 0.0
    before = {f: g.get_field(f) for f in (X.E, X.B, X.W0, X.W1, X.W2)}
    with pytest.raises(X.XpicError, match="same vector"):
        g.grad_abs_field(X.B, X.B)
    for f, b in before.items():
        assert bits(g.get_field(f)) == bits(b), f
    g.close()


# ---- 2. a set on static fields is the open trace
@pytest.fixture(scope="module", params=[(k, r) for k in KINDS for r in REGIONS])
def case(request, X, ctx):
    kind, region = request.param
    p = batch(X, ctx, kind, region)
    ref = open_trace(X, ctx, kind, p, O.STEPS, REGIONS[region], sample_every=O.EVERY)
    assert 0 < ref.removed < len(p)
    return kind, region, p, ref


@pytest.mark.parametrize("compact", ["auto", "never", "always"])
def test_set_equals_open_trace(X, ctx, case, compact):
    kind, region, p, ref = case
    s = make_set(X, ctx, kind, p, REGIONS[region], compact=compact, sample_every=O.EVERY, sample_capacity=O.STEPS // O.EVERY)
    s.advance(O.STEPS)
    got = s.get()
    assert (got.steps, got.held, got.dropped) == (O.STEPS, O.STEPS // O.EVERY, 0)
    samples, alive = s.samples()
    same_as_open(got, samples, alive, ref, (kind, region, compact))
    assert s.get().held == 0
    s.close()


def test_advance_composes(X, ctx, case):
    """70 + 80 steps equal 150, the sample rows included, whether the buffer is drained in between or not"""
    kind, region, p, ref = case
    for drain in (False, True):
        s = make_set(X, ctx, kind, p, REGIONS[region], compact="always", sample_every=O.EVERY, sample_capacity=O.STEPS // O.EVERY)
        s.advance(O.SPLIT)
        first = s.samples() if drain else None
        s.advance(O.STEPS - O.SPLIT)
        samples, alive = s.samples()
        if drain:
            assert len(first[0]) == O.SPLIT // O.EVERY
            samples, alive = np.concatenate([first[0], samples]), np.concatenate([first[1], alive])
        same_as_open(s.get(), samples, alive, ref, (kind, region, drain))
        s.close()


def test_every_full_orbit_scheme(X, ctx):
    p = batch(X, ctx, "fo", "box")[:300]
    for scheme in X.FO_SCHEMES:
        kw = O.CN_KW if scheme == "CN" else {}
        ref = ctx.full_orbit_trace_open(p, 70, scheme, O.QM, O.DT, O.REGION, sample_every=O.EVERY, step0=5, **kw)
        s = ctx.tracers("full_orbit", p, scheme, O.QM, O.DT, region=O.REGION, step0=5, sample_every=O.EVERY, sample_capacity=10, **kw)
        s.advance(70)
        same_as_open(s.get(), *s.samples(), ref, scheme)
        s.close()


def test_no_region_removes_nothing(X, ctx):
    p = batch(X, ctx, "fo", "box")
    closed = ctx.full_orbit_trace(p, 70, "EB2B", O.QM, O.DT, sample_every=O.EVERY)
    s = ctx.tracers("full_orbit", p, "EB2B", O.QM, O.DT, sample_every=O.EVERY, sample_capacity=10)
    s.advance(70)
    got = s.get()
    samples, alive = s.samples()
    assert bits(got.state) == bits(closed[0]) and bits(samples) == bits(closed[1])
    assert (got.exit_step == -1).all() and got.removed == 0 and (alive == len(p)).all()
    s.close()


# ---- 3. XPIC_GRADB_AUTO
def test_gradb_auto_recomputes(X):
    g = static_context(X)
    p = batch(X, g, "dk", "box")
    guard = np.full(g.fshape(), 7.25)
    g.set_field(X.W0, O.grad_abs(g.get_field(X.B)))
    ref1 = open_trace(X, g, "dk", p, 40, O.REGION, sample_every=O.EVERY)
    for f in (X.W0, X.W1, X.W2):
        g.set_field(f, guard)
    E0, B0 = g.get_field(X.E), g.get_field(X.B)
    s = make_set(X, g, "dk", p, O.REGION, gradB="auto", sample_every=O.EVERY, sample_capacity=20)
    s.advance(40)
    for f in (X.W0, X.W1, X.W2):
        assert bits(g.get_field(f)) == bits(guard), f
    assert bits(g.get_field(X.E)) == bits(E0) and bits(g.get_field(X.B)) == bits(B0)
    mid = s.get()
    for f in ("state", "exit_step", "iterations_sum", "iterations_max"):
        assert bits(getattr(mid, f)) == bits(getattr(ref1, f)), f
    # another mirror field: the set must follow it
    B2 = np.zeros(g.fshape()) + np.array(O.B_UNIFORM) + O.mirror_field(O.N, O.D, D=6.0, R=2.5, I=3.0)
    g.set_field(X.B, B2)
    s.advance(40)
    assert bits(g.get_field(X.B)) == bits(B2)
    for f in (X.W0, X.W1, X.W2):
        assert bits(g.get_field(f)) == bits(guard), f
    got = s.get()
    samples, alive = s.samples()
    g.set_field(X.W0, T.grad_abs(B2, O.D))
    ref2 = open_trace(X, g, "dk", ref1.state, 40, O.REGION, sample_every=O.EVERY, exit_step=ref1.exit_step, step0=40)
    assert not np.array_equal(T.grad_abs(B2, O.D), O.grad_abs(B0))
    for f in ("state", "exit_step"):
        assert bits(getattr(got, f)) == bits(getattr(ref2, f)), f
    assert bits(got.iterations_sum) == bits(ref1.iterations_sum + ref2.iterations_sum)
    assert bits(got.iterations_max) == bits(np.maximum(ref1.iterations_max, ref2.iterations_max))
    assert got.removed == ref1.removed + ref2.removed
    # rows 0 .. 4 are the first call's (steps 7 .. 35); step 42 is the second call's step 2: not on its own sample grid,
    # so the second half is compared through the state and the exit steps above, the first through its rows
    assert bits(samples[:5]) == bits(ref1.samples) and bits(alive[:5]) == bits(ref1.alive) and len(samples) == 80 // O.EVERY
    s.close()
    g.close()


# ---- 4. attached to a run
def loaded_context(X, scheme, n, ppc=4, seed=2):
    d, dt = (0.5, 0.5, 0.5), 0.1  # (inside the explicit scheme's Courant limit d / sqrt(3))
    g = X.Context(scheme, n, d, dt)
    rng = np.random.default_rng(seed)
    L = np.array(n) * np.array(d)
    sorts = []
    for q, m in ((-1.0, 1.0), (1.0, 100.0)):
        s = g.add_sort(ppc, 1.0, q, m, capacity=4 * ppc * n[0] * n[1] * n[2])
        npart = ppc * n[0] * n[1] * n[2]
        pts = np.empty((npart, 6))
        pts[:, :3] = rng.random((npart, 3)) * L
        pts[:, 3:] = rng.normal(0, 0.05 / np.sqrt(m), (npart, 3))
        assert g.add_particles(s, pts) == npart
        sorts.append(s)
    B = np.zeros(g.fshape()) + np.array([0.0, 0.0, 0.3]) + 0.05 * rng.normal(size=g.fshape())
    g.set_field(X.B, B)
    g.set_field(X.B0, np.zeros(g.fshape()) + np.array([0.0, 0.0, 0.3]))
    g.set_tolerances(1e-10, 1e-50, 200)
    return g, sorts, d, L


def tracer_batches(L, nt=300, seed=9):
    rng = np.random.default_rng(seed)
    r = 0.5 * L + (rng.random((nt, 3)) - 0.5)
    fo = np.column_stack([r, rng.normal(0, 0.4, (nt, 3))])
    dk = np.column_stack([r, rng.normal(0, 0.4, nt), 0.1 + 0.2 * rng.random(nt), 0.05 + 0.05 * rng.random(nt)])
    return fo, dk


@pytest.mark.parametrize("scheme,n", [("ecsim", (8, 8, 8)), ("basic", (6, 6, 6)), ("ecsimcorr", (6, 6, 6))])
def test_attached_sets_follow_the_run(X, scheme, n):
    g, sorts, d, L = loaded_context(X, scheme, n)
    region = {"name": "box", "min": (0.0, 0.0, 1.0), "max": (float(L[0]), float(L[1]), float(L[2]) - 1.0)}
    fo, dk = tracer_batches(L)
    qm, mp, dt, every, steps = -1.0, 1.0, 0.3, 2, 6
    sf = g.tracers("full_orbit", fo, "B1B", qm, dt, region=region, sample_every=every, sample_capacity=8)
    sd = g.tracers("drift_kinetic", dk, qm, mp, dt, region=region, gradB_field="auto", sample_every=every, sample_capacity=8)
    small = g.tracers("drift_kinetic", dk[:40], qm, mp, dt, region=region, gradB_field="auto", sample_every=1, sample_capacity=2)
    sf.attach()
    sd.attach()
    small.attach()  # a second guiding-centre set, whose buffer fills after two steps: the steps go on
    shadow = {"fo": [fo, np.full(len(fo), -1, dtype=np.int64), []], "dk": [dk, np.full(len(dk), -1, dtype=np.int64), []]}
    B_seen = []
    for k in range(steps):
        g.step()
        B = g.get_field(X.B)
        B_seen.append(B)
        g.set_field(X.W0, T.grad_abs(B, d))  # (a scratch vector of the step: nothing reads it before the step rewrites it)
        a = g.full_orbit_trace_open(shadow["fo"][0], 1, "B1B", qm, dt, region, exit_step=shadow["fo"][1], step0=k)
        b = g.drift_kinetic_trace_open(shadow["dk"][0], 1, qm, mp, dt, region, gradB_field=X.W0, exit_step=shadow["dk"][1], step0=k)
        for name, r in (("fo", a), ("dk", b)):
            shadow[name][0], shadow[name][1] = r.state, r.exit_step
            if (k + 1) % every == 0:
                shadow[name][2].append(r.state)
    assert not np.array_equal(B_seen[0], B_seen[-1])  # the fields did move
    for name, s in (("fo", sf), ("dk", sd)):
        got = s.get()
        samples, alive = s.samples()
        assert got.steps == steps and got.held == steps // every
        assert bits(got.state) == bits(shadow[name][0]), (scheme, name)
        assert bits(got.exit_step) == bits(shadow[name][1]), (scheme, name)
        assert bits(samples) == bits(np.array(shadow[name][2])), (scheme, name)
        assert got.removed == (shadow[name][1] >= 0).sum() and 0 < got.alive
        assert not np.array_equal(got.state, fo if name == "fo" else dk)
    got = small.get()
    assert (got.steps, got.held, got.dropped) == (steps, 2, steps - 2)
    assert bits(small.samples()[0][1]) == bits(np.array(shadow["dk"][2])[0][:40])  # (row 1 is step 2: the shadow's first row)
    # detach: the step no longer carries the set, advance still does
    sf.detach()
    g.step()
    assert sf.get().steps == steps and sd.get().steps == steps + 1
    sf.advance(2)
    assert sf.get().steps == steps + 2
    g.close()


# ---- 5. passivity
def test_sets_are_passive(X):
    g, sorts, d, L = loaded_context(X, "ecsim", (8, 8, 8))
    g.step()
    fo, dk = tracer_batches(L)
    sf = g.tracers("full_orbit", fo, "EB2B", -1.0, 0.3, sample_every=1, sample_capacity=4)
    sd = g.tracers("drift_kinetic", dk, -1.0, 1.0, 0.3, gradB_field="auto", sample_every=1, sample_capacity=4)
    before = [g.get_field(X.E), g.get_field(X.B)] + [a for s in sorts for a in g.particles(s)]
    sf.advance(3)
    sd.advance(3)
    sf.samples(), sd.samples(), sf.get(), sd.get()
    after = [g.get_field(X.E), g.get_field(X.B)] + [a for s in sorts for a in g.particles(s)]
    for a, b in zip(before, after):
        assert bits(a) == bits(b)
    assert not np.array_equal(sf.get().state, fo) and not np.array_equal(sd.get().state, dk)
    g.close()


# ---- 6. limits
def test_limits(X):
    g = static_context(X)
    p = batch(X, g, "fo", "box")
    empty = g.tracers("full_orbit", np.zeros((0, 6)), "B1B", O.QM, O.DT, region=O.REGION, sample_every=2, sample_capacity=3)
    empty.advance(5)
    e = empty.get()
    assert e.state.shape == (0, 6) and (e.steps, e.removed, e.alive, e.held, e.dropped) == (5, 0, 0, 2, 0)
    assert empty.samples()[0].shape == (2, 0, 6)
    sets = [empty] + [g.tracers("full_orbit", p[:4], "B1B", O.QM, O.DT) for _ in range(X.TRACERS_MAX_SETS - 1)]
    with pytest.raises(X.XpicError, match="already has 8 sets"):
        g.tracers("full_orbit", p[:4], "B1B", O.QM, O.DT)
    gone = sets.pop().id
    g._ck(g.L.xpic_tracers_destroy(g.h, gone))
    for call in (lambda: g.L.xpic_tracers_advance(g.h, gone, 1), lambda: g.L.xpic_tracers_attach(g.h, gone, 1),
                 lambda: g.L.xpic_tracers_get(g.h, gone, None, None, None, None, None),
                 lambda: g.L.xpic_tracers_destroy(g.h, gone), lambda: g.L.xpic_tracers_advance(g.h, 12345, 1)):
        with pytest.raises(X.XpicError, match="does not exist"):
            g._ck(call())
    # a buffer of 3 rows with 10 due: 3 held, 7 dropped, and the calls succeed; the rows held are the first three
    s = g.tracers("full_orbit", p, "B1B", O.QM, O.DT, region=O.REGION, sample_every=O.EVERY, sample_capacity=3)
    s.advance(O.SPLIT)
    got = s.get()
    assert (got.steps, got.held, got.dropped) == (O.SPLIT, 3, 7)
    ref = g.full_orbit_trace_open(p, O.SPLIT, "B1B", O.QM, O.DT, O.REGION, sample_every=O.EVERY)
    samples, alive = s.samples()
    assert bits(samples) == bits(ref.samples[:3]) and bits(alive) == bits(ref.alive[:3]) and bits(got.state) == bits(ref.state)
    s.advance(O.EVERY)  # the next row due lands in the emptied buffer's row 0
    rest = g.full_orbit_trace_open(ref.state, O.EVERY, "B1B", O.QM, O.DT, O.REGION, sample_every=O.EVERY, exit_step=ref.exit_step,
                                   step0=O.SPLIT)
    samples, alive = s.samples()
    assert bits(samples) == bits(rest.samples) and bits(alive) == bits(rest.alive) and s.get().dropped == 7
    s.close()
    # a particle whose cell fails the region at the start: exit_step = step0, the record untouched
    q = p[:8].copy()
    q[:3, 2] = (0.5, 7.5, 7.999)
    s = g.tracers("full_orbit", q, "B1B", O.QM, O.DT, region=O.REGION, step0=11)
    s.advance(3)
    got = s.get()
    assert (got.exit_step[:3] == 11).all() and bits(got.state[:3]) == bits(q[:3]) and (got.exit_step[3:] == -1).all()
    assert not np.array_equal(got.state[3:], q[3:]) and (got.removed, got.alive) == (3, 5)
    s.close()
    g.close()
    for kw in (dict(self_ring=True), dict(rank=0, nranks=2)):
        h = X.Context("basic", (8, 8, 12), (0.5, 0.5, 0.5), 0.7, **kw)
        with pytest.raises(X.XpicError, match="several z-slabs"):
            h.tracers("full_orbit", p[:4], "B1B", O.QM, O.DT)
        with pytest.raises(X.XpicError, match="several z-slabs"):
            h.grad_abs_field(X.B, X.W0)
        h.close()


# ---- 7. the host mirror's "TracedParticles" diagnostic
def test_host_mirror_traced_particles(X, tmp_path):
    """Configuration used: one sort that is never loaded (the executable's tables want a sort; no particle exists), ecsim
    on 8 x 8 x 8, a coils field set into B alone (B0 = 0), so rot B drives E and
    both fields change every step.  Without particles the step has no floating-point atomics, so the executable's run and
    the same run made here, in another process, agree bit for bit, and the rows are compared on evolving fields.  (With
    sorts the deposits' atomics make two runs differ in the last bits, as the issue foresees.)"""
    import json
    import os
    import subprocess

    exe = os.path.join(os.path.dirname(os.path.abspath(X.__file__)), "host", "xpic_hip.out")
    n, d, dt, nt, period = (8, 8, 8), 0.5, 0.5, 6, 2
    coils = [{"z0": 1.0, "R": 1.5, "I": 2.0}, {"z0": 3.0, "R": 1.5, "I": 2.0}]
    rng = np.random.default_rng(21)
    r = 2.0 + (rng.random((5, 3)) - 0.5)
    fo = np.column_stack([r, rng.normal(0, 0.4, (5, 3))])
    dk = np.column_stack([r, rng.normal(0, 0.4, 5), 0.1 + 0.2 * rng.random(5), 0.05 + 0.05 * rng.random(5)])
    region = {"name": "BoxGeometry", "min": [0.0, 0.0, 1.0], "max": [4.0, 4.0, 3.0]}

    def points(p):
        return [{"coordinate": {"name": "PreciseCoordinate", "value": list(map(float, q[:3]))},
                 "momentum": {"name": "PreciseMomentum", "value": list(map(float, q[3:]))}} for q in p]
    cfg = {
        "Simulation": "ecsim", "OutputDirectory": str(tmp_path),
        "Geometry": {"x": 4.0, "y": 4.0, "z": 4.0, "t": nt * dt, "dx": d, "dy": d, "dz": d, "dt": dt, "diagnose_period": period * dt,
                     "da_boundary_x": "DM_BOUNDARY_PERIODIC", "da_boundary_y": "DM_BOUNDARY_PERIODIC",
                     "da_boundary_z": "DM_BOUNDARY_PERIODIC"},
        "Particles": [{"sort_name": "electrons", "Np": 1, "n": 1.0, "q": -1.0, "m": 1.0, "T": 0.0}],
        "Presets": [{"command": "SetMagneticField", "field": "B", "setter": {"name": "SetCoilsField", "coils": coils}}],
        "Diagnostics": [
            {"diagnostic": "TracedParticles", "name": "fo", "kind": "full_orbit", "scheme": "EB2B", "qm": -1.0, "dt": 0.3,
             "points": points(fo), "region": region},
            {"diagnostic": "TracedParticles", "name": "gc", "kind": "drift_kinetic", "qm": -1.0, "mp": 1.0, "dt": 0.3,
             "points": points(dk)}],
    }
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    out = subprocess.run([exe, str(tmp_path / "config.json")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    # the same run from Python
    g = X.Context("ecsim", n, (d, d, d), dt)
    g.add_sort(1, 1.0, -1.0, 1.0, capacity=1 << 16)
    g.set_coils_field([(c["z0"], c["R"], c["I"]) for c in coils], field=X.B)
    B_first = g.get_field(X.B)
    box = {"name": "box", "min": region["min"], "max": region["max"]}
    sets = {"fo": g.tracers("full_orbit", fo, "EB2B", -1.0, 0.3, region=box, compact="auto", sample_every=1, sample_capacity=period + 1),
            "gc": g.tracers("drift_kinetic", dk, -1.0, 1.0, 0.3, gradB_field="auto", sample_every=1, sample_capacity=period + 1)}
    for s in sets.values():
        s.attach()
    for t in range(1, nt + 1):
        g.step()
        if t % period:
            continue
        for name, s in sets.items():
            want = s.samples()[0]
            path = tmp_path / ("traced_particles_" + name) / str(t)
            got = np.fromfile(path, dtype=np.float64).reshape(-1, 5, 6)
            assert got.shape == want.shape == (period, 5, 6) and bits(got) == bits(want), (name, t)
    assert not np.array_equal(g.get_field(X.B), B_first) and np.abs(g.get_field(X.E)).max() > 0.0  # the fields did move
    assert not np.array_equal(sets["fo"].get().state, fo) and not np.array_equal(sets["gc"].get().state, dk)
    assert sorted(os.listdir(tmp_path / "traced_particles_fo")) == ["2", "4", "6"]
    g.close()
