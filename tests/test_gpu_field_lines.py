"""The field-line tracer on the device (xpic_amd/csrc/field_lines.hip, include/xpic_field_lines.h) against its numpy
restatement (tests/field_lines_ref.py, pinned on closed forms by tests/test_field_lines_ref.py), against the closed forms
themselves, and against itself (launch lengths, directions, samples, batch sizes).

Tolerances.  One step: 1e-13 of the compared quantity's scale, the project's bound for a gather reached through one step
(tests/test_gpu_full_orbit.py).  Forty steps: measured, not fixed -- the restatement runs in float64 and in np.longdouble on
the same inputs, and the device may differ from the float64 run by 16 x their largest difference (the margin is for the
device's different but legal order of the gather's sum), but not by less than 1e-13 of scale.  Both numbers are printed.
The seeds of these two comparisons are full_orbit_ref.case_particles' positions (beyond both faces on every axis) less the
lanes whose line meets |F| < 0.05: the direction F / |F| magnifies a gather's rounding by scale / |F|, which says nothing
about the tracer."""
import json
import os
import subprocess

import numpy as np
import pytest

import analytic_trace_ref as AT
import field_lines_ref as R
import full_orbit_ref as FO
import open_trace_ref as O
import test_field_lines_ref as T

pytestmark = pytest.mark.gpu
FIELDS = ("length", "volume", "fmin", "smin", "fmax")


@pytest.fixture(scope="module")
def X():
    import xpic_amd

    return xpic_amd


@pytest.fixture(scope="module")
def fields():
    return FO.case_fields()


@pytest.fixture(scope="module")
def ctx(X, fields):
    g = X.Context("basic", FO.N, FO.D, 0.7)
    g.set_field(X.E, fields[0])
    g.set_field(X.B, fields[1])
    return g


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def row(res, d):
    """direction d of a FieldLines (or of field_lines_ref.lines' result) as field_lines_ref.Lines"""
    return R.Lines(*(None if getattr(res, f) is None else getattr(res, f)[d] for f in R.Lines._fields))


def same_bits(a, b, what):
    for f in R.Lines._fields:
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None) and (x is None or (x.shape == y.shape and bits(x) == bits(y))), (what, f)


def steady_seeds(F, stagger, h, steps):
    """case_particles' positions whose lines, both ways, stay where |F| >= 0.05 (see the top of this file)"""
    seeds = FO.case_particles()[:, :3]
    ref = R.lines(R.grid_source(F, FO.D, stagger), seeds, h, steps)
    seeds = seeds[ref.fmin.min(axis=0) >= 0.05]
    assert len(seeds) > 700 and ((seeds < 0).any(axis=0) & (seeds > 8).any(axis=0)).all()  # the seam is still exercised
    return seeds


def compare(got, ref, wide, what, rel=1e-13):
    """steps and code exact; end and the accumulators within max(16 x |ref - wide|, rel x scale) -> those tolerances"""
    assert np.array_equal(got.steps, ref.steps) and np.array_equal(got.code, ref.code), what
    tol = {}
    for f in ("end",) + FIELDS:
        x, y = getattr(got, f), getattr(ref, f)
        scale = np.abs(y).max()
        spread = 0.0 if wide is None else float(np.abs(y - getattr(wide, f).astype(np.float64)).max())
        err = np.abs(x - y).max()
        print(what, f, "max |gpu - restatement| =", err, " |float64 - longdouble| =", spread, " scale", scale)
        tol[f] = max(16 * spread, rel * scale)
        assert np.isfinite(x).all() and err <= tol[f], (what, f)
    return tol


@pytest.mark.parametrize("stagger", ["B", "E"])
def test_one_step(X, ctx, fields, stagger):
    F, fid, sid = (fields[1], X.B, R.STAGGER_B) if stagger == "B" else (fields[0], X.E, R.STAGGER_E)
    h = 0.3
    seeds = steady_seeds(F, sid, h, 1)
    got = ctx.field_lines(seeds, field=fid, h=h, max_steps=1)
    ref = R.lines(R.grid_source(F, FO.D, sid), seeds, h, 1)
    assert (got.steps == 1).all() and (got.code == R.MAXSTEPS).all()
    compare(got, ref, None, "one step " + stagger)
    # the field itself, through fmin and fmax of a lane: to 1e-13 of the field's scale
    assert np.abs(got.fmax - ref.fmax).max() <= 1e-13 * np.abs(F).max() and np.abs(got.fmin - ref.fmin).max() <= 1e-13 * np.abs(F).max()


@pytest.mark.parametrize("stagger", ["B", "E"])
def test_forty_steps(X, ctx, fields, stagger):
    F, fid, sid = (fields[1], X.B, R.STAGGER_B) if stagger == "B" else (fields[0], X.E, R.STAGGER_E)
    h, S = 0.1, 40
    seeds = steady_seeds(F, sid, h, S)
    src = R.grid_source(F, FO.D, sid)
    got = ctx.field_lines(seeds, field=fid, h=h, max_steps=S)
    ref, wide = R.lines(src, seeds, h, S), R.lines(src, seeds, h, S, dtype=np.longdouble)
    assert (ref.steps == S).all()
    compare(got, ref, wide, "forty steps " + stagger)
    assert np.array_equal(got.total_length, got.length[0] + got.length[1])
    assert np.array_equal(got.mirror_ratio, got.fmax.max(axis=0) / got.fmin.min(axis=0)) and (got.mirror_ratio >= 1.0).all()
    assert got.codes.shape == (len(seeds), 2) and got.ends.shape == (len(seeds), 2, 3)


def test_uniform_field(X):
    g = X.Context("basic", R.UNIFORM_N, R.UNIFORM_D, 0.7)
    g.set_field(X.B, R.uniform_field())
    seeds = T.uniform_seeds()
    got = g.field_lines(seeds, h=T.H_UNIFORM, max_steps=T.S_UNIFORM)
    for d, sign in ((0, +1), (1, -1)):
        T.check_uniform(row(got, d), seeds, sign)
    assert np.abs(got.total_volume - 2 * T.S_UNIFORM * T.H_UNIFORM / 2.0).max() <= 1e-13
    g.close()


@pytest.mark.parametrize("stagger", ["B", "E"])
def test_circle_field(X, stagger):
    sid = X.STAGGERS[stagger]
    F = R.circle_field(sid)
    g = X.Context("basic", R.CIRCLE_N, R.CIRCLE_D, 0.7)
    g.set_field(X.W0, F)  # a work vector filled like B, or like E
    rad, seeds = np.array(R.CIRCLE_RADII), R.circle_seeds()
    got = g.field_lines(seeds, field=X.W0, stagger=stagger, h=R.CIRCLE_H, max_steps=T.S_CIRCLE)
    closed = g.field_lines(seeds, field=X.W0, stagger=stagger, h=R.CIRCLE_H, max_steps=400, close_tol=R.CIRCLE_H)
    ref = R.lines(R.grid_source(F, R.CIRCLE_D, sid), seeds, R.CIRCLE_H, 400, close_tol=R.CIRCLE_H)
    for d in (0, 1):
        T.check_circle(row(got, d), rad)
        T.check_closed(row(closed, d), rad)
    assert np.array_equal(closed.steps, ref.steps) and np.array_equal(closed.code, ref.code)  # the restatement's count
    if stagger == "B":  # the wrong stagger is as visible here as in the restatement
        wrong = g.field_lines(seeds, field=X.W0, stagger="E", h=R.CIRCLE_H, max_steps=T.S_CIRCLE)
        with pytest.raises(AssertionError):
            T.check_circle(row(wrong, 0), rad)
    g.close()


def test_model_source(X):
    """the Gaussian mirror: the model form against the restatement on xpic_model_fields' values, and against the grid form
    on xpic_set_model_field of the same model, within the restatement's own difference between the two"""
    n, d = (40, 40, 40), (0.25, 0.25, 0.25)
    g = X.Context("basic", n, d, 0.7)
    model = X.field_model("gaussian_mirror", **AT.GAUSSIAN)
    rng = np.random.default_rng(3)
    seeds = np.column_stack([5.0 + 0.6 * (rng.random((65, 2)) - 0.5), 3.0 + 4.0 * rng.random(65)])
    h, S = 0.05, 40
    got = g.model_field_lines(model, seeds, h=h, max_steps=S)
    src = R.function_source(lambda r: g.model_fields(model, r)[1])
    ref, wide = R.lines(src, seeds, h, S), R.lines(src, seeds, h, S, dtype=np.longdouble)
    tol_model = compare(got, ref, wide, "model")
    assert (got.mirror_ratio > 1.0).all() and (got.code == R.MAXSTEPS).all()
    g.set_model_field(model, E_field=None, B_field=X.B)
    on_grid = g.field_lines(seeds, field=X.B, h=h, max_steps=S)
    gsrc = R.grid_source(g.get_field(X.B), d)
    gref, gwide = R.lines(gsrc, seeds, h, S), R.lines(gsrc, seeds, h, S, dtype=np.longdouble)
    tol_grid = compare(on_grid, gref, gwide, "model on the grid")
    for f in ("end",) + FIELDS:
        between, allowed = np.abs(getattr(on_grid, f) - getattr(got, f)), np.abs(getattr(gref, f) - getattr(ref, f))
        print("grid form - model form", f, between.max(), " the restatement's:", allowed.max())
        assert (between <= allowed + tol_model[f] + tol_grid[f]).all(), f  # (each device result is that close to its restatement)
    # the model form needs no single z-slab
    two = X.Context("basic", (8, 8, 12), (0.5, 0.5, 0.5), 0.7, rank=0, nranks=2)
    other = two.model_field_lines(model, seeds, h=h, max_steps=S)
    assert bits(other.end) == bits(got.end) and bits(other.volume) == bits(got.volume)
    two.close()
    g.close()


BOX = {"name": "box", "min": (1.0, 1.0, 1.0), "max": (7.0, 7.0, 7.0)}  # strictly inside the 8 x 8 x 8 domain


def region_seeds():
    rng = np.random.default_rng(11)
    seeds = 2.5 + 3.0 * rng.random((257, 3))
    seeds[:3] = [(0.5, 4.0, 4.0), (7.6, 7.5, 4.0), (4.0, 4.0, 7.2)]  # outside either region at the start
    return seeds


@pytest.mark.parametrize("name", ["box", "cylinder"])
def test_left(X, ctx, fields, name):
    region = BOX if name == "box" else O.CYLINDER
    seeds, h, S = region_seeds(), 0.1, 120
    got = ctx.field_lines(seeds, h=h, max_steps=S, region=region)
    ref = R.lines(R.grid_source(fields[1], FO.D), seeds, h, S, keep=R.region_keep(region, FO.D))
    assert (ref.steps[:, :3] == 0).all() and (ref.code[:, :3] == R.LEFT).all()
    left = ref.code == R.LEFT
    assert left.sum() > 300 and (ref.steps[left] > 0).sum() > 300 and len(np.unique(ref.steps[left])) > 20
    assert np.array_equal(got.steps, ref.steps) and np.array_equal(got.code, ref.code)  # the exact step at which each leaves
    assert bits(got.end[:, :3]) == bits(np.stack([seeds[:3], seeds[:3]]))


def test_null(X, fields):
    """a block of B nodes zeroed, as test_gpu_full_orbit.test_zero_field_patch does, and f_floor = 0.05: seeds inside the
    block stop at once, lines that run into it stop at its edge, with the restatement's step"""
    B = fields[1].copy()
    B[2:6, 2:6, 2:6, :] = 0.0
    g = X.Context("basic", FO.N, FO.D, 0.7)
    g.set_field(X.B, B)
    rng = np.random.default_rng(7)
    seeds = np.vstack([4.0 + (rng.random((16, 3)) * 2 - 1) * 0.4, np.column_stack([1.0 + 6.0 * rng.random((100, 2)), 0.2 + 0.6 * rng.random(100)])])
    seeds[0] = 4.0
    assert not R.grid_source(B, FO.D)(seeds[:16]).any()
    h, S = 0.1, 80
    got = g.field_lines(seeds, h=h, max_steps=S, f_floor=0.05)
    ref = R.lines(R.grid_source(B, FO.D), seeds, h, S, f_floor=0.05)
    assert (ref.code[:, :16] == R.NULL).all() and (ref.steps[:, :16] == 0).all()
    later = (ref.code == R.NULL) & (ref.steps > 0)
    assert later.sum() >= 10 and (ref.code == R.MAXSTEPS).sum() >= 10
    assert np.array_equal(got.steps, ref.steps) and np.array_equal(got.code, ref.code)
    assert bits(got.end[:, :16]) == bits(np.stack([seeds[:16], seeds[:16]]))
    assert (got.fmin[:, :16] == 0.0).all() and (got.fmax[:, :16] == 0.0).all() and (got.volume[:, :16] == 0.0).all()
    assert np.isfinite(got.volume).all() and np.isfinite(got.end).all() and (got.fmin[later] >= 0.05).all()
    g.close()


def test_launches_directions_and_samples(X, ctx):
    seeds, h, S = region_seeds(), 0.1, 45
    kw = dict(h=h, max_steps=S, region=BOX, sample_every=4)
    whole = ctx.field_lines(seeds, **kw)
    assert {0, 1} <= set(np.unique(whole.code)) and whole.samples.shape == (2, len(seeds), 11, 3)
    for ls in (1, 7):
        same_bits(ctx.field_lines(seeds, launch_steps=ls, **kw), whole, "launch_steps %d" % ls)
    for name, d in (("+", 0), ("-", 1)):
        one = ctx.field_lines(seeds, directions=name, **kw)
        same_bits(row(one, d), row(whole, d), "direction " + name)
        assert (one.code[1 - d] == -1).all() and not one.end[1 - d].any() and one.directions == d + 1
        assert np.array_equal(one.total_length, whole.length[d])
    # a row that was not asked for is not written: the library leaves the caller's array alone
    n = len(seeds)
    end = np.full((2, n, 3), 7.25)
    arr = [np.full((2, n), 7.25) for _ in range(5)]
    steps, code = np.full((2, n), 7, dtype=np.int64), np.full((2, n), 7, dtype=np.int32)
    P = X.LineParams(h, S, 0.0, 0.0, 0, 2, 0, 0)
    ptr = lambda a: a.ctypes.data_as(X.c_dp)  # noqa: E731
    ctx._ck(ctx.L.xpic_field_lines(ctx.h, X.B, n, ptr(np.ascontiguousarray(seeds)), P, None, 0, ptr(end), *(ptr(a) for a in arr),
                                   steps.ctypes.data_as(X.CTYPES["int64_t*"]), code.ctypes.data_as(X.CTYPES["int32_t*"]), None))
    assert (end[0] == 7.25).all() and all((a[0] == 7.25).all() for a in arr) and (steps[0] == 7).all() and (code[0] == 7).all()
    assert (code[1] == R.MAXSTEPS).all() and (steps[1] == S).all() and not (end[1] == 7.25).any()
    # sample row k is the end point of a call of (k + 1) * 4 steps; behind a lane's last step its last point repeats
    free = ctx.field_lines(seeds, h=h, max_steps=S, sample_every=4)
    for k in (0, 4, 10):
        short = ctx.field_lines(seeds, h=h, max_steps=4 * (k + 1))
        assert bits(free.samples[:, :, k]) == bits(short.end), k
    held = np.minimum(whole.steps // 4, 11)
    stopped = 0
    for d in (0, 1):
        for q in range(n):
            assert (whole.samples[d, q, held[d, q]:] == whole.end[d, q]).all()
            assert bits(whole.samples[d, q, :held[d, q]]) == bits(free.samples[d, q, :held[d, q]])
            stopped += held[d, q] < 11
    assert stopped > 100


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_ragged_sizes(X, ctx, n):
    seed = np.array([[3.3, 4.1, 2.7]])
    kw = dict(h=0.1, max_steps=30, region=BOX, sample_every=5)
    one = ctx.field_lines(seed, **kw)
    many = ctx.field_lines(np.repeat(seed, n, axis=0), **kw)
    for f in R.Lines._fields:
        x, y = getattr(many, f), getattr(one, f)
        assert x.shape[:2] == (2, n) and bits(x) == bits(np.repeat(y, n, axis=1)), f


def test_refusals_and_limits(X, ctx):
    seeds = region_seeds()[3:8]
    n = len(seeds)
    model = X.field_model("gaussian_mirror", **AT.GAUSSIAN)
    ok = dict(h=0.1, max_steps=5)
    for kw, message in ((dict(ok, h=0.0), "h must be positive"), (dict(ok, h=-1.0), "h must be positive"),
                        (dict(ok, h=np.inf), "h must be positive"), (dict(ok, max_steps=0), "max_steps must be within"),
                        (dict(ok, max_steps=(1 << 24) + 1), "max_steps must be within"), (dict(ok, field=99), "unknown or unallocated field id"),
                        (dict(ok, field=-1), "unknown or unallocated field id"), (dict(ok, f_floor=-1.0), "f_floor is negative"),
                        (dict(ok, close_tol=np.nan), "close_tol is negative"), (dict(ok, directions=0), "directions must be"),
                        (dict(ok, directions=4), "directions must be"), (dict(ok, stagger=2), "stagger must be"),
                        (dict(ok, launch_steps=-1), "launch_steps must be"), (dict(ok, launch_steps=1 << 17), "launch_steps must be"),
                        (dict(ok, sample_every=-1), "sample_every")):
        with pytest.raises(X.XpicError, match=message):
            ctx.field_lines(seeds, **kw)
    with pytest.raises(X.XpicError, match="unknown model kind"):
        ctx.model_field_lines(X.field_model(17), seeds, **ok)
    with pytest.raises(X.XpicError, match="gaussian mirror: W must not be 0"):
        ctx.model_field_lines(X.field_model("gaussian_mirror", B_min=1.0, B_max=2.0, L=1.0), seeds, **ok)
    with pytest.raises(X.XpicError, match="component must be"):
        ctx.model_field_lines(model, seeds, component=3, **ok)
    # null pointers and a bad region, through the typed entry points themselves
    end, arr = np.zeros((2, n, 3)), [np.zeros((2, n)) for _ in range(5)]
    steps, code = np.zeros((2, n), dtype=np.int64), np.zeros((2, n), dtype=np.int32)
    P = X.LineParams(0.1, 5, 0.0, 0.0, 0, 3, 0, 0)
    ptr = lambda a: None if a is None else a.ctypes.data_as(X.c_dp)  # noqa: E731

    def call(seeds=seeds, P=P, region=None, every=0, end=end, arr=arr, steps=steps, code=code, samples=None, model=None):
        tail = (n, ptr(seeds), P, region, every, ptr(end), *(ptr(a) for a in arr),
                None if steps is None else steps.ctypes.data_as(X.CTYPES["int64_t*"]),
                None if code is None else code.ctypes.data_as(X.CTYPES["int32_t*"]), ptr(samples))
        if model is not None:
            return ctx._ck(ctx.L.xpic_model_field_lines(ctx.h, model, *tail))
        return ctx._ck(ctx.L.xpic_field_lines(ctx.h, X.B, *tail))
    call()
    call(model=model)
    for kw, message in ((dict(seeds=None), "seeds3 is null"), (dict(P=None), "params is null"), (dict(end=None), "a null output array"),
                        (dict(arr=[None] + arr[1:]), "a null output array"), (dict(arr=arr[:4] + [None]), "a null output array"),
                        (dict(steps=None), "a null output array"), (dict(code=None), "a null output array"),
                        (dict(every=2), "samples and sample_every go together"),
                        (dict(samples=np.zeros((2, n, 2, 3))), "samples and sample_every go together"),
                        (dict(region=X.TraceRegion(5, 1, (C_double7())), every=0), "unknown geometry kind"),
                        (dict(region=X.TraceRegion(0, 1, (C_double7()), -3)), "step0 is negative")):
        for m in (None, model):
            with pytest.raises(X.XpicError, match=message):
                call(model=m, **kw)
    with pytest.raises(X.XpicError, match="model is null"):
        ctx._ck(ctx.L.xpic_model_field_lines(ctx.h, None, n, ptr(seeds), P, None, 0, ptr(end), *(ptr(a) for a in arr),
                                             steps.ctypes.data_as(X.CTYPES["int64_t*"]), code.ctypes.data_as(X.CTYPES["int32_t*"]), None))
    # n == 0 succeeds and touches nothing, null arrays included
    ctx._ck(ctx.L.xpic_field_lines(ctx.h, X.B, 0, None, P, None, 0, None, None, None, None, None, None, None, None, None))
    empty = ctx.field_lines(np.zeros((0, 3)), **ok)
    assert empty.end.shape == (2, 0, 3) and empty.total_length.shape == (0,)
    # several z-slabs: the grid form is refused with the tracers' text
    for kw in (dict(self_ring=True), dict(rank=0, nranks=2)):
        two = X.Context("basic", (8, 8, 12), (0.5, 0.5, 0.5), 0.7, **kw)
        with pytest.raises(X.XpicError, match="a context of several z-slabs"):
            two.field_lines(seeds, **ok)
        two.close()


def C_double7():
    import ctypes

    return (ctypes.c_double * 7)(0.0, 0.0, 0.0, 8.0, 8.0, 8.0, 0.0)


def test_the_call_is_passive(X, ctx):
    """the call writes nothing but its outputs: E, B and the work vectors are what they were"""
    rng = np.random.default_rng(2)
    for f in (X.W0, X.W1, X.W2):
        ctx.set_field(f, rng.normal(size=ctx.fshape()))
    ids = (X.E, X.B, X.W0, X.W1, X.W2)
    before = [ctx.get_field(f) for f in ids]
    seeds = region_seeds()
    a = ctx.field_lines(seeds, h=0.1, max_steps=300, region=BOX, sample_every=7)
    b = ctx.field_lines(seeds, field=X.W1, stagger="E", h=0.1, max_steps=20)
    c = ctx.model_field_lines(X.field_model("gaussian_mirror", **AT.GAUSSIAN), seeds, h=0.1, max_steps=20)
    assert a.steps.max() > 0 and b.steps.max() == 20 and c.steps.max() == 20
    for f, was in zip(ids, before):
        assert bits(ctx.get_field(f)) == bits(was), f


def test_host_mirror_field_lines(X, tmp_path):
    """a coils field set into B0 and B by a preset and a "FieldLines" entry for each: the files equal, bit for bit, the rows of
    the same calls made from Python on the same field"""
    exe = os.path.join(os.path.dirname(os.path.abspath(X.__file__)), "host", "xpic_hip.out")
    n, d, dt, nt, period = (8, 8, 8), 0.5, 0.5, 2, 2
    coils = [{"z0": 1.0, "R": 1.5, "I": 2.0}, {"z0": 3.0, "R": 1.5, "I": 2.0}]
    rng = np.random.default_rng(23)
    seeds = 2.0 + (rng.random((5, 3)) - 0.5)
    region = {"name": "BoxGeometry", "min": [0.5, 0.5, 0.5], "max": [3.5, 3.5, 3.5]}
    points = [{"coordinate": {"name": "PreciseCoordinate", "value": list(map(float, q))}} for q in seeds]
    cfg = {
        "Simulation": "ecsim", "OutputDirectory": str(tmp_path),
        "Geometry": {"x": 4.0, "y": 4.0, "z": 4.0, "t": nt * dt, "dx": d, "dy": d, "dz": d, "dt": dt, "diagnose_period": period * dt,
                     "da_boundary_x": "DM_BOUNDARY_PERIODIC", "da_boundary_y": "DM_BOUNDARY_PERIODIC",
                     "da_boundary_z": "DM_BOUNDARY_PERIODIC"},
        "Particles": [{"sort_name": "electrons", "Np": 1, "n": 1.0, "q": -1.0, "m": 1.0, "T": 0.0}],
        "Presets": [{"command": "SetMagneticField", "field": "B0", "setter": {"name": "SetCoilsField", "coils": coils}}],
        "Diagnostics": [
            {"diagnostic": "FieldLines", "field": "B0", "points": points, "h": 0.05, "max_steps": 300, "region": region,
             "f_floor": 1e-3},
            {"diagnostic": "FieldLines", "name": "free", "field": "B0", "points": points, "h": 0.1, "max_steps": 20,
             "diagnose_period": dt}],
    }
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    out = subprocess.run([exe, str(tmp_path / "config.json")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    g = X.Context("ecsim", n, (d, d, d), dt)
    g.set_coils_field([(c["z0"], c["R"], c["I"]) for c in coils], field=X.B0)
    box = {"name": "box", "min": region["min"], "max": region["max"]}

    def rows(res):
        cols = [res.end[..., 0], res.end[..., 1], res.end[..., 2], res.length, res.volume, res.fmin, res.smin, res.fmax,
                res.steps.astype(np.float64), res.code.astype(np.float64)]
        return np.stack(cols, axis=-1).transpose(1, 0, 2)  # [n][2][10]
    want = {"field_lines": rows(g.field_lines(seeds, field=X.B0, h=0.05, max_steps=300, region=box, f_floor=1e-3)),
            "field_lines_free": rows(g.field_lines(seeds, field=X.B0, h=0.1, max_steps=20))}
    assert (want["field_lines"][..., 9] == R.LEFT).any() and (want["field_lines_free"][..., 8] == 20).all()
    assert sorted(os.listdir(tmp_path / "field_lines")) == ["0", "2"] and sorted(os.listdir(tmp_path / "field_lines_free")) == ["0", "1", "2"]
    for name, w in want.items():
        for t in os.listdir(tmp_path / name):  # B0 does not change during the run: every file holds the same rows
            got = np.fromfile(tmp_path / name / t, dtype=np.float64).reshape(-1, 2, 10)
            assert got.shape == w.shape == (5, 2, 10) and bits(got) == bits(w), (name, t)
    g.close()
