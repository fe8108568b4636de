"""The paired trace on the device (xpic_amd/csrc/compare_trace.hip, include/xpic_hip.h: xpic_paired_trace): a guiding
centre beside the full orbit of the same particle, with the reference's comparison of the two reduced on the device.  On
the grid and the seeded fields of drift_kinetic_ref.case_fields (9 x 8 x 7 nodes, unequal spacings) with 300 pairs -- two
workgroups of 256, the second partial -- over 70 steps, which cross the 64-step launch boundary."""
import ctypes as C

import numpy as np
import pytest

import drift_kinetic_ref as DK
import paired_trace_ref as P

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
N, D = DK.N, DK.D
QM, MP, DT = DK.QM, DK.MP, DK.DT
NPAIR, STEPS = 300, 70


@pytest.fixture(scope="module")
def X():
    import xpic_amd

    return xpic_amd


@pytest.fixture(scope="module")
def fields():
    return DK.case_fields()


@pytest.fixture(scope="module")
def ctx(X, fields):
    E, B, gB = fields
    g = X.Context("basic", N, D, 0.7)
    g.set_field(X.E, E)
    g.set_field(X.B, B)
    g.set_field(X.W0, gB)
    return g


def make_pairs(X, B, n, seed=41):
    """orbits all over the box and a tenth of it beyond every face (the footprints cross the periodic seam), speeds
    0.5 .. 1 at pitch cosines 0.4 .. 0.9 along +B (PointByField keeps |p_parallel| only), and their guiding centres from
    guiding_centre(..., orbit_centre=True) with the field at the particle"""
    rng = np.random.default_rng(seed)
    L = np.array(N) * np.array(D)
    r = (-0.1 + 1.2 * rng.random((n, 3))) * L
    (Bp,) = DK.interpolate_B([B], D, r)
    b = Bp / DK._len(Bp)[:, None]
    e1 = np.cross(b, rng.normal(size=(n, 3)))
    e1 /= DK._len(e1)[:, None]
    speed, cos = 0.5 + 0.5 * rng.random(n), 0.4 + 0.5 * rng.random(n)
    v = speed[:, None] * (cos[:, None] * b + np.sqrt(1 - cos * cos)[:, None] * e1)
    fo = np.column_stack([r, v])
    return fo, X.guiding_centre(fo, Bp, MP, QM, orbit_centre=True)


@pytest.fixture(scope="module")
def pairs(X, fields):
    fo, gc = make_pairs(X, fields[1], NPAIR)
    L = np.array(N) * np.array(D)
    assert ((fo[:, :3] < 0).any(axis=0) & (fo[:, :3] > L).any(axis=0)).all()  # beyond both faces on every axis
    return fo, gc


def run(ctx, X, pairs, steps=STEPS, scheme="EB2B", grad=True, **kw):
    fo, gc = pairs
    return ctx.paired_trace(fo, gc, steps, scheme, QM, MP, DT, gradB_field=X.W0 if grad else None, **kw)


@pytest.fixture(scope="module")
def base(ctx, X, pairs):
    """EB2B with grad B, 70 steps, the curve at every step: shared, and left unchanged, by the tests below"""
    return run(ctx, X, pairs, sample_every=1)


@pytest.mark.parametrize("grad", [True, False])
@pytest.mark.parametrize("scheme", ["EB2B", "CN"])
def test_states_and_counters_are_the_closed_traces(ctx, X, pairs, scheme, grad):
    """guarantee (a)"""
    fo, gc = pairs
    out = run(ctx, X, pairs, scheme=scheme, grad=grad)
    f, _, fsum, fmax = ctx.full_orbit_trace(fo, STEPS, scheme, QM, DT)
    s, _, dtot, dmax = ctx.drift_kinetic_trace(gc, STEPS, QM, MP, DT, X.W0 if grad else None)
    assert np.isfinite(out.p).all() and np.isfinite(out.state).all() and np.isfinite(out.stats).all()
    assert np.array_equal(out.p, f) and np.array_equal(out.state, s)
    assert np.array_equal(out.fo_iterations_sum, fsum) and np.array_equal(out.fo_iterations_max, fmax)
    assert np.array_equal(out.dk_iterations_total, dtot) and np.array_equal(out.dk_iterations_max, dmax)
    assert dtot.min() >= STEPS
    assert (out.stats > 0).all() and out.curve is None


@pytest.mark.parametrize("scheme", ["EB2B", "CN"])
def test_calls_compose(ctx, X, pairs, scheme):
    """guarantee (b): 70 steps = 45 steps, then 25 fed the first call's outputs"""
    whole = run(ctx, X, pairs, scheme=scheme)
    a = run(ctx, X, pairs, steps=45, scheme=scheme)
    b = run(ctx, X, (a.p, a.state), steps=25, scheme=scheme, stats=a.stats)
    assert np.array_equal(b.p, whole.p) and np.array_equal(b.state, whole.state)
    assert np.array_equal(b.stats, whole.stats)
    assert (b.stats >= a.stats).all() and (b.stats > a.stats).any()
    assert np.array_equal(a.dk_iterations_total + b.dk_iterations_total, whole.dk_iterations_total)


def test_stats_against_the_host(ctx, X, pairs, base):
    """The two closed traces sampled at every step, Bg of every step from xpic_drift_kinetic_interpolate on consecutive
    samples, the four errors from paired_trace_ref.compare_step.  A device maximum |a - b| agrees with the host's within
    32 eps max(|a|, |b|) of the two operands at the step that attains it: a dozen roundings on either side (a dot
    product, a division, a hypot and a square), not a measured number."""
    fo, gc = pairs
    _, fs, _, _ = ctx.full_orbit_trace(fo, STEPS, "EB2B", QM, DT, sample_every=1)
    _, gs, _, _ = ctx.drift_kinetic_trace(gc, STEPS, QM, MP, DT, X.W0, sample_every=1)
    before = np.concatenate([gc[None], gs[:-1]])
    _, Bg, _ = ctx.drift_kinetic_interpolate(gs[:, :, :3].reshape(-1, 3), before[:, :, :3].reshape(-1, 3), X.W0)
    a, b = P.operands(gs.reshape(-1, 6), fs.reshape(-1, 6), Bg, MP)
    a, b = a.reshape(STEPS, NPAIR, 4), b.reshape(STEPS, NPAIR, 4)
    err = np.abs(a - b)
    at = err.argmax(axis=0)                                  # [pair][stat]: the step that attains the maximum
    host = np.take_along_axis(err, at[None], axis=0)[0]
    scale = np.maximum(np.abs(np.take_along_axis(a, at[None], axis=0)[0]), np.abs(np.take_along_axis(b, at[None], axis=0)[0]))
    diff = np.abs(base.stats - host)
    for j, name in enumerate(P.STATS):
        print(name, "largest stat", host[:, j].max(), "max |device - host| / (eps scale) =", (diff[:, j] / (EPS * scale[:, j])).max())
    assert (diff <= 32 * EPS * scale).all()
    # and the curve's rows are the largest of the host's errors at their steps, to the same bound
    cscale = np.maximum(np.abs(a), np.abs(b)).max(axis=1)
    assert (np.abs(base.curve - err.max(axis=1)) <= 32 * EPS * cscale).all()


def test_curve_is_the_maximum_over_the_pairs(ctx, X, pairs, base):
    """guarantee (c): the error of every pair at every step from 70 composed calls of one step with fresh zero stats
    (their stats are that step's errors), and the curve with sample_every 1 and 3 bit for bit the maxima over the pairs
    at the sampled steps"""
    p, s = pairs
    table = np.zeros((STEPS, NPAIR, 4))
    for k in range(STEPS):
        o = run(ctx, X, (p, s), steps=1)
        p, s, table[k] = o.p, o.state, o.stats
    assert np.array_equal(p, base.p) and np.array_equal(s, base.state)
    assert np.array_equal(table.max(axis=0), base.stats)
    assert base.curve.shape == (STEPS, 4) and np.array_equal(base.curve, table.max(axis=1))
    third = run(ctx, X, pairs, sample_every=3)
    assert third.curve.shape == (STEPS // 3, 4) and np.array_equal(third.curve, table[2::3].max(axis=1))
    assert np.array_equal(third.stats, base.stats)
    # a stride longer than a launch: one row, from the second launch
    far = run(ctx, X, pairs, sample_every=X.PAIR_LAUNCH_STEPS + 1)
    assert far.curve.shape == (1, 4) and np.array_equal(far.curve[0], table[X.PAIR_LAUNCH_STEPS].max(axis=0))


def _same(name, got, ref, rel=1e-13):
    """the bound of test_gpu_drift_kinetic.py and test_gpu_full_orbit.py: rel of the column group's largest reference value"""
    assert np.isfinite(got).all() and np.isfinite(ref).all(), name
    err, scale = np.abs(got - ref).max(), np.abs(ref).max()
    print(name, "max |gpu - restatement| =", err, "scale", scale)
    assert err <= rel * scale, name


@pytest.mark.parametrize("scheme", ["EB2B", "CN"])
def test_parity_with_the_restatement(ctx, X, fields, pairs, scheme):
    """20 pairs, 10 steps against paired_trace_ref.paired_trace, with both iterations pinned (eps = delta = 0 and
    atol = rtol = 0: no residual is < 0, so both sides make exactly maxit updates), as the parity tests of the two pushers
    pin them; the states to their bound, 1e-13 of the column group's scale.  The statistics are differences of two
    numbers formed from those states, each good to that bound: 2e-13 of the largest state entry."""
    E, B, gB = fields
    fo, gc = pairs[0][:20], pairs[1][:20]
    kw = dict(eps=0.0, delta=0.0, dk_maxit=5, atol=0.0, rtol=0.0, maxit=3)
    rf, rg, rstats, rcurve, _ = P.paired_trace(E, B, gB, D, fo, gc, 10, scheme, QM, MP, DT, sample_every=2, **kw)
    out = ctx.paired_trace(fo, gc, 10, scheme, QM, MP, DT, gradB_field=X.W0, sample_every=2, **kw)
    assert (out.dk_iterations_max == 5).all() and (out.dk_iterations_total == 50).all()
    if scheme == "CN":
        assert (out.fo_iterations_max == 3).all() and (out.fo_iterations_sum == 30).all()
    _same("fo r", out.p[:, :3], rf[:, :3])
    _same("fo p", out.p[:, 3:], rf[:, 3:])
    _same("gc r", out.state[:, :3], rg[:, :3])
    _same("gc p_parallel", out.state[:, 3], rg[:, 3])
    _same("gc p_perp", out.state[:, 4], rg[:, 4])
    assert np.array_equal(out.state[:, 5], gc[:, 5])
    bound = 2e-13 * max(np.abs(rf).max(), np.abs(rg).max())
    print("stats: max |gpu - restatement| =", np.abs(out.stats - rstats).max(), "curve", np.abs(out.curve - rcurve).max(), "bound", bound)
    assert np.abs(out.stats - rstats).max() <= bound
    assert out.curve.shape == (5, 4) and np.abs(out.curve - rcurve).max() <= bound


def test_edges(ctx, X, pairs, base):
    fo, gc = pairs
    # n = 0: success, nothing touched
    o = ctx.paired_trace(np.zeros((0, 6)), np.zeros((0, 6)), 5, "EB2B", QM, MP, DT, sample_every=2)
    assert o.p.shape == (0, 6) and o.state.shape == (0, 6) and o.stats.shape == (0, 4) and not o.curve.any()
    # n = 1 is the first pair of the batch
    one = run(ctx, X, (fo[:1], gc[:1]))
    assert np.array_equal(one.p[0], base.p[0]) and np.array_equal(one.state[0], base.state[0])
    assert np.array_equal(one.stats[0], base.stats[0])
    assert one.dk_iterations_total[0] == base.dk_iterations_total[0]
    # steps = 0 returns the inputs
    given = np.arange(4.0 * NPAIR).reshape(NPAIR, 4)
    z = run(ctx, X, pairs, steps=0, stats=given, sample_every=1)
    assert np.array_equal(z.p, fo) and np.array_equal(z.state, gc) and np.array_equal(z.stats, given)
    assert z.curve.shape == (0, 4) and not z.dk_iterations_total.any() and not z.dk_iterations_max.any()
    # statistics preloaded with large values come back unchanged; an infinite one is kept
    big = np.full((NPAIR, 4), 1e30)
    big[7] = np.inf
    o = run(ctx, X, pairs, stats=big)
    assert np.array_equal(o.stats, big) and np.array_equal(o.p, base.p)


def test_a_pair_that_is_not_a_number(ctx, X, pairs, base):
    """pair 5 with a NaN position on both sides: every error of it is a NaN at every step, so its statistics stay at
    their input values, and the curve is the curve of the other pairs alone; its Picard loop never meets a tolerance, so
    its counters are maxit at every step, and the run goes on"""
    fo, gc = pairs[0].copy(), pairs[1].copy()
    fo[5, :3] = np.nan
    gc[5, :3] = np.nan
    given = np.zeros((NPAIR, 4))
    given[5] = [0.5, 0.25, 0.125, 2.0]
    o = run(ctx, X, (fo, gc), stats=given, sample_every=1)
    assert np.array_equal(o.stats[5], given[5])
    assert o.dk_iterations_max[5] == 30 and o.dk_iterations_total[5] == 30 * STEPS
    keep = np.arange(NPAIR) != 5
    assert np.array_equal(o.stats[keep], base.stats[keep]) and np.array_equal(o.p[keep], base.p[keep])
    rest = run(ctx, X, (fo[keep], gc[keep]), sample_every=1)
    assert np.array_equal(o.curve, rest.curve) and np.isfinite(o.curve).all()


def test_loops_that_run_out_of_maxit(ctx, X, pairs):
    """atol = rtol = 0 and eps = delta = 0: no residual is < 0, every loop runs out; the counters say so and the run
    continues, with the states of the closed traces"""
    fo, gc = pairs
    o = run(ctx, X, pairs, scheme="CN", atol=0.0, rtol=0.0, maxit=3, eps=0.0, delta=0.0, dk_maxit=4)
    assert (o.fo_iterations_max == 3).all() and (o.fo_iterations_sum == 3 * STEPS).all()
    assert (o.dk_iterations_max == 4).all() and (o.dk_iterations_total == 4 * STEPS).all()
    f, _, _, _ = ctx.full_orbit_trace(fo, STEPS, "CN", QM, DT, atol=0.0, rtol=0.0, maxit=3)
    s, _, _, _ = ctx.drift_kinetic_trace(gc, STEPS, QM, MP, DT, X.W0, eps=0.0, delta=0.0, maxit=4)
    assert np.array_equal(o.p, f) and np.array_equal(o.state, s) and np.isfinite(o.stats).all()


def test_argument_checks(ctx, X, pairs):
    fo, gc = pairs[0][:4].copy(), pairs[1][:4].copy()
    L_, dp = ctx.L, C.POINTER(C.c_double)
    n, one, zero = C.c_int64(4), C.c_int64(1), C.c_int64(0)
    stats, curve = np.zeros((4, 4)), np.zeros((1, 4))
    fsum, dtot = (C.c_int64 * 4)(), (C.c_int64 * 4)()
    fmax, dmax = (C.c_int * 4)(), (C.c_int * 4)()
    F = X.FoParams(QM, DT, 1e-7, 1e-7, X.FO_SCHEMES["EB2B"], 30)
    Fcn = X.FoParams(QM, DT, 1e-7, 1e-7, X.FO_SCHEMES["CN"], 30)
    K = X.DkParams(QM, MP, DT, 1e-12, 1e-12, 30)
    pf, pg, ps, pc = (a.ctypes.data_as(dp) for a in (fo, gc, stats, curve))

    def call(h=None, F=F, K=K, grad=-1, steps=one, every=one, p=pf, s=pg, st=ps, cv=pc, a=fsum, b=fmax, c=dtot, d=dmax):
        return L_.xpic_paired_trace(ctx.h if h is None else h, n, C.byref(F) if F else None, C.byref(K) if K else None, grad,
                                    steps, every, p, s, st, cv, a, b, c, d)

    assert call() == 0
    assert call(a=None, b=None) == 0  # a Chin id takes no fo counters
    bad = [
        (dict(F=X.FoParams(QM, 2 * DT, 1e-7, 1e-7, 16, 30)), "dt"),
        (dict(F=X.FoParams(-QM, DT, 1e-7, 1e-7, 16, 30)), "qm"),
        (dict(F=None), "fo"), (dict(K=None), "dk"),
        (dict(p=None), "p_6"), (dict(s=None), "state_6"), (dict(st=None), "stats_4"),
        (dict(c=None), "dk_iterations_total"), (dict(d=None), "dk_iterations_max"),
        (dict(F=Fcn, a=None), "fo_iterations_sum"), (dict(F=Fcn, b=None), "fo_iterations_max"),
        (dict(every=zero), "sample_every"),
        (dict(steps=C.c_int64(-1)), "steps"),
        (dict(grad=99), "gradB_field"),
        (dict(F=X.FoParams(QM, DT, 1e-7, 1e-7, 18, 30)), "scheme"),
        (dict(F=X.FoParams(QM, DT, 1e-7, 1e-7, 17, 65)), "maxit"),
        (dict(K=X.DkParams(QM, MP, DT, 1e-12, 1e-12, 0)), "maxit"),
        (dict(K=X.DkParams(QM, MP, DT, 1e-12, 1e-12, X.PAIR_DK_MAXIT + 1)), "maxit"),
        (dict(K=X.DkParams(QM, 0.0, DT, 1e-12, 1e-12, 30)), "mp"),
    ]
    for kw, word in bad:
        assert call(**kw) != 0, word
        assert word in L_.xpic_last_error().decode(), word
    assert call(every=zero, cv=None) == 0  # no curve: sample_every is not looked at
    assert L_.xpic_paired_trace(None, n, C.byref(F), C.byref(K), -1, one, one, pf, pg, ps, pc, fsum, fmax, dtot, dmax) != 0
    # contexts with ghost planes, or of several slabs, are refused with a message
    ring = X.Context("basic", N, D, 0.7, self_ring=True)
    with pytest.raises(X.XpicError, match="self_ring"):
        ring.paired_trace(pairs[0][:4], pairs[1][:4], 2, "EB2B", QM, MP, DT)
    two = X.Context("basic", (8, 8, 12), (0.5, 0.5, 0.5), 0.7, rank=0, nranks=2)
    with pytest.raises(X.XpicError, match="z-slab"):
        two.paired_trace(pairs[0][:4], pairs[1][:4], 2, "CN", QM, MP, DT)
    with pytest.raises(X.XpicError, match="different numbers"):
        ctx.paired_trace(pairs[0][:4], pairs[1][:3], 2, "EB2B", QM, MP, DT)
