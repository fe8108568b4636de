"""The triplet trace on the device (xpic_amd/csrc/compare_trace.hip, include/xpic_hip.h: xpic_triplet_trace): a guiding
centre on an analytic model, a guiding centre on the grid filled from that model and a full orbit on the model, with the
reference's seven-way comparison reduced on the device; and the grid-less pair, the same kernel without the grid member.
On the grid of tests/test_gpu_paired_trace.py (9 x 8 x 7 nodes, unequal spacings) filled by xpic_set_model_field from a
quadratic and from a Gaussian mirror that sit in the middle of the box, grad |B| in the scratch vector W0; 300 triplets --
two workgroups of 256, the second partial -- over 70 steps, which cross the 64-step launch boundary.  The periodic grid
does not resolve either mirror, so the three grid statistics are large; no bit-for-bit claim needs it to."""
import ctypes as C

import numpy as np
import pytest

import analytic_trace_ref as A
import drift_kinetic_ref as DK
import triplet_trace_ref as T

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
N, D = DK.N, DK.D                      # a box of 4.5 x 3.2 x 2.1
QM, MP, DT = DK.QM, DK.MP, DK.DT
NTRI, STEPS = 300, 70
MODELS = {
    "quadratic_mirror": dict(B_min=1.0, B_max=4.0, W=3.0, D=2.0, E_phi=0.003, phi=0.05),  # axis (1.5, 1.5), midplane z = 1
    "gaussian_mirror": dict(B_min=1.0, B_max=4.0, L=1.0, W=1.0),                          # axis (1, 1), throats z = 0, 2
}
CENTRE = {"quadratic_mirror": (1.5, 1.5, 1.0), "gaussian_mirror": (1.0, 1.0, 1.0)}

# ---- stats_7 against the host evaluation: the largest |device - host| of each statistic in eps of the larger operand at
# the step that attains the maximum, measured on an MI355X over both mirrors; the bound is 8 x the largest
# of them and never above the paired test's cap
STATS_MEASURED_EPS = {"B": 0.115, "gradB": 1.444, "pos": 0.043, "z": 0.0, "p_parallel": 2.153, "mu": 2.542, "energy": 1.728}
STATS_CAP_EPS = 32.0
STATS_BOUND_EPS = min(8.0 * max(STATS_MEASURED_EPS.values()), STATS_CAP_EPS)


@pytest.fixture(scope="module")
def X():
    import xpic_amd

    return xpic_amd


def make_triplets(X, name, n, seed=61):
    """orbits within 0.3 of the mirror's centre, speeds 0.2 .. 0.5 at pitch cosines 0.3 .. 0.9 along +B, and their guiding
    centres from guiding_centre(..., orbit_centre=True) with the model's field at the particle: the start of both centres"""
    rng = np.random.default_rng(seed)
    r = np.array(CENTRE[name]) + 0.6 * (rng.random((n, 3)) - 0.5)
    Bp = A.model(name, **MODELS[name])(r)[1]
    b = Bp / DK._len(Bp)[:, None]
    e1 = np.cross(b, rng.normal(size=(n, 3)))
    e1 /= DK._len(e1)[:, None]
    speed, cos = 0.2 + 0.3 * rng.random(n), 0.3 + 0.6 * rng.random(n)
    v = speed[:, None] * (cos[:, None] * b + np.sqrt(1 - cos * cos)[:, None] * e1)
    fo = np.column_stack([r, v])
    return fo, X.guiding_centre(fo, Bp, MP, QM, orbit_centre=True)


class Case:
    """one model: its context with the grid filled from it, its triplets, and the results the tests share (each computed
    once and left unchanged)"""

    def __init__(self, X, name):
        self.X, self.name = X, name
        self.m = X.field_model(name, **MODELS[name])
        self.ctx = X.Context("basic", N, D, 0.7)
        self.ctx.set_model_field(self.m, X.E, X.B, X.W0)
        self.fo, self.gc = make_triplets(X, name, NTRI)
        self._cache = {}

    def run(self, steps=STEPS, scheme="EB2B", grad=True, grid=True, tri=None, **kw):
        fo, gm, gg = tri if tri is not None else (self.fo, self.gc, self.gc)
        return self.ctx.triplet_trace(fo, gm, gg if grid else None, steps, scheme, QM, MP, DT, self.m,
                                      gradB_field=self.X.W0 if grad else None, **kw)

    def once(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    def base(self, grid=True):
        """EB2B with grad B, 70 steps, the curve at every step"""
        return self.once(("base", grid), lambda: self.run(grid=grid, sample_every=1))

    def closed(self, scheme="EB2B", grad=True, steps=STEPS, every=0, fo_kw={}, dk_kw={}):
        """the three closed traces -> (model fo, model dk, grid dk (state, samples, total, max))"""
        c, X = self.ctx, self.X
        f = c.model_full_orbit_trace(self.fo, steps, scheme, QM, DT, self.m, sample_every=every, **fo_kw)
        a = c.model_drift_kinetic_trace(self.gc, steps, QM, MP, DT, self.m, sample_every=every, **dk_kw)
        g = c.drift_kinetic_trace(self.gc, steps, QM, MP, DT, X.W0 if grad else None, sample_every=every, **dk_kw)
        return f, a, g


@pytest.fixture(scope="module", params=list(MODELS))
def case(request, X):
    return Case(X, request.param)


def same_members(out, f, a, g=None):
    assert np.array_equal(out.p, f.state) and np.array_equal(out.state_model, a.state)
    assert np.array_equal(out.fo_iterations_sum, f.iterations_sum) and np.array_equal(out.fo_iterations_max, f.iterations_max)
    assert np.array_equal(out.dkm_iterations_total, a.iterations_sum)
    assert np.array_equal(out.dkm_iterations_max, a.iterations_max)
    if g is None:
        assert out.state_grid is None and out.dkg_iterations_total is None and out.dkg_iterations_max is None
        return
    assert np.array_equal(out.state_grid, g[0])
    assert np.array_equal(out.dkg_iterations_total, g[2]) and np.array_equal(out.dkg_iterations_max, g[3])


@pytest.mark.parametrize("grad", [True, False])
@pytest.mark.parametrize("scheme", ["EB2B", "CN"])
def test_members_are_the_closed_traces(case, scheme, grad):
    """guarantee (a)"""
    out = case.run(scheme=scheme, grad=grad)
    f, a, g = case.closed(scheme, grad)
    assert np.isfinite(out.p).all() and np.isfinite(out.state_model).all() and np.isfinite(out.state_grid).all()
    same_members(out, f, a, g)
    assert a.iterations_sum.min() >= STEPS and g[2].min() >= STEPS
    if scheme != "CN":
        assert not out.fo_iterations_sum.any() and not out.fo_iterations_max.any()
    assert np.isfinite(out.stats).all() and out.curve is None
    assert (out.stats > 0).all()  # every statistic is alive (without a grid vector of grad B, err_gradB is |gBa| itself)


@pytest.mark.parametrize("scheme", ["EB2B", "CN"])
def test_gridless_pair_is_its_closed_traces(case, scheme):
    """guarantees (a) and (d): the preloaded columns 0 .. 2 -- a NaN, an infinity and a negative number among them -- come
    back byte for byte"""
    given = np.zeros((NTRI, 7))
    given[:, :3] = np.random.default_rng(5).normal(size=(NTRI, 3))
    given[3, :3] = [np.nan, np.inf, -0.0]
    out = case.run(scheme=scheme, grid=False, stats=given)
    f, a, _ = case.closed(scheme)
    same_members(out, f, a)
    assert out.stats[:, :3].tobytes() == given[:, :3].tobytes()
    assert np.isfinite(out.stats[:, 3:]).all() and (out.stats[:, 3:] > 0).all()


@pytest.mark.parametrize("grid", [True, False], ids=["triplet", "pair"])
@pytest.mark.parametrize("scheme", ["EB2B", "CN"])
def test_calls_compose(case, scheme, grid):
    """guarantee (b): 70 steps = 45 steps, then 25 fed the first call's outputs"""
    whole = case.run(scheme=scheme, grid=grid)
    a = case.run(steps=45, scheme=scheme, grid=grid)
    b = case.run(steps=25, scheme=scheme, grid=grid, tri=(a.p, a.state_model, a.state_grid), stats=a.stats)
    assert np.array_equal(b.p, whole.p) and np.array_equal(b.state_model, whole.state_model)
    assert np.array_equal(b.stats, whole.stats)
    j0 = 0 if grid else 3
    assert (b.stats[:, j0:] >= a.stats[:, j0:]).all() and (b.stats > a.stats).any()
    assert np.array_equal(a.dkm_iterations_total + b.dkm_iterations_total, whole.dkm_iterations_total)
    if grid:
        assert np.array_equal(b.state_grid, whole.state_grid)
        assert np.array_equal(a.dkg_iterations_total + b.dkg_iterations_total, whole.dkg_iterations_total)
    else:
        assert not whole.stats[:, :3].any()


@pytest.mark.parametrize("grid", [True, False], ids=["triplet", "pair"])
def test_curve_is_the_maximum_over_the_triplets(case, grid):
    """guarantee (c): the error of every triplet at every step from 70 composed calls of one step with fresh zero stats
    (their stats are that step's errors), and the curve with strides 1, 3 and 65 bit for bit the maxima over the triplets
    at the sampled steps"""
    base = case.base(grid)
    tri = (case.fo, case.gc, case.gc)
    table = np.zeros((STEPS, NTRI, 7))
    for k in range(STEPS):
        o = case.run(steps=1, grid=grid, tri=tri)
        tri, table[k] = (o.p, o.state_model, o.state_grid), o.stats
    assert np.array_equal(tri[0], base.p) and np.array_equal(tri[1], base.state_model)
    assert np.array_equal(table.max(axis=0), base.stats)
    assert base.curve.shape == (STEPS, 7) and np.array_equal(base.curve, table.max(axis=1))
    third = case.run(grid=grid, sample_every=3)
    assert third.curve.shape == (STEPS // 3, 7) and np.array_equal(third.curve, table[2::3].max(axis=1))
    assert np.array_equal(third.stats, base.stats)
    # a stride longer than a launch: one row, from the second launch
    far = case.run(grid=grid, sample_every=case.X.TRIPLET_LAUNCH_STEPS + 1)
    assert far.curve.shape == (1, 7) and np.array_equal(far.curve[0], table[case.X.TRIPLET_LAUNCH_STEPS].max(axis=0))
    assert (base.curve[:, 3:] > 0).all() and (base.curve[:, :3] > 0).all() == grid and base.curve[:, :3].any() == grid


def test_stats_against_the_host(case):
    """The three closed traces sampled at every step, Ba and gBa from xpic_model_fields at the analytic centre's positions,
    Bg and gBg from xpic_drift_kinetic_interpolate on the grid centre's segments -- existing entry points, not the code
    under test -- and the seven errors from triplet_trace_ref.compare_step.  A device maximum agrees with the host's within
    STATS_BOUND_EPS eps of the larger operand at the step that attains it (for the three vector differences: the longer
    vector)."""
    base, ctx, X = case.base(), case.ctx, case.X
    f, a, g = case.closed(every=1)
    fs, ms, gs = f.samples, a.samples, g[1]
    before = np.concatenate([case.gc[None], gs[:-1]])
    _, Ba, gBa = ctx.model_fields(case.m, ms[:, :, :3].reshape(-1, 3))
    _, Bg, gBg = ctx.drift_kinetic_interpolate(gs[:, :, :3].reshape(-1, 3), before[:, :, :3].reshape(-1, 3), X.W0)
    gm6, gg6, fo6 = ms.reshape(-1, 6), gs.reshape(-1, 6), fs.reshape(-1, 6)
    err = T.compare_step(gm6, gg6, fo6, Ba, gBa, Bg, gBg, MP).reshape(STEPS, NTRI, 7)
    import paired_trace_ref as P

    pa, pb = P.operands(gg6, fo6, Ba, MP)
    L = DK._len
    scale = np.column_stack([np.maximum(L(Ba), L(Bg)), np.maximum(L(gBa), L(gBg)), np.maximum(L(gm6[:, :3]), L(gg6[:, :3])),
                             np.maximum(np.abs(pa), np.abs(pb))]).reshape(STEPS, NTRI, 7)
    at = err.argmax(axis=0)                                  # [triplet][stat]: the step that attains the maximum
    host = np.take_along_axis(err, at[None], axis=0)[0]
    sc = np.take_along_axis(scale, at[None], axis=0)[0]
    diff = np.abs(base.stats - host)
    for j, name in enumerate(T.STATS):
        print(case.name, name, "largest stat", host[:, j].max(), "max |device - host| / (eps scale) =",
              (diff[:, j] / (EPS * sc[:, j])).max())
    cdiff = np.abs(base.curve - err.max(axis=1)) / (EPS * scale.max(axis=1))
    print(case.name, "curve: max |device - host| / (eps scale) per statistic =", cdiff.max(axis=0))
    assert (diff <= STATS_BOUND_EPS * EPS * sc).all()
    # and the curve's rows are the largest of the host's errors at their steps, to the same bound
    assert (cdiff <= STATS_BOUND_EPS).all()


def _same(name, got, ref, rel=1e-13):
    """the bound of test_gpu_drift_kinetic.py and test_gpu_full_orbit.py: rel of the column group's largest reference value"""
    assert np.isfinite(got).all() and np.isfinite(ref).all(), name
    err, scale = np.abs(got - ref).max(), np.abs(ref).max()
    print(name, "max |gpu - restatement| =", err, "scale", scale)
    assert err <= rel * scale, name


@pytest.mark.parametrize("grid", [True, False], ids=["triplet", "pair"])
@pytest.mark.parametrize("scheme", ["EB2B", "CN"])
def test_parity_with_the_restatement(case, scheme, grid):
    """20 triplets, 10 steps against triplet_trace_ref.triplet_trace on the grid the device filled, with the iterations
    pinned (eps = delta = 0 and atol = rtol = 0: no residual is < 0, so every loop makes exactly maxit updates: 4 and 3),
    as the parity tests of the pushers pin them; the states to their bound, 1e-13 of the column group's scale.  A
    statistic is the difference of two numbers formed from those states and from the fields at them, each good to that
    bound: 2e-13 of the largest state or field entry."""
    X, ctx = case.X, case.ctx
    fo, gc = case.fo[:20], case.gc[:20]
    kw = dict(eps=0.0, delta=0.0, dk_maxit=4, atol=0.0, rtol=0.0, maxit=3)
    field = A.model(case.name, **MODELS[case.name])
    fields = (ctx.get_field(X.E), ctx.get_field(X.B), ctx.get_field(X.W0))
    ref = T.triplet_trace(field, fields if grid else None, D, fo, gc, gc if grid else None, 10, scheme, QM, MP, DT,
                          sample_every=2, **kw)
    out = case.run(steps=10, scheme=scheme, grid=grid, tri=(fo, gc, gc), sample_every=2, **kw)
    assert np.array_equal(out.dkm_iterations_max, ref.dm_max) and np.array_equal(out.dkm_iterations_total, ref.dm_total)
    assert (out.dkm_iterations_max == 4).all() and (out.dkm_iterations_total == 40).all()
    assert np.array_equal(out.fo_iterations_sum, ref.fo_sum) and np.array_equal(out.fo_iterations_max, ref.fo_max)
    if scheme == "CN":
        assert (out.fo_iterations_max == 3).all() and (out.fo_iterations_sum == 30).all()
    members = [("fo", out.p, ref.fo), ("model gc", out.state_model, ref.gm)]
    if grid:
        assert np.array_equal(out.dkg_iterations_max, ref.dg_max) and np.array_equal(out.dkg_iterations_total, ref.dg_total)
        assert (out.dkg_iterations_max == 4).all()
        members.append(("grid gc", out.state_grid, ref.gg))
    for name, got, want in members:
        _same(name + " r", got[:, :3], want[:, :3])
        _same(name + " p", got[:, 3:5], want[:, 3:5])
        if name == "fo":
            _same(name + " pz", got[:, 5], want[:, 5])
        else:
            assert np.array_equal(got[:, 5], gc[:, 5])
    bound = 2e-13 * max(np.abs(ref.fo).max(), np.abs(ref.gm).max(), np.abs(fields[1]).max(), np.abs(fields[2]).max())
    print("stats: max |gpu - restatement| =", np.abs(out.stats - ref.stats).max(), "curve", np.abs(out.curve - ref.curve).max(),
          "bound", bound)
    assert np.abs(out.stats - ref.stats).max() <= bound
    assert out.curve.shape == (5, 7) and np.abs(out.curve - ref.curve).max() <= bound


def test_edges(case):
    ctx, X, base = case.ctx, case.X, case.base()
    z6 = np.zeros((0, 6))
    # n = 0: success, nothing touched
    for gg in (z6, None):
        o = ctx.triplet_trace(z6, z6, gg, 5, "EB2B", QM, MP, DT, case.m, sample_every=2)
        assert o.p.shape == (0, 6) and o.state_model.shape == (0, 6) and o.stats.shape == (0, 7) and not o.curve.any()
    # n = 1 is the first triplet of the batch
    one = case.run(tri=(case.fo[:1], case.gc[:1], case.gc[:1]))
    assert np.array_equal(one.p[0], base.p[0]) and np.array_equal(one.state_model[0], base.state_model[0])
    assert np.array_equal(one.state_grid[0], base.state_grid[0]) and np.array_equal(one.stats[0], base.stats[0])
    assert one.dkg_iterations_total[0] == base.dkg_iterations_total[0]
    # steps = 0 returns the inputs
    given = np.arange(7.0 * NTRI).reshape(NTRI, 7)
    z = case.run(steps=0, stats=given, sample_every=1)
    assert np.array_equal(z.p, case.fo) and np.array_equal(z.state_model, case.gc) and np.array_equal(z.state_grid, case.gc)
    assert np.array_equal(z.stats, given) and z.curve.shape == (0, 7)
    assert not z.dkm_iterations_total.any() and not z.dkg_iterations_max.any()
    # statistics preloaded with large values come back unchanged; an infinite one is kept
    big = np.full((NTRI, 7), 1e30)
    big[7] = np.inf
    o = case.run(stats=big)
    assert np.array_equal(o.stats, big) and np.array_equal(o.p, base.p) and np.array_equal(o.state_grid, base.state_grid)
    # smaller preloads are only raised
    low = np.full((NTRI, 7), 1e-9)
    o = case.run(stats=low)
    assert np.array_equal(o.stats, np.maximum(base.stats, 1e-9))


def test_a_triplet_that_is_not_a_number(case):
    """triplet 5 with a NaN position in all three members: every error of it is a NaN at every step, so its statistics
    stay at their input values and the curve is that of the other triplets alone; its Picard loops never meet a tolerance,
    so their counters are maxit at every step, and the run goes on"""
    base = case.base()
    fo, gm, gg = case.fo.copy(), case.gc.copy(), case.gc.copy()
    fo[5, :3] = np.nan
    gm[5, :3] = np.nan
    gg[5, :3] = np.nan
    given = np.zeros((NTRI, 7))
    given[5] = [0.5, 0.25, 0.125, 2.0, 3.0, 4.0, 5.0]
    o = case.run(tri=(fo, gm, gg), stats=given, sample_every=1)
    assert np.array_equal(o.stats[5], given[5])
    assert o.dkm_iterations_max[5] == 30 and o.dkm_iterations_total[5] == 30 * STEPS
    assert o.dkg_iterations_max[5] == 30 and o.dkg_iterations_total[5] == 30 * STEPS
    keep = np.arange(NTRI) != 5
    assert np.array_equal(o.stats[keep], base.stats[keep]) and np.array_equal(o.p[keep], base.p[keep])
    assert np.array_equal(o.state_grid[keep], base.state_grid[keep])
    rest = case.run(tri=(fo[keep], gm[keep], gg[keep]), sample_every=1)
    assert np.array_equal(o.curve, rest.curve) and np.isfinite(o.curve).all()


def test_loops_that_run_out_of_maxit(case):
    """atol = rtol = 0 and eps = delta = 0: no residual is < 0, every loop runs out; the counters say so and the run
    continues, with the states of the closed traces"""
    kw_fo, kw_dk = dict(atol=0.0, rtol=0.0, maxit=3), dict(eps=0.0, delta=0.0, maxit=4)
    o = case.run(scheme="CN", atol=0.0, rtol=0.0, maxit=3, eps=0.0, delta=0.0, dk_maxit=4)
    assert (o.fo_iterations_max == 3).all() and (o.fo_iterations_sum == 3 * STEPS).all()
    assert (o.dkm_iterations_max == 4).all() and (o.dkm_iterations_total == 4 * STEPS).all()
    assert (o.dkg_iterations_max == 4).all() and (o.dkg_iterations_total == 4 * STEPS).all()
    f, a, g = case.closed("CN", fo_kw=kw_fo, dk_kw=kw_dk)
    same_members(o, f, a, g)
    assert np.isfinite(o.stats).all()


def test_every_scheme_runs(case):
    tri = (case.fo[:70], case.gc[:70], case.gc[:70])
    for sid in case.X.FO_SCHEMES:
        o = case.run(steps=2, scheme=sid, tri=tri)
        f = case.ctx.model_full_orbit_trace(tri[0], 2, sid, QM, DT, case.m)
        assert np.array_equal(o.p, f.state) and np.isfinite(o.stats).all(), sid
        assert np.array_equal(case.run(steps=2, scheme=sid, tri=tri, grid=False).p, f.state), sid


def test_argument_checks(case):
    X, ctx = case.X, case.ctx
    fo, gm, gg = case.fo[:4].copy(), case.gc[:4].copy(), case.gc[:4].copy()
    L_, dp = ctx.L, C.POINTER(C.c_double)
    n, one, zero = C.c_int64(4), C.c_int64(1), C.c_int64(0)
    stats, curve = np.zeros((4, 7)), np.zeros((1, 7))
    fsum, mtot, gtot = (C.c_int64 * 4)(), (C.c_int64 * 4)(), (C.c_int64 * 4)()
    fmax, mmax, gmax = (C.c_int * 4)(), (C.c_int * 4)(), (C.c_int * 4)()
    F = X.FoParams(QM, DT, 1e-7, 1e-7, X.FO_SCHEMES["EB2B"], 30)
    Fcn = X.FoParams(QM, DT, 1e-7, 1e-7, X.FO_SCHEMES["CN"], 30)
    K = X.DkParams(QM, MP, DT, 1e-12, 1e-12, 30)
    pf, pm, pg, ps, pc = (a.ctypes.data_as(dp) for a in (fo, gm, gg, stats, curve))

    def call(h=None, F=F, K=K, M=case.m, grid=1, grad=-1, steps=one, every=one, p=pf, sm=pm, sg=pg, st=ps, cv=pc, a=fsum,
             b=fmax, c=mtot, d=mmax, e=gtot, f=gmax):
        return L_.xpic_triplet_trace(ctx.h if h is None else h, n, C.byref(F) if F else None, C.byref(K) if K else None,
                                     C.byref(M) if M else None, grid, grad, steps, every, p, sm, sg, st, cv, a, b, c, d, e, f)

    assert call() == 0 and call(grad=X.W0) == 0
    assert call(a=None, b=None) == 0  # a Chin id takes no fo counters
    # the grid-less pair reads nothing of the grid member: null array and counters, any gradB_field
    assert call(grid=0, sg=None, e=None, f=None, grad=99) == 0
    bad = [
        (dict(F=X.FoParams(QM, 2 * DT, 1e-7, 1e-7, 16, 30)), "dt"),
        (dict(F=X.FoParams(-QM, DT, 1e-7, 1e-7, 16, 30)), "qm"),
        (dict(F=None), "fo"), (dict(K=None), "dk"),
        (dict(M=None), "model is null"), (dict(M=X.field_model(7)), "kind"),
        (dict(M=X.field_model("quadratic_mirror", B_min=1, B_max=4, W=0.0, D=40.0)), "W and D"),
        (dict(M=X.field_model("quadratic_mirror", B_min=1, B_max=4, W=20.0, D=0.0)), "W and D"),
        (dict(M=X.field_model("gaussian_mirror", B_min=1, B_max=4, L=5.0, W=0.0), grid=0), "W must"),
        (dict(p=None), "p_6"), (dict(sm=None), "state_model_6"), (dict(sg=None), "state_grid_6"), (dict(st=None), "stats_7"),
        (dict(c=None), "dkm_iterations_total"), (dict(d=None), "dkm_iterations_max"),
        (dict(e=None), "dkg_iterations_total"), (dict(f=None), "dkg_iterations_max"),
        (dict(F=Fcn, a=None), "fo_iterations_sum"), (dict(F=Fcn, b=None), "fo_iterations_max"),
        (dict(every=zero), "sample_every"),
        (dict(steps=C.c_int64(-1)), "steps"),
        (dict(grad=99), "gradB_field"),
        (dict(F=X.FoParams(QM, DT, 1e-7, 1e-7, 18, 30)), "scheme"),
        (dict(F=X.FoParams(QM, DT, 1e-7, 1e-7, 17, 65)), "maxit"),
        (dict(K=X.DkParams(QM, MP, DT, 1e-12, 1e-12, 0)), "maxit"),
        (dict(K=X.DkParams(QM, MP, DT, 1e-12, 1e-12, X.TRIPLET_DK_MAXIT + 1)), "maxit"),
        (dict(K=X.DkParams(QM, 0.0, DT, 1e-12, 1e-12, 30)), "mp"),
    ]
    for kw, word in bad:
        assert call(**kw) != 0, word
        assert word in L_.xpic_last_error().decode(), word
    assert call(every=zero, cv=None) == 0  # no curve: sample_every is not looked at
    assert call(h=C.c_void_p()) != 0
    # with the grid member, contexts with ghost planes or of several slabs are refused with a message; the grid-less pair
    # reads no grid vector and runs on them, with the results of the single-slab context
    ref = case.run(steps=2, tri=(fo, gm, gg), grid=False)
    ring = X.Context("basic", N, D, 0.7, self_ring=True)
    two = X.Context("basic", (8, 8, 12), D, 0.7, rank=0, nranks=2)
    for other, word in ((ring, "self_ring"), (two, "z-slab")):
        with pytest.raises(X.XpicError, match=word):
            other.triplet_trace(fo, gm, gg, 2, "EB2B", QM, MP, DT, case.m)
        o = other.triplet_trace(fo, gm, None, 2, "EB2B", QM, MP, DT, case.m)
        assert np.array_equal(o.p, ref.p) and np.array_equal(o.state_model, ref.state_model)
        assert np.array_equal(o.stats, ref.stats)
    with pytest.raises(X.XpicError, match="different numbers"):
        ctx.triplet_trace(fo, gm[:3], gg, 2, "EB2B", QM, MP, DT, case.m)
