"""The open-trap traces on the device (xpic_full_orbit_trace_open, xpic_drift_kinetic_trace_open) for a Chin id (EB2B),
Crank-Nicolson and the drift-kinetic pusher.  Every comparison is between device results, bit for bit: the open trace
against the device's own one-step calls with the region rule applied on the host (tests/open_trace_ref.py: trace_open),
against the closed traces, against itself in two parts, and among the three compaction policies.  The inputs are
open_trace_ref's (pinned without a GPU by tests/test_open_trace_ref.py): an 8 x 8 x 8 grid, a uniform B plus the mirror
field, 3 x 256 + 7 particles, 150 steps sampled every 7, a box that ends one cell inside the domain in z."""
import ctypes as C

import numpy as np
import pytest

import commands_ref as CR
import open_trace_ref as O

pytestmark = pytest.mark.gpu
KINDS = ["EB2B", "CN", "dk"]
FIELDS = ("state", "samples", "exit_step", "alive", "removed", "iterations_sum", "iterations_max")


@pytest.fixture(scope="module")
def X():
    import xpic_amd

    return xpic_amd


@pytest.fixture(scope="module")
def ctx(X):
    g = X.Context("basic", O.N, O.D, 0.7)
    shape = g.fshape()
    g.set_field(X.E, np.zeros(shape) + np.array(O.E_UNIFORM))
    g.set_field(X.B, np.zeros(shape) + np.array(O.B_UNIFORM))
    g.set_mirror_field(field=X.B, **O.MIRROR)
    g.set_field(X.W0, O.grad_abs(g.get_field(X.B)))
    return g


class Run:
    """one pusher on the shared context: its one-step call, its closed trace, its open trace, and the results the tests
    share (each computed once)"""

    def __init__(self, X, ctx, kind):
        self.kind, self.ctx, self.d = kind, ctx, O.D
        self.p = O.particles("dk" if kind == "dk" else "fo", ctx.get_field(X.B))
        self.W0 = X.W0
        self.kw = O.CN_KW if kind == "CN" else {}
        self._cache = {}

    def push(self, p):
        if self.kind == "dk":
            return self.ctx.drift_kinetic_push(p, O.QM, O.MP, O.DT, self.W0)
        return self.ctx.full_orbit_push(p, self.kind, O.QM, O.DT, **self.kw)

    def closed(self, p, steps, sample_every=0):
        if self.kind == "dk":
            return self.ctx.drift_kinetic_trace(p, steps, O.QM, O.MP, O.DT, self.W0, sample_every=sample_every)
        return self.ctx.full_orbit_trace(p, steps, self.kind, O.QM, O.DT, sample_every=sample_every, **self.kw)

    def open(self, p, steps, region=O.REGION, **kw):
        kw.setdefault("sample_every", O.EVERY)
        if self.kind == "dk":
            return self.ctx.drift_kinetic_trace_open(p, steps, O.QM, O.MP, O.DT, region, gradB_field=self.W0, **kw)
        return self.ctx.full_orbit_trace_open(p, steps, self.kind, O.QM, O.DT, region, **self.kw, **kw)

    def host(self, p, steps, region=O.REGION, **kw):
        """the device's one-step call, step by step, with the rule applied on the host to the positions it returned"""
        kw.setdefault("sample_every", O.EVERY)
        return O.trace_open(self.push, p, steps, region, self.d, **kw)

    def once(self, name, make):
        if name not in self._cache:
            self._cache[name] = make()
        return self._cache[name]

    @property
    def full(self):
        return self.once("full", lambda: self.open(self.p, O.STEPS))

    @property
    def every_step(self):
        """the closed trace's state after 0 .. STEPS steps, [STEPS + 1][n][6], and its counters"""
        def make():
            out, samples, tot, mx = self.closed(self.p, O.STEPS, sample_every=1)
            assert np.array_equal(samples[-1], out)
            return np.concatenate([self.p[None], samples]), tot, mx
        return self.once("every_step", make)


@pytest.fixture(scope="module", params=KINDS)
def run(request, X, ctx):
    return Run(X, ctx, request.param)


def same(a, b, what=""):
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert np.asarray(x).shape == np.asarray(y).shape, (what, f)
        assert np.asarray(x).tobytes() == np.asarray(y).astype(np.asarray(x).dtype).tobytes(), (what, f)


def test_exact_against_the_one_step_calls(run):
    got = run.full
    first, later, never = O.groups(got.exit_step)
    print(run.kind, "removed within 64 steps:", first, "later:", later, "never:", never)
    assert min(first, later, never) >= O.NPART // 5
    same(got, run.host(run.p, O.STEPS), run.kind)
    assert got.removed == first + later and got.alive[-1] >= never
    taken = np.where(got.exit_step < 0, O.STEPS, got.exit_step)  # steps each particle took
    if run.kind == "EB2B":
        assert not got.iterations_sum.any() and not got.iterations_max.any()
    elif run.kind == "CN":  # three iterations a step (open_trace_ref.CN_KW)
        assert np.array_equal(got.iterations_sum, 3 * taken) and (got.iterations_max == 3).all()
    else:
        assert (got.iterations_sum >= taken).all() and got.iterations_max.min() >= 1


def test_survivors_equal_the_closed_trace(run):
    got = run.full
    states, tot, mx = run.every_step
    stay = got.exit_step < 0
    assert stay.any()
    assert np.array_equal(got.state[stay], states[-1][stay])
    assert np.array_equal(got.iterations_sum[stay], tot[stay]) and np.array_equal(got.iterations_max[stay], mx[stay])
    # a region that holds everything: the closed trace, whole
    free = run.open(run.p, O.STEPS, region=O.EVERYWHERE)
    out, samples, tot7, mx7 = run.closed(run.p, O.STEPS, sample_every=O.EVERY)
    assert free.removed == 0 and (free.exit_step == -1).all() and (free.alive == O.NPART).all()
    assert free.state.tobytes() == out.tobytes() and free.samples.tobytes() == samples.tobytes()
    assert np.array_equal(free.iterations_sum, tot7) and np.array_equal(free.iterations_max, mx7)


def test_removed_particles_are_frozen(run):
    got = run.full
    states, _, _ = run.every_step
    gone = np.flatnonzero(got.exit_step >= 0)
    assert len(gone)
    assert got.state[gone].tobytes() == states[got.exit_step[gone], gone].tobytes()
    # and the rows behind a removed particle's last step repeat that state; the rows before are the closed trace's
    for k in range(got.samples.shape[0]):
        step = (k + 1) * O.EVERY
        moving = (got.exit_step < 0) | (got.exit_step >= step)
        assert np.array_equal(got.samples[k][moving], states[step][moving]), k
        assert np.array_equal(got.samples[k][~moving], got.state[~moving]), k


def test_composition(run):
    full = run.full
    a = run.open(run.p, O.SPLIT)
    b = run.open(a.state, O.STEPS - O.SPLIT, exit_step=a.exit_step, step0=O.SPLIT)
    assert 0 < a.removed < full.removed
    assert b.state.tobytes() == full.state.tobytes() and np.array_equal(b.exit_step, full.exit_step)
    assert np.concatenate([a.samples, b.samples]).tobytes() == full.samples.tobytes()
    assert np.array_equal(np.concatenate([a.alive, b.alive]), full.alive)
    assert a.removed + b.removed == full.removed
    assert np.array_equal(a.iterations_sum + b.iterations_sum, full.iterations_sum)
    assert np.array_equal(np.maximum(a.iterations_max, b.iterations_max), full.iterations_max)


def test_inputs_are_respected(run):
    """particles that enter removed (whatever the step they claim) come back untouched, in every sample row too, count
    neither as alive nor as removed by this call, and change nothing for the others"""
    idx = np.array([0, 1, 2, 300, O.NPART - 1])
    ex = np.full(O.NPART, -1, dtype=np.int64)
    ex[idx] = [0, 3, 200, 5, 1]
    got = run.open(run.p, O.SPLIT, exit_step=ex, step0=10)
    assert got.state[idx].tobytes() == run.p[idx].tobytes() and np.array_equal(got.exit_step[idx], ex[idx])
    assert (got.samples[:, idx] == run.p[idx]).all()
    assert not got.iterations_sum[idx].any() and not got.iterations_max[idx].any()
    assert got.alive.max() <= O.NPART - len(idx)
    same(got, run.host(run.p, O.SPLIT, exit_step=ex, step0=10), run.kind)
    rest = np.setdiff1d(np.arange(O.NPART), idx)
    plain = run.open(run.p, O.SPLIT)
    assert got.state[rest].tobytes() == plain.state[rest].tobytes()
    moved = plain.exit_step[rest] >= 0
    assert np.array_equal(got.exit_step[rest][moved], plain.exit_step[rest][moved] + 10)
    assert got.removed == moved.sum()


def test_compaction_policies_agree(run):
    """0 (auto), 1 (never) and 2 (always) return the same bits; the profile sections show that the list really was
    rebuilt as often as the policy says (open_trace_ref.compactions), and never under policy 1"""
    label = ("dk" if run.kind == "dk" else "fo") + "_trace_open_compact"
    full = run.full
    ctx = run.ctx
    ctx.profile_enable(True)
    try:
        for policy, name in ((0, "auto"), (1, "never"), (2, "always")):
            ctx.profile_reset()
            got = run.open(run.p, O.STEPS, compact=name)
            same(got, full, (run.kind, name))
            expect = O.compactions(full.exit_step, O.STEPS, policy)
            assert ctx.profile_get(label)[0] == expect, (name, expect)
            assert (policy == 1) == (expect == 0)
    finally:
        ctx.profile_enable(False)
    # an early end: a region that holds nobody removes everybody at the top of step 1, and the later launches are skipped
    nowhere = {"name": "box", "min": (0.0, 0.0, 0.0), "max": (1.0, 1.0, 1.0)}
    for c in (0, 1, 2):
        got = run.open(run.p, O.STEPS, region=nowhere, compact=c)
        assert got.removed == O.NPART and not got.exit_step.any() and not got.alive.any()
        assert got.state.tobytes() == run.p.tobytes() and (got.samples == run.p).all()
        assert not got.iterations_sum.any() and not got.iterations_max.any()


def test_cylinder(run):
    """WithinCylinder: r^2 <= R^2 at the corner, |z - centre| < height / 2 strictly.  Four probes at rest in chosen cells
    (open_trace_ref.with_cylinder_probes); what happens to each at the top of step 1 is commands_ref.within's verdict on
    its cell's corner, and the whole trace is the host rule's again"""
    p = O.with_cylinder_probes(run.p)
    c = O.corner(p[:4, :3], O.D)
    inside = CR.within(O.CYLINDER, c[:, 0], c[:, 1], c[:, 2])
    assert list(inside) == [True, False, False, True]  # on the radius: kept; beyond it, and on the lid: removed
    got = run.open(p, O.SPLIT, region=O.CYLINDER)
    assert list(got.exit_step[:4] == 0) == [not k for k in inside]
    assert got.state[:4][~inside].tobytes() == p[:4][~inside].tobytes()
    assert 0 < got.removed < O.NPART
    same(got, run.host(p, O.SPLIT, region=O.CYLINDER), run.kind)


def test_unequal_spacings(X, run):
    """d = (0.5, 0.4, 0.75), two of them no power of two, so the corner is formed with the divisions
    and the products by dx, dy, dz that d = 1 hides (floor(z / 0.75) 0.75, not floor(z)), and a region whose faces are no
    multiples of the spacings: its z faces 0.8 and 5.1 pass the corners 1.5 .. 4.5.  The batch of the other tests, scaled
    to these cells; again the device's own one-step calls with the rule applied on the host, bit for bit"""
    d = (0.5, 0.4, 0.75)
    g = X.Context("basic", O.N, d, 0.7)
    shape = g.fshape()
    g.set_field(X.E, np.zeros(shape) + np.array(O.E_UNIFORM))
    g.set_field(X.B, np.zeros(shape) + np.array(O.B_UNIFORM))
    g.set_mirror_field(4.0, 2.0, 1.0, field=X.B)
    g.set_field(X.W0, 0.1 * g.get_field(X.B))  # (any vector serves as grad |B|)
    r2 = Run(X, g, run.kind)
    r2.d = d
    p = run.p.copy()
    p[:, :3] *= d
    if run.kind == "dk":
        p[:, 3] *= d[2]
    else:
        p[:, 3:] *= d
    region = {"name": "box", "min": (0.3, 0.3, 0.8), "max": (3.9, 3.1, 5.1)}
    cz = O.corner(p[:, :3], d)[:, 2]
    assert O.keep(region, p[:, :3], d).all() and set(np.unique(cz)) == {2.25, 3.0}
    got = r2.open(p, O.SPLIT, region=region, compact="always")
    assert O.NPART // 5 <= got.removed <= O.NPART - O.NPART // 5
    same(got, r2.host(p, O.SPLIT, region=region), run.kind)
    # the removed stopped in the first cell plane that fails: corner 0.75 (< 0.8) or 5.25 (>= 5.1), not one cell later
    gone = got.exit_step >= 0
    assert set(np.unique(O.corner(got.state[gone, :3], d)[:, 2])) == {0.75, 5.25}


def test_argument_checks(X, run):
    ctx, p = run.ctx, run.p
    # n == 0 and steps == 0 succeed and remove nobody
    got = run.open(np.zeros((0, 6)), 20)
    assert got.state.shape == (0, 6) and got.samples.shape == (2, 0, 6) and got.removed == 0 and not got.alive.any()
    got = run.open(p, 0)
    assert got.state.tobytes() == p.tobytes() and got.removed == 0 and (got.exit_step == -1).all()
    assert got.samples.shape == (0, O.NPART, 6)
    with pytest.raises(X.XpicError, match="steps"):
        run.open(p, -1)
    with pytest.raises(X.XpicError, match="compact"):
        run.open(p, 2, compact=3)
    with pytest.raises(X.XpicError, match="step0"):
        run.open(p, 2, step0=-1)
    # a context of several z-slabs is refused with a message
    two = X.Context("basic", (8, 8, 12), (0.5, 0.5, 0.5), 0.7, rank=0, nranks=2)
    with pytest.raises(X.XpicError, match="z-slab"):
        Run.open(_With(run, two), p[:4], 2)
    # null pointers name themselves
    L_, dp, i64 = ctx.L, C.POINTER(C.c_double), C.POINTER(C.c_int64)
    buf, ex1, al1, rm1 = np.zeros(6), (C.c_int64 * 1)(-1), (C.c_int64 * 1)(), C.c_int64()
    tot1, it1 = (C.c_int64 * 1)(), (C.c_int * 1)()
    ptr, one = buf.ctypes.data_as(dp), C.c_int64(1)
    kind, gp = X._geom7(O.REGION)
    reg = X.TraceRegion(kind, 0, (C.c_double * 7)(*gp[:7]), 0)
    bad = X.TraceRegion(7, 0, (C.c_double * 7)(*gp[:7]), 0)
    if run.kind == "dk":
        P = X.DkParams(O.QM, O.MP, O.DT, 1e-12, 1e-12, 30)
        call = lambda region, ex, rm, state=ptr: L_.xpic_drift_kinetic_trace_open(  # noqa: E731
            ctx.h, one, C.byref(P), -1, one, one, state, None, tot1, it1, region, ex, al1, rm)
    else:
        P = X.FoParams(O.QM, O.DT, 1e-7, 1e-7, X.FO_SCHEMES[run.kind], 30)
        call = lambda region, ex, rm, state=ptr: L_.xpic_full_orbit_trace_open(  # noqa: E731
            ctx.h, one, C.byref(P), one, one, state, None, tot1, it1, region, ex, al1, rm)
    for args, word in (((C.byref(reg), None, C.byref(rm1)), "exit_step"), ((C.byref(reg), ex1, None), "removed"),
                       ((None, ex1, C.byref(rm1)), "region"), ((C.byref(bad), ex1, C.byref(rm1)), "geometry"),
                       ((C.byref(reg), ex1, C.byref(rm1), None), "null")):
        assert call(*args) != 0
        assert word in L_.xpic_last_error().decode(), word
    assert call(C.byref(reg), ex1, C.byref(rm1)) == 0


class _With:
    """a Run's pusher on another context"""

    def __init__(self, run, ctx):
        self.kind, self.ctx, self.W0, self.kw = run.kind, ctx, None, run.kw
