"""The analytic field models on the device (xpic_model_fields, xpic_set_model_field, xpic_model_full_orbit_trace,
xpic_model_drift_kinetic_trace) against the numpy restatement tests/analytic_trace_ref.py (pinned without a GPU by
tests/test_analytic_trace_ref.py), and the identities the header promises, bit for bit.  Shapes as in
tests/test_gpu_open_trace.py: a context of 9 x 8 x 7 nodes with spacings 0.5, 0.4, 0.75 (only the spacings matter: no grid
vector is read), 3 x 256 + 7 particles (300 for Crank-Nicolson), 150 steps sampled every 7 = three launches.

The iterative pushers run with pinned iteration counts in the parity tests, as tests/test_gpu_drift_kinetic.py and
tests/open_trace_ref.py do: with zero tolerances no residual passes, both sides make exactly maxit updates, nothing depends
on a data-dependent exit, and the counters say how many steps a particle took."""
import ctypes as C

import numpy as np
import pytest

import analytic_trace_ref as A

pytestmark = pytest.mark.gpu

N, D = (9, 8, 7), (0.5, 0.4, 0.75)
NPART, NPART_CN = 3 * 256 + 7, 300
STEPS, EVERY, SPLIT = 150, 7, 70
QM, MP, DT = -1.0, 1.0, 0.05
PIN = {"CN": dict(atol=0.0, rtol=0.0, maxit=3), "dk": dict(eps=0.0, delta=0.0, maxit=4)}
KINDS = ["EB2B", "M1A", "BLF", "CN", "dk"]  # EB2B, one A and one LF scheme, Crank-Nicolson, the drift-kinetic pusher
MODELS = {
    "uniform": dict(E0=(0.0, 0.01, 0.02), B0=(0.2, 0.3, 1.0)),
    "linear": dict(E0=(0.0, 0.01, 0.0), B0=(0.0, 0.0, 2.0), r0=(10.0, 10.0, 20.0), g=(0.1, 0.0, 0.02)),
    "quadratic_mirror": dict(E_phi=0.003, phi=0.05, **A.QUADRATIC),
    "gaussian_mirror": dict(A.GAUSSIAN),
}
CENTRE = {"quadratic_mirror": (10.0, 10.0, 20.0), "gaussian_mirror": (5.0, 5.0, 5.0), "uniform": (10.0, 10.0, 20.0),
          "linear": (10.0, 10.0, 20.0)}

# ---- tolerances (the issue's rules; measured on an MI355X)
TOL_PLAIN = 1e-14        # models without exp: sums and products of a handful of doubles
GAUSS_FIELD_MEASURED = 4.85e-16  # largest |device - restatement| / |vector| of the Gaussian model over model_positions()
TOL_GAUSS_FIELD = min(8 * GAUSS_FIELD_MEASURED, 1e-12)
TOL_TRACE = 1e-13        # trace parity on the models without exp: the bound of the pusher parity tests
GAUSS_TRACE_MEASURED = 5.56e-16  # largest deviation of a 150-step Gaussian trace from the restatement, over KINDS, on the scale
                            # of its column group
TOL_GAUSS_TRACE = min(8 * GAUSS_TRACE_MEASURED, 1e-9)


@pytest.fixture(scope="module")
def X():
    import xpic_amd

    return xpic_amd


@pytest.fixture(scope="module")
def ctx(X):
    return X.Context("basic", N, D, 0.7)


def region(name):
    """ends 3 length units from the midplane in z, on cell corners of dz = 0.75 (the box rule is half-open)"""
    zc = CENTRE[name][2]
    return {"name": "box", "min": (-1e6, -1e6, zc - 3.0), "max": (1e6, 1e6, zc + 3.0)}


def particles(name, kind, n, seed=51):
    """as open_trace_ref.particles: within half a unit of the model's centre, three interleaved groups by the speed along z
    (leaves within 64 steps, between 64 and 150, never)"""
    rng = np.random.default_rng(seed)
    r = np.array(CENTRE[name]) + (rng.random((n, 3)) - 0.5)
    group = np.arange(n) % 3
    lo, hi = np.array([1.3, 0.5, 0.1])[group], np.array([2.0, 0.72, 0.25])[group]
    vz = (lo + (hi - lo) * rng.random(n)) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    vperp = 0.1 + 0.2 * rng.random(n)
    ang = 2 * np.pi * rng.random(n)
    if kind != "dk":
        return np.column_stack([r, vperp * np.cos(ang), vperp * np.sin(ang), vz])
    lB = np.sqrt((A.model(name, **MODELS[name])(r)[1] ** 2).sum(axis=1))
    return np.column_stack([r, vz, vperp, MP * vperp * vperp / (2.0 * lB)])


def model_positions(name, n=NPART):
    """random positions around the model's centre out to the throats, then the axis (both branches of the r > tests: on
    it, 1e-11 and 1e-13 off it), the throats and the midplane"""
    rng = np.random.default_rng(7)
    c = np.array(CENTRE[name])
    span = np.array([2.0, 2.0, 2.2 * c[2]]) if name.endswith("mirror") else np.array([4.0, 4.0, 4.0])
    r = c + (rng.random((n, 3)) - 0.5) * span
    special = [c, c + [1e-11, 0, 0], c + [0, 1e-13, 0], c + [1e-9, 1e-9, 0.3], [c[0], c[1], 0.0], [c[0], c[1], 2 * c[2]],
               [c[0] + 0.1, c[1], 0.0], [c[0], c[1] - 0.2, 2 * c[2]], [c[0] + 0.1, c[1], c[2]]]
    r[: len(special)] = np.array(special, dtype=np.float64)
    return r


def vector_error(got, ref):
    """largest |got - ref| on the scale of the reference vector's length at that position (of the batch's largest where a
    vector is 0)"""
    l = np.sqrt((ref * ref).sum(axis=1))
    scale = np.where(l > 0, l, max(l.max(), 1e-300))
    return (np.abs(got - ref).max(axis=1) / scale).max()


@pytest.mark.parametrize("name", list(MODELS))
def test_model_fields(X, ctx, name):
    r = model_positions(name)
    got = ctx.model_fields(X.field_model(name, **MODELS[name]), r)
    ref = A.model(name, **MODELS[name])(r)
    errs = [vector_error(g, f) for g, f in zip(got, ref)]
    print(name, "E, B, gradB: largest |device - restatement| / |vector| =", errs)
    tol = TOL_GAUSS_FIELD if name == "gaussian_mirror" else TOL_PLAIN
    assert np.isfinite(np.concatenate(got)).all()
    assert max(errs) <= tol
    if name.endswith("mirror"):  # on the axis the transverse gradient is the else branch's exact 0; 1e-11 off it lies
        # under the quadratic mirror's threshold (1e-10) and over the Gaussian one's (1e-12)
        assert (got[2][[0, 2], :2] == 0).all() and (got[2][3, :2] != 0).any()
        assert (got[2][1, 0] == 0) == (name == "quadratic_mirror")


@pytest.mark.parametrize("n,d", [((8, 8, 8), (1.0, 1.0, 1.0)), (N, D)], ids=["cubic", "9x8x7"])
def test_set_model_field(X, n, d):
    """node by node against the restatement at (i dx, j dy, k dz), tolerance of tests/test_gpu_mirror_field.py; a skipped
    id leaves its vector untouched"""
    g = X.Context("basic", n, d, 0.7)
    base = np.random.default_rng(5).normal(size=g.fshape())
    k, j, i = np.meshgrid(np.arange(n[2]), np.arange(n[1]), np.arange(n[0]), indexing="ij")
    r = np.column_stack([i.ravel() * d[0], j.ravel() * d[1], k.ravel() * d[2]])
    for name in ("quadratic_mirror", "gaussian_mirror"):
        for fid in (X.E, X.B, X.W0):
            g.set_field(fid, base)
        m = X.field_model(name, **MODELS[name])
        ref = [f.reshape(g.fshape()) for f in A.model(name, **MODELS[name])(r)]
        g.set_model_field(m, X.E, X.B, X.W0)
        for fid, f in zip((X.E, X.B, X.W0), ref):
            assert np.abs(g.get_field(fid) - f).max() <= 1e-12 * max(np.abs(f).max(), 1e-300), (name, fid)
        g.set_field(X.E, base)
        g.set_field(X.W0, base)
        g.set_field(X.B, 0 * base)
        g.set_model_field(m, None, X.B, None)
        assert np.array_equal(g.get_field(X.E), base) and np.array_equal(g.get_field(X.W0), base)
        assert np.abs(g.get_field(X.B) - ref[1]).max() <= 1e-12 * np.abs(ref[1]).max()
    with pytest.raises(X.XpicError):
        g.set_model_field(m, X.B, X.B, None)
    with pytest.raises(X.XpicError):
        g.set_model_field(m, 99, X.B, None)


class Run:
    """one pusher on one model: the device call, the restatement, and the results the tests share (each computed once)"""

    def __init__(self, X, ctx, name, kind):
        self.X, self.ctx, self.name, self.kind = X, ctx, name, kind
        self.m = X.field_model(name, **MODELS[name])
        self.p = particles(name, kind, NPART_CN if kind == "CN" else NPART)
        self.kw = PIN.get(kind, {})
        self._cache = {}

    def call(self, p, steps, reg=None, **kw):
        if self.kind == "dk":
            return self.ctx.model_drift_kinetic_trace(p, steps, QM, MP, DT, self.m, reg, **self.kw, **kw)
        return self.ctx.model_full_orbit_trace(p, steps, self.kind, QM, DT, self.m, reg, **self.kw, **kw)

    def ref(self, p, steps, reg=None, **kw):
        push = A.pusher(self.kind, A.model(self.name, **MODELS[self.name]), QM, MP, DT, **self.kw)
        return A.trace(push, p, steps, reg, D, **kw)

    def once(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    @property
    def full(self):
        return self.once("full", lambda: self.call(self.p, STEPS, region(self.name), sample_every=EVERY))

    @property
    def closed_every_step(self):
        return self.once("closed", lambda: self.call(self.p, STEPS, None, sample_every=1))


@pytest.fixture(scope="module", params=[(m, k) for m in ("quadratic_mirror", "gaussian_mirror") for k in KINDS],
                ids=lambda mk: "%s-%s" % mk)
def run(request, X, ctx):
    return Run(X, ctx, *request.param)


def group_error(got, ref):
    """largest deviation of records [..][6] on the scale of the column group (positions, the rest)"""
    got, ref = np.asarray(got), np.asarray(ref)
    return max(np.abs(got[..., :3] - ref[..., :3]).max() / np.abs(ref[..., :3]).max(),
               np.abs(got[..., 3:] - ref[..., 3:]).max() / np.abs(ref[..., 3:]).max())


def test_trace_against_the_restatement(run):
    """final states, samples, iteration counters, exit_step, alive and removed of the open trace"""
    got = run.full
    ref = run.once("ref", lambda: run.ref(run.p, STEPS, region(run.name), sample_every=EVERY))
    ex = got.exit_step
    first, later, never = int(((ex >= 0) & (ex < 64)).sum()), int((ex >= 64).sum()), int((ex < 0).sum())
    err = max(group_error(got.state, ref.state), group_error(got.samples, ref.samples))
    print(run.name, run.kind, "removed within 64 steps:", first, "later:", later, "never:", never, "deviation", err)
    assert min(first, later, never) >= len(run.p) // 5
    assert err <= (TOL_GAUSS_TRACE if run.name == "gaussian_mirror" else TOL_TRACE)
    assert np.array_equal(got.exit_step, ref.exit_step) and np.array_equal(got.alive, ref.alive)
    assert got.removed == ref.removed == first + later
    assert np.array_equal(got.iterations_sum, ref.iterations_sum) and np.array_equal(got.iterations_max, ref.iterations_max)
    taken = np.where(ex < 0, STEPS, ex)
    if run.kind in PIN:  # pinned: every step ran out of maxit, and the call goes on
        assert np.array_equal(got.iterations_sum, taken * PIN[run.kind]["maxit"])
    else:
        assert not got.iterations_sum.any() and not got.iterations_max.any()


FIELDS = ("state", "samples", "exit_step", "alive", "removed", "iterations_sum", "iterations_max")


def same(a, b, what="", fields=FIELDS):
    for f in fields:
        x, y = np.asarray(getattr(a, f)), np.asarray(getattr(b, f))
        assert x.shape == y.shape, (what, f)
        assert x.tobytes() == y.astype(x.dtype).tobytes(), (what, f)


def test_trace_is_its_one_step_calls(run):
    """the open trace against the device's steps = 1 calls composed on the host with the rule applied there"""
    import open_trace_ref as O

    n = 64 * 3 + 5  # a ragged workgroup is enough here: the composition costs a call per step
    p = run.p[:n]

    def one(q):
        out = run.call(q, 1)
        return out.state, out.iterations_max
    host = O.trace_open(one, p, STEPS, region(run.name), D, sample_every=EVERY)
    same(run.call(p, STEPS, region(run.name), sample_every=EVERY), host, run.kind)


def test_composition_through_step0(run):
    reg = region(run.name)
    a = run.call(run.p, SPLIT, reg, sample_every=EVERY)
    b = run.call(a.state, STEPS - SPLIT, reg, sample_every=EVERY, exit_step=a.exit_step, step0=SPLIT)
    full = run.full
    assert full.state.tobytes() == b.state.tobytes() and np.array_equal(full.exit_step, b.exit_step)
    assert np.array_equal(full.samples, np.concatenate([a.samples, b.samples]))
    assert np.array_equal(full.alive, np.concatenate([a.alive, b.alive]))
    assert full.removed == a.removed + b.removed
    assert np.array_equal(full.iterations_sum, a.iterations_sum + b.iterations_sum)
    assert np.array_equal(full.iterations_max, np.maximum(a.iterations_max, b.iterations_max))
    # a particle that enters removed comes back untouched
    assert (a.exit_step >= 0).any()
    gone = a.exit_step >= 0
    assert b.state[gone].tobytes() == a.state[gone].tobytes() and not b.iterations_sum[gone].any()


def test_open_and_closed_agree(run):
    closed = run.closed_every_step
    assert (closed.exit_step == -1).all() and closed.removed == 0 and (closed.alive == len(run.p)).all()
    # a region nobody leaves: the open call is the "no region" call
    nobody = {"name": "box", "min": (-1e6,) * 3, "max": (1e6,) * 3}
    same(run.call(run.p, STEPS, nobody, sample_every=1), closed, run.kind)
    # explicit exit_step under "no region" (non-null outputs) says the same
    same(run.call(run.p, STEPS, None, sample_every=1, exit_step=np.full(len(run.p), -1)), closed, run.kind)
    # a removed particle is the closed call stopped at exit_step
    full = run.full
    every = np.concatenate([run.p[None], closed.samples])
    taken = np.where(full.exit_step < 0, STEPS, full.exit_step)
    assert full.state.tobytes() == every[taken, np.arange(len(run.p))].tobytes()


def test_loss_cone(X, ctx):
    """tests/test_analytic_trace_ref.py's 64 guiding centres on the device: the same half leaves, the same half stays, and
    exit_step is within one step of the restatement's"""
    p, dt = A.cone_batch()
    steps = A.cone_steps(dt)
    field = A.model("gaussian_mirror", **A.GAUSSIAN)
    ref = A.trace(A.pusher("dk", field, A.QM, A.MP, dt), p, steps, A.cone_region(), A.CONE_D)
    g = X.Context("basic", (8, 8, 8), A.CONE_D, 0.7)
    got = g.model_drift_kinetic_trace(p, steps, A.QM, A.MP, dt, X.field_model("gaussian_mirror", **A.GAUSSIAN), A.cone_region())
    h = A.CONE_N // 2
    assert (got.exit_step[:h] >= 0).all() and (got.exit_step[h:] < 0).all() and got.removed == h
    assert np.abs(got.exit_step[:h] - ref.exit_step[:h]).max() <= 1
    assert got.iterations_max.max() < 30


def test_edges(X, ctx):
    m = X.field_model("gaussian_mirror", **A.GAUSSIAN)
    p = particles("gaussian_mirror", "fo", 5)
    for n in (0, 1):
        for out in (ctx.model_full_orbit_trace(p[:n], 3, "EB2B", QM, DT, m, sample_every=1),
                    ctx.model_drift_kinetic_trace(p[:n], 3, QM, MP, DT, m, region("gaussian_mirror"), sample_every=1)):
            assert out.state.shape == (n, 6) and out.samples.shape == (3, n, 6) and np.isfinite(out.state).all()
            assert out.removed == 0 and (out.alive == n).all()
    for out in (ctx.model_full_orbit_trace(p, 0, "CN", QM, DT, m), ctx.model_drift_kinetic_trace(p, 0, QM, MP, DT, m)):
        assert out.state.tobytes() == p.tobytes() and not out.iterations_sum.any()
    # a NaN particle: no index is formed from a position, its neighbours are untouched, and it fails every region
    q = p.copy()
    q[2, 0] = np.nan
    for kind in ("EB2B", "CN"):
        a, b = ctx.model_full_orbit_trace(q, 5, kind, QM, DT, m), ctx.model_full_orbit_trace(p, 5, kind, QM, DT, m)
        assert np.isnan(a.state[2]).any() and np.delete(a.state, 2, 0).tobytes() == np.delete(b.state, 2, 0).tobytes()
    a = ctx.model_drift_kinetic_trace(q, 5, QM, MP, DT, m, region("gaussian_mirror"))
    assert a.exit_step[2] == 0 and a.removed == 1 and (np.delete(a.exit_step, 2) == -1).all()
    # a Picard loop that runs out of maxit: the call succeeds and the counters say so
    out = ctx.model_drift_kinetic_trace(p, 4, QM, MP, DT, m, eps=0.0, delta=0.0, maxit=2)
    assert (out.iterations_max == 2).all() and (out.iterations_sum == 8).all() and np.isfinite(out.state).all()
    # every scheme id runs
    for sid in X.FO_SCHEMES:
        assert np.isfinite(ctx.model_full_orbit_trace(p, 2, sid, QM, 0.01, m).state).all(), sid


def test_null_outputs_and_argument_checks(X, ctx):
    m = X.field_model("quadratic_mirror", **MODELS["quadratic_mirror"])
    p = np.ascontiguousarray(particles("quadratic_mirror", "fo", 3))
    L_, dp, i64 = ctx.L, C.POINTER(C.c_double), C.POINTER(C.c_int64)
    F, K = X.FoParams(QM, DT, 1e-7, 1e-7, X.FO_SCHEMES["EB2B"], 30), X.DkParams(QM, MP, DT, 1e-12, 1e-12, 30)
    none = X.TraceRegion(X.GEOM_NONE, 0, (C.c_double * 7)(), 0)
    box = X.TraceRegion(0, 0, (C.c_double * 7)(-1e6, -1e6, -1e6, 1e6, 1e6, 1e6, 0), 0)
    tot, mx = np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.int32)

    def fo(params=F, model=m, reg=none, state=p, ex=None, rm=None):
        s = state.copy()
        return L_.xpic_model_full_orbit_trace(ctx.h, C.c_int64(3), C.byref(params), C.byref(model) if model else None,
                                              C.c_int64(2), C.c_int64(0), s.ctypes.data_as(dp), None, None, None,
                                              C.byref(reg) if reg else None, ex, None, rm)

    def dk(params=K, model=m, reg=none):
        s = p.copy()
        return L_.xpic_model_drift_kinetic_trace(ctx.h, C.c_int64(3), C.byref(params), C.byref(model) if model else None,
                                                 C.c_int64(2), C.c_int64(0), s.ctypes.data_as(dp), None,
                                                 tot.ctypes.data_as(i64), mx.ctypes.data_as(C.POINTER(C.c_int)),
                                                 C.byref(reg) if reg else None, None, None, None)
    assert fo() == 0 and dk() == 0                      # every optional output null under "no region"
    assert fo(reg=box) != 0 and dk(reg=box) != 0        # a region needs exit_step and removed
    assert fo(model=None) != 0 and dk(model=None) != 0  # null model
    assert fo(reg=None) != 0
    bad = X.field_model(7)
    assert fo(model=bad) != 0 and b"kind" in L_.xpic_last_error()
    assert fo(model=X.field_model("quadratic_mirror", B_min=1, B_max=4, W=0.0, D=40.0)) != 0
    assert dk(model=X.field_model("gaussian_mirror", B_min=1, B_max=4, L=5.0, W=0.0)) != 0
    assert fo(params=X.FoParams(QM, DT, 1e-7, 1e-7, 18, 30)) != 0 and fo(params=X.FoParams(QM, DT, 1e-7, 1e-7, -1, 30)) != 0
    assert fo(params=X.FoParams(QM, DT, 1e-7, 1e-7, X.FO_SCHEMES["CN"], 65)) != 0
    assert dk(params=X.DkParams(QM, MP, DT, 1e-12, 1e-12, 0)) != 0
    assert dk(params=X.DkParams(QM, MP, DT, 1e-12, 1e-12, X.MODEL_DK_MAXIT + 1)) != 0
    assert fo(reg=X.TraceRegion(5, 0, (C.c_double * 7)(), 0)) != 0
    with pytest.raises(X.XpicError):
        ctx.model_fields(bad, p[:, :3])
    with pytest.raises(X.XpicError):
        X.field_model("uniform", nonsense=1.0)
