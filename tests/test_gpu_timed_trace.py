"""The model traces with a time envelope on the device (xpic_amd/csrc/model_trace.hip; include/xpic_hip.h:
xpic_field_envelope, xpic_model_full_orbit_trace_timed, xpic_model_drift_kinetic_trace_timed, xpic_envelope_factors)
against the reference's tables of crank_nicolson_push_ex3, against the untimed model traces, and against the numpy
restatement tests/timed_trace_ref.py (pinned without a GPU by tests/test_timed_trace_ref.py).  Shapes as in
tests/test_gpu_model_trace.py: a context of 9 x 8 x 7 nodes, 3 x 256 + 7 particles (300 for Crank-Nicolson), 150 steps
sampled every 7 = three launches; iterations pinned with zero tolerances in the parity cases."""
import ctypes as C
import os

import numpy as np
import pytest

import analytic_trace_ref as A
import full_orbit_ref as FO
import timed_trace_ref as T

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crank_nicolson_push_ex3")
TABLE_FLOOR = 1e-11  # tests/test_timed_trace_ref.py
KINDS, MODELS, ENVELOPES = T.KINDS, T.MODELS, T.ENVELOPES
STEPS, EVERY, SPLIT = T.STEPS, T.EVERY, T.SPLIT
EPS = np.finfo(np.float64).eps

# ---- tolerances (the issue's rules; measured on an MI355X)
TOL_TRACE = 1e-13  # the ramp on the models without exp: the bound of the pusher parity tests
# largest deviation of a 150-step trace from the restatement on the scale of its column group, over KINDS: the harmonic on
# every model, and either envelope on the Gaussian mirror
TRACE_MEASURED = 5.33e-15  # quadratic mirror, M1A and BLF (sin / cos of the rotation angle); EB2B, CN, dk: at most 9.7e-16
TOL_TRACE_MEASURED = min(8 * TRACE_MEASURED, 1e-9)
# largest |device - restatement| of sums_4 relative to the restatement's sum of |terms|, over the full-orbit kinds, the
# models and the envelopes.  The terms are those the sums are made of: 0.5 |pn.p|^2, 0.5 |p0.p|^2 and qm dt (vh . E_s) for
# the energy balance, vh and its parallel part for the transverse velocity (timed_trace_ref.step_sums).  What a whole step
# adds is no scale for the energy balance: Crank-Nicolson conserves it exactly, each step adds rounding only (1e-17 here),
# and on that scale the two sides differ by up to 0.49 of the sum (0.19 for the velocity component along B, which is
# rounding too; at most 4.8e-15 for the other two) -- printed below, not asserted.
SUMS_MEASURED = 2.99e-15  # Gaussian mirror, BLF
TOL_SUMS = min(8 * SUMS_MEASURED, 1e-12)
# largest |device - numpy| of the harmonic's factors (cos of arguments up to 1.7e5)
FACTOR_MEASURED = 1.12e-16  # one unit in the last place below 1
TOL_FACTOR = min(8 * FACTOR_MEASURED, 4 * EPS)


@pytest.fixture(scope="module")
def X():
    import xpic_amd

    return xpic_amd


@pytest.fixture(scope="module")
def ctx(X):
    return X.Context("basic", T.N, T.D, 0.7)


def envelope(X, env):
    if env is None:
        return None
    return X.field_envelope(env["kind"], **{k: v for k, v in env.items() if k != "kind"})


# ---- 1. crank_nicolson_push_ex3 on the device
@pytest.mark.parametrize("omega_dt,steps,rows", [(1000.0, 188, 189), (100.0, 1885, 126), (10.0, 18850, 124)])
def test_crank_nicolson_ex3_on_the_device(X, ctx, omega_dt, steps, rows):
    """one lane, the default tolerances: the start and the samples are the rows of the reference's table, and sums_4 of the
    geom_nt + 1 steps meets its two checks"""
    dt, nt, every = T.ex3_run(omega_dt)
    assert nt == steps
    gold = np.loadtxt(os.path.join(GOLD, "omega_dt_%.1f.txt" % omega_dt), skiprows=1)
    out = ctx.model_full_orbit_trace_timed([T.EX3_START], nt + 1, "CN", T.EX3_QM, dt, X.field_model("uniform", **T.EX3_MODEL),
                                           envelope(X, T.EX3_ENVELOPE), sample_every=every, sums=True)
    mine = T.ex3_rows(T.EX3_START, out.samples, dt, every, rows)
    assert mine.shape == gold.shape == (rows, 7)
    err = np.abs(mine - gold)
    bound = FO.table_bound(gold, TABLE_FLOOR)
    energy, drift = T.ex3_checks(out.sums[0], dt, nt)
    print("omega_dt", omega_dt, "steps", nt, "largest error / bound", (err / bound).max(), "energy", energy, "drift", drift,
          "iterations_max", out.iterations_max[0])
    assert out.iterations_max[0] < FO.CN_MAXIT
    assert (err <= bound).all()
    assert energy <= T.EX3_ENERGY_BOUND
    assert drift < T.EX3_DRIFT_BOUND


class Run:
    """one pusher on one model: the device calls, the restatement, and the results the tests share (each computed once)"""

    def __init__(self, X, ctx, name, kind):
        self.X, self.ctx, self.name, self.kind = X, ctx, name, kind
        self.m = X.field_model(name, **MODELS[name])
        self.p = T.particles(name, kind, T.NPART_CN if kind == "CN" else T.NPART)
        self.kw = T.PIN.get(kind, {})
        self.fo = kind != "dk"
        self._cache = {}

    def untimed(self, p, steps, reg=None, **kw):
        if self.kind == "dk":
            return self.ctx.model_drift_kinetic_trace(p, steps, T.QM, T.MP, T.DT, self.m, reg, **self.kw, **kw)
        return self.ctx.model_full_orbit_trace(p, steps, self.kind, T.QM, T.DT, self.m, reg, **self.kw, **kw)

    def call(self, env, p, steps, reg=None, **kw):
        e = envelope(self.X, env)
        if self.kind == "dk":
            return self.ctx.model_drift_kinetic_trace_timed(p, steps, T.QM, T.MP, T.DT, self.m, e, reg, **self.kw, **kw)
        return self.ctx.model_full_orbit_trace_timed(p, steps, self.kind, T.QM, T.DT, self.m, e, reg, **self.kw, **kw)

    def once(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    def full(self, ename):
        """the open trace of all steps with the named envelope (and the sums, for a full orbit)"""
        sums = dict(sums=True) if self.fo else {}
        return self.once(("full", ename), lambda: self.call(ENVELOPES[ename], self.p, STEPS, T.region(self.name),
                                                            sample_every=EVERY, **sums))

    def ref(self, ename):
        return self.once(("ref", ename), lambda: T.trace(
            self.kind, A.model(self.name, **MODELS[self.name]), ENVELOPES[ename], self.p, STEPS, T.QM, T.MP, T.DT,
            T.region(self.name), T.D, sample_every=EVERY, sums=True if self.fo else None, **self.kw))


@pytest.fixture(scope="module", params=[(m, k) for m in MODELS for k in KINDS], ids=lambda mk: "%s-%s" % mk)
def run(request, X, ctx):
    return Run(X, ctx, *request.param)


FIELDS = ("state", "samples", "exit_step", "alive", "removed", "iterations_sum", "iterations_max")


def same(a, b, what="", fields=FIELDS):
    for f in fields:
        x, y = np.asarray(getattr(a, f)), np.asarray(getattr(b, f))
        assert x.shape == y.shape, (what, f)
        assert x.tobytes() == y.astype(x.dtype).tobytes(), (what, f)


# ---- 2. envelope off
@pytest.mark.parametrize("with_region", [False, True], ids=["closed", "region"])
def test_envelope_off_is_the_model_trace(run, with_region):
    """a null and a constant envelope against xpic_model_full_orbit_trace / xpic_model_drift_kinetic_trace, bit for bit"""
    reg = T.region(run.name) if with_region else None
    base = run.untimed(run.p, STEPS, reg, sample_every=EVERY)
    assert (base.removed > 0) == with_region
    for env in (None, {"kind": "constant"}):
        same(run.call(env, run.p, STEPS, reg, sample_every=EVERY), base, (run.kind, env))
    if run.fo:  # asking for the sums does not change the trace
        same(run.call(None, run.p, STEPS, reg, sample_every=EVERY, sums=True), base, (run.kind, "sums"))


# ---- 3. composition
@pytest.mark.parametrize("ename", list(ENVELOPES))
def test_composition_through_step0(run, ename):
    """150 = 70 + 80: a launch boundary inside both parts; states, samples, counters, exit_step and sums_4 fed back"""
    env, reg = ENVELOPES[ename], T.region(run.name)
    sums = dict(sums=True) if run.fo else {}
    a = run.call(env, run.p, SPLIT, reg, sample_every=EVERY, **sums)
    back = dict(sums=a.sums) if run.fo else {}
    b = run.call(env, a.state, STEPS - SPLIT, reg, sample_every=EVERY, exit_step=a.exit_step, step0=SPLIT, **back)
    full = run.full(ename)
    assert full.state.tobytes() == b.state.tobytes() and np.array_equal(full.exit_step, b.exit_step)
    assert np.array_equal(full.samples, np.concatenate([a.samples, b.samples]))
    assert np.array_equal(full.alive, np.concatenate([a.alive, b.alive]))
    assert full.removed == a.removed + b.removed
    assert np.array_equal(full.iterations_sum, a.iterations_sum + b.iterations_sum)
    assert np.array_equal(full.iterations_max, np.maximum(a.iterations_max, b.iterations_max))
    if run.fo:
        assert full.sums.tobytes() == b.sums.tobytes()
    # the clock matters wherever the model has an E and the pusher reads it (the magnetic Chin kicks do not)
    if run.kind in ("EB2B", "CN", "dk") and run.name != "gaussian_mirror":
        c = run.call(env, a.state, STEPS - SPLIT, reg, exit_step=a.exit_step, step0=0)
        assert c.state.tobytes() != b.state.tobytes()


# ---- 4. parity with the restatement, 6. region
def group_error(got, ref):
    """largest deviation of records [..][6] on the scale of the column group (positions, the rest)"""
    got, ref = np.asarray(got), np.asarray(ref)
    return max(np.abs(got[..., :3] - ref[..., :3]).max() / np.abs(ref[..., :3]).max(),
               np.abs(got[..., 3:] - ref[..., 3:]).max() / np.abs(ref[..., 3:]).max())


@pytest.mark.parametrize("ename", list(ENVELOPES))
def test_trace_against_the_restatement(run, ename):
    """final states, samples and sums_4 within the bounds; iteration counters, exit_step, alive and removed exactly"""
    got, ref = run.full(ename), run.ref(ename)
    err = max(group_error(got.state, ref.state), group_error(got.samples, ref.samples))
    ex = got.exit_step
    first, later, never = int(((ex >= 0) & (ex < 64)).sum()), int((ex >= 64).sum()), int((ex < 0).sum())
    print(run.name, run.kind, ename, "removed within 64 steps:", first, "later:", later, "never:", never, "deviation", err)
    measured = ename == "harmonic" or run.name == "gaussian_mirror"
    assert err <= (TOL_TRACE_MEASURED if measured else TOL_TRACE)
    assert min(first, later, never) >= len(run.p) // 5
    assert np.array_equal(got.exit_step, ref.exit_step) and np.array_equal(got.alive, ref.alive)
    assert got.removed == ref.removed == first + later
    assert np.array_equal(got.iterations_sum, ref.iterations_sum) and np.array_equal(got.iterations_max, ref.iterations_max)
    if run.fo:
        scale = np.where(ref.sums_abs > 0, ref.sums_abs, 1.0)
        serr = (np.abs(got.sums - ref.sums) / scale).max()
        steps_scale = np.where(ref.sums_steps_abs > 0, ref.sums_steps_abs, 1.0)
        print(run.name, run.kind, ename, "sums: largest |device - restatement| / sum of |terms|", serr,
              "; per column on the scale of what the steps added:", (np.abs(got.sums - ref.sums) / steps_scale).max(axis=0))
        assert np.isfinite(got.sums).all()
        assert serr <= TOL_SUMS
        # a removed particle adds nothing after its exit: its sums are those of the closed trace's first exit_step steps
        assert (got.sums[ex == 0] == 0).all()


# ---- 5. factors
@pytest.mark.parametrize("step0", [0, 1999990])
def test_envelope_factors(X, ctx, step0):
    """the device function of the traces against numpy: more than one workgroup, step0 near 2e6"""
    n, steps = 300, step0 + np.arange(300)
    for dt in (T.DT, 0.1):
        for env in ({"kind": "ramp", "a": 0.0, "b": 1.0}, ENVELOPES["ramp"], {"kind": "ramp", "a": -2.0, "b": 1e-3}):
            got = ctx.envelope_factors(envelope(X, env), dt, step0, n)
            assert got.tobytes() == T.factor(env, steps, dt).tobytes(), env
        for env in (None, {"kind": "constant"}):
            assert (ctx.envelope_factors(envelope(X, env), dt, step0, n) == 1.0).all()
        for env in (ENVELOPES["harmonic"], {"kind": "harmonic", "omega": 0.37, "phase": -1.0}):
            err = np.abs(ctx.envelope_factors(envelope(X, env), dt, step0, n) - T.factor(env, steps, dt)).max()
            print("harmonic", env, "dt", dt, "step0", step0, "largest |device - numpy|", err)
            assert err <= TOL_FACTOR
    assert ctx.envelope_factors(envelope(X, ENVELOPES["ramp"]), T.DT, 5, 0).shape == (0,)


# ---- 7. edges
def test_edges(X, ctx):
    name = "quadratic_mirror"
    m = X.field_model(name, **MODELS[name])
    ramp, reg = envelope(X, ENVELOPES["ramp"]), T.region(name)
    p = T.particles(name, "fo", 5)
    g = T.particles(name, "dk", 5)
    for n in (0, 1):
        for out in (ctx.model_full_orbit_trace_timed(p[:n], 3, "EB2B", T.QM, T.DT, m, ramp, sample_every=1, sums=True),
                    ctx.model_drift_kinetic_trace_timed(g[:n], 3, T.QM, T.MP, T.DT, m, ramp, reg, sample_every=1)):
            assert out.state.shape == (n, 6) and out.samples.shape == (3, n, 6) and np.isfinite(out.state).all()
            assert out.removed == 0 and (out.alive == n).all()
    one = ctx.model_full_orbit_trace_timed(p[:1], 3, "EB2B", T.QM, T.DT, m, ramp, sums=True)
    five = ctx.model_full_orbit_trace_timed(p, 3, "EB2B", T.QM, T.DT, m, ramp, sums=True)
    assert one.state.tobytes() == five.state[:1].tobytes() and one.sums.tobytes() == five.sums[:1].tobytes()
    # steps = 0: the inputs come back, the sums that went in too
    pre = np.arange(20.0).reshape(5, 4)
    out = ctx.model_full_orbit_trace_timed(p, 0, "CN", T.QM, T.DT, m, ramp, sums=pre)
    assert out.state.tobytes() == p.tobytes() and not out.iterations_sum.any() and out.sums.tobytes() == pre.tobytes()
    assert ctx.model_drift_kinetic_trace_timed(g, 0, T.QM, T.MP, T.DT, m, ramp).state.tobytes() == g.tobytes()
    # the sums go on from what went in
    out = ctx.model_full_orbit_trace_timed(p, 3, "EB2B", T.QM, T.DT, m, ramp, sums=pre)
    assert np.allclose(out.sums - pre, five.sums, rtol=0, atol=64 * EPS * np.abs(pre).max())
    # a NaN particle stays NaN, harms no neighbour and adds NaN only to its own sums
    q = p.copy()
    q[2, 0] = np.nan
    for kind in ("EB2B", "CN"):
        a = ctx.model_full_orbit_trace_timed(q, 5, kind, T.QM, T.DT, m, ramp, sums=True)
        b = ctx.model_full_orbit_trace_timed(p, 5, kind, T.QM, T.DT, m, ramp, sums=True)
        assert np.isnan(a.state[2]).any() and np.delete(a.state, 2, 0).tobytes() == np.delete(b.state, 2, 0).tobytes()
        assert np.isnan(a.sums[2]).any() and np.delete(a.sums, 2, 0).tobytes() == np.delete(b.sums, 2, 0).tobytes()
    gq = g.copy()
    gq[2, 0] = np.nan
    a = ctx.model_drift_kinetic_trace_timed(gq, 5, T.QM, T.MP, T.DT, m, ramp, reg)
    assert a.exit_step[2] == 0 and a.removed == 1 and (np.delete(a.exit_step, 2) == -1).all()
    # every scheme id runs, with and without the sums
    for sid in X.FO_SCHEMES:
        for sums in (None, True):
            assert np.isfinite(ctx.model_full_orbit_trace_timed(p, 2, sid, T.QM, 0.01, m, ramp, sums=sums).state).all(), sid
    # a z-slab context is accepted: no grid vector is read
    slab, whole = X.Context("basic", (8, 8, 12), T.D, 0.7, rank=0, nranks=2), ctx
    a = slab.model_full_orbit_trace_timed(p, 70, "CN", T.QM, T.DT, m, ramp, sums=True)
    b = whole.model_full_orbit_trace_timed(p, 70, "CN", T.QM, T.DT, m, ramp, sums=True)
    assert a.state.tobytes() == b.state.tobytes() and a.sums.tobytes() == b.sums.tobytes()
    a = slab.model_drift_kinetic_trace_timed(g, 70, T.QM, T.MP, T.DT, m, ramp)
    assert a.state.tobytes() == whole.model_drift_kinetic_trace_timed(g, 70, T.QM, T.MP, T.DT, m, ramp).state.tobytes()


def test_null_outputs_and_argument_checks(X, ctx):
    m = X.field_model("quadratic_mirror", **MODELS["quadratic_mirror"])
    p = np.ascontiguousarray(T.particles("quadratic_mirror", "fo", 3))
    L_, dp, i64 = ctx.L, C.POINTER(C.c_double), C.POINTER(C.c_int64)
    F, K = X.FoParams(T.QM, T.DT, 1e-7, 1e-7, X.FO_SCHEMES["EB2B"], 30), X.DkParams(T.QM, T.MP, T.DT, 1e-12, 1e-12, 30)
    ramp = X.field_envelope("ramp", a=0.5, b=0.3)
    none = X.TraceRegion(X.GEOM_NONE, 0, (C.c_double * 7)(), 0)
    box = X.TraceRegion(0, 0, (C.c_double * 7)(-1e6, -1e6, -1e6, 1e6, 1e6, 1e6, 0), 0)
    tot, mx = np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.int32)
    sums = np.zeros((3, 4))

    def fo(params=F, model=m, env=ramp, reg=none, steps=2, sums_4=None):
        s = p.copy()
        return L_.xpic_model_full_orbit_trace_timed(
            ctx.h, C.c_int64(3), C.byref(params), C.byref(model) if model else None, C.byref(env) if env else None,
            C.c_int64(steps), C.c_int64(0), s.ctypes.data_as(dp), None, None, None, C.byref(reg) if reg else None, None, None,
            None, sums_4)

    def dk(params=K, model=m, env=ramp, reg=none):
        s = p.copy()
        return L_.xpic_model_drift_kinetic_trace_timed(
            ctx.h, C.c_int64(3), C.byref(params), C.byref(model) if model else None, C.byref(env) if env else None,
            C.c_int64(2), C.c_int64(0), s.ctypes.data_as(dp), None, tot.ctypes.data_as(i64),
            mx.ctypes.data_as(C.POINTER(C.c_int)), C.byref(reg) if reg else None, None, None, None)

    def refused(rc, word):
        return rc != 0 and word in L_.xpic_last_error()
    assert fo() == 0 and dk() == 0 and fo(env=None) == 0 and dk(env=None) == 0  # every optional output null
    assert fo(sums_4=sums.ctypes.data_as(dp)) == 0 and sums.any()
    assert refused(fo(reg=box), b"exit_step") and refused(dk(reg=box), b"exit_step")  # a region needs exit_step and removed
    assert refused(fo(model=None), b"model is null") and refused(dk(model=None), b"model is null")
    assert refused(fo(reg=None), b"region is null")
    for bad in (X.field_envelope(3), X.field_envelope(-1)):
        assert refused(fo(env=bad), b"unknown envelope kind") and refused(dk(env=bad), b"unknown envelope kind")
    for bad in (X.field_envelope("ramp", a=np.nan, b=1.0), X.field_envelope("ramp", a=0.0, b=np.inf)):
        assert refused(fo(env=bad), b"finite") and refused(dk(env=bad), b"finite")
    for bad in (X.field_envelope("harmonic", omega=np.inf, phase=0.0), X.field_envelope("harmonic", omega=1.0, phase=np.nan)):
        assert refused(fo(env=bad), b"finite") and refused(dk(env=bad), b"finite")
    # a parameter the kind does not read is ignored
    assert fo(env=X.field_envelope("ramp", a=0.0, b=1.0, omega=np.nan)) == 0
    assert fo(env=X.field_envelope("constant", a=np.nan, phase=np.inf)) == 0
    assert refused(fo(steps=-1, sums_4=sums.ctypes.data_as(dp)), b"steps is negative")
    assert refused(fo(params=X.FoParams(T.QM, T.DT, 1e-7, 1e-7, 18, 30)), b"scheme")
    assert refused(fo(params=X.FoParams(T.QM, T.DT, 1e-7, 1e-7, X.FO_SCHEMES["CN"], 65)), b"maxit")
    assert refused(fo(params=X.FoParams(T.QM, T.DT, 1e-7, 1e-7, X.FO_SCHEMES["CN"], 0)), b"maxit")
    assert refused(dk(params=X.DkParams(T.QM, T.MP, T.DT, 1e-12, 1e-12, 0)), b"maxit")
    assert refused(dk(params=X.DkParams(T.QM, T.MP, T.DT, 1e-12, 1e-12, X.MODEL_DK_MAXIT + 1)), b"maxit")
    assert refused(fo(reg=X.TraceRegion(5, 0, (C.c_double * 7)(), 0)), b"geometry")
    with pytest.raises(X.XpicError):
        ctx.envelope_factors(X.field_envelope(7), 0.1, 0, 4)
    with pytest.raises(X.XpicError):
        ctx.envelope_factors(ramp, 0.1, -1, 4)
    with pytest.raises(X.XpicError):
        X.field_envelope("ramp", nonsense=1.0)
