"""The collisional model traces on the device (xpic_model_full_orbit_trace_collisional,
xpic_model_drift_kinetic_trace_collisional; xpic_amd/csrc/collide_trace.hip) against the numpy restatement
tests/collisional_trace_ref.py (pinned without a GPU by tests/test_collisional_trace_ref.py), the guarantees (a) .. (c) of
include/xpic_hip.h bit for bit, the edges, the two statistical limits of the CPU test at the same ensemble size, and the
purpose of it all: a trapped ensemble that the collisionless traces keep for ever leaves an open mirror.

The iterative pushers run with pinned iteration counts where the device is held to the restatement step by step, as in
tests/test_gpu_model_trace.py, whose open mirror set-up (models, region, spacings) is used as it is."""
import ctypes as C

import numpy as np
import pytest

import analytic_trace_ref as A
import collisional_trace_ref as R
import test_collisional_trace_ref as T
import test_gpu_model_trace as MT

pytestmark = pytest.mark.gpu

QM, MP, DT = MT.QM, MT.MP, MT.DT
KINDS = ["EB2B", "CN", "dk"]
PIN = MT.PIN
TOL_COLLISION = 1e-12  # of the largest |v|: tests/test_gpu_collisions.py's bound for one collision
TOL_PUSH = MT.TOL_TRACE  # what tests/test_gpu_model_trace.py allows the push itself on a model without exp (CN and the
#                          drift-kinetic pusher contract their expressions; with E = 0 and B = 0 a Chin step is exact)

BACKGROUNDS = [dict(q=1.0, m=4.0, n=1.0, vth=0.5, drift=(0.1, 0.0, -0.2)), dict(q=-2.0, m=0.25, n=0.5, vth=2.0),
               dict(q=1.0, m=1836.0, n=3.0, vth=0.01)]


@pytest.fixture(scope="module")
def X():
    import xpic_amd

    return xpic_amd


@pytest.fixture(scope="module")
def ctx(X):
    return X.Context("basic", (8, 8, 8), MT.D, 0.7)


def device(X, coll):
    return None if coll is None else X.trace_collisions(**coll)


def call(X, ctx, kind, p, steps, model, coll, reg=None, dt=DT, pin=True, **kw):
    kw = dict(PIN.get(kind, {}) if pin else {}, **kw)
    if kind == "dk":
        return ctx.model_drift_kinetic_trace_collisional(p, steps, QM, MP, dt, model, device(X, coll), reg, **kw)
    return ctx.model_full_orbit_trace_collisional(p, steps, kind, QM, dt, model, device(X, coll), reg, **kw)


def uniform(kind):
    """E = 0; B = 0 for a full orbit (the push leaves v alone), along (1, 2, 2) / 3 for a guiding centre"""
    return dict(B0=(1.0 / 3, 2.0 / 3, 2.0 / 3)) if kind == "dk" else {}


def ensemble(kind, n, seed=3):
    rng = np.random.default_rng(seed)
    r = 2.0 + rng.random((n, 3))
    if kind != "dk":
        return np.column_stack([r, rng.normal(size=(n, 3))])
    perp = np.abs(rng.normal(size=n)) + 0.1
    return np.column_stack([r, rng.normal(size=n), perp, MP * perp * perp / 2.0])  # |B| = 1


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nbg", [1, 3])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_parity_per_step(X, ctx, n, nbg, kind):
    """steps = 1 calls with step0 = k against the restatement applied to the device's own state before that step"""
    model, field = X.field_model("uniform", **uniform(kind)), A.model("uniform", **uniform(kind))
    coll = R.collisions(BACKGROUNDS[:nbg], strength=0.02, mass=2.0, every=1, seed=1234 + n, particle0=1000)
    p = ensemble(kind, n)
    worst = 0.0
    for k in range(8):
        got = call(X, ctx, kind, p, 1, model, coll, step0=k)
        ref, its, t = R.step(kind, field, p, QM, MP, DT, coll, k + 1, 1000 + np.arange(n), **PIN.get(kind, {}))
        vmax = np.sqrt((ref[:, 3:] ** 2).sum(axis=1)).max() if kind != "dk" else np.hypot(ref[:, 3], ref[:, 4]).max()
        scale = max(vmax, vmax * vmax)  # (mu_p is a square of a speed)
        err = np.abs(got.state[:, 3:] - ref[:, 3:]).max() / scale
        worst = max(worst, err)
        assert err <= TOL_COLLISION + (TOL_PUSH if kind != "EB2B" else 0.0), (k, err)
        assert np.abs(got.state[:, :3] - ref[:, :3]).max() <= TOL_PUSH * np.abs(ref[:, :3]).max()
        assert np.array_equal(got.coll[[0, 1, 3]], t[[0, 1, 3]]) and got.coll[0] == n * nbg
        assert abs(got.coll[2] - t[2]) <= 1e-12 * t[2]
        assert np.array_equal(got.iterations_max, its)
        p = got.state
    print(kind, n, nbg, "largest deviation of a step / largest |v|:", worst)


# ---- the guarantees, on the quadratic mirror of tests/test_gpu_model_trace.py with its open region
NAME = "quadratic_mirror"
COLL = R.collisions(BACKGROUNDS, strength=0.01, mass=1.0, every=2, seed=99, particle0=5)
FIELDS = MT.FIELDS + ("coll",)


def mirror(X, kind, n=257):
    return X.field_model(NAME, **MT.MODELS[NAME]), MT.particles(NAME, kind, n), MT.region(NAME)


@pytest.mark.parametrize("kind", KINDS)
def test_no_collisions_is_the_model_trace(X, ctx, kind):
    """(a): collisions == NULL, nbg == 0 and strength == 0, 130 steps sampled every 7"""
    model, p, reg = mirror(X, kind)
    kw = dict(PIN.get(kind, {}), sample_every=7)
    if kind == "dk":
        ref = ctx.model_drift_kinetic_trace(p, 130, QM, MP, DT, model, reg, **kw)
    else:
        ref = ctx.model_full_orbit_trace(p, 130, kind, QM, DT, model, reg, **kw)
    assert ref.removed > 0 and (ref.exit_step < 0).any()
    for coll in (None, R.collisions([], strength=0.01, mass=1.0), dict(COLL, strength=0.0)):
        got = call(X, ctx, kind, p, 130, model, coll, reg, sample_every=7)
        MT.same(got, ref, kind)
        assert not got.coll.any()


@pytest.mark.parametrize("kind", KINDS)
def test_composition_split_and_determinism(X, ctx, kind):
    """(b) with (s1, s2) = (64, 1), (1, 64), (65, 65); (c) with 257 = 100 + 157; two runs give equal bytes"""
    model, p, reg = mirror(X, kind)
    whole = {}
    for s1, s2 in ((64, 1), (1, 64), (65, 65)):
        steps = s1 + s2
        if steps not in whole:
            whole[steps] = call(X, ctx, kind, p, steps, model, COLL, reg, sample_every=1)
        full = whole[steps]
        assert full.coll[0] > 0
        a = call(X, ctx, kind, p, s1, model, COLL, reg, sample_every=1)
        b = call(X, ctx, kind, a.state, s2, model, COLL, reg, sample_every=1, exit_step=a.exit_step, step0=s1)
        assert full.state.tobytes() == b.state.tobytes() and np.array_equal(full.exit_step, b.exit_step)
        assert full.samples.tobytes() == np.concatenate([a.samples, b.samples]).tobytes()
        assert np.array_equal(full.alive, np.concatenate([a.alive, b.alive]))
        assert full.removed == a.removed + b.removed
        assert np.array_equal(full.iterations_sum, a.iterations_sum + b.iterations_sum)
        assert np.array_equal(full.coll[[0, 1, 3]], a.coll[[0, 1, 3]] + b.coll[[0, 1, 3]])
        assert abs(full.coll[2] - a.coll[2] - b.coll[2]) <= 1e-12 * full.coll[2]
    full = whole[130]
    assert full.removed > 0
    MT.same(call(X, ctx, kind, p, 130, model, COLL, reg, sample_every=1), full, kind, FIELDS)
    lo = call(X, ctx, kind, p[:100], 130, model, COLL, reg, sample_every=1)
    hi = call(X, ctx, kind, p[100:], 130, model, dict(COLL, particle0=COLL["particle0"] + 100), reg, sample_every=1)
    for f in ("state", "exit_step", "iterations_sum", "iterations_max"):
        assert np.concatenate([getattr(lo, f), getattr(hi, f)]).tobytes() == getattr(full, f).tobytes(), f
    assert np.concatenate([lo.samples, hi.samples], axis=1).tobytes() == full.samples.tobytes()
    assert np.array_equal(lo.alive + hi.alive, full.alive) and lo.removed + hi.removed == full.removed
    assert np.array_equal((lo.coll + hi.coll)[[0, 1, 3]], full.coll[[0, 1, 3]])
    # particle0 matters: the same particles under other global indices draw other partners
    assert call(X, ctx, kind, p[:100], 130, model, dict(COLL, particle0=0), reg).state.tobytes() != lo.state.tobytes()


def test_edges(X, ctx):
    for kind in KINDS:
        model, p, reg = mirror(X, kind, 5)
        out = call(X, ctx, kind, p[:0], 3, model, COLL, reg, sample_every=1)
        assert out.state.shape == (0, 6) and out.removed == 0 and not out.coll.any()
        out = call(X, ctx, kind, p, 0, model, COLL, reg)
        assert out.state.tobytes() == p.tobytes() and not out.coll.any() and not out.iterations_sum.any()
    # v == w: one cold background whose drift is everybody's velocity; E = B = 0, so it stays that
    v = (0.3, -0.4, 1.2)
    p = np.column_stack([2.0 + np.random.default_rng(1).random((70, 3)), np.tile(v, (70, 1))])
    cold = R.collisions([dict(q=1.0, m=1.0, n=1.0, vth=0.0, drift=v)], strength=0.1, mass=1.0)
    out = call(X, ctx, "EB2B", p, 5, X.field_model("uniform"), cold)
    assert np.array_equal(out.coll, [0.0, 350.0, 0.0, 0.0]) and out.state[:, 3:].tobytes() == p[:, 3:].tobytes()
    # a guiding centre where the model has |B| == 0: every collision of the step is counted as skipped
    g = ensemble("dk", 3)
    out = call(X, ctx, "dk", g, 1, X.field_model("uniform"), R.collisions(BACKGROUNDS, strength=0.1, mass=1.0), pin=False,
               maxit=2)
    assert np.array_equal(out.coll, [0.0, 9.0, 0.0, 0.0])


def test_refusals(X, ctx):
    """each refusal of the definition returns nonzero and leaves the state's bytes alone"""
    model = X.field_model("uniform", B0=(0.0, 0.0, 1.0))
    dp, i64 = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    F, K = X.FoParams(QM, DT, 1e-7, 1e-7, X.FO_SCHEMES["EB2B"], 30), X.DkParams(QM, MP, DT, 1e-12, 1e-12, 30)
    none = X.TraceRegion(X.GEOM_NONE, 0, (C.c_double * 7)(), 0)
    tot, mx = np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.int32)
    good = dict(backgrounds=BACKGROUNDS[:2], strength=0.1, mass=1.0, every=1, seed=0, particle0=0)

    def run(coll, kind):
        p = ensemble(kind, 3)
        s, out = p.copy(), np.full(4, 7.0)
        fn = ctx.L.xpic_model_drift_kinetic_trace_collisional if kind == "dk" else ctx.L.xpic_model_full_orbit_trace_collisional
        rc = fn(ctx.h, C.c_int64(3), C.byref(K if kind == "dk" else F), C.byref(model), C.c_int64(2), C.c_int64(0),
                s.ctypes.data_as(dp), None, tot.ctypes.data_as(i64), mx.ctypes.data_as(C.POINTER(C.c_int)), C.byref(none),
                None, None, None, C.byref(coll), out.ctypes.data_as(dp))
        return rc, s.tobytes() == p.tobytes()

    def bad(**change):
        c = X.trace_collisions(**good)
        for k, v in change.items():
            if k.startswith("bg_"):
                setattr(c.bg[1], k[3:], v)
            else:
                setattr(c, k, v)
        return c
    for kind in ("EB2B", "dk"):
        rc, same = run(bad(), kind)
        assert rc == 0 and not same
        for change in (dict(nbg=-1), dict(nbg=X.TRACE_BG_MAX + 1), dict(every=0), dict(every=-3), dict(particle0=-1),
                       dict(strength=-1e-300), dict(strength=float("nan")), dict(mass=0.0), dict(mass=-1.0), dict(bg_m=0.0),
                       dict(bg_m=-2.0), dict(bg_n=-1.0), dict(bg_vth=-0.5)):
            rc, same = run(bad(**change), kind)
            assert rc != 0 and same, (kind, change)
        # a background beyond nbg is not read
        c = bad()
        c.bg[3].m = -1.0
        assert run(c, kind)[0] == 0
    # coll_4 may be NULL
    s = ensemble("EB2B", 3)
    assert ctx.L.xpic_model_full_orbit_trace_collisional(
        ctx.h, C.c_int64(3), C.byref(F), C.byref(model), C.c_int64(2), C.c_int64(0), s.ctypes.data_as(dp), None, None, None,
        C.byref(none), None, None, None, C.byref(bad()), None) == 0


# ---- the two statistical limits of tests/test_collisional_trace_ref.py on the device, same ensembles, seeds and limits
def test_lorentz_limit(X, ctx):
    coll = T.lorentz_collisions(T.LORENTZ_V0)
    p = np.column_stack([np.full((T.N, 3), 2.0), np.tile(T.LORENTZ_V0, (T.N, 1))])
    out = call(X, ctx, "EB2B", p, 1, X.field_model("uniform"), coll, dt=T.DT)
    v = out.state[:, 3:]
    assert out.coll[0] == T.N and abs(out.coll[2] / T.N - 0.01) <= 1e-14
    speed = np.sqrt((v * v).sum(axis=1)) / np.sqrt(np.dot(T.LORENTZ_V0, T.LORENTZ_V0))
    mean = T.tan2_half(T.LORENTZ_V0, v).mean()
    print("largest | |v'| / |v| - 1 | =", np.abs(speed - 1.0).max(), "mean tan^2(Theta / 2) / sigma^2 =", mean / 0.01)
    assert np.abs(speed - 1.0).max() <= 4e-16
    assert abs(mean / 0.01 - 1.0) <= 5 * np.sqrt(2.0 / T.N)


def test_stationarity_and_relaxation(X, ctx):
    coll = T.stationary_collisions()
    model = X.field_model("uniform")
    limit = 5 * np.sqrt(2.0 / T.N)

    def variances(temperature, seed):
        p = np.column_stack([np.full((T.N, 3), 2.0), T.maxwellian(temperature, seed)])
        out = call(X, ctx, "EB2B", p, T.STATIONARY_STEPS, model, coll, dt=T.DT, sample_every=T.STATIONARY_SAMPLE)
        return out.samples[:, :, 3:].var(axis=1) / (T.T_B / T.M_A), out.coll
    var, t = variances(T.T_B, 21)
    print("component variances / (T_b / m_a) every 100 steps:", var, "mean sigma^2", t[2] / t[0], "share > 1", t[3] / t[0])
    assert t[0] == T.N * T.STATIONARY_STEPS and 1e-2 <= t[2] / t[0] <= 9e-2
    assert t[3] / t[0] < 0.01
    assert np.abs(var - 1.0).max() <= limit
    hot, _ = variances(4 * T.T_B, 22)
    print("started at 4 T_b:", hot)
    assert (np.diff(hot, axis=0) < 0).all() and (hot[0] < 4.0).all() and (hot[-1] > 1.0).all()
    # guiding centres in B along (1, 2, 2) / 3: p_parallel is a component, p_perp^2 / 2 is the mean of two components'
    # squares, an exponential variate whose mean has the relative standard error 1 / sqrt(N) = sqrt(2 / (2 N))
    v = T.maxwellian(T.T_B, 23)
    g = np.column_stack([np.full((T.N, 3), 2.0), v[:, 0], np.hypot(v[:, 1], v[:, 2]), MP * (v[:, 1] ** 2 + v[:, 2] ** 2) / 2])
    out = call(X, ctx, "dk", g, T.STATIONARY_STEPS, X.field_model("uniform", **uniform("dk")), coll, dt=T.DT, pin=False,
               sample_every=T.STATIONARY_SAMPLE)
    par, perp = out.samples[:, :, 3].var(axis=1), (out.samples[:, :, 4] ** 2).mean(axis=1) / 2
    print("guiding centres: var p_parallel", par, "<p_perp^2> / 2", perp)
    assert np.abs(par - 1.0).max() <= limit and np.abs(perp - 1.0).max() <= 5 / np.sqrt(T.N)
    assert np.abs(out.samples[-1, :, 5] - MP * out.samples[-1, :, 4] ** 2 / 2).max() <= 1e-14 * out.samples[-1, :, 5].max()


# ---- the loss cone is refilled.  The Gaussian mirror of tests/test_gpu_model_trace.py with its open region (z within 3
# of the midplane, where B = 1.055 B_min: the trapped have |v_z| / v < 0.228 at the midplane).  CONE_N particles of speed
# 0.1 start on the midplane within 0.05 of the axis with |v_z| / v <= 0.1, every gyrophase.  The background is cold and
# heavy (m_b = 1836), so the collisions change the pitch angle and next to nothing else; sigma^2 = CONE_SIGMA2 per step
# turns the velocity by <Theta^2> = 4 sigma^2 CONE_STEPS of about 1 rad^2 over the run.
CONE_N, CONE_STEPS, CONE_DT, CONE_EVERY, CONE_SIGMA2 = 256, 600, 0.5, 50, 4e-4
# What tests/collisional_trace_ref.py removes of the ensemble, measured on the CPU (`python
# tests/test_gpu_collisional_trace.py` prints the figures): 186 of 256 for both pushers -- a cold heavy scatterer changes
# v_z by an amount that does not depend on the gyrophase, so the full orbits and the guiding centres, which draw the same
# numbers, leave alike -- with alive = 256 256 246 214 173 139 121 106 98 86 75 70 every 50 steps; and how many particles
# change sides in the restatement when its initial velocities are perturbed by 1e-12 relative: none.
CONE_REF_REMOVED = {"EB2B": 186, "dk": 186}
CONE_REF_FLIPS = {"EB2B": 0, "dk": 0}


def cone_setup(kind):
    rng = np.random.default_rng(17)
    n = CONE_N
    r = np.array(MT.CENTRE["gaussian_mirror"]) + np.column_stack([0.1 * (rng.random((n, 2)) - 0.5), np.zeros(n)])
    mu, ang = 0.2 * rng.random(n) - 0.1, 2 * np.pi * rng.random(n)
    vz, vperp = 0.1 * mu, 0.1 * np.sqrt(1.0 - mu * mu)
    if kind == "dk":
        lB = np.sqrt((A.model("gaussian_mirror", **A.GAUSSIAN)(r)[1] ** 2).sum(axis=1))
        p = np.column_stack([r, vz, vperp, MP * vperp * vperp / (2.0 * lB)])
    else:
        p = np.column_stack([r, vperp * np.cos(ang), vperp * np.sin(ang), vz])
    coll = R.collisions([dict(q=1.0, m=1836.0, n=1.0, vth=1e-4)], strength=CONE_SIGMA2 * 0.1 ** 3 / CONE_DT, mass=1.0, seed=31)
    return p, coll


def cone_restatement(kind, perturb=0.0):
    p, coll = cone_setup(kind)
    if perturb:
        p[:, 3:5 if kind == "dk" else 6] *= 1.0 + perturb * np.random.default_rng(2).uniform(-1, 1, size=(CONE_N, 1))
    return R.trace(kind, A.model("gaussian_mirror", **A.GAUSSIAN), p, CONE_STEPS, MT.region("gaussian_mirror"), MT.D, QM, MP,
                   CONE_DT, coll, sample_every=CONE_EVERY)


@pytest.mark.parametrize("kind", ["EB2B", "dk"])
def test_the_loss_cone_is_refilled(X, ctx, kind):
    p, coll = cone_setup(kind)
    model, reg = X.field_model("gaussian_mirror", **A.GAUSSIAN), MT.region("gaussian_mirror")
    # without collisions the ensemble is trapped: the model trace removes nobody
    if kind == "dk":
        quiet = ctx.model_drift_kinetic_trace(p, CONE_STEPS, QM, MP, CONE_DT, model, reg, sample_every=CONE_EVERY)
    else:
        quiet = ctx.model_full_orbit_trace(p, CONE_STEPS, kind, QM, CONE_DT, model, reg, sample_every=CONE_EVERY)
    assert quiet.removed == 0 and (quiet.exit_step == -1).all() and (quiet.alive == CONE_N).all()
    got = call(X, ctx, kind, p, CONE_STEPS, model, coll, reg, dt=CONE_DT, pin=False, sample_every=CONE_EVERY)
    print(kind, "removed", got.removed, "of", CONE_N, "alive", got.alive, "restatement", CONE_REF_REMOVED[kind])
    assert got.removed > 0
    assert cone_restatement(kind).removed == CONE_REF_REMOVED[kind]  # (about a second on the host)
    assert 0.05 * CONE_N <= CONE_REF_REMOVED[kind] <= 0.95 * CONE_N
    assert (np.diff(got.alive) <= 0).all() and got.alive[-1] == CONE_N - got.removed
    assert got.removed == (got.exit_step >= 0).sum()
    ex = np.where(got.exit_step < 0, CONE_STEPS + 1, got.exit_step)
    at = CONE_EVERY * (1 + np.arange(CONE_STEPS // CONE_EVERY))
    assert np.array_equal(got.alive, [(ex >= s).sum() for s in at])  # (alive at a sample: the step was completed)
    assert abs(got.removed - CONE_REF_REMOVED[kind]) <= 2 * CONE_REF_FLIPS[kind] + 1


if __name__ == "__main__":  # the restatement's figures for CONE_REF_REMOVED and CONE_REF_FLIPS
    for kind_ in ("EB2B", "dk"):
        base, pert = cone_restatement(kind_), cone_restatement(kind_, 1e-12)
        print(kind_, "removed", base.removed, "alive", base.alive, "mean sigma^2", base.coll[2] / base.coll[0], "flips",
              int(((base.exit_step >= 0) != (pert.exit_step >= 0)).sum()))
