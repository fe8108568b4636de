"""The drift-kinetic (guiding-centre) pusher on the device (xpic_amd/csrc/drift_kinetic.hip) against the numpy
restatement of the reference's algorithms in tests/drift_kinetic_ref.py (pinned by tests/test_drift_kinetic_ref.py), on
the grid of tests/test_eccapfim_kernels.py with 1001 particles: four workgroups with a ragged tail."""
import numpy as np
import pytest

import drift_kinetic_ref as R

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps


@pytest.fixture(scope="module")
def X():
    import xpic_amd

    return xpic_amd


@pytest.fixture(scope="module")
def fields():
    return R.case_fields()


def make_ctx(X, E, B, gB):
    g = X.Context("basic", R.N, R.D, 0.7)
    g.set_field(X.E, E)
    g.set_field(X.B, B)
    if gB is not None:
        g.set_field(X.W0, gB)
    return g


@pytest.fixture(scope="module")
def ctx(X, fields):
    return make_ctx(X, *fields)


def test_interpolation_parity(X, ctx, fields):
    E, B, gB = fields
    rn, r0 = R.case_segments()
    L = np.array(R.N) * np.array(R.D)
    outside = ((np.minimum(rn, r0) < 0) | (np.maximum(rn, r0) > L)).any(axis=1)
    assert outside[: R.NPART // 2].mean() > 0.5  # the seam is exercised
    Eo, Bo, Go = R.interpolate(E, B, gB, R.D, rn, r0)
    Eg, Bg, Gg = ctx.drift_kinetic_interpolate(rn, r0, X.W0)
    for name, a, b, F in (("E", Eo, Eg, E), ("B", Bo, Bg, B), ("gradB", Go, Gg, gB)):
        err = np.abs(a - b).max()
        print(name, "max |gpu - restatement| =", err, "of max|field| =", np.abs(F).max())
        assert err <= 1e-13 * np.abs(F).max(), name
    # gradB_field = -1: the reference's gradB_g == nullptr
    E2, B2, G2 = ctx.drift_kinetic_interpolate(rn, r0, None)
    assert np.array_equal(E2, Eg) and np.array_equal(B2, Bg)
    assert not G2.any()
    # the E gather is ImplicitEsirkepov's, bit for bit
    Ei, _ = ctx.implicit_esirkepov_interpolate(rn, r0)
    assert np.array_equal(Ei, Eg)


def _same(name, got, ref, rel=1e-13):
    """agreement to rel of the largest finite reference value of the column group; non-finite values (p_perp over a
    B0 = 0: inf or NaN as the reference's expression gives) must be the same non-finite values"""
    fin = np.isfinite(ref)
    assert np.array_equal(fin, np.isfinite(got)), name
    assert np.array_equal(np.isnan(ref), np.isnan(got)), name
    assert np.array_equal(ref[~fin & ~np.isnan(ref)], got[~fin & ~np.isnan(ref)]), name
    err = np.abs(got[fin] - ref[fin]).max()
    scale = np.abs(ref[fin]).max()
    print(name, "max |gpu - restatement| =", err, "scale", scale)
    assert err <= rel * scale, name


@pytest.fixture(scope="module")
def patched(X, fields):
    """the fields with a patch of B = 0 nodes wide enough to hold whole 4^3 footprints, and 40 particles in it.  A
    particle on the patch's rim sees a small |B|: its drift E x h / |B| and its mu_p ~ 1 / |B| are huge and nothing
    about it is conditioned to 1e-13, so the rim (0 < |B| < 0.5, where the unpatched field has |B| ~ 1) is cleared:
    those particles take the place of others, one box length further in x."""
    E, B, gB = fields
    B = B.copy()
    B[0:5, 0:5, 0:5, :] = 0.0
    p0 = R.case_particles(B)
    rng = np.random.default_rng(5)
    inside = slice(60, 100)
    p0[inside, :3] = (2.0 + (rng.random((40, 3)) * 2 - 1) * 0.25) * np.array(R.D)
    lB = R._len(R.interpolate_B([B], R.D, p0[:, :3])[0])
    rim = (lB > 0) & (lB < 0.5)
    p0[rim, :3] = p0[lB >= 0.5][: rim.sum(), :3] + np.array([R.N[0] * R.D[0], 0.0, 0.0])
    lB = R._len(R.interpolate_B([B], R.D, p0[:, :3])[0])
    assert not lB[inside].any() and not ((lB > 0) & (lB < 0.5)).any() and (lB >= 0.5).sum() > 900
    p0[:, 5] = np.divide(R.MP * p0[:, 4] ** 2, 2 * lB, out=np.full(R.NPART, 0.01), where=lB > 0)  # (in no field: any value)
    return make_ctx(X, E, B, gB), (E, B, gB), p0


@pytest.mark.parametrize("k", [1, 2, 5])
def test_push_parity_with_pinned_iterations(X, patched, k):
    """eps = delta = 0: no residual is < 0, so both sides make exactly k updates and nothing depends on a data-dependent
    exit.  The first 50 particles have p_parallel = 0 (|Vh| < 1e-12 in the first iteration), 40 sit in a patch of
    B = 0 nodes (get_Vd's Bh guard; their p_perp is p_perp0 sqrt(|Bp| / 0) as in the reference)."""
    g, (E, B, gB), p0 = patched
    assert (p0[:50, 3] == 0).all()
    ref, its_ref = R.push(E, B, gB, R.D, p0, R.QM, R.MP, R.DT, eps=0.0, delta=0.0, maxit=k)
    got, its = g.drift_kinetic_push(p0, R.QM, R.MP, R.DT, X.W0, eps=0.0, delta=0.0, maxit=k)
    assert (its_ref == k).all() and (its == k).all()
    assert not np.isfinite(ref[60:100, 4]).any()  # the guard case is in the data
    _same("r", got[:, :3], ref[:, :3])
    _same("p_parallel", got[:, 3], ref[:, 3])
    _same("p_perp", got[:, 4], ref[:, 4])
    assert np.array_equal(got[:, 5], p0[:, 5])


def test_convergence(X, ctx, fields):
    """Default tolerances.  At R.DT every particle converges in the restatement (tests/test_drift_kinetic_ref.py).  The
    device's counts are within one of it (a residual that ends next to eps falls on either side by rounding), and its
    returned states pass the restatement's own residuals: the exit test guarantees < eps on the device, the margin of
    64 ulp of the largest coordinate covers the rounding between the two evaluations."""
    E, B, gB = fields
    p0 = R.case_particles(B, zero_par=0)
    ref, its_ref = R.push(E, B, gB, R.D, p0, R.QM, R.MP, R.DT)
    assert its_ref.max() < 30
    got, its = ctx.drift_kinetic_push(p0, R.QM, R.MP, R.DT, X.W0)
    assert its.min() >= 1 and its.max() < 30
    assert np.abs(its.astype(int) - its_ref).max() <= 1
    R1, R2 = R.residuals(E, B, gB, R.D, p0, got, R.QM, R.MP, R.DT)
    margin = 64 * EPS * np.abs(got[:, :4]).max()
    print("R1 max", R1.max(), "R2 max", R2.max(), "margin", margin)
    assert R1.max() <= 1e-12 + margin and R2.max() <= 1e-12 + margin
    assert np.abs(got - ref).max() <= 1e-11  # two converged iterates of one fixed point, each within ~eps of it
    # a step 50 times longer, three iterations: nothing converges, the call succeeds and returns finite numbers
    got, its = ctx.drift_kinetic_push(p0, R.QM, R.MP, 50 * R.DT, X.W0, maxit=3)
    assert its.min() >= 1 and its.max() == 3 and (its == 3).sum() > R.NPART // 2
    assert np.isfinite(got).all()


def test_trace_equals_repeated_pushes(X, ctx, fields):
    E, B, gB = fields
    p0 = R.case_particles(B, zero_par=0)
    long_run = X.DK_LAUNCH_STEPS + 6  # spans two launches
    states, counts = [], []
    p = p0
    for _ in range(long_run):
        p, its = ctx.drift_kinetic_push(p, R.QM, R.MP, R.DT, X.W0)
        states.append(p)
        counts.append(its.astype(np.int64))
    out, samples, tot, mx = ctx.drift_kinetic_trace(p0, 7, R.QM, R.MP, R.DT, X.W0, sample_every=3)
    assert np.array_equal(out, states[6])
    assert samples.shape == (2, R.NPART, 6)
    assert np.array_equal(samples[0], states[2]) and np.array_equal(samples[1], states[5])
    assert np.array_equal(tot, np.sum(counts[:7], axis=0)) and np.array_equal(mx, np.max(counts[:7], axis=0))
    out, samples, tot, mx = ctx.drift_kinetic_trace(p0, long_run, R.QM, R.MP, R.DT, X.W0, sample_every=X.DK_LAUNCH_STEPS + 1)
    assert np.array_equal(out, states[-1])
    assert samples.shape[0] == 1 and np.array_equal(samples[0], states[X.DK_LAUNCH_STEPS])
    assert np.array_equal(tot, np.sum(counts, axis=0)) and np.array_equal(mx, np.max(counts, axis=0))
    out, samples, _, _ = ctx.drift_kinetic_trace(p0, long_run, R.QM, R.MP, R.DT, X.W0)
    assert samples is None and np.array_equal(out, states[-1])


def test_mirror_physics(X):
    """300 steps in B = (0, 0, 1 + 0.3 cos(2 pi z / Lz)), E = 0, |B| at a position from drift_kinetic_interpolate(r, r).

    p_perp^2 / |B(r)| is constant by construction (update_v_perp), to the roundings of 300 steps: 1e-13.

    H = p_par^2 / 2 + (mu_p / mp) |B(r)|: a step leaves the loop with R2 = |(pn - p0) + (mu_p / mp) (|Bp| - |B0|) / Vh|
    < delta (E = 0, so the drive term is 0), where pn, p0 are the parallel momenta, Vh = (pn + p0) / 2, Bp the field at
    the returned position and B0 at the old one.  Times |Vh|: |(pn^2 - p0^2) / 2 + (mu_p / mp) (|Bp| - |B0|)| =
    |H_n - H_0| < |Vh| delta <= max|p_par| delta per step, so steps * max|p_par| * delta after `steps` of them.  That
    needs every step converged (iterations_max < maxit) and |Vh| >= 1e-12 (no particle turns: asserted).  Rounding: R2 is
    evaluated to a few ulp of p_par, which the product with Vh turns into 16 ulp of max p_par^2 per step at most, and the
    two evaluations of H here add 16 ulp of max H."""
    E, B, gB = R.mirror_fields(R.N, R.D)
    g = make_ctx(X, E, B, gB)
    rng = np.random.default_rng(21)
    n, steps, every, delta = R.NPART, 300, 50, 1e-12
    L = np.array(R.N) * np.array(R.D)
    p0 = np.column_stack([rng.random((n, 3)) * L, 0.8 + 0.7 * rng.random(n), 0.1 + 0.3 * rng.random(n), np.zeros(n)])

    def absB(r):
        return R._len(g.drift_kinetic_interpolate(r, r, X.W0)[1])

    b0 = absB(p0[:, :3])
    p0[:, 5] = R.MP * p0[:, 4] ** 2 / (2 * b0)
    out, samples, tot, mx = g.drift_kinetic_trace(p0, steps, R.QM, R.MP, R.DT, X.W0, sample_every=every, delta=delta)
    assert mx.max() < 30 and tot.min() >= steps
    assert np.array_equal(samples[-1], out)
    inv0, H0 = p0[:, 4] ** 2 / b0, 0.5 * p0[:, 3] ** 2 + p0[:, 5] / R.MP * b0
    pmax = max(np.abs(p0[:, 3]).max(), np.abs(samples[..., 3]).max())
    assert np.abs(samples[..., 3]).min() > 0.1  # nobody turns
    assert np.abs(out[:, 2] - p0[:, 2]).min() > 4 * L[2]  # through several periods of the mirror, unfolded
    for k in range(samples.shape[0]):
        s, done = samples[k], (k + 1) * every
        b = absB(s[:, :3])
        inv = s[:, 4] ** 2 / b
        H = 0.5 * s[:, 3] ** 2 + s[:, 5] / R.MP * b
        bound = done * pmax * delta + done * 16 * EPS * pmax * pmax + 16 * EPS * np.abs(H0).max()
        print("step", done, "mu drift", np.abs(inv / inv0 - 1).max(), "H drift", np.abs(H - H0).max(), "bound", bound)
        assert np.abs(inv / inv0 - 1).max() <= 1e-13
        assert np.abs(H - H0).max() <= bound


def test_edges(X, ctx, fields):
    import ctypes as C

    E, B, gB = fields
    p0 = R.case_particles(B, zero_par=0)
    # n = 0: success, nothing touched
    pn, its = ctx.drift_kinetic_push(np.zeros((0, 6)), R.QM, R.MP, R.DT, X.W0)
    assert pn.shape == (0, 6) and its.shape == (0,)
    a = ctx.drift_kinetic_interpolate(np.zeros((0, 3)), np.zeros((0, 3)), X.W0)
    assert all(v.shape == (0, 3) for v in a)
    out, samples, tot, mx = ctx.drift_kinetic_trace(np.zeros((0, 6)), 5, R.QM, R.MP, R.DT, X.W0, sample_every=2)
    assert out.shape == (0, 6) and samples.shape == (2, 0, 6)
    # n = 1 is the first particle of the batch
    all_, its_all = ctx.drift_kinetic_push(p0, R.QM, R.MP, R.DT, X.W0)
    one, its_one = ctx.drift_kinetic_push(p0[:1], R.QM, R.MP, R.DT, X.W0)
    assert np.array_equal(one[0], all_[0]) and its_one[0] == its_all[0]
    # steps = 0 returns the state
    out, _, tot, mx = ctx.drift_kinetic_trace(p0, 0, R.QM, R.MP, R.DT, X.W0)
    assert np.array_equal(out, p0) and not tot.any() and not mx.any()
    # bad arguments name themselves
    for kw, word in ((dict(maxit=0), "maxit"), (dict(mp=0.0), "mp")):
        args = dict(qm=R.QM, mp=R.MP, dt=R.DT, gradB_field=X.W0)
        args.update(kw)
        with pytest.raises(X.XpicError, match=word):
            ctx.drift_kinetic_push(p0, **args)
        with pytest.raises(X.XpicError, match=word):
            ctx.drift_kinetic_trace(p0, 2, **args)
    with pytest.raises(X.XpicError, match="steps"):
        ctx.drift_kinetic_trace(p0, -1, R.QM, R.MP, R.DT, X.W0)
    with pytest.raises(X.XpicError, match="gradB_field"):
        ctx.drift_kinetic_push(p0, R.QM, R.MP, R.DT, 99)
    L_, dp, n1 = ctx.L, C.POINTER(C.c_double), C.c_int64(1)
    buf = np.zeros(6)
    ptr = buf.ctypes.data_as(dp)
    it1, tot1 = (C.c_int * 1)(), (C.c_int64 * 1)()
    P = X.DkParams(R.QM, R.MP, R.DT, 1e-12, 1e-12, 30)
    calls = [
        (lambda: L_.xpic_drift_kinetic_interpolate(ctx.h, n1, None, ptr, -1, ptr, ptr, ptr), "rn3"),
        (lambda: L_.xpic_drift_kinetic_interpolate(ctx.h, n1, ptr, ptr, -1, ptr, ptr, None), "gradBp3"),
        (lambda: L_.xpic_drift_kinetic_push(ctx.h, n1, None, -1, ptr, ptr, it1), "params"),
        (lambda: L_.xpic_drift_kinetic_push(ctx.h, n1, C.byref(P), -1, None, ptr, it1), "p0_6"),
        (lambda: L_.xpic_drift_kinetic_push(ctx.h, n1, C.byref(P), -1, ptr, ptr, None), "iterations"),
        (lambda: L_.xpic_drift_kinetic_trace(ctx.h, n1, C.byref(P), -1, C.c_int64(1), C.c_int64(0), None, None, tot1, it1), "state_6"),
        (lambda: L_.xpic_drift_kinetic_trace(ctx.h, n1, C.byref(P), -1, C.c_int64(1), C.c_int64(0), ptr, ptr, tot1, it1), "sample_every"),
        (lambda: L_.xpic_drift_kinetic_trace(ctx.h, n1, C.byref(P), -1, C.c_int64(1), C.c_int64(0), ptr, None, None, it1), "iterations_total"),
        # a sample buffer whose size overflows 64 bits is refused before anything is allocated or launched
        (lambda: L_.xpic_drift_kinetic_trace(ctx.h, n1, C.byref(P), -1, C.c_int64(1 << 62), C.c_int64(1), ptr, ptr, tot1, it1), "sample buffer"),
    ]
    for call, word in calls:
        assert call() != 0
        assert word in L_.xpic_last_error().decode(), word
    assert L_.xpic_drift_kinetic_push(None, n1, C.byref(P), -1, ptr, ptr, it1) != 0
    # a two-slab context is refused with a message
    two = X.Context("basic", (8, 8, 12), (0.5, 0.5, 0.5), 0.7, rank=0, nranks=2)
    with pytest.raises(X.XpicError, match="z-slab"):
        two.drift_kinetic_push(p0[:4], R.QM, R.MP, R.DT)
    with pytest.raises(X.XpicError, match="z-slab"):
        two.drift_kinetic_interpolate(p0[:4, :3], p0[:4, :3])
