"""The restatement of the tracer-set moments (tests/tracer_moments_ref.py) held to what is known without a device: on a
cell-sorted batch it is DistributionMoment's restatement (tests/moments_ref.py); the gyro-averaged tensor has the trace and
is the phase average of the full-orbit tensor; and the bugs the device suite is there to catch show in it when planted."""
import numpy as np
import pytest

import moments_ref as M
import tracer_moments_ref as T

N, D = (6, 5, 4), (0.5, 0.4, 0.25)
REGIONS = (None, (1, 1, 0, 4, 3, 3), (0, 1, 1, 6, 3, 2))  # the box, a partial region, one spanning x in full


def batch(count=400, seed=0):
    rng = np.random.default_rng(seed)
    pts = np.empty((count, 6))
    pts[:, :3] = rng.random((count, 3)) * (np.array(N) * np.array(D))
    pts[:, 3:] = rng.normal(0.0, 0.3, (count, 3))
    return pts


def unit(rng, count):
    b = rng.normal(size=(count, 3))
    return b / np.sqrt((b * b).sum(axis=1))[:, None]


@pytest.mark.parametrize("region", REGIONS)
@pytest.mark.parametrize("name", M.MOMENTS)
def test_cell_sorted_batch_is_distribution_moment(name, region):
    pts = batch()
    c = np.floor(pts[:, :3] / np.array(D)).astype(np.int64)
    cells = (c[:, 2] * N[1] + c[:, 1]) * N[0] + c[:, 0]
    order = np.argsort(cells, kind="stable")
    pts, cells = pts[order], cells[order]
    want = M.moment(name, pts, cells, -1.5, 2.0, 0.25, N, D, region)
    got = T.moment(name, pts, np.full(len(pts), -1), -1.5, 2.0, 0.25, N, D, region)
    start, end, _ = T.region_of(N, region)
    g = np.stack([cells % N[0], (cells // N[0]) % N[1], cells // (N[0] * N[1])], axis=1)
    assert got.counted == int(np.all((g >= start) & (g < end), axis=1).sum()) > 0
    assert np.abs(got.out - want).max() <= 1e-13 * np.abs(want).max()  # (the two sum in different orders)
    assert np.all(np.abs(got.out) <= got.absum * (1 + 1e-15)) and np.all((got.contributions > 0) == (got.absum > 0))


def test_positions_outside_the_box_do_not_count():
    pts = batch(50)
    L = np.array(N) * np.array(D)
    out = np.vstack([pts[:10] + [L[0], 0, 0, 0, 0, 0], pts[10:20] - [0, 0.5 * L[1], 0, 0, 0, 0], pts[20:30] + [0, 0, 3 * L[2], 0, 0, 0]])
    out = out[np.any((out[:, :3] < 0) | (out[:, :3] >= L), axis=1)]
    nan = pts[:2].copy()
    nan[:, 1] = np.nan
    both = np.vstack([pts, out, nan])
    a = T.moment("current", pts, np.full(len(pts), -1), 1.0, 1.0, 1.0, N, D)
    b = T.moment("current", both, np.full(len(both), -1), 1.0, 1.0, 1.0, N, D)
    assert a.counted == b.counted == 50 and np.array_equal(a.out, b.out)


def test_gyro_averaged_tensor_trace_and_phase_average():
    rng = np.random.default_rng(3)
    k, m = 40, 1.7
    b = unit(rng, k)
    ppar, pperp = rng.normal(0.0, 0.4, k), np.abs(rng.normal(0.0, 0.4, k))
    t6 = T.tensor_values("momentum_flux", m, ppar, pperp, b)
    t3 = T.tensor_values("momentum_flux_diag", m, ppar, pperp, b)
    assert np.array_equal(t3, t6[:, [0, 3, 5]])
    assert np.allclose(t3.sum(axis=1), m * (ppar ** 2 + pperp ** 2), rtol=1e-14, atol=0)
    # the same particle as a full orbit: v = p_par b + p_perp (cos e1 + sin e2), averaged over 64 phases
    e1 = np.cross(b, np.roll(b, 1, axis=1))
    e1 /= np.sqrt((e1 * e1).sum(axis=1))[:, None]
    e2 = np.cross(b, e1)
    avg = np.zeros((k, 6))
    for ph in 2 * np.pi * np.arange(64) / 64:
        v = ppar[:, None] * b + pperp[:, None] * (np.cos(ph) * e1 + np.sin(ph) * e2)
        avg += M.moment_values("momentum_flux", np.hstack([np.zeros((k, 3)), v]), 0.0, m, N, D) / 64
    assert np.abs(avg - t6).max() <= 64 * np.finfo(float).eps * np.abs(t6).max()
    # a vanishing field: b = 0 leaves the isotropic perpendicular part
    z = T.tensor_values("momentum_flux", m, ppar, pperp, np.zeros((k, 3)))
    assert np.array_equal(z[:, [1, 2, 4]], np.zeros((k, 3))) and np.array_equal(z[:, 0], m * (0.5 * (pperp * pperp)))


def test_cylindrical_tensor_rotates_b():
    rng = np.random.default_rng(4)
    k = 30
    pts = batch(k, 5)
    pts[0, :2] = 0.5 * np.array(N[:2]) * np.array(D[:2])  # on the axis: the Cartesian components
    b = unit(rng, k)
    cyl = T.dk_values("momentum_flux_cyl", pts, 1.0, 1.3, N, D, b)
    car = T.dk_values("momentum_flux", pts, 1.0, 1.3, N, D, b)
    assert np.array_equal(cyl[0], car[0])
    assert np.allclose(cyl[:, [0, 3, 5]].sum(axis=1), car[:, [0, 3, 5]].sum(axis=1), rtol=1e-13)  # the trace is invariant
    assert np.allclose(cyl[:, 5], car[:, 5], rtol=0, atol=0) and not np.allclose(cyl[1:, 0], car[1:, 0])
    assert np.array_equal(T.dk_values("momentum_flux_diag_cyl", pts, 1.0, 1.3, N, D, b), cyl[:, [0, 3, 5]])


def test_direction_of_a_uniform_and_of_a_null_field():
    r = batch(20)[:, :3]
    B = np.zeros((N[2], N[1], N[0], 3)) + np.array([0.0, 3.0, 4.0])
    assert np.allclose(T.direction(B, D, r), [0.0, 0.6, 0.8], rtol=0, atol=4e-16)
    assert np.array_equal(T.direction(np.zeros_like(B), D, r), np.zeros((20, 3)))


def test_map_is_the_sum_over_due_steps():
    pts = batch(60)
    deps = []
    for s in range(4):
        moved = pts.copy()
        moved[:, :3] *= 1.0 - 0.01 * s  # (towards the origin: nobody leaves the box)
        deps.append(T.moment("density", moved, np.where(np.arange(60) < 5 * s, s, -1), 1.0, 1.0, 0.5, N, D))
    tot, made = T.map_sum(deps)
    assert made == 4 and tot.counted == sum(x.counted for x in deps) == 60 + 55 + 50 + 45
    assert np.isclose(tot.out.sum(), 0.5 * tot.counted)


@pytest.mark.parametrize("bug", T.BUGS)
def test_planted_bugs_show(bug):
    """each on the smallest case that isolates it"""
    L = np.array(N) * np.array(D)
    v = [0.3, -0.2, 0.1]
    if bug == "round_cell":  # the upper half of cell 1 along x rounds into cell 2, outside a region that ends at 2
        pts, ex, kw = np.array([[1.75 * D[0], 1.2, 0.4] + v]), [-1], dict(region=(0, 0, 0, 2, 5, 4))
    elif bug == "count_dead":
        pts, ex, kw = np.array([[1.3, 1.2, 0.4] + v, [1.4, 1.1, 0.3] + v]), [-1, 7], {}
    elif bug == "wrap_partial":  # next to x = 0 in a region that does not span x: the lower deposit is dropped, not wrapped
        pts, ex, kw = np.array([[0.1 * D[0], 1.2, 0.4] + v]), [-1], dict(region=(0, 0, 0, 5, 5, 4))
    else:
        pts, ex, kw = np.array([[1.3, 1.2, 0.4, 0.3, 0.5, 0.0]]), [-1], dict(kind="drift_kinetic", B=np.zeros((N[2], N[1], N[0], 3)) + [0.0, 0.0, 1.0])
    name = "momentum_flux" if bug == "no_delta" else "density"
    good = T.moment(name, pts, np.array(ex), 1.0, 1.0, 1.0, N, D, **kw)
    bad = T.moment(name, pts, np.array(ex), 1.0, 1.0, 1.0, N, D, bug=bug, **kw)
    assert np.abs(good.out - bad.out).max() > 0.01 * np.abs(good.out).max() > 0
    if bug in ("round_cell", "count_dead"):
        assert good.counted != bad.counted
    assert np.all(pts[:, :3] < L)
