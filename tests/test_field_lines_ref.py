"""The numpy restatement of the field-line tracer (tests/field_lines_ref.py) against closed forms, without a GPU: a uniform
field, whose lines are straight, and the circle field F = (-(y - y_c), x - x_c, 0) on a 16 x 16 x 4 grid, whose lines are
circles.  Every planted bug of the restatement (and the wrong stagger) must break one of the checks made here, which are
the checks tests/test_gpu_field_lines.py makes of the device."""
import numpy as np
import pytest

import field_lines_ref as R

EPS = np.finfo(float).eps
S_UNIFORM = 50
H_UNIFORM = 0.07
S_CIRCLE = 60


def uniform_seeds():
    rng = np.random.default_rng(5)
    return 1.0 + 6.0 * rng.random((7, 3))


def check_uniform(L, seeds, sign, S=S_UNIFORM, h=H_UNIFORM):
    """straight lines along z: length = S h, volume = S h / 2 to a few eps S"""
    f = 2.0
    assert (L.code == R.MAXSTEPS).all() and (L.steps == S).all()
    assert np.array_equal(L.end[:, :2], seeds[:, :2])
    assert np.abs(L.end[:, 2] - (seeds[:, 2] + sign * S * h)).max() <= 4 * EPS * S * 8.0
    assert np.abs(L.length - S * h).max() <= 4 * EPS * S * (S * h)
    assert np.abs(L.volume - S * h / f).max() <= 4 * EPS * S * (S * h / f)
    assert np.abs(L.fmin - f).max() <= 16 * EPS and np.abs(L.fmax - f).max() <= 16 * EPS  # (the weights sum to 1 up to rounding)


def drift_bound(S, h, rad):
    """RK4 on a rotation by theta = h / r a step shrinks the radius by less than theta^6 / 72 of it; plus rounding"""
    return S * (h / rad) ** 6 / 72 * rad + 1e-13


def check_circle(L, rad, S=S_CIRCLE, h=R.CIRCLE_H):
    delta = drift_bound(S, h, rad)
    assert (L.code == R.MAXSTEPS).all() and (L.steps == S).all()
    assert (np.abs(R.circle_radius(L.end) - rad) <= delta).all()
    assert (np.abs(L.fmin - rad) <= delta).all() and (np.abs(L.fmax - rad) <= delta).all()  # |F| = r
    # every 1 / f of the trapezoid is within delta / (r (r - delta)) of 1 / r
    assert (np.abs(L.volume - L.length / rad) <= L.length * delta / (rad * (rad - delta)) + 1e-13).all()
    assert np.abs(L.length - S * h).max() <= 4 * EPS * S * (S * h)


def check_closed(L, rad, h=R.CIRCLE_H):
    want = np.ceil(2 * np.pi * rad / h).astype(np.int64)
    assert (L.code == R.CLOSED).all()
    assert ((L.steps == want) | (L.steps == want + 1)).all(), (L.steps, want)


def uniform_run(sign=+1, bug=None, **kw):
    seeds = uniform_seeds()
    src = R.grid_source(R.uniform_field(), R.UNIFORM_D)
    return seeds, R.trace(src, seeds, H_UNIFORM, S_UNIFORM, s=sign, bug=bug, **kw)


def circle_run(stagger=R.STAGGER_B, sampled_as=None, bug=None, S=S_CIRCLE, **kw):
    src = R.grid_source(R.circle_field(stagger if sampled_as is None else sampled_as), R.CIRCLE_D, stagger)
    return R.trace(src, R.circle_seeds(), R.CIRCLE_H, S, bug=bug, **kw)


@pytest.mark.parametrize("sign", [+1, -1])
def test_uniform(sign):
    seeds, L = uniform_run(sign)
    check_uniform(L, seeds, sign)


@pytest.mark.parametrize("stagger", [R.STAGGER_B, R.STAGGER_E])
def test_circle(stagger):
    rad = np.array(R.CIRCLE_RADII)
    seeds = R.circle_seeds()
    src = R.grid_source(R.circle_field(stagger), R.CIRCLE_D, stagger)
    exact = np.column_stack([-(seeds[:, 1] - 2.0), seeds[:, 0] - 2.0, np.zeros(len(seeds))])
    assert np.abs(src(seeds) - exact).max() <= 8 * EPS  # the spline reproduces the linear field
    check_circle(circle_run(stagger), rad)
    for sign in (+1, -1):
        check_closed(circle_run(stagger, S=400, close_tol=R.CIRCLE_H, s=sign), rad)
    assert (2 * np.pi * rad / R.CIRCLE_H % 1 > 0.1).all() and (2 * np.pi * rad / R.CIRCLE_H % 1 < 0.9).all()  # no tie


def test_wrong_stagger_is_visible():
    """a B-staggered vector read with the electric products: the centre moves by half a cell"""
    with pytest.raises(AssertionError):
        check_circle(circle_run(R.STAGGER_E, sampled_as=R.STAGGER_B), np.array(R.CIRCLE_RADII))


def test_euler_is_visible():
    with pytest.raises(AssertionError):
        check_circle(circle_run(bug="euler"), np.array(R.CIRCLE_RADII))


def test_unnormalised_direction_is_visible():
    seeds, L = uniform_run(bug="unnormalised")
    with pytest.raises(AssertionError):
        check_uniform(L, seeds, +1)
    with pytest.raises(AssertionError):
        check_closed(circle_run(bug="unnormalised", S=400, close_tol=R.CIRCLE_H), np.array(R.CIRCLE_RADII))


def test_missing_half_is_visible():
    seeds, L = uniform_run(bug="no_half")
    with pytest.raises(AssertionError):
        check_uniform(L, seeds, +1)
    with pytest.raises(AssertionError):
        check_circle(circle_run(bug="no_half"), np.array(R.CIRCLE_RADII))


BOX = {"name": "box", "min": (0.0, 0.0, 2.0), "max": (8.0, 8.0, 6.0)}


def check_region(L, seeds, h=H_UNIFORM):
    """straight lines up z through a box that ends at z = 6: a lane leaves before the first step that would start in a
    cell whose corner is at z >= 6 (or < 2), a seed outside takes no step, and the point after the last step is not tested"""
    z0 = seeds[:, 2]
    k = np.arange(0, 32)  # (one point beyond the 30 steps of region_run)
    z = z0[:, None] + k[None, :] * h  # (exact enough: no z lands within rounding of a cell face, checked below)
    assert np.abs(z - np.round(z)).min() > 1e-9
    inside = (np.floor(z) >= 2.0) & (np.floor(z) < 6.0)
    want = np.where(inside.all(axis=1), len(k), np.argmin(inside, axis=1))  # the first point that fails
    cut = 30
    assert np.array_equal(L.steps, np.minimum(want, cut))
    assert np.array_equal(L.code, np.where(want < cut, R.LEFT, R.MAXSTEPS))


def region_run(bug=None):
    seeds = uniform_seeds()
    seeds[0, 2], seeds[1, 2] = 1.531, 6.469             # outside at the start
    seeds[2, 2] = 6.0 - 29.5 * H_UNIFORM             # its 30th step ends in the cell at z = 6: MAXSTEPS, not LEFT
    src = R.grid_source(R.uniform_field(), R.UNIFORM_D)
    return seeds, R.trace(src, seeds, H_UNIFORM, 30, keep=R.region_keep(BOX, R.UNIFORM_D), bug=bug)


def test_region_rule():
    seeds, L = region_run()
    check_region(L, seeds)
    assert (L.steps[:2] == 0).all() and np.array_equal(L.end[:2], seeds[:2]) and L.code[2] == R.MAXSTEPS
    assert (L.code == R.LEFT).sum() >= 3 and (L.code == R.MAXSTEPS).sum() >= 2


def test_region_after_the_step_is_visible():
    seeds, L = region_run(bug="region_after")
    with pytest.raises(AssertionError):
        check_region(L, seeds)


def test_null_floor_samples_and_directions():
    seeds = uniform_seeds()
    src = R.grid_source(R.uniform_field(), R.UNIFORM_D)
    L = R.trace(src, seeds, H_UNIFORM, 10, f_floor=2.5)
    assert (L.code == R.NULL).all() and (L.steps == 0).all() and np.array_equal(L.end, seeds) and np.abs(L.fmin - 2.0).max() <= 16 * EPS
    F = R.uniform_field()
    seeds[:, 2] = 1.0 + (seeds[:, 2] - 1.0) / 3.0  # z within 1 .. 3: every seed lies in the field
    F[5:, :, :, :] = 0.0  # no field above z = 4.5 or so: the lines up z stop where a stage or an end point finds |F| = 0
    up = R.trace(R.grid_source(F, R.UNIFORM_D), seeds, H_UNIFORM, 200, sample_every=3)
    assert (up.code == R.NULL).all() and (up.fmin > 0).all() and np.isfinite(up.volume).all()
    for q in range(len(seeds)):
        held = up.steps[q] // 3
        short = R.trace(R.grid_source(F, R.UNIFORM_D), seeds[q:q + 1], H_UNIFORM, 3 * held) if held else None
        if held:
            assert np.array_equal(up.samples[q, held - 1], short.end[0])
        assert (up.samples[q, held:] == up.end[q]).all()
    both = R.lines(src, seeds, H_UNIFORM, 10)
    only = R.lines(src, seeds, H_UNIFORM, 10, directions=2)
    assert both.end.shape == (2, len(seeds), 3) and np.array_equal(both.end[1], only.end[1]) and (only.code[0] == -1).all()
    assert np.abs((both.end[0, :, 2] - seeds[:, 2]) + (both.end[1, :, 2] - seeds[:, 2])).max() <= 64 * EPS


def test_extended_precision_agrees():
    """the same statement in np.longdouble: the difference is rounding, far below the closed-form bounds"""
    a = circle_run()
    b = circle_run(dtype=np.longdouble)
    assert np.array_equal(a.steps, b.steps) and np.array_equal(a.code, b.code)
    assert np.abs(a.end - b.end.astype(np.float64)).max() <= 1e-13
    assert np.abs(a.volume - b.volume.astype(np.float64)).max() <= 1e-12
