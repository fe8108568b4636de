"""CPU checks of tests/moments_ref.py, the numpy restatement of the reference's DistributionMoment and
VelocityDistribution that the GPU tests of xpic_moment / xpic_velocity_distribution take their values from."""
import numpy as np

import moments_ref as M


def _plasma(n, d, npart, seed):
    rng = np.random.default_rng(seed)
    pts = np.empty((npart, 6))
    pts[:, :3] = rng.random((npart, 3)) * (np.array(n) * np.array(d))
    pts[:, 3:] = rng.normal(0, 0.1, (npart, 3))
    return pts


def test_density_equals_the_cpu_model(oracle):
    """The helper's full-box density equals the CPU model's DistributionMoment density on the same particles."""
    n, d = (7, 5, 6), (0.5, 0.4, 0.25)
    o = oracle.OracleSim("ecsim", n, d, 1.0)
    s = o.add_sort(9, 1.3, -1.0, 1.0)
    pts = _plasma(n, d, 9 * 7 * 5 * 6, 3)
    pts[0, :3] = [0.0, 0.0, 0.0]          # on the lower corner of the box
    pts[1, :3] = [1.75, 1.0, 0.75]        # on cell faces and centres
    assert o.add_particles(s, pts) == len(pts)
    p, cells = o.particles(s)
    ref = o.moment_density(s)
    mine = M.moment("density", p, cells, -1.0, 1.0, 1.3 / 9, n, d)[..., 0]
    assert ref.shape == mine.shape
    assert np.abs(ref - mine).max() <= 1e-13 * np.abs(ref).max()


def test_round_is_half_away_from_zero():
    assert list(M.cround([-2.5, -1.5, -0.5, 0.5, 1.5, 2.5, 0.49999999999999994])) == [-3, -2, -1, 1, 2, 3, 0]


def test_region_rule_wraps_on_a_full_axis_and_drops_on_a_partial_one():
    """One particle in cell (0, 2, 2) near its lower x and y faces: its 2 x 2 x 2 deposit reaches x = -1 and y = 1.  The
    region spans x in full (the x = -1 deposit wraps to x = nx - 1) and y in part, from y = 2 (the y = 1 deposit is
    dropped); z is partial but the deposit stays inside it."""
    n, d = (6, 5, 5), (1.0, 1.0, 1.0)
    pt = np.array([[0.2, 2.3, 2.5, 0.0, 0.0, 0.0]])
    cell = np.array([(2 * n[1] + 2) * n[0] + 0])
    region = (0, 2, 1, 6, 3, 3)
    out = M.moment("density", pt, cell, 1.0, 1.0, 1.0, n, d, region)[..., 0]
    wx = {5: 0.3, 0: 0.7}   # centres -0.5 (wrapped to 5.5) and 0.5
    wy = {1: 0.2, 2: 0.8}   # centres 1.5 and 2.5
    wz = {2: 1.0}           # exactly on the centre 2.5: the upper neighbour gets 0
    exp = np.zeros((n[2], n[1], n[0]))
    for x, a in wx.items():
        for y, b in wy.items():
            if y >= 2:
                exp[2, y, x] = a * b * wz[2]
    assert np.allclose(out, exp, rtol=0, atol=1e-15)
    assert out[2, 2, 5] > 0            # wrapped on x
    assert out[2, 1].sum() == 0        # dropped on y
    assert np.isclose(out.sum(), 0.8)  # the y = 1 fifth is gone
    # whole box: nothing is dropped, the total is n/Np
    assert np.isclose(M.moment("density", pt, cell, 1.0, 1.0, 1.0, n, d).sum(), 1.0)
    # the storage cell outside the region: the particle does not count, even though its deposit reaches into it
    assert M.moment("density", pt, cell, 1.0, 1.0, 1.0, n, d, (1, 0, 0, 5, 5, 5)).sum() == 0


def test_current_and_cylinder_axis():
    n, d = (4, 4, 2), (1.0, 1.0, 1.0)
    pts = np.array([[2.0, 2.0, 0.5, 0.3, -0.2, 0.1],    # exactly on the cylinder axis (geom / 2)
                    [3.0, 2.0, 0.5, 0.3, -0.2, 0.1]])   # on the +x side: v_r = vx, v_phi = vy
    cells = np.array([(0 * 4 + 2) * 4 + 2, (0 * 4 + 2) * 4 + 3])
    cyl = M.moment_values("momentum_flux_cyl", pts, 1.0, 2.0, n, d)
    cart = M.moment_values("momentum_flux", pts, 1.0, 2.0, n, d)
    assert np.allclose(cyl, cart)
    j = M.moment("current", pts, cells, -2.0, 1.0, 0.5, n, d)
    assert np.allclose(j.sum(axis=(0, 1, 2)), -2.0 * 0.5 * pts[:, 3:].sum(axis=0))


def test_velocity_bins_follow_the_x_axis_as_written():
    """set_regions takes both axes' start and size from vx_min, vx_max, dvx (vy_min / vy_max never enter)."""
    vs, vn = M.vsizes((-0.6, -0.2), (0.4, 0.9), (0.05, 0.1))
    assert (vs, vn) == (-12, 20)
    n, d = (4, 4, 4), (1.0, 1.0, 1.0)
    pts = np.array([[0.5, 0.5, 0.5, 0.025, 0.05, 0.0],    # bins (1, 1): +0.5 rounds away from zero
                    [0.5, 0.5, 0.5, -0.6, -1.2, 0.0],     # bins (-12, -12): the first bin of both axes
                    [0.5, 0.5, 0.5, 0.0, 0.7, 0.0],       # v2 bin 7 < -12 + 20: kept
                    [0.5, 0.5, 0.5, 0.0, 0.8, 0.0]])      # v2 bin 8: dropped although vy_max = 0.9
    h, v0 = M.velocity_distribution("vx_vy", {"name": "box", "min": (0, 0, 0), "max": (4, 4, 4)}, pts, [0] * 4, 1.0, n, d,
                                    (-0.6, -0.2), (0.4, 0.9), (0.05, 0.1))
    assert h.shape == (20, 20) and v0 == (-12, -12)
    assert h[1 + 12, 1 + 12] == 1 and h[0, 0] == 1 and h[7 + 12, 0 + 12] == 1 and h.sum() == 3
