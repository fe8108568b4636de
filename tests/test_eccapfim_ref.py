"""CPU checks of tests/eccapfim_ref.py, the float64 restatement tests/test_gpu_eccapfim.py holds the device against: the
restatement against the C++ oracle on the whole edge list of the GPU test (periodic wrap far outside the box, folding
stencils, exact ties, degenerate and long moves), properties that need no oracle (weights sum to one, the traversal tiles
the path, the count, discrete continuity for moves through every face of the box), and -- as tests/test_precond_ref.py
does for the preconditioners -- that the bugs this restatement exists to catch break those same checks when they are
built into it."""
import numpy as np
import pytest

import eccapfim_ref as R

EPS = R.EPS


# ---- the checks (mutate: the bug built into the restatement, for test_mutations_are_visible)

def check_traversal(o, rn, r0, d, max_pts=16, mutate=None):
    """restatement against oracle: counts exact, points within 4 eps max|coordinate| (the GPU test's bound)"""
    pts, counts = R.cell_traversal(rn, r0, d, max_pts, cap=R.DEVICE_CAP, mutate=mutate)
    worst = 0.0
    for q in range(rn.shape[0]):
        po, cnt = o.cell_traversal(rn[q], r0[q], max_pts)
        assert counts[q] == cnt, (q, counts[q], cnt)
        m = min(cnt, max_pts)
        assert np.all(pts[q, m:] == 0.0)
        bound = 4 * EPS * np.abs(po).max()
        err = np.abs(pts[q, :m] - po).max()
        assert err <= bound, (q, err, bound)
        worst = max(worst, err / bound if bound > 0 else 0.0)
    return worst


def check_gather(o, E, B, rn, r0, n, d, mutate=None):
    """restatement against oracle within K eps sum |F w|; returns the largest error relative to the bound"""
    Ep, Bp, Es, Bs = R.interpolate(E, B, rn, r0, n, d, mutate=mutate)
    Eo, Bo = o.implicit_esirkepov_interpolate(rn, r0)
    assert np.all(np.abs(Ep - Eo) <= R.K_E * EPS * Es), np.max(np.abs(Ep - Eo) / (R.K_E * EPS * Es))
    assert np.all(np.abs(Bp - Bo) <= R.K_B * EPS * Bs), np.max(np.abs(Bp - Bo) / (R.K_B * EPS * Bs))
    return max(np.max(np.abs(Ep - Eo) / (R.K_E * EPS * Es)), np.max(np.abs(Bp - Bo) / (R.K_B * EPS * Bs)))


def check_deposit(o, alpha, v, rn, r0, n, d, mutate=None):
    """restatement against oracle within 2 eps * contributions * sum |contribution| at every node"""
    J, count, asum = R.decompose(alpha, v, rn, r0, n, d, mutate=mutate)
    o.set_field("J", np.zeros(o.fshape()))
    o.implicit_esirkepov_decompose(alpha, v, rn, r0, "J")
    Jo = o.get_field("J")
    bound = 2 * EPS * count * asum
    assert np.abs(J).max() > 0
    assert np.all(np.abs(J - Jo) <= bound), np.max(np.abs(J - Jo)[bound > 0] / bound[bound > 0])
    return np.max(np.abs(J - Jo)[bound > 0] / bound[bound > 0])


def check_weights_sum_to_one(rn, r0, d, mutate=None):
    _, w = R.ie_shape(rn, r0, d, mutate=mutate)
    for cx in range(3):
        s = w[:, 18 * cx:18 * cx + 18].sum(axis=1)
        # 18 weights of 11 roundings each and 17 additions, all of one sign inside a cell
        assert np.abs(s - 1.0).max() <= (11 + 17) * EPS, (cx, np.abs(s - 1.0).max())


def check_tiling(rn, r0, d, mutate=None):
    """properties of the traversal that need no oracle (the moves do not end on a face: no cap is needed)"""
    d = np.array(d)
    for q in range(rn.shape[0]):
        pts = R.traverse_one(rn[q], r0[q], d, cap=R.DEVICE_CAP, mutate=mutate)
        cnt = len(pts)
        assert np.array_equal(pts[0], r0[q]) and np.array_equal(pts[-1], rn[q])
        dr = rn[q] - r0[q]
        if np.dot(dr, dr) > 0:
            t = (pts - r0[q]) @ dr / np.dot(dr, dr)
            assert np.all(np.diff(t) >= -1e-15) and abs(t[-1] - 1) < 1e-14
            assert np.abs(pts - (r0[q] + np.outer(t, dr))).max() <= 1e-13 * max(1.0, np.abs(pts).max())
        # every segment stays inside one node-centred cell, and no two segments share one
        cells = R.c_round(0.5 * (pts[1:] + pts[:-1]) / d).astype(int)
        assert len({tuple(c) for c in cells}) == len(cells) == cnt - 1
        # number of points = 2 + L1 distance of the end cells
        assert cnt - 2 == np.abs(R.c_round(rn[q] / d) - R.c_round(r0[q] / d)).sum(), q


def cases(grid, seed):
    """the random part of the edge list on one grid: (name, rn, r0)"""
    n, d = R.GRIDS[grid]
    rng = np.random.default_rng(seed)
    return n, d, rng, [("wrap",) + R.wrap_moves(rng, 150, n, d), ("faces",) + R.face_moves(rng, 10, n, d),
                       ("degenerate",) + R.degenerate_moves(rng, n, d, each=8)]


def kernel_segments(rn, r0, d):
    """the segments of the restatement's traversal: what the scheme hands to interpolate and decompose"""
    _, se, ss, _ = R.segment_arrays(R.segments(lambda a, b: (lambda p: (p, len(p)))(R.traverse_one(a, b, d)), rn, r0))
    return se, ss


# ---- restatement against oracle

@pytest.mark.parametrize("grid", list(R.GRIDS))
def test_restatement_matches_oracle_on_the_edge_list(oracle, grid):
    n, d, rng, lists = cases(grid, 11)
    o = oracle.OracleSim("basic", n, d, R.DT)
    E, B = R.fields(rng, n)
    o.set_field("E", E)
    o.set_field("B", B)
    for name, rn, r0 in lists:
        check_traversal(o, rn, r0, d)
        se, ss = kernel_segments(rn, r0, d)
        check_gather(o, E, B, se, ss, n, d)
        check_deposit(o, rng.normal(0, 1, len(se)) * (rng.random(len(se)) > 0.1), rng.normal(0, 1, (len(se), 3)), se, ss, n, d)


def test_restatement_matches_oracle_on_exact_ties(oracle):
    n, d = R.GRIDS["pow2"]
    o = oracle.OracleSim("basic", n, d, R.DT)
    rng = np.random.default_rng(12)
    E, B = R.fields(rng, n)
    o.set_field("E", E)
    o.set_field("B", B)
    rn, r0 = R.tie_moves(d)
    check_traversal(o, rn, r0, d)
    _, counts = R.cell_traversal(rn, r0, d, 2, cap=R.DEVICE_CAP)
    assert (counts == R.DEVICE_CAP + 2).sum() >= 12  # the ties the reference does not return from are on the list
    check_gather(o, E, B, rn, r0, n, d)
    check_deposit(o, rng.normal(0, 1, len(rn)), rng.normal(0, 1, (len(rn), 3)), rn, r0, n, d)


@pytest.mark.parametrize("max_pts", [2, 8, 16])
def test_restatement_matches_oracle_on_long_moves(oracle, max_pts):
    n, d = R.GRIDS["general"]
    o = oracle.OracleSim("basic", n, d, R.DT)
    rn, r0 = R.long_moves(np.random.default_rng(13), 60, n, d)
    check_traversal(o, rn, r0, d, max_pts)
    _, counts = R.cell_traversal(rn, r0, d, max_pts)
    assert counts.max() - 2 >= 15 and (counts > max_pts).any()
    # more than 64 crossings: the guard of the C++ texts returns 1 + 64 + 1 points, the reference all 2 + 75
    rn, r0 = R.capped_move(d)
    check_traversal(o, rn, r0, d, max_pts)
    assert R.cell_traversal(rn, r0, d, max_pts, cap=R.DEVICE_CAP)[1][0] == R.DEVICE_CAP + 2
    assert R.cell_traversal(rn, r0, d, max_pts)[1][0] == 2 + 75


# ---- properties that hold without any oracle

@pytest.mark.parametrize("grid", list(R.GRIDS))
def test_weights_sum_to_one(grid):
    n, d, rng, lists = cases(grid, 14)
    for name, rn, r0 in lists:
        check_weights_sum_to_one(*kernel_segments(rn, r0, d), d)


@pytest.mark.parametrize("grid", list(R.GRIDS))
def test_traversal_tiles_the_path(grid):
    n, d, rng, lists = cases(grid, 15)
    for name, rn, r0 in lists:
        check_tiling(rn, r0, d)
    check_tiling(*R.long_moves(rng, 40, n, d), d)


def test_rounding_and_folding_rules():
    x = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.49999999999999994, -0.49999999999999994, 2.4, -2.6, 0.0])
    assert np.array_equal(R.c_round(x), [1, 2, 3, -1, -2, -3, 0, -0.0, 2, -3, 0])
    assert [R.fold(i, 3) for i in (-7, -3, -1, 0, 2, 3, 8)] == [2, 0, 2, 0, 2, 0, 2]


def check_continuity(oracle, n, d, rn, r0, mutate=None):
    """(rho1 - rho0) / dt + div J = 0 for the segment-wise deposit of eccapfim/particles.cpp, decompose(q n / Np * ds / d,
    v = (rn - r0) / dt, segment), with the oracle's 2nd-order charge density at the folded end points"""
    o = oracle.OracleSim("basic", n, d, R.DT)
    so = o.add_sort(3, 1.0, -1.0, 1.0)
    qn = -1.0 * 1.0 / 3
    rho = []
    for r in (r0, rn):
        o.clear(so)
        assert o.add_particles(so, np.hstack([R.fold_positions(r, n, d), np.zeros_like(r)])) == len(r)
        rho.append(o.charge_density(so))
    segs = R.segments(lambda a, b: (lambda p: (p, len(p)))(R.traverse_one(a, b, d, mutate=mutate)), rn, r0)
    q, se, ss, f = R.segment_arrays(segs)
    v = (rn - r0) / R.DT
    J, _, _ = R.decompose(qn * f, v[q], se, ss, n, d, mutate=mutate)
    o.set_field("J", np.zeros(o.fshape()))
    o.implicit_esirkepov_decompose(qn * f, v[q], se, ss, "J")
    for Jx in (J, o.get_field("J")):
        div = np.zeros(rho[0].shape)
        oracle.lib().orc_div_neg(o.h, oracle._dp(np.ascontiguousarray(Jx)), oracle._dp(div))
        res = (rho[1] - rho[0]) / R.DT + div
        assert np.abs(div).max() > 0
        assert np.abs(res).max() <= 1e-12 * np.abs(div).max(), np.abs(res).max() / np.abs(div).max()


@pytest.mark.parametrize("grid", ["general", "fold325"])
def test_continuity_across_every_face(oracle, grid):
    n, d = R.GRIDS[grid]
    rn, r0 = R.face_moves(np.random.default_rng(16), 25, n, d)
    L = np.array(n) * np.array(d)
    for axis in range(3):  # every face is crossed
        assert (rn[:, axis] < 0).sum() >= 25 and (rn[:, axis] >= L[axis]).sum() >= 25
    check_continuity(oracle, n, d, rn, r0)


# ---- the bugs this file exists to catch are visible in it

def test_mutations_are_visible(oracle):
    """Each bug, built into the restatement, breaks a check above on inputs of the edge list.  (A single fold leaves an
    index outside the grid: the gather then raises IndexError before it can compare.)"""
    n, d = R.GRIDS["pow2"]
    o = oracle.OracleSim("basic", n, d, R.DT)
    rng = np.random.default_rng(17)
    E, B = R.fields(rng, n)
    o.set_field("E", E)
    o.set_field("B", B)
    rn, r0 = R.tie_moves(d)
    alpha, v = rng.normal(0, 1, len(rn)), rng.normal(0, 1, (len(rn), 3))
    # the unmutated restatement passes what the mutated ones must fail
    check_traversal(o, rn, r0, d)
    check_gather(o, E, B, rn, r0, n, d)
    check_deposit(o, alpha, v, rn, r0, n, d)
    # half-even rounding: the ties of the cells (traversal), of the segment shape and of the midpoint shape (gather)
    with pytest.raises(AssertionError):
        check_traversal(o, rn, r0, d, mutate="half_even")
    with pytest.raises(AssertionError):
        check_gather(o, E, B, rn, r0, n, d, mutate="half_even")
    with pytest.raises(AssertionError):
        check_deposit(o, alpha, v, rn, r0, n, d, mutate="half_even")
    # the tie of the ladder taking x instead of z: a move that touches the x face where it crosses the z face
    with pytest.raises(AssertionError):
        check_traversal(o, rn, r0, d, mutate="tie_x")
    tie = np.array([[2.0, 3.0, 4.0]]) * d, np.array([[-0.5, 0.0, 0.5]]) * d
    check_tiling(tie[0] + tie[1], tie[0], d)
    with pytest.raises(AssertionError):
        check_tiling(tie[0] + tie[1], tie[0], d, mutate="tie_x")
    # s0 / sn swapped in one weight: sums to one no longer, and the deposit is not continuous
    n, d, rng, lists = cases("general", 18)
    se, ss = kernel_segments(lists[0][1], lists[0][2], d)
    check_weights_sum_to_one(se, ss, d)
    with pytest.raises(AssertionError):
        check_weights_sum_to_one(se, ss, d, mutate="swap")
    rn, r0 = R.face_moves(np.random.default_rng(16), 25, n, d)
    with pytest.raises(AssertionError):
        check_continuity(oracle, n, d, rn, r0, mutate="swap")
    # a single fold: start points up to two box lengths away
    for grid in ("general", "fold325"):
        n, d, rng, lists = cases(grid, 19)
        o = oracle.OracleSim("basic", n, d, R.DT)
        E, B = R.fields(rng, n)
        o.set_field("E", E)
        o.set_field("B", B)
        se, ss = kernel_segments(lists[0][1], lists[0][2], d)
        check_gather(o, E, B, se, ss, n, d)
        with pytest.raises((AssertionError, IndexError)):
            check_gather(o, E, B, se, ss, n, d, mutate="single_fold")
        with pytest.raises((AssertionError, IndexError)):
            check_deposit(o, np.ones(len(se)), np.ones((len(se), 3)), se, ss, n, d, mutate="single_fold")
