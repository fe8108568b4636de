"""The device kernels of xpic_amd/csrc/eccapfim.hip (k_cell_traversal, k_ie_interpolate, k_ie_decompose) and the segment
shape of ie_shape.h against the float64 restatement tests/eccapfim_ref.py, through the C ABI on single-slab contexts, at
the edges no other test reaches on the device: the periodic wrap far outside the box, grids of 2 and 3 nodes where the
stencils fold onto themselves, exact ties of every round(), degenerate and long moves, the truncation and the 64-crossing
guard, batch sizes around the workgroup, and the entry points of the deposit.

Bounds (derived in eccapfim_ref's docstring, none fitted to the device): counts and truncation exact; traversal points
4 eps max|coordinate| (the device contracts start + dir * t); a gathered component K eps sum |F w| with K_E = 29 and
K_B = 72; a deposited node 2 eps * contributions * sum |contribution| (a value the vector held before counts as one
more contribution).  Each check prints its largest error relative to its bound."""
import ctypes as C

import numpy as np
import pytest

import eccapfim_ref as R

pytestmark = pytest.mark.gpu

EPS = R.EPS
_ctx = {}


def context(grid):
    """one context per grid for the whole module, its E and B set to the grid's random fields"""
    import xpic_amd as X

    if grid not in _ctx:
        n, d = R.GRIDS[grid]
        g = X.Context("basic" if min(n) >= 4 else "ecsim", n, d, R.DT)  # (basic wants extents of 4 cells; the kernels are the same)
        E, B = R.fields(np.random.default_rng(21), n)
        g.set_field(X.E, E)
        g.set_field(X.B, B)
        _ctx[grid] = (g, E, B)
    return (X,) + _ctx[grid] + R.GRIDS[grid]


def ref_segments(rn, r0, d):
    _, se, ss, _ = R.segment_arrays(R.segments(lambda a, b: (lambda p: (p, len(p)))(R.traverse_one(a, b, d)), rn, r0))
    return se, ss


def check_traversal(g, rn, r0, d, max_pts=16, expect=None, what=""):
    """device against restatement (or `expect`, (pts, counts)): every lane, counts exact, the buffer behind the points 0"""
    pe, ce = expect if expect is not None else R.cell_traversal(rn, r0, d, max_pts, cap=R.DEVICE_CAP)
    pts, counts = g.cell_traversal(rn, r0, max_pts)
    assert np.array_equal(counts, ce), np.flatnonzero(counts != ce)[:8]
    worst = 0.0
    for q in range(rn.shape[0]):
        m = min(int(ce[q]), max_pts)
        assert np.all(pts[q, m:] == 0.0), q
        bound = 4 * EPS * np.abs(pe[q, :m]).max()
        err = np.abs(pts[q, :m] - pe[q, :m]).max()
        assert err <= bound, (q, err, bound)
        worst = max(worst, err / bound if bound > 0 else 0.0)
    print("traversal %s: %d lanes, largest error / bound = %.3f" % (what, rn.shape[0], worst))


def check_gather(g, E, B, rn, r0, n, d, what=""):
    Ep, Bp, Es, Bs = R.interpolate(E, B, rn, r0, n, d)
    Eg, Bg = g.implicit_esirkepov_interpolate(rn, r0)
    re, rb = np.abs(Eg - Ep) / (R.K_E * EPS * Es), np.abs(Bg - Bp) / (R.K_B * EPS * Bs)
    print("gather %s: %d lanes, largest error / bound: E %.3f, B %.3f" % (what, rn.shape[0], re.max(), rb.max()))
    assert np.all(np.abs(Eg - Ep) <= R.K_E * EPS * Es), (np.argmax(re), re.max())
    assert np.all(np.abs(Bg - Bp) <= R.K_B * EPS * Bs), (np.argmax(rb), rb.max())


def check_deposit(X, g, alpha, v, rn, r0, n, d, J0=None, what=""):
    """g's J after decompose() calls on it against the restatement's fsum; J0: what J held before"""
    J, count, asum = R.decompose(alpha, v, rn, r0, n, d)
    if J0 is not None:  # the earlier value is one more contribution to its node
        J, count, asum = J + J0, count + (J0 != 0), asum + np.abs(J0)
    Jg = g.get_field(X.J)
    bound = 2 * EPS * count * asum
    assert np.abs(J).max() > 0
    ratio = np.abs(Jg - J)[bound > 0] / bound[bound > 0]
    print("deposit %s: %d lanes, up to %d contributions to a node, largest error / bound = %.3f"
          % (what, rn.shape[0], count.max(), ratio.max()))
    assert np.all(np.abs(Jg - J) <= bound), ratio.max()


def deposit(X, g, alpha, v, rn, r0, n, d, what=""):
    g.vec_set(X.J, 0.0)
    g.implicit_esirkepov_decompose(alpha, v, rn, r0, X.J)
    check_deposit(X, g, alpha, v, rn, r0, n, d, what=what)


def amplitudes(rng, m, zeros=True):
    """alpha with a tenth of the lanes exactly 0 (the kernel skips w == 0), and v"""
    alpha = rng.normal(0, 1, m)
    if zeros:
        alpha[rng.random(m) < 0.1] = 0.0
    return alpha, rng.normal(0, 1, (m, 3))


@pytest.mark.parametrize("grid", list(R.GRIDS))
def test_wrap_and_degenerate_moves(grid):
    """start points over [-2 L, 3 L), moves of up to 2.5 cells; moves out through every face; zero-length, axis-aligned,
    in-plane and same-cell moves: all three kernels, the gathers and the deposit on the segments of the traversal"""
    X, g, E, B, n, d = context(grid)
    rng = np.random.default_rng(22)
    for what, (rn, r0) in (("wrap", R.wrap_moves(rng, 400, n, d)), ("faces", R.face_moves(rng, 20, n, d)),
                           ("degenerate", R.degenerate_moves(rng, n, d))):
        check_traversal(g, rn, r0, d, what=grid + " " + what)
        se, ss = ref_segments(rn, r0, d)
        check_gather(g, E, B, se, ss, n, d, what=grid + " " + what)
        alpha, v = amplitudes(rng, len(se))
        deposit(X, g, alpha, v, se, ss, n, d, what=grid + " " + what)


def test_exact_ties():
    """dyadic coordinates on the power-of-two grid: end points on faces, edges and corners, midpoints on half-integers
    and integers in each axis with both signs, whole-cell diagonal moves; no lane is left out of any comparison"""
    X, g, E, B, n, d = context("pow2")
    rn, r0 = R.tie_moves(d)
    check_traversal(g, rn, r0, d, what="ties")
    check_gather(g, E, B, rn, r0, n, d, what="ties")
    alpha, v = amplitudes(np.random.default_rng(23), len(rn), zeros=False)
    deposit(X, g, alpha, v, rn, r0, n, d, what="ties")


@pytest.mark.parametrize("max_pts", [2, 8, 16])
def test_long_moves_truncate(oracle, max_pts):
    """L1 distances up to 20 cells: the count is the full count, the first max_pts points are there, the rest of the
    buffer is zero -- against the restatement and against the oracle; and what the 64-crossing guard returns, from the
    oracle: 1 + 64 + 1 points counted where the reference would return 2 + 75"""
    X, g, E, B, n, d = context("general")
    o = oracle.OracleSim("basic", n, d, R.DT)
    rn, r0 = R.long_moves(np.random.default_rng(24), 300, n, d)
    check_traversal(g, rn, r0, d, max_pts, what="long, max_pts %d" % max_pts)
    rc, r0c = R.capped_move(d)
    rn, r0 = np.vstack([rn, rc]), np.vstack([r0, r0c])
    pe, ce = np.zeros((len(rn), max_pts, 3)), np.zeros(len(rn), dtype=np.int32)
    for q in range(len(rn)):
        po, ce[q] = o.cell_traversal(rn[q], r0[q], max_pts)
        pe[q, :len(po)] = po
    assert ce[:-1].max() - 2 >= 15 and (ce > max_pts).any() and ce[-1] == R.DEVICE_CAP + 2
    check_traversal(g, rn, r0, d, max_pts, expect=(pe, ce), what="long and capped against the oracle, max_pts %d" % max_pts)


@pytest.fixture(scope="module")
def batch():
    """1001 wrap moves on the general grid and one segment of each, with the restatement's per-lane results"""
    n, d = R.GRIDS["general"]
    rng = np.random.default_rng(25)
    rn, r0 = R.wrap_moves(rng, 1001, n, d)
    se, ss = np.zeros_like(rn), np.zeros_like(r0)
    for q in range(len(rn)):  # the segment in the middle of each move
        p = R.traverse_one(rn[q], r0[q], d)
        se[q], ss[q] = p[len(p) // 2], p[len(p) // 2 - 1]
    alpha, v = amplitudes(rng, len(rn))
    alpha[0] = 0.75  # the batch of one deposits something
    return rn, r0, se, ss, alpha, v


@pytest.mark.parametrize("m", [1, 255, 256, 257, 1001])
def test_batch_sizes(batch, m):
    X, g, E, B, n, d = context("general")
    rn, r0, se, ss, alpha, v = (a[:m] for a in batch)
    check_traversal(g, rn, r0, d, what="batch %d" % m)
    check_gather(g, E, B, se, ss, n, d, what="batch %d" % m)
    deposit(X, g, alpha, v, se, ss, n, d, what="batch %d" % m)


def test_empty_batch_touches_nothing(batch):
    X, g, E, B, n, d = context("general")
    rn, r0, se, ss, alpha, v = (np.ascontiguousarray(a[:4]) for a in batch)
    pts, counts = np.full((4, 8, 3), 7.5), np.full(4, -3, dtype=np.int32)
    g._ck(g.L.xpic_cell_traversal(g.h, C.c_int64(0), X._dp(rn), X._dp(r0), 8, X._dp(pts), counts.ctypes.data_as(C.POINTER(C.c_int))))
    assert np.all(pts == 7.5) and np.all(counts == -3)
    Ep, Bp = np.full((4, 3), 7.5), np.full((4, 3), -7.5)
    g._ck(g.L.xpic_implicit_esirkepov_interpolate(g.h, C.c_int64(0), X._dp(se), X._dp(ss), X._dp(Ep), X._dp(Bp)))
    assert np.all(Ep == 7.5) and np.all(Bp == -7.5)
    J0 = np.random.default_rng(26).normal(0, 1, g.fshape())
    g.set_field(X.J, J0)
    g._ck(g.L.xpic_implicit_esirkepov_decompose(g.h, C.c_int64(0), X._dp(alpha), X._dp(v), X._dp(se), X._dp(ss), X.J))
    assert np.array_equal(g.get_field(X.J), J0)


def test_deposit_contention_in_one_cell():
    """4096 segments inside one node-centred cell: every one of their 54 atomics meets 4095 others at its address"""
    X, g, E, B, n, d = context("general")
    rng = np.random.default_rng(27)
    cell = np.array([4.0, 3.0, 2.0])
    r0 = (cell + (rng.random((4096, 3)) - 0.5) * 0.98) * np.array(d)
    rn = (cell + (rng.random((4096, 3)) - 0.5) * 0.98) * np.array(d)
    alpha, v = amplitudes(rng, 4096)
    deposit(X, g, alpha, v, rn, r0, n, d, what="one cell")


@pytest.mark.parametrize("grid", ["general", "fold325"])
def test_deposit_accumulates(grid):
    """a call on a J that holds random values adds to it, and two calls equal one call of the concatenation"""
    X, g, E, B, n, d = context(grid)
    rng = np.random.default_rng(28)
    se, ss = ref_segments(*R.wrap_moves(rng, 300, n, d), d)
    alpha, v = amplitudes(rng, len(se))
    J0 = rng.normal(0, 1, g.fshape())
    g.set_field(X.J, J0)
    half = len(se) // 2
    g.implicit_esirkepov_decompose(alpha[:half], v[:half], se[:half], ss[:half], X.J)
    check_deposit(X, g, alpha[:half], v[:half], se[:half], ss[:half], n, d, J0=J0, what=grid + " on a filled J")
    g.implicit_esirkepov_decompose(alpha[half:], v[half:], se[half:], ss[half:], X.J)
    check_deposit(X, g, alpha, v, se, ss, n, d, J0=J0, what=grid + " two calls")


def test_refused_calls_change_nothing(batch):
    X, g, E, B, n, d = context("general")
    rn, r0, se, ss, alpha, v = (np.ascontiguousarray(a[:4]) for a in batch)
    J0 = np.random.default_rng(29).normal(0, 1, g.fshape())
    W0 = np.random.default_rng(30).normal(0, 1, g.fshape())
    g.set_field(X.J, J0)
    g.set_field(X.W2, W0)
    for field in (X.W2, -1, 11, 1000):  # the scratch vector of the call; no such field id
        with pytest.raises(X.XpicError):
            g.implicit_esirkepov_decompose(alpha, v, se, ss, field)
    assert np.array_equal(g.get_field(X.J), J0) and np.array_equal(g.get_field(X.W2), W0)
    for max_pts in (1, 0, -1):
        pts, counts = np.full((4, 8, 3), 7.5), np.full(4, -3, dtype=np.int32)
        rc = g.L.xpic_cell_traversal(g.h, C.c_int64(4), X._dp(rn), X._dp(r0), max_pts, X._dp(pts), counts.ctypes.data_as(C.POINTER(C.c_int)))
        assert rc != 0 and np.all(pts == 7.5) and np.all(counts == -3)


@pytest.mark.parametrize("grid", ["general", "fold325"])
def test_continuity_across_the_faces_on_device(oracle, grid):
    """device cell_traversal -> device decompose -> J closes (rho1 - rho0) / dt + div J = 0 with the device's own charge
    density before and after, for moves out through every face of the box (the divergence is the oracle's)"""
    X, g, E, B, n, d = context(grid)
    rn, r0 = R.face_moves(np.random.default_rng(31), 25, n, d)
    qn = -1.0 * 1.0 / 3
    s = g.add_sort(3, 1.0, -1.0, 1.0, capacity=1024)
    rho = []
    for r in (r0, rn):
        g.clear(s)
        assert g.add_particles(s, np.hstack([R.fold_positions(r, n, d), np.zeros_like(r)])) == len(r)
        rho.append(g.charge_density(s))
    g.clear(s)
    pts, counts = g.cell_traversal(rn, r0, 16)
    assert counts.max() <= 16
    q = np.repeat(np.arange(len(rn)), counts - 1)
    se = np.vstack([pts[k, 1:counts[k]] for k in range(len(rn))])
    ss = np.vstack([pts[k, :counts[k] - 1] for k in range(len(rn))])
    f = np.linalg.norm(se - ss, axis=1) / np.linalg.norm(rn - r0, axis=1)[q]
    v = (rn - r0) / R.DT
    g.vec_set(X.J, 0.0)
    g.implicit_esirkepov_decompose(qn * f, v[q], se, ss, X.J)
    J = g.get_field(X.J)
    o = oracle.OracleSim("basic", n, d, R.DT)
    div = np.zeros(rho[0].shape)
    oracle.lib().orc_div_neg(o.h, oracle._dp(np.ascontiguousarray(J)), oracle._dp(div))
    res = (rho[1] - rho[0]) / R.DT + div
    print("continuity %s: |residual| / |div J| = %.3e" % (grid, np.abs(res).max() / np.abs(div).max()))
    assert np.abs(div).max() > 0
    assert np.abs(res).max() <= 1e-11 * np.abs(div).max()  # test_esirkepov_continuity_on_device's bound
