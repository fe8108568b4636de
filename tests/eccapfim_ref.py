"""The inner kernels of the reference's `eccapfim` scheme restated in numpy float64: the second statement that
xpic_amd/csrc/eccapfim.hip and ie_shape.h (and oracle/xpic_oracle.cpp's C++ text of the same) are held to.  Written from
the algorithms the kernel header cites, not from either C++ text:

  cell_traversal(rn, r0, d, max_pts)     src/impls/eccapfim/cell_traversal.cpp:3-77
  ie_shape(rn, r0, d)                    ImplicitEsirkepov::Shape::setup, src/algorithms/implicit_esirkepov.cpp:11-57
  interpolate(E, B, rn, r0, n, d)        ImplicitEsirkepov::interpolate, :60-90
  decompose(alpha, v, rn, r0, n, d)      ImplicitEsirkepov::decompose, :92-117

Fields are arrays [nz][ny][nx][3]; positions are [lanes][3].  Every floating-point expression is written in the
reference's order and rounded operation by operation.  Two rules decide the integers:

  * rounding is half away from zero, as C's round() (np.round is half to even and is not used);
  * node indices fold with a true modulus on all three axes, whatever the distance from the box (the reference reads a
    ghosted local array and is defined only within four nodes of the box; a single-slab context folds any index).

The traversal of the reference does not terminate on some exact ties (see traverse_one); the C++ texts stop it after 64
crossings.  That guard is the `cap` argument here: None restates the reference, DEVICE_CAP what the library returns.

Round-off budget of a gather (test_gpu_eccapfim.py, test_eccapfim_ref.py), in units of eps = 2^-52, against
sum |F_node * w_node| of the lane and component, between any two evaluations of the same expressions (contracted into
fused multiply-adds or not, summed in any order).  The arguments of the shape functions -- r / d, the midpoint, round,
and the differences node - position -- are single IEEE operations on the inputs that no evaluation can do differently, so
the count starts behind them, and it is a bound where no sum cancels: the segment lies in the node-centred cell of its
midpoint, as every segment of cell_traversal does, so that every factor below is >= 0.

  E, K_E = 18 + 11 = 29.  One weight shx * (sny * (2 snz + s0z) + s0y * (2 s0z + snz)): 2 roundings in each sfunc_2
      value (s * s and 0.75 - ., or 1.5 - s and its square; halving is exact), 1 in 2 snz + s0z, 1 in the product with
      sny: 2 + (2 + 1) + 1 = 6 for each product, 1 for their sum (7), 3 in shx (the difference, 1 - |.|, the sixth),
      1 for the last product: 11.  18 terms: 1 rounding in F * w and at most 17 additions behind it.
  B, K_B = 64 + 8 = 72.  One weight S * S * N: 2 roundings in each spline value, 2 products: 8.  At most 4 x 4 x 4 = 64
      terms: 1 rounding in F * w and at most 63 additions.

Each evaluation is within K * eps / 2 of the exact value of the expressions, two of them within K * eps of each other.

A deposit is bounded node by node with 2 eps * (number of contributions) * sum |contribution|, both factors returned by
decompose(); its sums are math.fsum, so the restatement carries no ordering error of its own."""
import math

import numpy as np

EPS = np.finfo(np.float64).eps
K_E, K_B = 29, 72
DEVICE_CAP = 64  # crossings after which the C++ texts give up (include/xpic_hip.h: xpic_cell_traversal)
DBL_MAX = np.finfo(np.float64).max

MUTATIONS = ("half_even", "single_fold", "swap", "tie_x")  # tests/test_eccapfim_ref.py: the bugs this file exists to catch


def c_round(x, mutate=None):
    """C's round(): to the nearest integer, halves away from zero; elementwise, returns floats"""
    x = np.asarray(x, dtype=np.float64)
    if mutate == "half_even":
        return np.round(x)
    a = np.abs(x)
    f = np.floor(a)
    return np.copysign(f + (a - f >= 0.5), x)  # a - f is exact


def fold(i, n, mutate=None):
    """node index i of an axis of n nodes folded into [0, n)"""
    if mutate == "single_fold":
        return i + n if i < 0 else (i - n if i >= n else i)
    return i % n  # Python's % is the true modulus


# ---- moves and segments (shared by the tests of these kernels)

def random_moves(rng, n, max_cells=1.4, N=(9, 8, 7), D=(0.5, 0.4, 0.3)):
    """n moves that start in the middle 60 % of the box and go up to max_cells cells along every axis"""
    L = np.array(N) * np.array(D)
    r0 = rng.random((n, 3)) * L * 0.6 + L * 0.2
    rn = r0 + (rng.random((n, 3)) * 2 - 1) * max_cells * np.array(D)
    return rn, r0


def wrap_moves(rng, n, N, D, max_cells=2.5):
    """n moves of up to max_cells cells whose start points are uniform over [-2 L, 3 L)"""
    L = np.array(N) * np.array(D)
    r0 = (rng.random((n, 3)) * 5 - 2) * L
    rn = r0 + (rng.random((n, 3)) * 2 - 1) * max_cells * np.array(D)
    return rn, r0


def face_moves(rng, per_face, N, D, max_cells=2.5):
    """per_face moves out of the box through each of its six faces: the start less than a cell inside the face, the end
    up to max_cells cells further out, up to 1.4 cells along the other two axes"""
    N, D = np.array(N), np.array(D, dtype=np.float64)
    L = N * D
    r0s, rns = [], []
    for axis in range(3):
        for side in (0, 1):
            r0 = rng.random((per_face, 3)) * L
            rn = r0 + (rng.random((per_face, 3)) * 2 - 1) * 1.4 * D
            depth = rng.random(per_face) * D[axis]
            out = depth + rng.random(per_face) * (max_cells * D[axis] - depth)
            r0[:, axis] = depth if side == 0 else L[axis] - depth
            rn[:, axis] = r0[:, axis] - out if side == 0 else r0[:, axis] + out
            r0s.append(r0)
            rns.append(rn)
    return np.vstack(rns), np.vstack(r0s)


def segments(traverse, rn, r0):
    """[(move, segment end, segment start, fraction of the path)] per move, from cell_traversal's points."""
    out = []
    for q in range(rn.shape[0]):
        pts, cnt = traverse(rn[q], r0[q])
        assert cnt == len(pts)
        d = np.linalg.norm(rn[q] - r0[q])
        for s in range(1, cnt):
            ds = np.linalg.norm(pts[s] - pts[s - 1])
            out.append((q, pts[s], pts[s - 1], ds / d if d > 0 else 1.0))
    return out


def segment_arrays(segs):
    """(move index, ends, starts, fractions) of segments() as arrays"""
    return (np.array([s[0] for s in segs]), np.array([s[1] for s in segs]), np.array([s[2] for s in segs]),
            np.array([s[3] for s in segs]))


# ---- cell_traversal

def traverse_one(end, start, d, cap=None, mutate=None):
    """All points of the move start -> end: the start, the crossings of the faces of the node-centred cells
    (cell of r = round(r / d)) in the order of the path, the end.

    The ladder prefers z over y over x when crossing parameters tie.  Where the preferred axis does not have to be crossed
    at all -- its end coordinate lies exactly on a face and rounds back into the cell it came from, e.g. from 2.0 to 1.5
    cells, while another axis crosses at the same parameter 1 -- the reference steps it nevertheless, never finds the
    last cell and does not return.  cap = k stops such a walk once 1 + k points are stored, as the C++ texts do; without a
    cap a walk of more than 10^4 crossings raises."""
    end, start, d = (np.asarray(a, dtype=np.float64) for a in (end, start, d))
    curr = [int(c) for c in c_round(start / d, mutate)]
    last = [int(c) for c in c_round(end / d, mutate)]
    if curr == last:
        return np.array([start, end])
    dr = end - start
    sg = [1 if dr[c] > 0 else -1 for c in range(3)]
    tt, dtt = [0.0] * 3, [0.0] * 3
    for c in range(3):
        nxt = np.float64(curr[c] + sg[c] * 0.5) * d[c]
        tt[c] = (nxt - start[c]) / dr[c] if dr[c] != 0 else DBL_MAX
        dtt[c] = d[c] / dr[c] * sg[c] if dr[c] != 0 else 0.0
    pts = [start]
    while curr != last:
        if tt[0] < tt[1]:
            c = 0 if (tt[0] <= tt[2] if mutate == "tie_x" else tt[0] < tt[2]) else 2
        else:
            c = 1 if tt[1] < tt[2] else 2
        t = tt[c]
        curr[c] += sg[c]
        tt[c] = tt[c] + dtt[c]
        pts.append(start + dr * t)
        if cap is not None and len(pts) > cap:
            break
        if len(pts) > 10000:
            raise RuntimeError("cell_traversal does not terminate for %r -> %r" % (start, end))
    pts.append(end)
    return np.array(pts)


def cell_traversal(rn, r0, d, max_pts, cap=None, mutate=None):
    """(pts [lanes][max_pts][3], counts [lanes]): the first max_pts points of every move r0 -> rn, zeros behind them, and
    the full number of points"""
    rn, r0 = np.atleast_2d(rn), np.atleast_2d(r0)
    pts = np.zeros((rn.shape[0], max_pts, 3))
    counts = np.zeros(rn.shape[0], dtype=np.int32)
    for q in range(rn.shape[0]):
        p = traverse_one(rn[q], r0[q], d, cap, mutate)
        counts[q] = len(p)
        pts[q, :min(len(p), max_pts)] = p[:max_pts]
    return pts, counts


# ---- the segment shape

def _sfunc_1(s):
    return 1.0 - np.abs(s)


def _sfunc_2(j, s):
    s = np.abs(s)
    return 0.75 - s * s if j == 1 else 0.5 * (1.5 - s) * (1.5 - s)


def ie_shape(rn, r0, d, mutate=None):
    """(start [lanes][3] int, w [lanes][54]).  Weight m belongs to component cx = m // 18 and to the node
    start + i with i[cx] = (m % 18) // 9 in {0, 1}, i[cy] = (m % 9) // 3, i[cz] = m % 3, cy = cx + 1, cz = cx + 2 mod 3."""
    rn, r0 = np.atleast_2d(np.asarray(rn, dtype=np.float64)), np.atleast_2d(np.asarray(r0, dtype=np.float64))
    d = np.asarray(d, dtype=np.float64)
    prn, pr0 = rn / d, r0 / d
    prh = 0.5 * (prn + pr0)
    gc = c_round(prh, mutate)
    start = gc.astype(np.int64) - 1
    gv = gc + 0.5
    w = np.zeros((rn.shape[0], 54))
    sixth = 1.0 / 6.0
    m = 0
    for cx in range(3):
        cy, cz = (cx + 1) % 3, (cx + 2) % 3
        for i in range(2):
            shx = sixth * _sfunc_1(gv[:, cx] + (i - 1) - prh[:, cx])
            for j in range(3):
                sny = _sfunc_2(j, gc[:, cy] + (j - 1) - prn[:, cy])
                s0y = _sfunc_2(j, gc[:, cy] + (j - 1) - pr0[:, cy])
                for k in range(3):
                    snz = _sfunc_2(k, gc[:, cz] + (k - 1) - prn[:, cz])
                    s0z = _sfunc_2(k, gc[:, cz] + (k - 1) - pr0[:, cz])
                    if mutate == "swap" and m == 22:
                        sny, s0y = s0y, sny
                    w[:, m] = shx * (sny * (2 * snz + s0z) + s0y * (2 * s0z + snz))
                    if mutate == "swap" and m == 22:
                        sny, s0y = s0y, sny
                    m += 1
    return start, w


def shape_nodes(start, n, mutate=None):
    """[(m, cx, z, y, x)] of the 54 weights of one lane, indices folded into the grid n = (nx, ny, nz)"""
    out = []
    m = 0
    for cx in range(3):
        cy, cz = (cx + 1) % 3, (cx + 2) % 3
        i = [0, 0, 0]
        for i[cx] in range(2):
            for i[cy] in range(3):
                for i[cz] in range(3):
                    x, y, z = (fold(int(start[a]) + i[a], n[a], mutate) for a in range(3))
                    out.append((m, cx, z, y, x))
                    m += 1
    return out


# ---- gather

def spline2(s):
    """spline_of_2nd_order, src/interfaces/sort_parameters.cpp:21"""
    s = abs(s)
    if s <= 0.5:
        return 0.75 - s * s
    if s < 1.5:
        return 0.5 * (1.5 - s) * (1.5 - s)
    return 0.0


def interpolate(E, B, rn, r0, n, d, mutate=None):
    """(Ep, Bp, Esum, Bsum), each [lanes][3].  E_p with the segment shape; B_p with Shape::setup(midpoint, 1.5, spline2)
    (src/utils/shape.cpp:12-41) and SimpleInterpolation's magnetic products (shape.h:65-72).  Esum and Bsum are
    sum |F_node * w_node|, what the round-off bound of a gather is stated against."""
    rn, r0 = np.atleast_2d(np.asarray(rn, dtype=np.float64)), np.atleast_2d(np.asarray(r0, dtype=np.float64))
    d = np.asarray(d, dtype=np.float64)
    start, w = ie_shape(rn, r0, d, mutate)
    Ep, Bp, Es, Bs = (np.zeros((rn.shape[0], 3)) for _ in range(4))
    for q in range(rn.shape[0]):
        for m, cx, z, y, x in shape_nodes(start[q], n, mutate):
            t = E[z, y, x, cx] * w[q, m]
            Ep[q, cx] += t
            Es[q, cx] += abs(t)
        pr = 0.5 * (rn[q] + r0[q]) / d
        st = [int(v) for v in c_round(pr - 1.5, mutate)]
        sz = [int(math.floor(pr[a] + 1.5)) + 1 - st[a] for a in range(3)]
        No = [[spline2(pr[a] - (st[a] + t)) for t in range(sz[a])] for a in range(3)]
        Sh = [[spline2(pr[a] - (st[a] + t + 0.5)) for t in range(sz[a])] for a in range(3)]
        for kz in range(sz[2]):
            for jy in range(sz[1]):
                for ix in range(sz[0]):
                    x, y, z = fold(st[0] + ix, n[0], mutate), fold(st[1] + jy, n[1], mutate), fold(st[2] + kz, n[2], mutate)
                    ws = (Sh[2][kz] * Sh[1][jy] * No[0][ix], Sh[2][kz] * No[1][jy] * Sh[0][ix],
                          No[2][kz] * Sh[1][jy] * Sh[0][ix])
                    for c in range(3):
                        t = B[z, y, x, c] * ws[c]
                        Bp[q, c] += t
                        Bs[q, c] += abs(t)
    return Ep, Bp, Es, Bs


# ---- deposit

def decompose(alpha, v, rn, r0, n, d, mutate=None):
    """(J, count, asum), each [nz][ny][nx][3]: the current alpha[q] * v[q] * shape(q) summed over the lanes, and for every
    node and component the number of non-zero contributions and the sum of their absolute values.  Sums are math.fsum."""
    rn, r0 = np.atleast_2d(np.asarray(rn, dtype=np.float64)), np.atleast_2d(np.asarray(r0, dtype=np.float64))
    alpha, v = np.asarray(alpha, dtype=np.float64).reshape(-1), np.atleast_2d(np.asarray(v, dtype=np.float64))
    start, w = ie_shape(rn, r0, d, mutate)
    terms = {}
    for q in range(rn.shape[0]):
        av = alpha[q] * v[q]
        for m, cx, z, y, x in shape_nodes(start[q], n, mutate):
            t = av[cx] * w[q, m]
            if t != 0.0:
                terms.setdefault((z, y, x, cx), []).append(t)
    shape = (n[2], n[1], n[0], 3)
    J, asum, count = np.zeros(shape), np.zeros(shape), np.zeros(shape, dtype=np.int64)
    for key, ts in terms.items():
        J[key] = math.fsum(ts)
        asum[key] = math.fsum(abs(t) for t in ts)
        count[key] = len(ts)
    return J, count, asum


# ---- the edge list of tests/test_eccapfim_ref.py (restatement against oracle) and tests/test_gpu_eccapfim.py (device
# against restatement)

GRIDS = {
    "general": ((9, 8, 7), (0.5, 0.4, 0.3)),
    "pow2": ((8, 8, 8), (0.5, 0.25, 0.5)),       # x / d is exact: ties are ties
    "fold325": ((3, 2, 5), (0.5, 0.4, 0.25)),    # the 3-node and the up-to-4-node stencils fold onto themselves
    "fold2232": ((2, 2, 32), (0.5, 0.4, 0.25)),  # the reference's shipped quasi-1D box
}
DT = 0.7


def tie_moves(D):
    """(rn, r0) in dyadic coordinates, for power-of-two spacings D: every product below is exact, so each tie is one.
    From cell centres on both sides of the origin: half-cell moves in every sign pattern (end points on faces, edges and
    corners of the cell, among them the ties the reference's ladder does not survive), whole-cell moves in every sign
    pattern of (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1) and of the single axes (crossing parameters tie on both
    sides), and, per axis, short segments whose midpoint lies on a half-integer (the tie of the segment shape's round) or on
    an integer (the tie of the midpoint shape's round(p - 1.5)), in both directions."""
    D = np.array(D, dtype=np.float64)
    r0, rn = [], []
    patterns = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]
    for centre in ((2.0, 3.0, 4.0), (-3.0, -2.0, -1.0)):
        c0 = np.array(centre)
        for p in patterns:
            for length in (0.5, 1.0):
                r0.append(c0)
                rn.append(c0 + length * np.array(p))
            # an end point on a face, from a point off the centre
            if sum(abs(v) for v in p) == 1:
                off = np.array([0.125, -0.25, 0.0625])
                r0.append(c0 + off)
                rn.append(np.where(np.array(p) != 0, c0 + 0.5 * np.array(p), c0 - off))
        for axis in range(3):
            for tie in (0.5, 0.0):
                a, b = c0 + np.array([0.125, -0.125, 0.25]), c0 + np.array([-0.0625, 0.25, 0.125])
                a[axis], b[axis] = c0[axis] + tie - 0.25, c0[axis] + tie + 0.25
                r0 += [a, b]
                rn += [b, a]
    return np.array(rn) * D, np.array(r0) * D


def degenerate_moves(rng, N, D, each=24):
    """(rn, r0): zero-length moves, moves along one axis and in one coordinate plane (up to 2.5 cells), moves inside one
    cell; start points anywhere in [-L, 2 L)"""
    N, D = np.array(N), np.array(D, dtype=np.float64)
    r0s, rns = [], []

    def starts():
        return (rng.random((each, 3)) * 3 - 1) * (N * D)

    r0 = starts()
    r0s.append(r0)
    rns.append(r0.copy())
    for keep in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):
        r0 = starts()
        r0s.append(r0)
        rns.append(r0 + (rng.random((each, 3)) * 2 - 1) * 2.5 * D * np.array(keep))
    cells = np.floor(starts() / D)
    r0s.append((cells + (rng.random((each, 3)) - 0.5) * 0.9) * D)
    rns.append((cells + (rng.random((each, 3)) - 0.5) * 0.9) * D)
    return np.vstack(rns), np.vstack(r0s)


def long_moves(rng, n, N, D, cells=6.6):
    """(rn, r0): moves of up to `cells` cells along every axis (L1 distances up to 3 * cells)"""
    N, D = np.array(N), np.array(D, dtype=np.float64)
    r0 = rng.random((n, 3)) * (N * D)
    return r0 + (rng.random((n, 3)) * 2 - 1) * cells * D, r0


def capped_move(D):
    """(rn, r0) of one move of 30 + 25 + 20 = 75 crossings"""
    D = np.array(D, dtype=np.float64)
    r0 = np.array([[0.3, 0.1, 0.2]]) * D
    return r0 + np.array([[30.0, -25.0, 20.0]]) * D, r0


def fields(rng, N):
    """random E and B [nz][ny][nx][3]"""
    shape = (N[2], N[1], N[0], 3)
    return rng.normal(0, 1, shape), rng.normal(0, 1, shape)


def fold_positions(r, N, D):
    """positions folded into [0, L)"""
    L = np.array(N) * np.array(D, dtype=np.float64)
    r = np.mod(r, L)
    r[r >= L] = 0.0
    return r
