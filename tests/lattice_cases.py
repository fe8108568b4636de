"""Lattice-aligned particle families: positions on cell faces and half-cell planes, moves of exactly 0, 1/4, 1/2 and 1 cell,
landings on the planes and crossings of the periodic edge -- the values at which the particle kernels branch (floor, round
half away from zero, the half-cell octant, the 4-node limit of Shape::shape, the periodic fold).  Plain numpy.

Everything is built in scaled coordinates u = r / d and scaled moves w = tau v / d, tau being the time over which the
kernel under test moves a particle (dt for basic_push and the ecsim first push, dt / 2 for the ecsimcorr pushes).  On the
exact grid (all spacings and tau powers of two) every u and w is a dyadic rational of a few bits (node and half-cell
planes, odd multiples of 1/1024 for the generic values), so r, tau v, (tau / 2) v and their sums are exact with or
without FMA contraction and "on the plane" is meant bit for bit.  The only exceptions are the classes that are one ulp off
a plane on purpose.  On the general grid the same u and w are multiplied by d (dy = 0.4 rounds: a tie there is an ulp
wide and the oracle decides its side).

A family pins one tie class on ONE axis (the other two axes carry generic values), so a failure names the class and the
axis.  The families `still`, `cross` and `overflow` span the three axes by their nature.
"""
import collections

import numpy as np

EXACT = ((12, 8, 8), (0.5, 0.5, 0.25))    # test_gpu_ecsim.GRID_P2FX: power-of-two spacings, nx % 4 == 0
GENERAL = ((12, 10, 8), (0.5, 0.4, 0.25))  # test_gpu_ecsim.GRID: dy is not dyadic
GRIDS = {"p2fx": EXACT, "general": GENERAL}

REPS = 10  # particles per (value of the class, value of the move): the generator's own floor is 8 per (class, axis, place)

# name: family, u / w: scaled positions and moves (N, 3), ties: the (axis, place, kind) the family is built to hit, with
# place in {"old", "mid", "new"} and kind in {"face", "half"} (a cell face, a half-cell plane), overflow: how many particles exceed the reference's 4-node box (Shape::shape)
Family = collections.namedtuple("Family", "name u w ties overflow")


def round_away(x):
    """std::round: halves away from zero (no x + 0.5, which rounds 0.49999999999999994 up)"""
    f, c = np.floor(x), np.ceil(x)
    return np.where(x >= 0, f + ((x - f) >= 0.5), c - ((c - x) >= 0.5))


def box_size(po, pn):
    """Shape::setup(old, new) (shape.cpp:12-28, 43-54): nodes per axis of the box [round(min - 1.5), floor(max + 1.5) + 1)"""
    return np.floor(np.maximum(po, pn) + 1.5) + 1 - round_away(np.minimum(po, pn) - 1.5)


def on_plane(x, kind=None):
    """scaled coordinate exactly on a cell face ("face"), on a half-cell plane ("half"), or on either"""
    face, half = x == np.floor(x), x - 0.5 == np.floor(x - 0.5)
    return {"face": face, "half": half, None: face | half}[kind]


def cells_of(n, a):
    """cells 0, 1, an interior one and n - 1 of axis a: round(u - 1.5) changes sign next to the origin, the stencil wraps
    at both ends"""
    return np.array([0, 1, n[a] // 2, n[a] - 1], dtype=np.float64)


class _Gen:
    def __init__(self, n, seed):
        self.n = n
        self.rng = np.random.default_rng(seed)

    def generic_u(self, count, a):
        """inside a random cell, at an odd multiple of 1/1024: never on a plane, nor a quarter cell"""
        return self.rng.integers(0, self.n[a], count) + (2 * self.rng.integers(0, 512, count) + 1) / 1024.0

    def generic_w(self, count):
        """odd multiples of 1/1024 below 0.3 cell: half of it is no plane either"""
        return (2 * self.rng.integers(-150, 150, count) + 1) / 1024.0

    def family(self, name, a, ua, wa, ties):
        """values (ua, wa) on axis a, generic ones on the other two"""
        cnt = len(ua)
        u, w = np.empty((cnt, 3)), np.empty((cnt, 3))
        for b in range(3):
            u[:, b] = ua if b == a else self.generic_u(cnt, b)
            w[:, b] = wa if b == a else self.generic_w(cnt)
        return Family(name, u, w, tuple((a, p, kind) for p, kind in ties), 0)


def _product(us, ws):
    us, ws = np.asarray(us, dtype=np.float64), np.asarray(ws, dtype=np.float64)
    U, W = np.meshgrid(np.tile(us, REPS), ws, indexing="ij")
    return U.ravel(), W.ravel()


def _keep(f, ok, n, d):
    """drops the (start, move) pairs that the class cannot hold: boxes of 5 nodes (they belong to `overflow`: an integer
    start in the cells next to the origin rounds its box start down; on the general grid r / d decides, an ulp either
    side of the plane) and starts outside the box"""
    d = np.array(d, dtype=np.float64)
    inside = np.all((f.u >= 0) & (f.u < np.array(n, dtype=np.float64)), axis=1)
    r, h = f.u * d, f.w * d / 2
    for new in (r + 2 * h, (r + h) + h):  # one move of tau, or basic_push's two halves
        ok = ok & np.all(box_size(r / d, new / d) <= 4, axis=1)
    ok = ok & inside
    return f._replace(u=f.u[ok], w=f.w[ok])


def families(n, d, seed=0):
    """dict name -> Family on a box of n cells of size d"""
    G = _Gen(n, seed)
    ulp = np.finfo(np.float64).eps
    out = collections.OrderedDict()
    everything = lambda f: np.ones(len(f.u), dtype=bool)

    def put(f, ok=everything):
        f = _keep(f, ok(f), n, d)
        assert len(f.u) <= 400, (f.name, len(f.u))
        out[f.name] = f

    for a, ax in enumerate("xyz"):
        k = cells_of(n, a)
        below_n = np.nextafter(float(n[a]), 0.0)
        # ---- coordinate classes with generic moves: what the gathers, the assembly and the densities see
        # (above 0 the step is the ulp of a cell, not the smallest subnormal)
        near = np.concatenate([np.nextafter(k[1:], -np.inf), np.where(k == 0, ulp, np.nextafter(k, np.inf)), np.nextafter(k + 0.5, -np.inf),
                               np.nextafter(k + 0.5, np.inf), [below_n]])            # one ulp off each plane, and below n
        for name, vals, ties in (("node_", k, [("old", "face")]), ("half_", k + 0.5, [("old", "half")]), ("near_", near, [])):
            ua = np.tile(vals, REPS)                                                 # (node_: k = 0 is exactly 0)
            put(G.family(name + ax, a, ua, G.generic_w(len(ua)), ties=ties))
        # ---- move classes from the planes
        put(G.family("quarter_" + ax, a, *_product(np.concatenate([k, k + 0.5]), [0.25, -0.25]), ties=[("old", "face"), ("old", "half")]))
        # +-1/2 from a node lands on a half-cell plane, from a half-cell plane on a face, from a quarter cell it passes a
        # plane at mid-step; one ulp around 1/2 is the two sides of the kernels' fast / slow threshold
        half = [0.5, -0.5, 0.5 * (1 + ulp), 0.5 * (1 - ulp), -0.5 * (1 + ulp), -0.5 * (1 - ulp)]
        put(G.family("halfmove_" + ax, a, *_product(np.concatenate([k, k + 0.5]), half),
                     ties=[(p, kind) for p in ("old", "new") for kind in ("face", "half")]))
        put(G.family("halfmove_mid_" + ax, a, *_product(np.concatenate([k + 0.25, k + 0.75]), [0.5, -0.5]),
                     ties=[("mid", "face"), ("mid", "half")]))
        # +-1 from a node: the reference's limit, a box of exactly 4 nodes (5 next to the origin: dropped by _keep); the
        # mid-step position is on a half-cell plane
        put(G.family("unit_" + ax, a, *_product(np.arange(n[a], dtype=np.float64), [1.0, -1.0]),
                     ties=[("old", "face"), ("mid", "half"), ("new", "face")]),
            ok=lambda f: box_size(f.u, f.u + f.w)[:, a] == 4)
        # ---- landings from generic (dyadic) starts: on a face, on a half-cell plane, on 0 and on L from inside
        fr = np.array([1, 3, 5, 7]) / 8.0
        st = np.concatenate([c + fr for c in k])
        lands = []
        for target in (0.0, 0.5, 1.0):  # the planes of the start's own cell, below and above
            ua = np.tile(st, REPS // 2)
            lands.append((ua, np.floor(ua) + target - ua))
        ua = np.concatenate([l[0] for l in lands])
        wa = np.concatenate([l[1] for l in lands])
        put(G.family("land_" + ax, a, ua, wa, ties=[("new", "face"), ("new", "half")]), ok=lambda f: f.w[:, a] != 0.0)
        # the box edges: onto 0 from cell 0 (kept in cell 0), onto L from cell n - 1 (s == L is not folded: outside), and
        # past them by an eighth of a cell (folded once)
        ua = np.tile(np.concatenate([fr, n[a] - 1 + fr]), REPS)
        wa = np.where(ua < 1, -ua, n[a] - ua)
        put(G.family("edge_" + ax, a, np.concatenate([ua, ua]), np.concatenate([wa, wa + np.sign(wa) / 8.0]),
                     ties=[("new", "face")]))
        # ---- the mid-step position u + w / 2 on the planes and one ulp either side of them, moves below half a cell (a
        # field's kick on top still fits the 4-node box): where basic_push gathers.  Kept where u and u + w / 2 are exact.
        T, W = np.meshgrid(np.tile(np.concatenate([k, k + 0.5, near[:-1]]), 3), [0.25, -0.25, 0.375, -0.375], indexing="ij")
        T, W = T.ravel(), W.ravel()
        put(G.family("mid_" + ax, a, T - W / 2, W, ties=[("mid", "face"), ("mid", "half")]),
            ok=lambda f: f.u[:, a] + f.w[:, a] / 2 == T)

    # ---- no move at all, from every coordinate class on every axis at once
    cnt = 24 * REPS
    u = np.empty((cnt, 3))
    for a in range(3):
        k = cells_of(n, a)
        vals = np.concatenate([k, k + 0.5, np.nextafter(k + 0.5, np.inf), [np.nextafter(float(n[a]), 0.0)], G.generic_u(3, a)])
        u[:, a] = G.rng.choice(vals, cnt)
        u[:16, a] = np.tile(np.concatenate([k, k + 0.5]), 2)  # (and the planes of all three axes at once)
    out["still"] = Family("still", u, np.zeros((cnt, 3)), tuple((a, p, kind) for a in range(3) for p in ("old", "mid", "new") for kind in ("face", "half")), 0)

    # ---- across the periodic edge in one, two and all three axes at once
    us, ws = [], []
    for mask in range(1, 8):
        for side in (0, 1):
            cnt = REPS
            u, w = np.empty((cnt, 3)), np.empty((cnt, 3))
            for a in range(3):
                if mask >> a & 1:
                    f8 = G.rng.choice([1, 2, 3, 4], cnt) / 8.0  # at most half a cell from the edge, the edge itself included
                    f8[0] = 0.0
                    u[:, a] = f8 if side == 0 else n[a] - 0.125 - f8
                    w[:, a] = (-1 if side == 0 else 1) * (f8 + G.rng.choice([1, 2, 3], cnt) / 8.0)
                else:
                    u[:, a], w[:, a] = G.generic_u(cnt, a), G.generic_w(cnt)
            us.append(u)
            ws.append(w)
    out["cross"] = _keep(Family("cross", np.vstack(us), np.vstack(ws), (), 0), np.ones(14 * REPS, dtype=bool), n, d)

    # ---- the reference's overflow: ONE particle from k + 1/2 by exactly one cell along x (5 nodes) among generic ones
    cnt = 12 * REPS
    u = np.stack([G.generic_u(cnt, a) for a in range(3)], axis=1)
    w = np.stack([G.generic_w(cnt) for a in range(3)], axis=1)
    u[cnt // 2, 0], w[cnt // 2, 0] = n[0] // 2 + 0.5, 1.0
    out["overflow"] = Family("overflow", u, w, (), 1)
    return out


def moves_twice(fam, n, d):
    """mask of the particles whose SECOND move by the same w -- from where the first one left them, folded into the box as
    the re-binning does -- fits the reference's 4-node box too and that the re-binning keeps (s == L leaves): what a
    first push, a re-binning and a second push in zero fields can take"""
    d = np.array(d, dtype=np.float64)
    L = np.array(n, dtype=np.float64) * d
    s = fam.u * d + fam.w * d
    r = np.where(s < 0, L - (0.0 - s), np.where(s > L, 0.0 + (s - L), s))
    stays = np.all(np.floor(r / d) < np.array(n), axis=1)
    return stays & np.all(box_size(r / d, (r + fam.w * d) / d) <= 4, axis=1)


def points(fam, d, tau):
    """(N, 6) records r = u d, v = w d / tau"""
    d = np.array(d, dtype=np.float64)
    return np.hstack([fam.u * d, fam.w * d / tau])


def scaled(pts, d, tau, place):
    """r / d at the old, mid-step or new position of a move over tau, with the kernels' own operations"""
    step = {"old": 0.0, "mid": tau / 2.0, "new": tau}[place]
    return (pts[:, :3] + pts[:, 3:] * step) / np.array(d, dtype=np.float64)


def storage_cell(pts, n, d):
    """FLOOR_STEP cell of every record (utils.h), -1 outside the box"""
    c = np.floor(pts[:, :3] / np.array(d, dtype=np.float64)).astype(np.int64)
    inside = np.all((c >= 0) & (c < np.array(n)), axis=1)
    return np.where(inside, (c[:, 2] * n[1] + c[:, 1]) * n[0] + c[:, 0], -1)


def quiet_start(n, d, dt, sign=+1):
    """One particle on every node and one in every cell centre, all drifting by exactly a quarter cell per step along the
    three axes: on a plane again every other step, across the periodic edge within the first."""
    idx = np.stack(np.meshgrid(*[np.arange(m, dtype=np.float64) for m in n], indexing="ij"), axis=-1).reshape(-1, 3)
    u = np.vstack([idx, idx + 0.5])
    w = np.full(u.shape, 0.25 * sign)
    return points(Family("quiet", u, w, (), 0), d, dt)
