"""Binary Coulomb collisions (Takizuka and Abe, J. Comput. Phys. 25, 205, 1977) restated in numpy float64: the second
statement of include/xpic_hip.h: xpic_collide, which xpic_amd/csrc/collide.hip is held to.  An extension: the reference has
no collision operator.  The streams are this build's splitmix / u01 (xpic_amd/csrc/device_common.h), stated again here as
tests/commands_ref.py states them for InjectParticles.

Everything that decides the pairing is integer arithmetic.  The floating-point expressions are written in the kernel's
order and rounded operation by operation (the kernel is compiled without contraction); log, cos and sin come from another
library than the device's and may differ in the last place.

The pairs of a call are laid out in `rounds`: the pairs of one round touch every record at most once and are collided
together (vectorised); the rounds follow each other, which is the order the definition prescribes for the odd cell's
triple and for the meetings of one record of the short side."""
import numpy as np

M64 = (1 << 64) - 1
_G = 0x9E3779B97F4A7C15
_C_STEP = 0xD1342543DE82EF95
_C_SORTS = 0x9FB21C651E98DF25
_C_CELL = 0xD6E8FEB86659FD93
_C_TAG = 0xA0761D6478BD642F
_C_ITEM = 0x2545F4914F6CDD1D
TAG_PERM_A, TAG_PERM_B, TAG_PAIRS = 0, 1, 2


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def _splitmix(x):
    """(new state, output) of one splitmix64 step on an array of states"""
    with np.errstate(over="ignore"):
        x = _u64(x) + np.uint64(_G)
        z = x.copy()
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x, z ^ (z >> np.uint64(31))


def _u01(st):
    st, z = _splitmix(st)
    return st, ((z >> np.uint64(11)).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


def _splitmix_int(x):
    st, out = _splitmix(np.array([x & M64], dtype=np.uint64))
    return int(st[0]), int(out[0])


def call_key(seed, step, ia, ib):
    """the stream of (seed, step, sort_a, sort_b): inject_particles' key of (seed, step), then the two sorts"""
    k, _ = _splitmix_int(seed)
    k ^= (step * _C_STEP) & M64
    _, k = _splitmix_int(k)
    k ^= ((((ia & 0xFFFFFFFF) << 32) | (ib & 0xFFFFFFFF)) * _C_SORTS) & M64
    return _splitmix_int(k)[1]


def cell_keys(call, gcell):
    with np.errstate(over="ignore"):
        return _splitmix(np.uint64(call) ^ (_u64(gcell) * np.uint64(_C_CELL)))[1]


def sub_keys(ck, tag):
    return _splitmix(_u64(ck) ^ np.uint64(((tag + 1) * _C_TAG) & M64))[1]


def item_states(sub, i):
    with np.errstate(over="ignore"):
        return _u64(sub) + _u64(i) * np.uint64(_C_ITEM)


def item_keys(sub, i):
    return _splitmix(item_states(sub, i))[1]


def global_cells(ncell_local, n, z0=0):
    """GLOBAL index ((z0 + cz) ny + cy) nx + cx of every local cell"""
    c = np.arange(ncell_local, dtype=np.int64)
    return c + np.int64(z0) * n[1] * n[0]  # (local cell = (cz ny + cy) nx + cx)


class Layout:
    """the cell-sorted records of one sort: counts, starts and the permutation of every cell.  perm[start[c] + r] is the
    (global) index of the record of rank r in cell c, records ordered by (key, i)."""

    def __init__(self, cells, ncell, ck, tag):
        cells = np.asarray(cells, dtype=np.int64)
        assert np.all(np.diff(cells) >= 0), "the records must be cell-sorted"
        self.count = np.bincount(cells, minlength=ncell).astype(np.int64)
        self.start = np.concatenate([[0], np.cumsum(self.count)]).astype(np.int64)
        i = np.arange(len(cells), dtype=np.int64) - self.start[cells]
        keys = item_keys(sub_keys(ck, tag)[cells], i) if len(cells) else np.zeros(0, dtype=np.uint64)
        self.perm = np.lexsort((i, keys, cells))
        self.cells = cells
        self.rank = i  # (of position s in the sorted order: s - start[cell]; the same array)


def plan_intra(lay):
    """rounds of (first record, second record, pair index p, cell, dt factor)"""
    N = lay.count[lay.cells]            # population of the cell of sorted position s
    r = lay.rank
    first = np.where(N % 2 == 1, 3, 0)
    lead = (N >= 2) & (r >= first) & ((r - first) % 2 == 0) & (r + 1 < N)
    s = np.nonzero(lead)[0]
    rounds = [(lay.perm[s], lay.perm[s + 1], (first[s] + (r[s] - first[s]) // 2), lay.cells[s], np.ones(len(s)))]
    t = np.nonzero((N % 2 == 1) & (N >= 3) & (r == 0))[0]  # the triple: (pi0, pi1), (pi1, pi2), (pi2, pi0), dt / 2 each
    half = np.full(len(t), 0.5)
    tri = [(lay.perm[t], lay.perm[t + 1], np.zeros(len(t), dtype=np.int64), lay.cells[t], half),
           (lay.perm[t + 1], lay.perm[t + 2], np.ones(len(t), dtype=np.int64), lay.cells[t], half),
           (lay.perm[t + 2], lay.perm[t], np.full(len(t), 2, dtype=np.int64), lay.cells[t], half)]
    # round 0: the regular pairs and the triples' first pair touch different records
    r0 = tuple(np.concatenate([a, b]) for a, b in zip(rounds[0], tri[0]))
    return [r0, tri[1], tri[2]]


def plan_inter(la, lb):
    """rounds of (a record, b record, pair index p = j, cell, dt factor 1): the long side's record of rank j meets the
    short side's of rank j mod N_short; round = j // N_short"""
    out = {}
    for long_, short, a_is_long in ((la, lb, True), (lb, la, False)):
        Nl, Ns = long_.count[long_.cells], short.count[long_.cells]
        # the short side is the call's b unless a has fewer records in the cell
        use = (Ns > 0) & ((Nl >= Ns) if a_is_long else (Nl > Ns))
        s = np.nonzero(use)[0]
        j = long_.rank[s]
        c = long_.cells[s]
        il = long_.perm[s]
        is_ = short.perm[short.start[c] + j % Ns[s]]
        rnd = j // Ns[s]
        for k in np.unique(rnd):
            m = rnd == k
            ia, ib = (il[m], is_[m]) if a_is_long else (is_[m], il[m])
            out.setdefault(int(k), []).append((ia, ib, j[m], c[m], np.ones(int(m.sum()))))
    return [tuple(np.concatenate(x) for x in zip(*out[k])) for k in sorted(out)]


def collide_pairs(va, vb, cdt, pairs_sub, p, fa, fb):
    """one collision of every pair (arrays): -> new va, new vb, collided (bool), sigma^2, delta"""
    ux, uy, uz = va[:, 0] - vb[:, 0], va[:, 1] - vb[:, 1], va[:, 2] - vb[:, 2]
    u = np.sqrt(ux * ux + uy * uy + uz * uz)
    ok = u != 0.0
    us = np.where(ok, u, 1.0)
    with np.errstate(over="ignore", divide="ignore"):
        s2 = cdt / (us * us * us)
    st = item_states(pairs_sub, p)
    st, u1 = _u01(st)
    st, u2 = _u01(st)
    st, u3 = _u01(st)
    delta = np.sqrt(s2) * np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    phi = 2.0 * np.pi * u3
    with np.errstate(over="ignore", invalid="ignore"):
        d2 = delta * delta
        back = ~(d2 <= 1e300)  # (sigma^2 or delta^2 at the end of the range: Theta = pi, the limit)
        sinT, omc = np.where(back, 0.0, 2.0 * delta / (1.0 + d2)), np.where(back, 2.0, 2.0 * d2 / (1.0 + d2))
    cp, sp = np.cos(phi), np.sin(phi)
    up = np.sqrt(ux * ux + uy * uy)
    axial = up == 0.0
    ups = np.where(axial, 1.0, up)
    dx = np.where(axial, u * sinT * cp, (ux / ups) * uz * sinT * cp - (uy / ups) * u * sinT * sp - ux * omc)
    dy = np.where(axial, u * sinT * sp, (uy / ups) * uz * sinT * cp + (ux / ups) * u * sinT * sp - uy * omc)
    dz = np.where(axial, -uz * omc, -up * sinT * cp - uz * omc)
    d = np.stack([dx, dy, dz], axis=1)
    na, nb = va + fa * d, vb - fb * d
    na[~ok], nb[~ok] = va[~ok], vb[~ok]
    return na, nb, ok, s2, delta


def collide(pts_a, cells_a, par_a, pts_b, cells_b, par_b, S, dt, seed, step, n, z0=0, nzl=None, sorts=(0, 0), trace=None):
    """xpic_collide on the cell-sorted records of sort a and sort b (the SAME arrays and sorts[0] == sorts[1]: the
    intra-species call).  pts: [N][6] records, cells: their local cells (Context.particles), par: (Np, n, q, m), n: the
    global grid, z0 / nzl: the slab -> (new velocities of a, new velocities of b, out4).  trace: a list that receives
    (a index, b index, cell, |u| before, sigma^2, delta, collided) of every round."""
    nzl = n[2] if nzl is None else nzl
    ncell = n[0] * n[1] * nzl
    intra = sorts[0] == sorts[1]
    (Npa, na_, qa, ma), (Npb, nb_, qb, mb) = par_a, par_b
    wa, wb = na_ / Npa, nb_ / Npb
    if wa != wb:
        raise ValueError("the two sorts must carry the same weight n / Np")
    va = np.array(np.asarray(pts_a, dtype=np.float64)[:, 3:6])
    vb = va if intra else np.array(np.asarray(pts_b, dtype=np.float64)[:, 3:6])
    out4 = np.zeros(4)
    if S == 0.0:
        return va, (va if intra else vb), out4
    mab = ma * mb / (ma + mb)
    c0 = S * (qa * qa) * (qb * qb) / (mab * mab)
    fa, fb = mab / ma, mab / mb
    ck = cell_keys(call_key(seed, step, sorts[0], sorts[1]), global_cells(ncell, n, z0))
    pairs_sub = sub_keys(ck, TAG_PAIRS)
    la = Layout(cells_a, ncell, ck, TAG_PERM_A)
    if intra:
        rounds = plan_intra(la)
        nL = wa * la.count.astype(np.float64)
    else:
        lb = Layout(cells_b, ncell, ck, TAG_PERM_B)
        rounds = plan_inter(la, lb)
        nL = wa * np.minimum(la.count, lb.count).astype(np.float64)
    cn = c0 * nL
    for ia, ib, p, c, f in rounds:
        if len(ia) == 0:
            continue
        cdt = cn[c] * np.where(f == 1.0, dt, 0.5 * dt)
        xa, xb, ok, s2, delta = collide_pairs(va[ia], vb[ib], cdt, pairs_sub[c], p, fa, fb)
        if trace is not None:
            d = va[ia] - vb[ib]
            trace.append((ia, ib, c, np.sqrt((d * d).sum(axis=1)), s2, delta, ok))
        va[ia] = xa
        vb[ib] = xb
        fin = ok & (s2 <= np.finfo(np.float64).max)  # (an overflowed sigma^2 is counted above 1, left out of the sum)
        out4 += [ok.sum(), (~ok).sum(), s2[fin].sum(), (s2[ok] > 1.0).sum()]
    return va, (va if intra else vb), out4
