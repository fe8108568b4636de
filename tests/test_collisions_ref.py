"""The numpy restatement of the binary collisions (tests/collisions_ref.py) against the properties the definition
(include/xpic_hip.h: xpic_collide) promises: the pairing rules, the conservation laws of one collision and of a call, the
distribution of the scattering variable, and the skipped pair.  No GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import collisions_ref as R  # noqa: E402

POPS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 64, 65, 200]


def _layout(pops, tag=R.TAG_PERM_A, seed=3, step=5):
    n = (len(pops), 1, 1)
    cells = np.repeat(np.arange(len(pops)), pops)
    ck = R.cell_keys(R.call_key(seed, step, 0, 0), R.global_cells(len(pops), n))
    return R.Layout(cells, len(pops), ck, tag), ck


def test_permutation_orders_by_key_then_index():
    lay, ck = _layout(POPS)
    sub = R.sub_keys(ck, R.TAG_PERM_A)
    for c, N in enumerate(POPS):
        keys = [int(k) for k in R.item_keys(np.full(N, sub[c]), np.arange(N))]
        want = sorted(range(N), key=lambda i: (keys[i], i))
        got = lay.perm[lay.start[c]:lay.start[c + 1]] - lay.start[c]
        assert list(got) == want
    assert len(set(int(k) for k in sub)) == len(POPS)  # (every cell has its own stream)


def test_intra_pairing_rules():
    lay, _ = _layout(POPS)
    rounds = R.plan_intra(lay)
    for c, N in enumerate(POPS):
        pi = lay.perm[lay.start[c]:lay.start[c + 1]]
        seq = []  # the cell's pairs in execution order
        for ia, ib, p, cc, f in rounds:
            m = cc == c
            seq.append(sorted(zip(p[m], ia[m], ib[m], f[m])))
        pairs = [x for rnd in seq for x in rnd]
        if N < 2:
            assert pairs == []
            continue
        meets = np.bincount(np.array([[a, b] for _, a, b, _ in pairs]).ravel() - lay.start[c], minlength=N)
        if N % 2 == 0:
            assert np.all(meets == 1) and all(f == 1.0 for *_, f in pairs)
            assert sorted((p, a, b) for p, a, b, _ in pairs) == [(k, pi[2 * k], pi[2 * k + 1]) for k in range(N // 2)]
        else:
            # the triple, one pair after the other (one per round), each with half the step; then (pi3, pi4), ...
            tri = [[x for x in rnd if x[3] == 0.5] for rnd in seq]
            assert [[(p, a, b) for p, a, b, _ in t] for t in tri] == [[(0, pi[0], pi[1])], [(1, pi[1], pi[2])], [(2, pi[2], pi[0])]]
            rest = sorted((p, a, b) for p, a, b, f in pairs if f == 1.0)
            assert rest == [(3 + k, pi[3 + 2 * k], pi[4 + 2 * k]) for k in range((N - 3) // 2)]
            want = np.ones(N, dtype=np.int64)
            want[pi[:3] - lay.start[c]] = 2
            assert np.array_equal(meets, want)


def test_inter_pairing_rules():
    counts = [(5, 5), (7, 3), (3, 7), (6, 0), (1, 64), (0, 4)]
    la, ck = _layout([a for a, _ in counts], R.TAG_PERM_A)
    lb = R.Layout(np.repeat(np.arange(len(counts)), [b for _, b in counts]), len(counts), ck, R.TAG_PERM_B)
    rounds = R.plan_inter(la, lb)
    for c, (Na, Nb) in enumerate(counts):
        pa, pb = la.perm[la.start[c]:la.start[c + 1]], lb.perm[lb.start[c]:lb.start[c + 1]]
        seq = []
        for ia, ib, p, cc, f in rounds:
            m = cc == c
            assert np.all(f[m] == 1.0)
            seq.append(sorted(zip(p[m], ia[m], ib[m])))
        pairs = [x for rnd in seq for x in rnd]
        if Na == 0 or Nb == 0:
            assert pairs == []
            continue
        a_long = Na >= Nb  # the short side is b unless a has fewer records
        Nl, Ns = max(Na, Nb), min(Na, Nb)
        pl, ps = (pa, pb) if a_long else (pb, pa)
        want = [(j, pl[j], ps[j % Ns]) for j in range(Nl)]
        got = [(j, a, b) if a_long else (j, b, a) for j, a, b in pairs]
        assert sorted(got) == want  # every record of the long side meets exactly once, p = j
        # the meetings of one short record: one per round, in increasing j
        for rnd, k in zip(seq, range(len(seq))):
            assert [j for j, _, _ in rnd] == list(range(k * Ns, min((k + 1) * Ns, Nl)))


def _random_pairs(N, seed):
    rng = np.random.default_rng(seed)
    va, vb = rng.normal(0, 0.1, (N, 3)), rng.normal(0, 0.05, (N, 3))
    # relative velocities along +z and -z (u_perp == 0), and a pair at rest relative to each other
    vb[:8, :2] = va[:8, :2]
    vb[:4, 2] = va[:4, 2] - 0.3
    vb[4:8, 2] = va[4:8, 2] + 0.3
    vb[8] = va[8]
    return va, vb


def test_one_collision_keeps_speed_momentum_energy():
    N = 4096
    va, vb = _random_pairs(N, 1)
    ma, mb = 1.0, 7.5
    mab = ma * mb / (ma + mb)
    for cdt in (1e-6, 1e-3, 1.0):  # small angles, and sigma^2 far above 1
        xa, xb, ok, s2, delta = R.collide_pairs(va, vb, np.full(N, cdt), np.full(N, 99, dtype=np.uint64), np.arange(N),
                                                mab / ma, mab / mb)
        assert not ok[8] and ok.sum() == N - 1
        assert np.array_equal(xa[8], va[8]) and np.array_equal(xb[8], vb[8])
        u0, u1 = np.linalg.norm(va - vb, axis=1), np.linalg.norm(xa - xb, axis=1)
        assert np.all(np.abs(u1 - u0) <= 1e-14 * u0)
        assert np.any(xa != va)
        p0, p1 = ma * va + mb * vb, ma * xa + mb * xb
        scale = ma * np.linalg.norm(va, axis=1) + mb * np.linalg.norm(vb, axis=1)
        assert np.all(np.abs(p1 - p0).max(axis=1) <= 1e-13 * scale)
        e0 = 0.5 * ma * (va * va).sum(axis=1) + 0.5 * mb * (vb * vb).sum(axis=1)
        e1 = 0.5 * ma * (xa * xa).sum(axis=1) + 0.5 * mb * (xb * xb).sum(axis=1)
        assert np.all(np.abs(e1 - e0) <= 1e-13 * e0)


def _cells_case(seed, n=(4, 3, 5), pops=None):
    rng = np.random.default_rng(seed)
    ncell = n[0] * n[1] * n[2]
    pops = rng.integers(0, 12, ncell) if pops is None else pops
    cells = np.repeat(np.arange(ncell), pops)
    pts = np.zeros((len(cells), 6))
    pts[:, 3:] = rng.normal(0, 0.1, (len(cells), 3)) * np.array([1.0, 1.0, 0.5])
    return n, cells, pts


def _per_cell(cells, v, m, ncell):
    mom = np.stack([np.bincount(cells, m * v[:, k], ncell) for k in range(3)], axis=1)
    mabs = np.bincount(cells, m * np.linalg.norm(v, axis=1), ncell)
    en = np.bincount(cells, 0.5 * m * (v * v).sum(axis=1), ncell)
    return mom, mabs, en


@pytest.mark.parametrize("kind", ["intra", "inter"])
def test_call_conserves_momentum_and_energy_per_cell(kind):
    pa, pb = (8, 1.0, -1.0, 1.0), (8, 1.0, 2.0, 7.5)
    n, ca, A = _cells_case(11)
    _, cb, B = _cells_case(12)
    ncell = n[0] * n[1] * n[2]
    if kind == "intra":
        va, _, out4 = R.collide(A, ca, pa, A, ca, pa, 2e-3, 0.7, 5, 9, n, sorts=(0, 0))
        m0, s0, e0 = _per_cell(ca, A[:, 3:], pa[3], ncell)
        m1, _, e1 = _per_cell(ca, va, pa[3], ncell)
        pops = np.bincount(ca, minlength=ncell)
        assert out4[0] == sum(N // 2 if N % 2 == 0 else (N - 3) // 2 + 3 for N in pops if N >= 2)
    else:
        va, vb, out4 = R.collide(A, ca, pa, B, cb, pb, 2e-3, 0.7, 5, 9, n, sorts=(0, 1))
        ma, sa, ea = _per_cell(ca, A[:, 3:], pa[3], ncell)
        mb, sb, eb = _per_cell(cb, B[:, 3:], pb[3], ncell)
        m0, s0, e0 = ma + mb, sa + sb, ea + eb
        m1 = _per_cell(ca, va, pa[3], ncell)[0] + _per_cell(cb, vb, pb[3], ncell)[0]
        e1 = _per_cell(ca, va, pa[3], ncell)[2] + _per_cell(cb, vb, pb[3], ncell)[2]
        na, nb = np.bincount(ca, minlength=ncell), np.bincount(cb, minlength=ncell)
        assert out4[0] == np.where((na > 0) & (nb > 0), np.maximum(na, nb), 0).sum()
        assert not np.array_equal(vb, B[:, 3:])
    assert out4[1] == 0 and out4[2] > 0
    assert not np.array_equal(va, A[:, 3:])
    assert np.all(np.abs(m1 - m0).max(axis=1) <= 1e-13 * s0)
    assert np.all(np.abs(e1 - e0) <= 1e-13 * e0)


def test_scattering_variable_has_unit_variance():
    """delta / sigma over 2^18 pairs: the sample variance of a standard normal within 3 standard errors of 1 (the standard
    error of the variance of N normal draws is sqrt(2 / N))"""
    N = 1 << 18
    va, vb = _random_pairs(N, 2)
    vb[8] += 0.01
    _, _, ok, s2, delta = R.collide_pairs(va, vb, np.full(N, 1e-4), np.full(N, 12345, dtype=np.uint64), np.arange(N), 0.5, 0.5)
    assert ok.all()
    g = delta / np.sqrt(s2)
    assert abs(g.var() - 1.0) <= 3.0 * np.sqrt(2.0 / N), g.var()
    assert abs(g.mean()) <= 3.0 / np.sqrt(N), g.mean()


def test_slowest_pairs_scatter_by_pi():
    """|u| so small that u^3 underflows (sigma^2 = inf): Theta = pi, u -> -u; at the edge of the range (sigma^2 finite,
    delta^2 may overflow) nothing is NaN and |u| is kept"""
    N = 64
    va = np.zeros((N, 3))
    vb = np.zeros((N, 3))
    vb[:, 0], vb[:, 1], vb[:, 2] = -1e-110, -2e-110, 1e-110
    vb[1] = (0.0, 0.0, -3e-120)
    vb[2:] = np.array([1.0, -1.0, 1.0]) * 1.2e-104  # (u^3 is denormal, sigma^2 ~ 1e308)
    with np.errstate(all="ignore"):
        xa, xb, ok, s2, delta = R.collide_pairs(va, vb, np.full(N, 1e-3), np.full(N, 7, dtype=np.uint64), np.arange(N), 0.5, 0.5)
    assert ok.all() and np.isinf(s2[:2]).all() and np.isfinite(s2[2:]).all() and (np.abs(delta[2:]) > 1e154).any()
    assert np.isfinite(xa).all() and np.isfinite(xb).all()
    assert np.allclose((xa - xb)[:2], -(va - vb)[:2], rtol=1e-12, atol=0)
    u0, u1 = np.linalg.norm(va - vb, axis=1), np.linalg.norm(xa - xb, axis=1)
    assert np.all(np.abs(u1 - u0) <= 1e-14 * u0)


def test_identical_velocities_are_skipped():
    n = (2, 1, 1)
    pts = np.zeros((2, 6))
    pts[:, 3:] = (0.1, -0.2, 0.3)
    cells = np.array([1, 1])
    par = (8, 1.0, -1.0, 1.0)
    va, _, out4 = R.collide(pts, cells, par, pts, cells, par, 1e-2, 0.7, 1, 0, n, sorts=(0, 0))
    assert list(out4) == [0, 1, 0, 0]
    assert va.tobytes() == pts[:, 3:].tobytes()


def test_zero_strength_and_unequal_weights():
    n, cells, pts = _cells_case(4)
    par = (8, 1.0, -1.0, 1.0)
    va, _, out4 = R.collide(pts, cells, par, pts, cells, par, 0.0, 0.7, 1, 0, n, sorts=(0, 0))
    assert va.tobytes() == pts[:, 3:].tobytes() and not out4.any()
    with pytest.raises(ValueError):
        R.collide(pts, cells, par, pts, cells, (5, 0.6, 2.0, 7.5), 1e-3, 0.7, 1, 0, n, sorts=(0, 1))


def test_slabs_draw_the_single_box_numbers():
    """the stream key uses the GLOBAL cell: a slab (z0, nzl) of the box gives the records of its cells the box's result"""
    n, cells, pts = _cells_case(6, n=(3, 2, 6))
    par = (8, 1.0, -1.0, 1.0)
    whole, _, _ = R.collide(pts, cells, par, pts, cells, par, 1e-3, 0.7, 2, 4, n, sorts=(0, 0))
    plane = n[0] * n[1]
    for z0 in (0, 2, 4):
        m = (cells >= z0 * plane) & (cells < (z0 + 2) * plane)
        part, _, _ = R.collide(pts[m], cells[m] - z0 * plane, par, pts[m], cells[m] - z0 * plane, par, 1e-3, 0.7, 2, 4, n,
                               z0=z0, nzl=2, sorts=(0, 0))
        assert part.tobytes() == whole[m].tobytes()
