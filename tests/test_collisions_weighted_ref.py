"""The numpy restatement of the unequal-weight binary collisions (tests/collisions_weighted_ref.py) against what the
definition (include/xpic_hip.h: xpic_collide_weighted) promises: xpic_collide's bits at equal weights, the update rule of
every meeting, the share of heavier-side updates, weighted momentum and energy in expectation, the relaxation rate of a
temperature difference whichever side carries the heavy weight, and the slabs against the box.  No GPU."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import collisions_ref as R  # noqa: E402
import collisions_weighted_ref as W  # noqa: E402

COUNTS = [(5, 5), (7, 3), (3, 7), (6, 0), (1, 64), (0, 4)]  # test_collisions_ref.py: test_inter_pairing_rules' cells
S, DT = 2e-3, 0.7


def _case(counts, seed, n=None):
    """cell-sorted records of two sorts with counts[c] = (Na, Nb) in cell c"""
    n = (len(counts), 1, 1) if n is None else n
    rng = np.random.default_rng(seed)
    out = []
    for k in range(2):
        cells = np.repeat(np.arange(len(counts)), [c[k] for c in counts])
        pts = np.zeros((len(cells), 6))
        pts[:, 3:] = rng.normal(0, 0.1 / (k + 1), (len(cells), 3))
        out.append((pts, cells))
    return n, out[0], out[1]


def test_equal_weights_give_xpic_collide_bit_for_bit():
    pa, pb = (8, 1.0, -1.0, 1.0), (4, 0.5, 2.0, 7.5)  # equal weights 1/8, different Np, n, q and m
    n, (A, ca), (B, cb) = _case(COUNTS, 1)
    for sorts in ((0, 1), (1, 0)):
        va, vb, out4 = R.collide(A, ca, pa, B, cb, pb, S, DT, 9, 4, n, sorts=sorts)
        xa, xb, out6 = W.collide_weighted(A, ca, pa, B, cb, pb, S, DT, 9, 4, n, sorts=sorts)
        assert xa.tobytes() == va.tobytes() and xb.tobytes() == vb.tobytes()
        assert out6[:4].tobytes() == out4.tobytes()
        assert out6[4] == out6[0] > 0 and out6[5] == 0
        assert not np.array_equal(va, A[:, 3:])
    # the same sort twice forwards to xpic_collide's intra-species path
    va, _, out4 = R.collide(A, ca, pa, A, ca, pa, S, DT, 9, 4, n, sorts=(0, 0))
    xa, _, out6 = W.collide_weighted(A, ca, pa, A, ca, pa, S, DT, 9, 4, n, sorts=(0, 0))
    assert xa.tobytes() == va.tobytes() and out6.tolist() == out4.tolist() + [out4[0], 0.0]


@pytest.mark.parametrize("par", [((8, 1.0, -1.0, 1.0), (4, 1.0, 2.0, 7.5)), ((8, 1.0, -1.0, 1.0), (8, 0.125, 2.0, 7.5)),
                                 ((4, 1.0, -1.0, 1.0), (8, 1.0, 2.0, 7.5)), ((8, 0.125, -1.0, 1.0), (8, 1.0, 2.0, 7.5))],
                         ids=["r2_heavy_b", "r8_heavy_a", "r2_heavy_a", "r8_heavy_b"])
def test_every_meeting_follows_the_update_rule(par):
    """replayed meeting by meeting from the decisions: the pair collision is collide_pairs' with n_L = w_max N_short, the
    lighter record takes it, the heavier one takes it iff u4 < r and keeps its bits otherwise, u4 is the stream's fourth
    draw -- and the replay ends on the velocities the call returned"""
    pa, pb = par
    counts = COUNTS + [(9, 2), (2, 9), (12, 12)]
    n, (A, ca), (B, cb) = _case(counts, 2)
    B[0, 3:] = A[0, 3:]  # (cell 0: one pair at rest relative to each other unless the permutations part them)
    dec = []
    va, vb, out6 = W.collide_weighted(A, ca, pa, B, cb, pb, S, DT, 3, 7, n, decisions=dec)
    wa, wb = pa[1] / pa[0], pb[1] / pb[0]
    wmax, r, a_heavy = max(wa, wb), min(wa, wb) / max(wa, wb), wa > wb
    assert r in (0.5, 0.125)
    mab = pa[3] * pb[3] / (pa[3] + pb[3])
    c0 = S * pa[2] ** 2 * pb[2] ** 2 / (mab * mab)
    nshort = np.array([min(c) for c in counts], dtype=np.float64)
    pairs_sub = R.sub_keys(R.cell_keys(R.call_key(3, 7, 0, 1), R.global_cells(len(counts), n)), R.TAG_PAIRS)
    ya, yb = A[:, 3:].copy(), B[:, 3:].copy()
    tally = np.zeros(6)
    met_a, met_b = np.zeros(len(A), dtype=np.int64), np.zeros(len(B), dtype=np.int64)
    for ia, ib, c, p, xa, xb, ok, u4, rr, ah in dec:
        assert rr == r and ah == a_heavy
        assert len(set(ia)) == len(ia) and len(set(ib)) == len(ib)  # (a round touches a record once)
        cdt = c0 * (wmax * nshort[c]) * DT
        za, zb, zok, s2, _ = R.collide_pairs(ya[ia], yb[ib], cdt, pairs_sub[c], p, mab / pa[3], mab / pb[3])
        assert za.tobytes() == xa.tobytes() and zb.tobytes() == xb.tobytes() and np.array_equal(zok, ok)
        st = R.item_states(pairs_sub[c], p)
        for _ in range(3):
            st, _ = R._u01(st)
        assert np.array_equal(R._u01(st)[1], u4)
        keep = ok & (u4 < r)
        light_new, heavy_new = (zb, za) if a_heavy else (za, zb)
        light, heavy, il, ih = (yb, ya, ib, ia) if a_heavy else (ya, yb, ia, ib)
        light[il] = light_new  # (a skipped pair's "new" velocity is its old one, bit for bit)
        heavy[ih[keep]] = heavy_new[keep]
        tally += [ok.sum(), (~ok).sum(), s2[ok].sum(), (s2[ok] > 1).sum(), keep.sum(), (ok & ~keep).sum()]
        met_a[ia] += 1
        met_b[ib] += 1
    assert ya.tobytes() == va.tobytes() and yb.tobytes() == vb.tobytes()
    assert np.array_equal(tally[[0, 1, 3, 4, 5]], out6[[0, 1, 3, 4, 5]]) and abs(tally[2] - out6[2]) <= 1e-12 * out6[2]
    assert out6[4] > 0 and out6[5] > 0 and out6[4] + out6[5] == out6[0]
    # every record of a populated cell met (long side: once; short side: its share of the long side's records)
    for c, (Na, Nb) in enumerate(counts):
        ma_, mb_ = met_a[ca == c], met_b[cb == c]
        if Na and Nb:
            assert ma_.sum() == mb_.sum() == max(Na, Nb) and ma_.min() >= 1 and mb_.min() >= 1
        else:
            assert ma_.sum() == mb_.sum() == 0
    # a record whose every meeting was rejected keeps its bytes; with r = 1/8 there are such records
    heavy_v, heavy_0 = (va, A[:, 3:]) if a_heavy else (vb, B[:, 3:])
    same = (heavy_v == heavy_0).all(axis=1)
    if r == 0.125:
        assert same.sum() > (met_a if a_heavy else met_b).astype(bool).sum() // 4


@pytest.mark.parametrize("r", [0.5, 0.125])
def test_share_of_heavier_side_updates(r):
    """one call on 16 x 16 x 16 cells with 64 light-weighted and 8 heavy-weighted records each: N = 262144 meetings, the
    share of accepted heavier-side updates within 5 sqrt(r (1 - r) / N) of r"""
    n = (16, 16, 16)
    ncell = 4096
    _, (A, ca), (B, cb) = _case([(64, 8)] * ncell, 5, n=n)
    pa, pb = (64, 1.0, -1.0, 1.0), (int(64 * r), 1.0, 1.0, 4.0)
    _, _, out6 = W.collide_weighted(A, ca, pa, B, cb, pb, 1e-4, DT, 1, 0, n)
    N = out6[0]
    share = out6[4] / N
    print("r", r, "meetings", N, "share", share, "bound", 5 * np.sqrt(r * (1 - r) / N))
    assert N == 64 * ncell >= 2e5 and out6[1] == 0 and out6[4] + out6[5] == N
    assert abs(share - r) <= 5 * np.sqrt(r * (1 - r) / N)


def test_weighted_sums_are_kept_in_expectation():
    """one call from one state under 400 seeds: the change of sum w m v and of sum w m v^2 / 2 over both sorts has a mean
    within 5 standard errors (of the seed-to-seed spread) of zero.  The state has a relative drift and two temperatures,
    so momentum and energy do pass between the sorts: the same sums without the weights move by more than 5 standard
    errors, which is what keeps this test from passing by accident."""
    n = (4, 4, 4)
    ncell = 64
    pa, pb = (16, 1.0, -1.0, 1.0), (2, 1.0, 1.0, 3.0)  # r = 1/8, the heavy weight on b
    _, (A, ca), (B, cb) = _case([(16, 2)] * ncell, 8, n=n)
    A[:, 3] += 0.08
    wa, wb = pa[1] / pa[0], pb[1] / pb[0]

    def sums(va, vb, ua, ub):
        p = ua * pa[3] * va.sum(axis=0) + ub * pb[3] * vb.sum(axis=0)
        e = 0.5 * ua * pa[3] * (va * va).sum() + 0.5 * ub * pb[3] * (vb * vb).sum()
        return np.concatenate([p, [e]])

    w0, u0 = sums(A[:, 3:], B[:, 3:], wa, wb), sums(A[:, 3:], B[:, 3:], 1.0, 1.0)
    dw, du = [], []
    for seed in range(400):
        va, vb, out6 = W.collide_weighted(A, ca, pa, B, cb, pb, 2e-4, DT, seed, 0, n)
        dw.append(sums(va, vb, wa, wb) - w0)
        du.append(sums(va, vb, 1.0, 1.0) - u0)
    dw, du = np.array(dw), np.array(du)
    se_w, se_u = dw.std(axis=0, ddof=1) / np.sqrt(len(dw)), du.std(axis=0, ddof=1) / np.sqrt(len(du))
    print("weighted: mean / standard error", dw.mean(axis=0) / se_w, "unweighted", du.mean(axis=0) / se_u,
          "mean sigma^2", out6[2] / out6[0])
    assert np.all(np.abs(dw.mean(axis=0)) <= 5 * se_w)
    assert np.all(dw.std(axis=0) > 0)  # (a single call does not conserve them)
    assert abs(du.mean(axis=0)[0]) > 5 * se_u[0] and abs(du.mean(axis=0)[3]) > 5 * se_u[3]  # p_x and the energy drift


def _relax_run(kind, seed, K=W.RELAX_K):
    """K inter-species calls of the restatement on the relaxation case -> (T_a - T_b after over before, the largest
    accumulated mean sigma^2, the largest share of a call's pairs with sigma^2 > 1)"""
    n = W.RELAX_GRID[0]
    pa, pb = W.relax_sorts(kind)
    (A, ca), (B, cb) = W.relax_state(kind, seed)
    d0 = W.temperature(A[:, 3:]) - W.temperature(B[:, 3:])
    tot, acc, share = np.zeros(6), 0.0, 0.0
    for k in range(K):
        va, vb, o = W.collide_weighted(A, ca, pa, B, cb, pb, W.RELAX_S, W.RELAX_DT, seed, k, n)
        A[:, 3:], B[:, 3:] = va, vb
        tot += o
        acc, share = max(acc, tot[2] / tot[0]), max(share, o[3] / o[0])
    return (W.temperature(A[:, 3:]) - W.temperature(B[:, 3:])) / d0, acc, share


def test_rates():
    """collisions_weighted_ref.py's relaxation case: T_a = 4 T_b, equal masses, physical density 1 each, 8 x 8 x 8 cells,
    RELAX_K = 180 inter-species calls at S = 3e-6, dt = 0.7; every seed draws its own state and its own streams.
    S, dt and K were chosen with the equal-weight restatement alone (64 / 64 records per cell, 32768 pairs a call), which
    over its 8 seeds leaves 0.6360 +- 0.0026 of T_a - T_b (every seed below 2 / 3: it falls by more than a third), with
    the accumulated mean sigma^2 at most 0.040 after every call (limit 0.1) and at most 2.8e-3 of one call's pairs above
    1 (limit 3.5e-3; a larger S or fewer calls does not keep that).
    The weighted runs, r = 1/8, 4 seeds each: heavy weight on b (64 / 8 records per cell) 0.6309 +- 0.0099, on a (8 / 64)
    0.6351 +- 0.0089.  The margin is 4 standard deviations of the equal-weight run's spread plus the weighted run's own
    standard deviation: 0.0201 and 0.0192; the means differ by 0.0050 and 0.0009.
    With n_L = w_min N_short in place of w_max N_short the heavy-b run (seed 0) leaves 0.9270: it falls 5.0 times less,
    0.29 from the equal-weight mean, 14 margins (asserted: more than 5).
    The small-angle conditions are asserted for the equal-weight run only.  In the weighted runs they say nothing: with
    equal masses a pair scattered by Theta = pi exchanges its velocities, and when the heavier record's update is
    rejected the lighter one becomes its copy to the last place; should the two meet again, 1 / u^3 is astronomically
    large (and the collision, by pi again, changes nothing)."""
    kinds = ("equal", "heavy_b", "heavy_a")
    jobs = [(kind, seed) for kind in kinds for seed in W.RELAX_SEEDS[kind]]
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:  # (numpy releases the lock in its loops)
        res = dict(zip(jobs, pool.map(lambda j: _relax_run(*j), jobs)))
    left = {kind: np.array([res[kind, s][0] for s in W.RELAX_SEEDS[kind]]) for kind in kinds}
    for kind in kinds:
        print(kind, "T_a - T_b over its start: mean", left[kind].mean(), "standard deviation", left[kind].std(ddof=1),
              "accumulated sigma^2", max(res[kind, s][1] for s in W.RELAX_SEEDS[kind]),
              "share above 1", max(res[kind, s][2] for s in W.RELAX_SEEDS[kind]))
    assert len(W.RELAX_SEEDS["equal"]) >= 8
    for s in W.RELAX_SEEDS["equal"]:  # the equal-weight run keeps the small-angle step resolved and relaxes by a third
        assert res["equal", s][1] < 0.1 and res["equal", s][2] < 3.5e-3
    assert np.all(left["equal"] <= 2.0 / 3.0)
    sd = left["equal"].std(ddof=1)
    for kind in ("heavy_b", "heavy_a"):
        margin = 4 * sd + left[kind].std(ddof=1)
        print(kind, "difference of the means", left[kind].mean() - left["equal"].mean(), "margin", margin)
        assert abs(left[kind].mean() - left["equal"].mean()) <= margin
    # the wrong density factor (the lighter weight) is far outside: the test tells the two apart
    true_factor = W.density_factor
    try:
        W.density_factor = lambda wa, wb, n_short: min(wa, wb) * n_short
        wrong = _relax_run("heavy_b", 0)[0]
    finally:
        W.density_factor = true_factor
    margin = 4 * sd + left["heavy_b"].std(ddof=1)
    print("n_L = w_min N_short:", wrong, "falls", (1 - left["equal"].mean()) / (1 - wrong), "times less;",
          abs(wrong - left["equal"].mean()) / margin, "margins away")
    assert abs(wrong - left["equal"].mean()) > 5 * margin


def test_slabs_draw_the_single_box_numbers():
    """a slab (z0, nzl) of the box gives the records of its cells the box's result, and the slabs' out6 add up"""
    n = (3, 2, 6)
    rng = np.random.default_rng(6)
    counts = list(zip(rng.integers(0, 12, 36), rng.integers(0, 5, 36)))
    _, (A, ca), (B, cb) = _case(counts, 7, n=n)
    pa, pb = (8, 1.0, -1.0, 1.0), (2, 1.0, 2.0, 7.5)
    wa_, wb_, whole = W.collide_weighted(A, ca, pa, B, cb, pb, S, DT, 2, 4, n)
    plane, tot = n[0] * n[1], np.zeros(6)
    for z0 in (0, 2, 4):
        ma = (ca >= z0 * plane) & (ca < (z0 + 2) * plane)
        mb = (cb >= z0 * plane) & (cb < (z0 + 2) * plane)
        xa, xb, o = W.collide_weighted(A[ma], ca[ma] - z0 * plane, pa, B[mb], cb[mb] - z0 * plane, pb, S, DT, 2, 4, n,
                                       z0=z0, nzl=2)
        assert xa.tobytes() == wa_[ma].tobytes() and xb.tobytes() == wb_[mb].tobytes()
        tot += o
    assert np.array_equal(tot[[0, 1, 3, 4, 5]], whole[[0, 1, 3, 4, 5]]) and abs(tot[2] - whole[2]) <= 1e-12 * whole[2]
    assert whole[5] > 0


def test_refusals_and_zero_strength():
    n, (A, ca), (B, cb) = _case(COUNTS, 3)
    pa = (8, 1.0, -1.0, 1.0)
    va, vb, out6 = W.collide_weighted(A, ca, pa, B, cb, (2, 1.0, 2.0, 7.5), 0.0, DT, 1, 0, n)
    assert va.tobytes() == A[:, 3:].tobytes() and vb.tobytes() == B[:, 3:].tobytes() and not out6.any()
    for bad in ((2, 0.0, 2.0, 7.5), (2, -1.0, 2.0, 7.5), (2, float("inf"), 2.0, 7.5), (2, float("nan"), 2.0, 7.5)):
        with pytest.raises(ValueError):
            W.collide_weighted(A, ca, pa, B, cb, bad, S, DT, 1, 0, n)
