"""tests/collisional_grid_trace_ref.py held to what it restates, without a GPU: the pair conservation laws, the inert empty
cell, the constant profile against the uniform restatement bit for bit, the per-cell moments on hand-made cells, and the
three bugs the restatement must be able to see (swapped axes, a fold by truncation, a variance divided by N - 1).

The grid has three different extents and unequal spacings, particles start outside [0, L) on both sides of every axis
and one lies exactly on a cell face: whatever slips in the lookup changes a cell."""
import numpy as np

import collisional_grid_trace_ref as G
import collisional_trace_ref as CT

N, D = (6, 5, 4), (0.5, 0.4, 0.25)
SHAPE = (N[2], N[1], N[0])
L = np.array(N) * np.array(D)
QM, MP, DT = -1.0, 1.0, 0.05
BACKGROUNDS = [dict(q=1.0, m=4.0, n=1.0, vth=0.5, drift=(0.1, 0.0, -0.2)), dict(q=-2.0, m=0.25, n=0.5, vth=2.0),
               dict(q=1.0, m=1836.0, n=3.0, vth=0.01), dict(q=1.0, m=1.0, n=0.7, vth=1.0, drift=(0.0, 0.3, 0.0))]


def positions(n, seed=5):
    """inside and up to two boxes outside on both sides of every axis; the first on a cell face of every axis"""
    rng = np.random.default_rng(seed)
    r = (rng.random((n, 3)) * 5.0 - 2.0) * L
    r[0] = (3 * D[0], -2 * D[1], 5 * D[2] + L[2])
    return r


def graded(seed=9):
    """a profile that differs in every cell, zero density in the cells with x >= L / 2"""
    rng = np.random.default_rng(seed)
    n = 0.5 + rng.random(SHAPE)
    n[:, :, N[0] // 2:] = 0.0
    return G.profile(n, 0.2 + rng.random(SHAPE), 0.3 * rng.normal(size=SHAPE + (3,)))


def test_the_lookup():
    r = positions(200)
    c = G.cell_index(r, N, D)
    assert c.min() >= 0 and c.max() < N[0] * N[1] * N[2]
    # folded by hand: the particle's position brought into the box first
    inside = r - np.floor(r / L) * L
    i = np.minimum(np.floor(inside / np.array(D)).astype(int), np.array(N) - 1)
    ok = np.abs(inside / np.array(D) - np.round(inside / np.array(D))) > 1e-9  # (away from a face the two agree)
    keep = ok.all(axis=1)
    assert keep.sum() > 150
    assert np.array_equal(c[keep], ((i[:, 2] * N[1] + i[:, 1]) * N[0] + i[:, 0])[keep])
    # on the faces: x = 3 dx is cell 3, y = -2 dy folds to cell 3 of 5, z = 5 dz + Lz is cell 1 of 4
    assert c[0] == (1 * N[1] + 3) * N[0] + 3
    # positions outside the box are used: the fold matters
    assert (r < 0).any(axis=0).all() and (r >= L).any(axis=0).all()


def test_pairs_conserve_momentum_and_energy():
    rng = np.random.default_rng(3)
    n = 300
    r, v = positions(n), rng.normal(size=(n, 3))
    coll = CT.collisions(BACKGROUNDS, strength=0.05, mass=2.0, every=3, seed=77, particle0=11)
    slots = {0: graded(), 2: graded(10)}
    pairs = []
    vn, t = G.collide_fo(v, r, coll, [0, -1, 2, -1], slots, (N, D), QM, DT, 6, 11 + np.arange(n), pairs=pairs)
    assert len(pairs) == 4 and t[0] > n
    worst = 0.0
    for b, i, v0, w0, v1, w1, ok, fa, fb in pairs:
        ma, mb = coll["mass"], BACKGROUNDS[b]["m"]
        scale = np.abs(np.concatenate([v0, w0])).max()
        dp = ma * (v1 - v0) + mb * (w1 - w0)
        dE = 0.5 * ma * ((v1 * v1).sum(1) - (v0 * v0).sum(1)) + 0.5 * mb * ((w1 * w1).sum(1) - (w0 * w0).sum(1))
        worst = max(worst, np.abs(dp).max() / (max(ma, mb) * scale), np.abs(dE).max() / (max(ma, mb) * scale * scale))
    print("largest pair momentum / energy defect, relative:", worst)
    assert worst <= 1e-14 * 10


def test_an_empty_cell_is_inert():
    n = 257
    rng = np.random.default_rng(4)
    r, v = positions(n), rng.normal(size=(n, 3))
    prof = graded()
    coll = CT.collisions(BACKGROUNDS[:1], strength=0.05, mass=1.0, seed=1)
    filled = prof["n"].reshape(-1)[G.cell_index(r, N, D)] > 0.0
    assert filled.sum() > 50 and (~filled).sum() > 50
    vn, t = G.collide_fo(v, r, coll, [0], {0: prof}, (N, D), QM, DT, 1, np.arange(n))
    assert vn[~filled].tobytes() == v[~filled].tobytes() and (vn[filled] != v[filled]).any(axis=1).all()
    assert t[0] == filled.sum() and t[1] == 0
    # a guiding centre alike, and where |B| == 0 only the filled cells count as skipped
    rec = np.column_stack([r, rng.normal(size=n), np.abs(rng.normal(size=n)) + 0.1, np.ones(n)])
    B = np.tile([0.3, -0.4, 1.2], (n, 1))
    B[::7] = 0.0
    out, t = G.collide_dk(rec, B, coll, [0], {0: prof}, (N, D), QM, MP, DT, 1, np.arange(n))
    dead = np.zeros(n, bool)
    dead[::7] = True
    assert out[~filled | dead].tobytes() == rec[~filled | dead].tobytes()
    assert t[0] == (filled & ~dead).sum() and t[1] == (filled & dead).sum()


def test_a_constant_profile_is_the_uniform_background():
    n = 130
    rng = np.random.default_rng(6)
    r, v = positions(n), rng.normal(size=(n, 3))
    coll = CT.collisions(BACKGROUNDS, strength=0.02, mass=2.0, every=1, seed=5, particle0=1000)
    slots = {s: G.profile(b["n"], b["vth"], b.get("drift"), SHAPE) for s, b in enumerate(BACKGROUNDS)}
    particles = 1000 + np.arange(n)
    ref, tr = CT.collide_fo(v, coll, QM, DT, 4, particles)
    for prof in (None, [-1, -1, -1, -1], [0, 1, 2, 3], [0, -1, 2, -1]):
        got, t = G.collide_fo(v, r, coll, prof, slots, (N, D), QM, DT, 4, particles)
        assert got.tobytes() == ref.tobytes() and t.tobytes() == tr.tobytes(), prof
    rec = np.column_stack([r, rng.normal(size=n), np.abs(rng.normal(size=n)) + 0.1, np.ones(n)])
    B = rng.normal(size=(n, 3))
    B[5] = 0.0
    ref, tr = CT.collide_dk(rec, B, coll, QM, MP, DT, 4, particles)
    got, t = G.collide_dk(rec, B, coll, [3, 2, 1, 0][::-1], slots, (N, D), QM, MP, DT, 4, particles)
    assert got.tobytes() == ref.tobytes() and t.tobytes() == tr.tobytes()


def hand_cells():
    """cells of 0, 1, 2, 64 and 65 records with a drift and a spread that differ per cell"""
    rng = np.random.default_rng(8)
    pops = [0, 1, 2, 64, 65]
    cells = np.repeat(np.arange(len(pops)), pops)
    v = rng.normal(size=(len(cells), 3)) * (0.1 + cells[:, None]) + np.array([1.0, -2.0, 0.5]) * cells[:, None]
    return pops, cells, v


def test_the_moments_on_hand_made_cells():
    pops, cells, v = hand_cells()
    w = 3.0 / 8
    n, vth, u = G.moments(v, cells, len(pops), w)
    assert np.array_equal(n, w * np.array(pops, dtype=np.float64))
    assert n[0] == 0 and vth[0] == 0 and not u[0].any()                    # empty: zeros
    assert vth[1] == 0.0 and u[1].tobytes() == v[cells == 1][0].tobytes()  # one record: itself, no spread
    a, b = v[cells == 2]
    assert np.abs(u[2] - (a + b) / 2).max() <= 2e-16 * np.abs(u[2]).max()
    assert abs(vth[2] - np.sqrt(((a - b) ** 2).sum() / 12.0)) <= 4e-16 * vth[2]  # sum |v - u|^2 = |a - b|^2 / 2, / (3 * 2)
    for c in (3, 4):
        vc = v[cells == c]
        assert np.abs(u[c] - vc.mean(axis=0)).max() <= 1e-14 * np.abs(vc).max()
        assert abs(vth[c] - np.sqrt(vc.var(axis=0).mean())) <= 1e-14 * vth[c]


def test_the_restatement_sees_its_bugs():
    """each of the three slips changes a result that a check above pins"""
    r = positions(200)
    good = G.cell_index(r, N, D)
    assert (G.cell_index(r, N, D, axes=(1, 0, 2)) != good).any()   # x and y swapped
    assert (G.cell_index(r, N, D, axes=(2, 1, 0)) != good).any()   # x and z swapped
    trunc = G.cell_index(r, N, D, fold=np.fmod)                     # a fold by truncation: negative indices survive
    assert (trunc != good).any() and trunc.min() < 0
    # ... and the collisions see them: other cells, other backgrounds, other bits
    rng = np.random.default_rng(4)
    v = rng.normal(size=(200, 3))
    coll = CT.collisions(BACKGROUNDS[:1], strength=0.05, mass=1.0, seed=1)
    ref, _ = G.collide_fo(v, r, coll, [0], {0: graded()}, (N, D), QM, DT, 1, np.arange(200))
    try:  # (with three different extents a swapped lookup may even leave the profile)
        bad, _ = G.collide_fo(v, r, coll, [0], {0: graded()}, (N, D), QM, DT, 1, np.arange(200), axes=(1, 0, 2))
        broke = bad.tobytes() != ref.tobytes()
    except IndexError:
        broke = True
    assert broke
    # vth over N - 1: the two-record cell no longer gives |a - b| / sqrt(12)
    pops, cells, v = hand_cells()
    _, vth, _ = G.moments(v, cells, len(pops), 1.0, ddof=1)
    a, b = v[cells == 2]
    assert abs(vth[2] - np.sqrt(((a - b) ** 2).sum() / 12.0)) > 0.1 * vth[2]
