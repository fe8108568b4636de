"""Binary collisions between sorts of unequal weight on the GPU (xpic_collide_weighted,
xpic_amd/csrc/collide.hip) against tests/collisions_weighted_ref.py on the same records: parity and identical
update decisions on hand-populated cells, xpic_collide's bits at equal weights, determinism, refusals, three z-slabs, the
relaxation rate whichever side carries the heavy weight, the weighted sums in expectation, and the host executable.  An
extension: the reference has no collision operator; the restatement is the second statement of the definition."""
import ctypes as C
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import collisions_weighted_ref as W  # noqa: E402
from test_gpu_collisions import DT, EXE, GOLD, GRID, GRID_P2, _ctx  # noqa: E402  (the grids and helpers of 5r's tests)

pytestmark = pytest.mark.gpu

BASE = ((8, 1.0, -1.0, 1.0), (8, 1.0, 2.0, 7.5))  # Np, n, q, m: equal weights, different q and m
S = 2e-4  # (chains of up to 37 meetings of one short record: moderate angles, see test_gpu_collisions._hand_pops)
COUNTS = [(0, 3), (3, 0), (1, 1), (1, 5), (5, 1), (4, 4), (63, 64), (64, 63), (65, 130), (130, 65)]


def _sorts(r, heavy):
    """BASE with the density of the lighter-weighted sort scaled by r; heavy: 0 (a) or 1 (b)"""
    s = [list(p) for p in BASE]
    s[1 - heavy][1] = r
    return tuple(tuple(p) for p in s)


WEIGHTS = pytest.mark.parametrize("r,heavy", [(1.0, 1), (0.5, 0), (0.5, 1), (0.125, 0), (0.125, 1)],
                                  ids=["equal", "r2_heavy_a", "r2_heavy_b", "r8_heavy_a", "r8_heavy_b"])


def _hand_pops(ncell, lds_cell):
    big = lds_cell + 3  # (259 at the built limit of 256: the second path)
    rng = np.random.default_rng(78)
    a, b = rng.integers(0, 11, ncell), rng.integers(0, 11, ncell)
    counts = COUNTS + [(big, 7), (7, big)]
    a[:len(counts)] = [c[0] for c in counts]
    b[:len(counts)] = [c[1] for c in counts]
    return a, b


def _out6(out):
    return [out[k] for k in ("pairs", "skipped", "sigma2_sum", "sigma2_over_1", "heavy_updates", "heavy_rejected")]


def _check_out6(out, ref):
    got = _out6(out)
    assert [got[k] for k in (0, 1, 3, 4, 5)] == [ref[k] for k in (0, 1, 3, 4, 5)]
    assert abs(got[2] - ref[2]) <= 1e-12 * ref[2]


@WEIGHTS
@pytest.mark.parametrize("grid", [GRID, GRID_P2], ids=["general", "p2"])
def test_parity_with_the_restatement(grid, r, heavy):
    import xpic_amd as X

    n, d = grid
    ncell = n[0] * n[1] * n[2]
    sorts = _sorts(r, heavy)
    pops = _hand_pops(ncell, X.COLLIDE_LDS_CELL)
    g = _ctx(n, d, pops, seed=1, sorts=sorts)
    assert g.collide_info()["lds_cell"] == X.COLLIDE_LDS_CELL
    before = [g.particles(s) for s in range(2)]
    assert [np.bincount(c, minlength=ncell).tolist() for _, c in before] == [p.tolist() for p in pops]
    state = [p.copy() for p, _ in before]
    cells = [c for _, c in before]
    vmax = max(np.abs(p[:, 3:]).max() for p in state)
    for sa, sb, step in ((0, 1, 4), (1, 0, 6)):
        start = [p[:, 3:].copy() for p in state]
        out = g.collide_weighted(sa, sb, S, step, seed=9, dt=DT)
        va, vb, ref = W.collide_weighted(state[sa], cells[sa], sorts[sa], state[sb], cells[sb], sorts[sb], S, DT, 9, step, n,
                                         sorts=(sa, sb))
        state[sa][:, 3:], state[sb][:, 3:] = va, vb
        print("call", (sa, sb), out, "restatement", ref.tolist())
        for s in range(2):
            got, gc = g.particles(s)
            print("  sort", s, "max |dv|", np.abs(got[:, 3:] - state[s][:, 3:]).max(), "of", vmax)
            assert got[:, :3].tobytes() == before[s][0][:, :3].tobytes() and gc.tobytes() == before[s][1].tobytes()
            assert np.abs(got[:, 3:] - state[s][:, 3:]).max() <= 1e-12 * vmax
            # the decisions: a record the restatement left untouched keeps its bytes on the device, and only those do
            kept = (state[s][:, 3:] == start[s]).all(axis=1)
            assert np.array_equal((got[:, 3:] == start[s]).all(axis=1), kept)
            assert got[kept, 3:].tobytes() == start[s][kept].tobytes()
            state[s][:, 3:] = got[:, 3:]  # (the next call starts from the device's own state)
        _check_out6(out, ref)
        assert g.collide_info()["large_cells"] == 2  # (the cells of 259 records of one sort; the others the LDS path)
        assert out["pairs"] > 0 and out["heavy_updates"] + out["heavy_rejected"] == out["pairs"]
        assert (out["heavy_rejected"] == 0) == (r == 1.0)


def _small_pops(ncell):
    import xpic_amd as X

    return [np.minimum(p, 64) for p in _hand_pops(ncell, X.COLLIDE_LDS_CELL)]  # (stored in input order: _points)


@pytest.mark.parametrize("sorts", [BASE, ((8, 1.0, -1.0, 1.0), (4, 0.5, 2.0, 7.5))], ids=["same_Np", "other_Np"])
def test_equal_weights_give_xpic_collide_bit_for_bit(sorts):
    n, d = GRID
    ncell = n[0] * n[1] * n[2]
    pops = _small_pops(ncell)
    g, h = _ctx(n, d, pops, seed=6, sorts=sorts), _ctx(n, d, pops, seed=6, sorts=sorts)
    for s in range(2):
        assert g.particles(s)[0].tobytes() == h.particles(s)[0].tobytes()
    for sa, sb, step in ((0, 1, 4), (1, 0, 6), (0, 0, 3), (1, 1, 5)):  # (the same sort twice: xpic_collide's own path)
        out, ref = g.collide_weighted(sa, sb, 2e-3, step, seed=3), h.collide(sa, sb, 2e-3, step, seed=3)
        assert _out6(out)[:4] == [ref[k] for k in ("pairs", "skipped", "sigma2_sum", "sigma2_over_1")]
        assert out["pairs"] > 0 and out["heavy_updates"] == out["pairs"] and out["heavy_rejected"] == 0
        for s in range(2):
            assert g.particles(s)[0].tobytes() == h.particles(s)[0].tobytes()


def test_determinism_and_zero_strength():
    n, d = GRID
    ncell = n[0] * n[1] * n[2]
    sorts = _sorts(0.125, 1)
    res = []
    for _ in range(2):
        g = _ctx(n, d, _small_pops(ncell), seed=6, sorts=sorts)
        before = [g.particles(s) for s in range(2)]
        zero = g.collide_weighted(0, 1, 0.0, 2, seed=3)
        assert zero == dict(pairs=0, skipped=0, sigma2_sum=0.0, sigma2_over_1=0, heavy_updates=0, heavy_rejected=0)
        for s in range(2):
            pts, cells = g.particles(s)
            assert pts.tobytes() == before[s][0].tobytes() and cells.tobytes() == before[s][1].tobytes()
        outs = [g.collide_weighted(a, b, 2e-3, step, seed=3) for a, b, step in ((0, 1, 4), (1, 0, 6), (0, 1, 7))]
        assert outs[0]["heavy_rejected"] > 0
        res.append((outs, [g.particles(s)[0].tobytes() for s in range(2)]))
    assert res[0] == res[1]


def test_refusals_change_nothing_and_collide_still_refuses():
    import xpic_amd as X

    n, d = GRID
    ncell = n[0] * n[1] * n[2]
    rng = np.random.default_rng(8)
    sorts = BASE + ((5, 0.6, 2.0, 7.5), (8, 0.0, 1.0, 1.0), (8, -1.0, 1.0, 1.0), (8, 1.0, 1.0, -2.0))
    g = _ctx(n, d, [rng.integers(0, 9, ncell) for _ in sorts], seed=7, sorts=sorts)
    before = [g.particles(s)[0].tobytes() for s in range(len(sorts))]
    for a, b, word in ((0, 6, "sort"), (-1, 0, "sort"), (0, 3, "weight"), (4, 1, "weight"), (0, 5, "mass"), (3, 3, "weight")):
        with pytest.raises(X.XpicError, match=word):
            g.collide_weighted(a, b, 2e-3, 0)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(X.XpicError, match="strength"):
            g.collide_weighted(0, 2, bad, 0)
    out = np.zeros(6)
    p = X.CollisionParams(2e-3, 0.0, 0)
    assert g.L.xpic_collide_weighted(g.h, 0, 2, None, 0, out.ctypes.data_as(X.c_dp)) != 0 and b"null" in g.L.xpic_last_error()
    assert g.L.xpic_collide_weighted(g.h, 0, 2, C.byref(p), 0, None) != 0 and b"null" in g.L.xpic_last_error()
    # the boundary between the two entry points: xpic_collide refuses the pair of unequal weight ...
    with pytest.raises(X.XpicError, match="weight"):
        g.collide(0, 2, 2e-3, 0)
    assert [g.particles(s)[0].tobytes() for s in range(len(sorts))] == before
    # ... which xpic_collide_weighted takes
    out = g.collide_weighted(0, 2, 2e-3, 0)
    assert out["pairs"] > 0 and out["heavy_rejected"] > 0
    assert g.particles(0)[0].tobytes() != before[0] and g.particles(1)[0].tobytes() == before[1]


def test_slabs_equal_one_context():
    from xpic_amd.parallel import ThreadRing

    n, d, nr = (4, 4, 18), (0.5, 0.4, 0.25), 3
    ncell = n[0] * n[1] * n[2]
    nloc = ncell // nr
    sorts = _sorts(0.125, 0)
    calls = ((0, 1, 4), (1, 0, 6), (0, 0, 3))
    rng = np.random.default_rng(10)
    pops = [rng.integers(0, 12, ncell), rng.integers(0, 12, ncell)]
    pops[0][[3, nloc + 1, 2 * nloc + 7]] = [63, 64, 2]  # (at most 64: the stored order is the input's on every slab)
    one = _ctx(n, d, pops, seed=11, sorts=sorts)
    routs = [one.collide_weighted(a, b, 2e-3, step, seed=2) for a, b, step in calls]
    rparts = [one.particles(s)[0] for s in range(2)]
    ring = ThreadRing(nr)
    res, errs = [None] * nr, []

    def rank_main(r):
        try:
            ctx = _ctx(n, d, pops, seed=11, rank=r, nranks=nr, sorts=sorts)
            ring.attach(ctx, r)
            outs = [ctx.collide_weighted(a, b, 2e-3, step, seed=2) for a, b, step in calls]
            res[r] = (outs, [ctx.particles(s)[0] for s in range(2)])
            ctx.close()
        except BaseException as e:  # noqa: BLE001 -- release the other ranks, report below
            errs.append((r, repr(e)))
            ring.bar.abort()

    th = [threading.Thread(target=rank_main, args=(r,)) for r in range(nr)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not errs and all(x is not None for x in res), errs
    for s in range(2):
        got = np.concatenate([res[r][1][s] for r in range(nr)])  # (local cells in order are global cells in order)
        assert got.tobytes() == rparts[s].tobytes()
    assert routs[0]["heavy_rejected"] > 0
    for r in range(nr):
        for out, ref in zip(res[r][0], routs):
            _check_out6(out, _out6(ref))  # (every slab holds the sum; the all-reduce adds sigma^2 in another order)


def _relax_ctx(kind, seed):
    """the relaxation case of collisions_weighted_ref.py on the device: its velocities at the centres of their cells"""
    import xpic_amd as X

    n, d = W.RELAX_GRID
    g = X.Context("ecsim", n, d, W.RELAX_DT)
    for par, (pts, cells) in zip(W.relax_sorts(kind), W.relax_state(kind, seed)):
        idx = np.stack([cells % n[0], (cells // n[0]) % n[1], cells // (n[0] * n[1])], axis=1)
        pts[:, :3] = (idx + 0.5) * np.array(d)
        s = g.add_sort(*par, capacity=len(pts))
        assert g.add_particles(s, pts) == len(pts)
    return g


def _relax_run(kind, seed):
    g = _relax_ctx(kind, seed)
    t = lambda: W.temperature(g.particles(0)[0][:, 3:]) - W.temperature(g.particles(1)[0][:, 3:])  # noqa: E731
    d0, tot, acc, share = t(), np.zeros(6), 0.0, 0.0
    for k in range(W.RELAX_K):
        o = np.array(_out6(g.collide_weighted(0, 1, W.RELAX_S, k, seed=seed)))
        tot += o
        acc, share = max(acc, tot[2] / tot[0]), max(share, o[3] / o[0])
    left = t() / d0
    g.close()
    return left, acc, share


def test_rates():
    """tests/test_collisions_weighted_ref.py: test_rates on the device, with its case, its seeds and its limits: the
    equal-weight run (two sorts through the new kernel) keeps the accumulated mean sigma^2 below 0.1 and every call's
    share of pairs above 1 below 3.5e-3 and loses a third of T_a - T_b; the runs with r = 1/8, the heavy weight on b and
    on a, end within 4 standard deviations of the equal-weight run's spread plus their own of it."""
    kinds = ("equal", "heavy_b", "heavy_a")
    res = {(kind, s): _relax_run(kind, s) for kind in kinds for s in W.RELAX_SEEDS[kind]}
    left = {kind: np.array([res[kind, s][0] for s in W.RELAX_SEEDS[kind]]) for kind in kinds}
    for kind in kinds:
        print(kind, "T_a - T_b over its start: mean", left[kind].mean(), "standard deviation", left[kind].std(ddof=1),
              "accumulated sigma^2", max(res[kind, s][1] for s in W.RELAX_SEEDS[kind]),
              "share above 1", max(res[kind, s][2] for s in W.RELAX_SEEDS[kind]))
    for s in W.RELAX_SEEDS["equal"]:
        assert res["equal", s][1] < 0.1 and res["equal", s][2] < 3.5e-3
    assert np.all(left["equal"] <= 2.0 / 3.0)
    sd = left["equal"].std(ddof=1)
    for kind in ("heavy_b", "heavy_a"):
        margin = 4 * sd + left[kind].std(ddof=1)
        print(kind, "difference of the means", left[kind].mean() - left["equal"].mean(), "margin", margin)
        assert abs(left[kind].mean() - left["equal"].mean()) <= margin


def test_weighted_sums_over_50_calls():
    """the CPU test's bound on the device: over 50 calls, each from the same state under its own seed, the change of
    sum w m v and of sum w m v^2 / 2 has a mean within 5 standard errors of its seed-to-seed spread of zero; the sums
    without the weights (momentum along the drift, and the energy) move by more"""
    n, d = (4, 4, 4), (0.5, 0.5, 0.5)
    sorts = ((16, 1.0, -1.0, 1.0), (2, 1.0, 1.0, 3.0))  # r = 1/8, the heavy weight on b
    g = _ctx(n, d, (np.full(64, 16), np.full(64, 2)), seed=8, sorts=sorts)
    pts, _ = g.particles(0)
    pts[:, 3] += 0.08  # (a relative drift: momentum passes between the sorts)
    g.clear(0)
    g.add_particles(0, pts)

    def sums(weights):
        out = np.zeros(4)
        for s, (w, (_, _, _, m)) in enumerate(zip(weights, sorts)):
            v = g.particles(s)[0][:, 3:]
            out += np.concatenate([w * m * v.sum(axis=0), [0.5 * w * m * (v * v).sum()]])
        return out

    ws = [p[1] / p[0] for p in sorts]
    start = [g.particles(s)[0] for s in range(2)]
    w0, u0 = sums(ws), sums((1.0, 1.0))
    dw, du = [], []
    for seed in range(50):  # (as the CPU test: every call from the same state, under its own seed)
        assert g.collide_weighted(0, 1, 2e-4, 0, seed=seed)["heavy_rejected"] > 0
        dw.append(sums(ws) - w0)
        du.append(sums((1.0, 1.0)) - u0)
        for s in range(2):
            g.clear(s)
            g.add_particles(s, start[s])
    dw, du = np.array(dw), np.array(du)
    se_w, se_u = dw.std(axis=0, ddof=1) / np.sqrt(50), du.std(axis=0, ddof=1) / np.sqrt(50)
    print("weighted: mean / standard error", dw.mean(axis=0) / se_w, "unweighted", du.mean(axis=0) / se_u)
    assert np.all(np.abs(dw.mean(axis=0)) <= 5 * se_w) and np.all(dw.std(axis=0) > 0)
    assert abs(du.mean(axis=0)[0]) > 5 * se_u[0] and abs(du.mean(axis=0)[3]) > 5 * se_u[3]


def _host_run(tmp_path, name, presets, expect_failure=False):
    """5 steps of the reference's ecsim_ex1 with a second sort of a quarter of the density through the executable ->
    (the backup's electron records [N][6] sorted by x, the log)"""
    cfg = json.load(open(os.path.join(GOLD, "ecsim_ex1", "config.json")))
    dt = cfg["Geometry"]["dt"]
    cfg["Geometry"]["t"] = 5 * dt
    cfg["Geometry"]["diagnose_period"] = 5 * dt
    cfg["Diagnostics"] = []
    cfg["SimulationBackup"] = {"diagnose_period": "5 [dt]"}
    cfg["Particles"].append(dict(cfg["Particles"][0], sort_name="minority", n=0.25, q=1.0, m=4.0))
    cfg["Presets"].append(dict(cfg["Presets"][0], particles="minority"))
    if presets is not None:
        cfg["StepPresets"] = presets
    out_dir = tmp_path / name
    out_dir.mkdir()
    cfg["OutputDirectory"] = str(out_dir)
    path = out_dir / "config.json"
    path.write_text(json.dumps(cfg))
    out = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=300)
    if expect_failure:
        return None, out.returncode, out.stdout + out.stderr
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    rec = np.fromfile(out_dir / "simulation_backup" / "5" / "electrons", dtype=">f8").astype(np.float64).reshape(-1, 6)
    return rec[np.argsort(rec[:, 0], kind="stable")], 0, out.stdout


def test_host_mirror(tmp_path):
    """"BinaryCollisions" with "weighted": true on two sorts of different n (weights 1 / 100 and 0.25 / 100), compared as
    test_gpu_collisions.test_host_mirror compares: two runs of one configuration differ by rounding in arrival order, so
    the records are held against the largest difference of two plain runs -- strength 0 within 8 x of it, the run with
    collisions 1000 x outside.  The same command without the key fails with xpic_collide's weight message."""
    cmd = {"command": "BinaryCollisions", "particles": ["electrons", "minority"], "strength": 1e-4, "seed": 3, "weighted": True}
    plain, _, _ = _host_run(tmp_path, "plain", None)
    with_c, _, log = _host_run(tmp_path, "collisions", [cmd])
    zero, _, zlog = _host_run(tmp_path, "zero", [dict(cmd, strength=0.0)])
    again, _, _ = _host_run(tmp_path, "plain2", None)
    _, rc, flog = _host_run(tmp_path, "unweighted", [{k: v for k, v in cmd.items() if k != "weighted"}], expect_failure=True)
    assert rc != 0 and "same weight" in flog and "equal-weight path" in flog
    assert "weighted path" in log and "Binary collisions (weighted)" in log and "heavier-side updates" in log
    assert ": 0 pairs" in zlog and ": 0 pairs" not in log
    assert plain.shape == with_c.shape == zero.shape == again.shape and len(plain) > 0
    dist = lambda a, b: float(np.abs(a - b).max())  # noqa: E731
    noise = dist(again, plain)
    print("records: plain again", noise, "strength 0", dist(zero, plain), "collisions", dist(with_c, plain))
    assert noise < 1e-9
    assert dist(zero, plain) <= 8 * noise
    assert dist(with_c, plain) >= 1000 * noise
