"""tests/collisional_trace_ref.py itself, without a GPU: what the definition of the collisional traces
(include/xpic_hip.h: xpic_trace_collisions) promises -- the conservation laws of every test-particle / partner pair, the
Lorentz limit against a cold infinitely heavy background, stationarity of a Maxwellian at the background's temperature and
the relaxation of a hotter one, the guiding centre's basis and re-projection, and which steps collide."""
import numpy as np
import pytest

import analytic_trace_ref as A
import collisional_trace_ref as R

N = 1 << 16
IDX = np.arange(N, dtype=np.int64)
QM, DT = -1.0, 0.05

# ---- the stationarity set-up, shared with tests/test_gpu_collisional_trace.py: m_a = 1 in a background of m_b = 4 at
# T_b = 1, so vth_a = 1 and vth_b = 1 / 2.  sigma^2 = cdt / |u|^3 with cdt = S q_a^2 q_b^2 n dt / m_ab^2 = 0.01: the mean
# over the pairs is a few 1e-2 (its tail in 1 / |u|^3 is heavy but integrable against u^2 du only logarithmically, so the
# figure is quoted from the run), and |u| < 0.215, where sigma^2 > 1, has a probability of about 2e-3
T_B, M_A, M_B = 1.0, 1.0, 4.0
STATIONARY_STEPS, STATIONARY_SAMPLE = 400, 100
M_AB = M_A * M_B / (M_A + M_B)


def stationary_collisions(seed=11):
    strength = 0.01 * M_AB * M_AB / DT  # q_a = q_b = n = 1
    return R.collisions([dict(q=1.0, m=M_B, n=1.0, vth=np.sqrt(T_B / M_B))], strength=strength, mass=M_A, seed=seed)


def maxwellian(temperature, seed):
    return np.random.default_rng(seed).normal(size=(N, 3)) * np.sqrt(temperature / M_A)


def lorentz_collisions(v0, sigma2=0.01, seed=3):
    """one cold, drift-free background of mass 1e30: m_ab = m_a, w = 0, |u| = |v| for everybody"""
    u = np.sqrt(np.dot(v0, v0))
    return R.collisions([dict(q=1.0, m=1e30, n=1.0, vth=0.0)], strength=sigma2 * u ** 3 / DT, mass=1.0, seed=seed)


LORENTZ_V0 = np.array([0.3, -0.4, 1.2])


def tan2_half(v0, v):
    c = (v * v0).sum(axis=1) / np.sqrt((v * v).sum(axis=1) * np.dot(v0, v0))
    return (1.0 - c) / (1.0 + c)


def run_stationary(collide, v):
    """400 steps of collide(v, k) -> the component variances after every 100 steps, and the tallies' sum"""
    var, t = [], np.zeros(4)
    for k in range(1, STATIONARY_STEPS + 1):
        v, tk = collide(v, k)
        t += tk
        if k % STATIONARY_SAMPLE == 0:
            var.append(v.var(axis=0))
    return np.array(var), t


def test_pair_conservation():
    """momentum and energy of every pair, the partner's side included (which the device does not store)"""
    rng = np.random.default_rng(1)
    n = 4096
    v = rng.normal(size=(n, 3))
    coll = R.collisions([dict(q=1.0, m=4.0, n=1.0, vth=0.5, drift=(0.1, 0.0, -0.2)), dict(q=-2.0, m=0.25, n=0.5, vth=2.0),
                         dict(q=1.0, m=1.0, n=3.0, vth=0.0)], strength=0.3, mass=2.0, seed=9, particle0=77)
    pairs = []
    vn, t = R.collide_fo(v, coll, QM, DT, 5, 77 + np.arange(n), pairs)
    assert t[0] == 3 * n and t[1] == 0 and len(pairs) == 3
    ma = coll["mass"]
    for b, va, w, va2, w2, ok in pairs:
        mb = coll["backgrounds"][b]["m"]
        scale = (ma * np.abs(va) + mb * np.abs(w)).max()
        assert np.abs(ma * va + mb * w - ma * va2 - mb * w2).max() <= 8e-16 * scale
        e0 = 0.5 * ma * (va * va).sum(axis=1) + 0.5 * mb * (w * w).sum(axis=1)
        e1 = 0.5 * ma * (va2 * va2).sum(axis=1) + 0.5 * mb * (w2 * w2).sum(axis=1)
        assert (np.abs(e1 - e0) <= 2e-14 * e0).all()
        assert (va2 != va).any(axis=1).all()
    assert np.array_equal(vn, pairs[-1][3])
    # a guiding centre's pairs too: the velocity it is given and the one it is projected from
    rec = np.column_stack([rng.normal(size=(n, 3)), rng.normal(size=n), np.abs(rng.normal(size=n)), np.zeros(n)])
    pairs = []
    R.collide_dk(rec, np.tile([1.0, 2.0, 2.0], (n, 1)), coll, QM, 1.0, DT, 5, np.arange(n), pairs=pairs)
    for b, va, w, va2, w2, ok in pairs:
        mb = coll["backgrounds"][b]["m"]
        assert np.abs(ma * va + mb * w - ma * va2 - mb * w2).max() <= 8e-16 * (ma * np.abs(va) + mb * np.abs(w)).max()


def test_lorentz_limit():
    coll = lorentz_collisions(LORENTZ_V0)
    v0 = np.tile(LORENTZ_V0, (N, 1))
    v, t = R.collide_fo(v0, coll, QM, DT, 1, IDX)
    assert t[0] == N and abs(t[2] / N - 0.01) <= 1e-15
    speed = np.sqrt((v * v).sum(axis=1))
    assert np.abs(speed / np.sqrt(np.dot(LORENTZ_V0, LORENTZ_V0)) - 1.0).max() <= 4e-16
    mean = tan2_half(LORENTZ_V0, v).mean()
    print("mean tan^2(Theta / 2) / sigma^2 =", mean / 0.01)
    assert abs(mean / 0.01 - 1.0) <= 5 * np.sqrt(2.0 / N)


def test_stationarity_and_relaxation():
    coll = stationary_collisions()
    var, t = run_stationary(lambda v, k: R.collide_fo(v, coll, QM, DT, k, IDX), maxwellian(T_B, 21))
    share = t[3] / t[0]
    print("component variances / (T_b / m_a) every 100 steps:", var / (T_B / M_A), "mean sigma^2", t[2] / t[0], "share > 1",
          share)
    assert t[0] == N * STATIONARY_STEPS and 1e-2 <= t[2] / t[0] <= 9e-2
    assert share < 0.01
    assert np.abs(var / (T_B / M_A) - 1.0).max() <= 5 * np.sqrt(2.0 / N)
    hot, _ = run_stationary(lambda v, k: R.collide_fo(v, coll, QM, DT, k, IDX), maxwellian(4 * T_B, 22))
    print("started at 4 T_b:", hot / (T_B / M_A))
    assert (np.diff(hot, axis=0) < 0).all() and (hot[0] < 4 * T_B / M_A).all() and (hot[-1] > T_B / M_A).all()


@pytest.mark.parametrize("B", [(2.0, 0, 0), (0, -3.0, 0), (0, 0, 0.5), (1.0, 1.0, 1.0), (1.0, 1.0, 2.0), (1.0, 2.0, 2.0),
                               (-1.0, 1e-300, 3.0)])
def test_basis(B):
    lenB, b, e1, e2 = R.basis(np.array([B]))
    m = np.array([b[0], e1[0], e2[0]])
    assert np.abs(m @ m.T - np.eye(3)).max() <= 1e-15
    assert np.linalg.det(m) > 0  # b, e1, e2 is right-handed
    assert abs(lenB[0] - np.sqrt(np.dot(B, B))) <= 1e-15 * lenB[0]
    # e_c: the smallest |b_c|, a tie the lowest index: e1 has no component along it
    c = int(np.argmin(np.abs(b[0])))  # (argmin returns the first of equal values)
    assert e1[0, c] == 0.0


def test_guiding_centre_projection():
    rng = np.random.default_rng(4)
    n = 4096
    rec = np.column_stack([rng.normal(size=(n, 3)), rng.normal(size=n), np.abs(rng.normal(size=n)), np.zeros(n)])
    B = np.tile([1.0, 2.0, 2.0], (n, 1)) * (0.5 + rng.random(n))[:, None]
    B[7] = 0.0
    coll = R.collisions([dict(q=1.0, m=4.0, n=1.0, vth=0.5), dict(q=1.0, m=1.0, n=1.0, vth=1.0)], strength=0.05, mass=1.0,
                        seed=2)
    pairs = []
    out, t = R.collide_dk(rec, B, coll, QM, 1.0, DT, 1, np.arange(n), pairs=pairs)
    assert t[0] == 2 * (n - 1) and t[1] == 2  # |B| == 0: both of that particle's collisions are skipped
    assert np.array_equal(out[7], rec[7]) and np.array_equal(out[:, :3], rec[:, :3])
    on = np.arange(n) != 7
    vn = pairs[-1][3]
    lenB = np.sqrt((B[on] ** 2).sum(axis=1))
    assert np.abs(out[on, 3] ** 2 + out[on, 4] ** 2 - (vn * vn).sum(axis=1)).max() <= 4e-15 * (vn * vn).sum(axis=1).max()
    assert np.abs(out[on, 5] - 1.0 * out[on, 4] ** 2 / (2 * lenB)).max() <= 4e-16 * out[on, 5].max()
    assert (out[on, 4] >= 0).all()
    # the first background's velocity is the guiding centre at the drawn gyrophase: its parallel and perpendicular parts
    v = pairs[0][1]
    b = B[on] / lenB[:, None]
    par = (v * b).sum(axis=1)
    assert np.abs(par - rec[on, 3]).max() <= 1e-15 * np.abs(rec[:, 3]).max()
    assert np.abs(np.sqrt(((v - par[:, None] * b) ** 2).sum(axis=1)) - rec[on, 4]).max() <= 1e-15 * rec[:, 4].max()


def test_statistics_do_not_depend_on_the_axis():
    """the energy change's mean under another e_c (the next axis round, never along b here) within sampling error"""
    rng = np.random.default_rng(6)
    rec = np.column_stack([np.zeros((N, 3)), rng.normal(size=N), np.sqrt(rng.normal(size=N) ** 2 + rng.normal(size=N) ** 2),
                           np.zeros(N)])
    B = np.tile([1.0, 2.0, 2.0], (N, 1))
    coll = R.collisions([dict(q=1.0, m=4.0, n=1.0, vth=1.0)], strength=0.2, mass=1.0, seed=8)  # a background at 4 T
    e0 = 0.5 * (rec[:, 3] ** 2 + rec[:, 4] ** 2)
    dE = []
    for axis in (None, 1, 2):  # the definition picks x (|b_x| is the smallest)
        out, _ = R.collide_dk(rec, B, coll, QM, 1.0, DT, 1, IDX, axis=axis)
        dE.append(0.5 * (out[:, 3] ** 2 + out[:, 4] ** 2) - e0)
    assert not np.array_equal(dE[0], dE[1])
    print("mean energy change:", [d.mean() for d in dE], "standard error", dE[0].std() / np.sqrt(N))
    assert dE[0].mean() > 5 * dE[0].std() / np.sqrt(N)  # (the background heats the ensemble: the mean is resolved)
    for d in dE[1:]:
        assert abs(d.mean() - dE[0].mean()) <= 5 * np.sqrt((d.var() + dE[0].var()) / N)


def test_step_gating():
    """every = 3 collides only after steps 3, 6, ... and with dt_c = 3 dt"""
    n = 100
    rng = np.random.default_rng(5)
    p = np.column_stack([rng.random((n, 3)), rng.normal(size=(n, 3))])
    field = A.model("uniform")  # E = B = 0: the push leaves v alone
    bgs = [dict(q=1.0, m=4.0, n=1.0, vth=0.5)]
    coll = R.collisions(bgs, strength=0.1, mass=1.0, every=3, seed=1, particle0=10)
    out = R.trace("EB2B", field, p, 7, None, (1.0, 1.0, 1.0), QM, 1.0, DT, coll, sample_every=1)
    v = out.samples[:, :, 3:]
    assert np.array_equal(v[0], p[:, 3:]) and np.array_equal(v[1], p[:, 3:])
    assert np.array_equal(v[3], v[2]) and np.array_equal(v[4], v[2]) and np.array_equal(v[6], v[5])
    assert (v[2] != v[1]).any(axis=1).all() and (v[5] != v[4]).any(axis=1).all()
    assert out.coll[0] == 2 * n
    # the same numbers from a call that collides every step with three times the step
    one = R.collisions(bgs, strength=0.1, mass=1.0, every=1, seed=1, particle0=10)
    ref3, _ = R.collide_fo(p[:, 3:], one, QM, 3 * DT, 3, 10 + np.arange(n))
    assert np.array_equal(v[2], ref3)
    ref6, _ = R.collide_fo(ref3, one, QM, 3 * DT, 6, 10 + np.arange(n))
    assert np.array_equal(v[5], ref6)
    # composition through step0: 7 steps = 4 + 3
    a = R.trace("EB2B", field, p, 4, None, (1.0, 1.0, 1.0), QM, 1.0, DT, coll)
    b = R.trace("EB2B", field, a.state, 3, None, (1.0, 1.0, 1.0), QM, 1.0, DT, coll, step0=4)
    assert np.array_equal(b.state, out.state)
