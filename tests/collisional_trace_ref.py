"""The collisional model traces (include/xpic_hip.h: xpic_trace_collisions) restated in numpy float64: the second
statement the kernels of xpic_amd/csrc/collide_trace.hip are held to.  An extension: the reference has no collision
operator.

  step_key, streams      the stream of (seed, particle, step k, background b): the constants of xpic_amd/csrc/collide_pair.h
                         stated a second time; draws(st) -> a1 a2 a3 a4, a5 and the state u1 u2 u3 come from
  partner                the partner's velocity from a1 .. a4
  basis, gc_to_v, v_to_gc    the basis across b, a guiding centre as a velocity and back
  collide_fo, collide_dk the collisions of one step (every background in turn), the pair collision itself being
                         tests/collisions_ref.py's collide_pairs
  step, trace            a push of tests/analytic_trace_ref.py, then the collisions; the open trace around it

`coll` is a dict: backgrounds (a list of dicts q, m, n, vth, drift), strength, mass, every, seed, particle0 -- the
arguments of xpic_amd.trace_collisions.  Everything is rounded operation by operation in the kernel's order; log, cos and
sin come from another library than the device's and may differ in the last place."""
import collections

import numpy as np

import analytic_trace_ref as A
import collisions_ref as CR
import open_trace_ref as OT

M64 = CR.M64
C_STEP = 0xD1342543DE82EF95      # step key <- (seed, k)
C_PARTICLE = 0xD6E8FEB86659FD93  # particle key <- (step key, particle0 + q)
C_BG = 0xA0761D6478BD642F        # stream state <- (particle key, b + 1)
BG_MAX = 4

CollRef = collections.namedtuple("CollRef", "state samples exit_step alive removed iterations_sum iterations_max coll")


def collisions(backgrounds, strength, mass, every=1, seed=0, particle0=0):
    return dict(backgrounds=[dict(b) for b in backgrounds], strength=strength, mass=mass, every=every, seed=seed,
                particle0=particle0)


def step_key(seed, k):
    x, _ = CR._splitmix_int(seed)
    x ^= (k * C_STEP) & M64
    return CR._splitmix_int(x)[1]


def streams(seed, k, particles, b):
    """the stream states of the global particle indices `particles` at step k against background b"""
    with np.errstate(over="ignore"):
        pk = CR._splitmix(np.uint64(step_key(seed, k)) ^ (CR._u64(particles) * np.uint64(C_PARTICLE)))[1]
    return CR._splitmix(pk ^ np.uint64(((b + 1) * C_BG) & M64))[1]


def draws(st):
    """-> (a1, a2, a3, a4), a5, the state behind them (u1 u2 u3 follow)"""
    a = []
    for _ in range(5):
        st, x = CR._u01(st)
        a.append(x)
    return a[:4], a[4], st


def partner(bg, a):
    a1, a2, a3, a4 = a
    r1, r3 = np.sqrt(-2.0 * np.log(a1)), np.sqrt(-2.0 * np.log(a3))
    g = [r1 * np.cos(2.0 * np.pi * a2), r1 * np.sin(2.0 * np.pi * a2), r3 * np.cos(2.0 * np.pi * a4)]
    drift = bg.get("drift", (0.0, 0.0, 0.0))
    return np.column_stack([drift[c] + bg["vth"] * g[c] for c in range(3)])


def coefficients(coll, qm, dt):
    """per background (cdt, fa, fb): sigma^2 = cdt / |u|^3, v += fa du, w -= fb du"""
    ma = coll["mass"]
    qa, dtc = qm * ma, float(coll["every"]) * dt
    out = []
    for bg in coll["backgrounds"]:
        mab = ma * bg["m"] / (ma + bg["m"])
        c0 = coll["strength"] * (qa * qa) * (bg["q"] * bg["q"]) / (mab * mab)
        out.append((c0 * bg["n"] * dtc, mab / ma, mab / bg["m"]))
    return out


def active(coll):
    return coll is not None and len(coll["backgrounds"]) > 0 and coll["strength"] != 0.0


def _tally(t, ok, s2):
    fin = ok & (s2 <= np.finfo(np.float64).max)
    t += [ok.sum(), (~ok).sum(), s2[fin].sum(), (s2[ok] > 1.0).sum()]


def collide_fo(v, coll, qm, dt, k, particles, pairs=None):
    """the collisions of step k for velocities v [n][3] of the global particles `particles` -> (v', tallies [4]).  pairs: a
    list that receives (background, v, w, v', w', collided) of every collision, the partner's side included"""
    v = np.array(v, dtype=np.float64)
    t = np.zeros(4)
    for b, (bg, (cdt, fa, fb)) in enumerate(zip(coll["backgrounds"], coefficients(coll, qm, dt))):
        a, _, st = draws(streams(coll["seed"], k, particles, b))
        w = partner(bg, a)
        vn, wn, ok, s2, _ = CR.collide_pairs(v, w, cdt, st, 0, fa, fb)
        if pairs is not None:
            pairs.append((b, v.copy(), w, vn.copy(), wn, ok))
        _tally(t, ok, s2)
        v = vn
    return v, t


def basis(B, axis=None):
    """-> |B|, b, e1, e2 for fields B [n][3] with |B| > 0.  axis: None, the definition's e_c (the smallest |b_c|, a tie the
    lowest index); a number or an array forces another choice (the statistics must not depend on it)"""
    B = np.asarray(B, dtype=np.float64)
    lenB = np.sqrt(B[:, 0] * B[:, 0] + B[:, 1] * B[:, 1] + B[:, 2] * B[:, 2])
    b = B / lenB[:, None]
    ab = np.abs(b)
    c = np.where(ab[:, 1] < ab[:, 0], 1, 0)
    least = np.where(c == 1, ab[:, 1], ab[:, 0])
    c = np.where(ab[:, 2] < least, 2, c)
    if axis is not None:
        c = np.broadcast_to(np.asarray(axis), c.shape)
    z = np.zeros(len(b))
    cross = [np.column_stack([z, b[:, 2], -b[:, 1]]), np.column_stack([-b[:, 2], z, b[:, 0]]),
             np.column_stack([b[:, 1], -b[:, 0], z])]  # b x e_x, b x e_y, b x e_z
    x = np.where((c == 0)[:, None], cross[0], np.where((c == 1)[:, None], cross[1], cross[2]))
    l = np.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2])
    e1 = x / l[:, None]
    e2 = np.column_stack([b[:, 1] * e1[:, 2] - b[:, 2] * e1[:, 1], b[:, 2] * e1[:, 0] - b[:, 0] * e1[:, 2],
                          b[:, 0] * e1[:, 1] - b[:, 1] * e1[:, 0]])
    return lenB, b, e1, e2


def gc_to_v(ppar, pperp, psi, b, e1, e2):
    cs, sn = np.cos(psi)[:, None], np.sin(psi)[:, None]
    return ppar[:, None] * b + pperp[:, None] * (cs * e1 + sn * e2)


def v_to_gc(v, b, lenB, mp):
    """-> p_parallel', p_perp', mu_p'"""
    par = v[:, 0] * b[:, 0] + v[:, 1] * b[:, 1] + v[:, 2] * b[:, 2]
    x, y, z = v[:, 0] - par * b[:, 0], v[:, 1] - par * b[:, 1], v[:, 2] - par * b[:, 2]
    perp = np.sqrt(x * x + y * y + z * z)
    return par, perp, mp * perp * perp / (2.0 * lenB)


def collide_dk(rec, B, coll, qm, mp, dt, k, particles, axis=None, pairs=None):
    """the collisions of step k for guiding centres rec [n][6] in the fields B [n][3] at their positions -> (records',
    tallies [4]).  |B| == 0: the particle's collisions are skipped and counted"""
    rec = np.array(rec, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    particles = np.asarray(particles)
    t = np.zeros(4)
    nbg = len(coll["backgrounds"])
    lenB_all = np.sqrt(B[:, 0] * B[:, 0] + B[:, 1] * B[:, 1] + B[:, 2] * B[:, 2])
    on = lenB_all != 0.0
    t[1] += nbg * int((~on).sum())
    if not on.any():
        return rec, t
    i = np.flatnonzero(on)
    lenB, b, e1, e2 = basis(B[i], None if axis is None else np.broadcast_to(np.asarray(axis), on.shape)[i])
    for k_b, (bg, (cdt, fa, fb)) in enumerate(zip(coll["backgrounds"], coefficients(coll, qm, dt))):
        a, a5, st = draws(streams(coll["seed"], k, particles[i], k_b))
        w = partner(bg, a)
        v = gc_to_v(rec[i, 3], rec[i, 4], 2.0 * np.pi * a5, b, e1, e2)
        vn, wn, ok, s2, _ = CR.collide_pairs(v, w, cdt, st, 0, fa, fb)
        if pairs is not None:
            pairs.append((k_b, v, w, vn, wn, ok))
        _tally(t, ok, s2)
        par, perp, mu = v_to_gc(vn, b, lenB, mp)
        j = i[ok]  # (a skipped collision leaves the record's bits)
        rec[j, 3], rec[j, 4], rec[j, 5] = par[ok], perp[ok], mu[ok]
    return rec, t


def step(kind, field, p, qm, mp, dt, coll, k, particles, **kw):
    """the push of `kind` ("dk", "CN" or a Chin id), then the collisions of global step k -> (records, iteration counts,
    tallies [4])"""
    pn, its = A.pusher(kind, field, qm, mp, dt, **kw)(p)
    t = np.zeros(4)
    if active(coll) and k % coll["every"] == 0 and len(pn):
        if kind == "dk":
            pn, t = collide_dk(pn, field(pn[:, :3])[1], coll, qm, mp, dt, k, particles)
        else:
            pn = np.array(pn)
            pn[:, 3:], t = collide_fo(pn[:, 3:], coll, qm, dt, k, particles)
    return pn, its, t


def trace(kind, field, p, steps, geometry, d, qm, mp, dt, coll, sample_every=0, exit_step=None, step0=0, **kw):
    """open_trace_ref.trace_open around step(): the step completed k-th in all (k = step0 + the steps of this call + 1)
    collides; the particles' global indices are particle0 + their place in the batch.  geometry None: no region"""
    geometry = OT.EVERYWHERE if geometry is None else geometry
    p = np.array(p, dtype=np.float64).reshape(-1, 6)
    n = p.shape[0]
    ex = np.full(n, -1, dtype=np.int64) if exit_step is None else np.array(exit_step, dtype=np.int64)
    nsamp = steps // sample_every if sample_every else 0
    samples = np.zeros((nsamp, n, 6)) if sample_every else None
    alive = np.zeros(nsamp, dtype=np.int64) if sample_every else None
    tot, mx = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32)
    removed, t = 0, np.zeros(4)
    p0 = coll["particle0"] if coll is not None else 0
    for s in range(steps):
        a = np.flatnonzero(ex < 0)
        out = a[~OT.keep(geometry, p[a, :3], d)]
        ex[out] = step0 + s
        removed += len(out)
        a = np.flatnonzero(ex < 0)
        if len(a):
            pn, its, ts = step(kind, field, p[a], qm, mp, dt, coll, step0 + s + 1, p0 + a, **kw)
            p[a] = pn
            tot[a] += its
            mx[a] = np.maximum(mx[a], its)
            t += ts
        if sample_every and (s + 1) % sample_every == 0:
            samples[(s + 1) // sample_every - 1] = p
            alive[(s + 1) // sample_every - 1] = (ex < 0).sum()
    return CollRef(p, samples, ex, alive, removed, tot, mx, t)
