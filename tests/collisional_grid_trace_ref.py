"""The collisional grid traces and the background profiles (include/xpic_hip.h: xpic_full_orbit_trace_collisional,
xpic_background_from_sort) restated in numpy float64: the second statement the kernels of xpic_amd/csrc/collide_trace.hip
and xpic_amd/csrc/background.hip are held to.  An extension: the reference has no collision operator.

Nothing of the collision or of the pushes is stated here a second time: the streams, the draws, the partner, the basis and
the tallies are tests/collisional_trace_ref.py's functions, the pair collision tests/collisions_ref.py's, the pushes and
gathers tests/full_orbit_ref.py's and tests/drift_kinetic_ref.py's, the region rule tests/open_trace_ref.py's.  What is
added is the cell lookup, the per-cell moments, and the loops that join them.

  cell_index        floor(r / d) per axis, folded by the true modulus -> the local cell, x fastest
  moments           per cell n = (n / Np) N, u = (sum v) / N, vth = sqrt(sum |v - u|^2 / (3 N)); sums by math.fsum, so the
                    restatement's own error is one rounding per operation behind an exact sum
  collide_fo / _dk  the collisions of one step: background b is coll's uniform one (profile[b] == -1) or slot profile[b] of
                    `slots` at each particle's cell; a cell with n == 0 is inert
  step, trace       a grid push, then the collisions; the open trace around it

A profile is a dict n [nz][ny][nx], vth [nz][ny][nx], drift [nz][ny][nx][3]; `grid` is (n, d), the cell counts and the
spacings (x, y, z); `fields` is (E, B, gradB or None) as the grid restatements take them."""
import math

import numpy as np

import collisional_trace_ref as CT
import collisions_ref as CR
import drift_kinetic_ref as DK
import full_orbit_ref as FO
import open_trace_ref as OT

BG_MAX = CT.BG_MAX


def cell_index(r, n, d, axes=(0, 1, 2), fold=np.mod):
    """the local cells of positions r [m][3].  axes and fold are the definition's; another choice is a bug a test must
    catch (axes: which coordinate counts along x, y, z; fold: np.fmod truncates where the true modulus folds)"""
    r = np.asarray(r, dtype=np.float64).reshape(-1, 3)
    i = [fold(np.floor(r[:, a] / d[a]), n[a]).astype(np.int64) for a in range(3)]
    i = [i[a] for a in axes]
    return (i[2] * n[1] + i[1]) * n[0] + i[0]


def profile(n, vth, drift=None, shape=None):
    """a profile dict from arrays or scalars broadcast to shape = (nz, ny, nx)"""
    shape = np.shape(n) if shape is None else tuple(shape)
    drift = np.zeros(3) if drift is None else drift
    return dict(n=np.array(np.broadcast_to(np.asarray(n, dtype=np.float64), shape)),
                vth=np.array(np.broadcast_to(np.asarray(vth, dtype=np.float64), shape)),
                drift=np.array(np.broadcast_to(np.asarray(drift, dtype=np.float64), shape + (3,))))


def moments(v, cells, ncell, weight, ddof=0):
    """the moments of records with velocities v [m][3] in local cells `cells` -> n [ncell], vth [ncell], u [ncell][3].
    ddof: 0 is the definition (vth^2 = sum / (3 N)); 1 divides by N - 1, the bug a test must catch"""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    n, vth, u = np.zeros(ncell), np.zeros(ncell), np.zeros((ncell, 3))
    for c in range(ncell):
        vc = v[np.asarray(cells) == c]
        N = len(vc)
        n[c] = weight * float(N)
        if N == 0:
            continue
        u[c] = [math.fsum(vc[:, k]) / float(N) for k in range(3)]
        dd = vc - u[c]
        s = math.fsum((dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2])
        vth[c] = np.sqrt(s / (3.0 * float(N - ddof))) if N > ddof else 0.0
    return n, vth, u


def as_profile(n, vth, u, shape):
    return dict(n=n.reshape(shape), vth=vth.reshape(shape), drift=u.reshape(tuple(shape) + (3,)))


def met(bg, slot, slots, grid, r, idx, **lookup):
    """of the particles idx (indices into r), those that meet somebody of this background, and the background as they see
    it: coll's own dict for slot -1, per-particle arrays n, vth, drift read at their cells otherwise"""
    if slot < 0:
        return idx, bg
    n, d = grid
    p = slots[slot]
    cells = cell_index(r[idx], n, d, **lookup)
    dens = p["n"].reshape(-1)[cells]
    on = dens > 0.0
    c = cells[on]
    drift = p["drift"].reshape(-1, 3)[c]
    return idx[on], dict(q=bg["q"], m=bg["m"], n=dens[on], vth=p["vth"].reshape(-1)[c],
                         drift=(drift[:, 0], drift[:, 1], drift[:, 2]))


def _slots_of(coll, prof):
    return [-1] * len(coll["backgrounds"]) if prof is None else list(prof)


def collide_fo(v, r, coll, prof, slots, grid, qm, dt, k, particles, pairs=None, **lookup):
    """the collisions of step k for velocities v [m][3] at the positions r -> (v', tallies [4])"""
    v, r, particles = np.array(v, dtype=np.float64), np.asarray(r, dtype=np.float64), np.asarray(particles)
    t = np.zeros(4)
    for b, (bg, s) in enumerate(zip(coll["backgrounds"], _slots_of(coll, prof))):
        i, seen = met(bg, s, slots, grid, r, np.arange(len(v)), **lookup)
        if not len(i):
            continue
        cdt, fa, fb = CT.coefficients(dict(coll, backgrounds=[seen]), qm, dt)[0]
        a, _, st = CT.draws(CT.streams(coll["seed"], k, particles[i], b))
        w = CT.partner(seen, a)
        vn, wn, ok, s2, _ = CR.collide_pairs(v[i], w, cdt, st, 0, fa, fb)
        if pairs is not None:
            pairs.append((b, i, v[i].copy(), w, vn.copy(), wn, ok, fa, fb))
        CT._tally(t, ok, s2)
        v[i] = vn
    return v, t


def collide_dk(rec, B, coll, prof, slots, grid, qm, mp, dt, k, particles, **lookup):
    """the collisions of step k for guiding centres rec [m][6] in the fields B [m][3] at their positions -> (records',
    tallies [4]).  |B| == 0: the collisions of the backgrounds the particle would have met are skipped and counted"""
    rec, B, particles = np.array(rec, dtype=np.float64), np.asarray(B, dtype=np.float64), np.asarray(particles)
    t = np.zeros(4)
    lenB_all = np.sqrt(B[:, 0] * B[:, 0] + B[:, 1] * B[:, 1] + B[:, 2] * B[:, 2])
    for b, (bg, s) in enumerate(zip(coll["backgrounds"], _slots_of(coll, prof))):
        dead, _ = met(bg, s, slots, grid, rec[:, :3], np.flatnonzero(lenB_all == 0.0), **lookup)
        t[1] += len(dead)
        i, seen = met(bg, s, slots, grid, rec[:, :3], np.flatnonzero(lenB_all != 0.0), **lookup)
        if not len(i):
            continue
        lenB, bb, e1, e2 = CT.basis(B[i])
        cdt, fa, fb = CT.coefficients(dict(coll, backgrounds=[seen]), qm, dt)[0]
        a, a5, st = CT.draws(CT.streams(coll["seed"], k, particles[i], b))
        w = CT.partner(seen, a)
        v = CT.gc_to_v(rec[i, 3], rec[i, 4], 2.0 * np.pi * a5, bb, e1, e2)
        vn, wn, ok, s2, _ = CR.collide_pairs(v, w, cdt, st, 0, fa, fb)
        CT._tally(t, ok, s2)
        par, perp, mu = CT.v_to_gc(vn, bb, lenB, mp)
        j = i[ok]
        rec[j, 3], rec[j, 4], rec[j, 5] = par[ok], perp[ok], mu[ok]
    return rec, t


def push(kind, fields, d, p, qm, mp, dt, **kw):
    """one grid step of `kind` ("dk", "CN" or a Chin id) -> (records, iteration counts)"""
    E, B, gradB = fields
    if kind == "dk":
        return DK.push(E, B, gradB, d, p, qm, mp, dt, **kw)
    if kind == "CN":
        return FO.cn_step(E, B, d, p, qm, dt, **kw)
    return FO.step(kind, E, B, d, p, qm, dt), np.zeros(len(p), dtype=np.int32)


def collide(kind, fields, grid, pn, qm, mp, dt, coll, prof, slots, k, particles, **lookup):
    """the collisions of global step k on pushed records pn -> (records, tallies [4])"""
    t = np.zeros(4)
    if not (CT.active(coll) and k % coll["every"] == 0 and len(pn)):
        return pn, t
    if kind == "dk":
        (Bp,) = DK.interpolate_B([fields[1]], grid[1], pn[:, :3])  # (the B_p of DK.interpolate for the segment (r, r))
        return collide_dk(pn, Bp, coll, prof, slots, grid, qm, mp, dt, k, particles, **lookup)
    pn = np.array(pn)
    pn[:, 3:], t = collide_fo(pn[:, 3:], pn[:, :3], coll, prof, slots, grid, qm, dt, k, particles, **lookup)
    return pn, t


def step(kind, fields, grid, p, qm, mp, dt, coll, prof, slots, k, particles, **kw):
    pn, its = push(kind, fields, grid[1], p, qm, mp, dt, **kw)
    pn, t = collide(kind, fields, grid, pn, qm, mp, dt, coll, prof, slots, k, particles)
    return pn, its, t


def trace(kind, fields, grid, p, steps, geometry, qm, mp, dt, coll, prof=None, slots=None, sample_every=0, exit_step=None,
          step0=0, visits=None, **kw):
    """the open trace (geometry None: no region) with the collisions of step k = step0 + the steps of this call + 1.
    visits: a list that receives (k, the global indices of the particles stepped, their pushed positions) per step"""
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
        out = a[~OT.keep(geometry, p[a, :3], grid[1])]
        ex[out] = step0 + s
        removed += len(out)
        a = np.flatnonzero(ex < 0)
        if len(a):
            pn, its = push(kind, fields, grid[1], p[a], qm, mp, dt, **kw)
            if visits is not None:
                visits.append((step0 + s + 1, p0 + a, np.array(pn[:, :3])))
            pn, ts = collide(kind, fields, grid, pn, qm, mp, dt, coll, prof, slots, step0 + s + 1, p0 + a)
            p[a] = pn
            tot[a] += its
            mx[a] = np.maximum(mx[a], its)
            t += ts
        if sample_every and (s + 1) % sample_every == 0:
            samples[(s + 1) // sample_every - 1] = p
            alive[(s + 1) // sample_every - 1] = (ex < 0).sum()
    return CT.CollRef(p, samples, ex, alive, removed, tot, mx, t)
