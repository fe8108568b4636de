"""Plain numpy restatement of the time loop of the reference's grid tests and of all seven maxima of its ComparisonStats,
the model the kernel of xpic_amd/csrc/compare_trace.hip is tested against:

  grid_from_model(...)   FieldContext::initialize, tests/drift_kinetic_push/drift_kinetic_push.h:176-209: every component of
                         node (i, j, k) is the model at (i dx, j dy, k dz)
  compare_step(...)      update_comparison_stats, :293-329, all of it; the last four errors are paired_trace_ref's with
                         B = B_analytical (:314)
  triplet_trace(...)     the loop of tests/drift_kinetic_push/drift_kinetic_grid_boris_ex1.cpp:79-98: analytic_trace_ref's
                         dk_push and chin_step / cn_step on the model, drift_kinetic_ref's push and interpolate on the grid

A guiding centre is {x, y, z, p_parallel, p_perp, mu_p}, an orbit {x, y, z, px, py, pz}; grid fields are [nz][ny][nx][3].
Everything is vectorised over the triplets."""
import collections

import numpy as np

import analytic_trace_ref as A
import drift_kinetic_ref as DK
import full_orbit_ref as FO
import paired_trace_ref as P

STATS = ("B", "gradB", "pos", "z", "p_parallel", "mu", "energy")

Triplet = collections.namedtuple(
    "Triplet", "fo gm gg stats curve errors fo_sum fo_max dm_total dm_max dg_total dg_max")


def grid_from_model(field, n, d):
    """-> (E, B, gradB), each [nz][ny][nx][3]"""
    k, j, i = np.meshgrid(np.arange(n[2]), np.arange(n[1]), np.arange(n[0]), indexing="ij")
    r = np.column_stack([i.ravel() * d[0], j.ravel() * d[1], k.ravel() * d[2]])
    return tuple(f.reshape(n[2], n[1], n[0], 3) for f in field(r))


def compare_step(gm, gg, fo, Ba, gBa, Bg, gBg, mp):
    """-> [n][7]: err_B, err_gradB, err_pos, err_z, err_parallel, err_mu, err_energy of every triplet; gm, gg: the
    analytic and the grid centre after the step"""
    e = np.empty((len(fo), 7))
    e[:, 0] = DK._len(Ba - Bg)
    e[:, 1] = DK._len(gBa - gBg)
    e[:, 2] = DK._len(gm[:, :3] - gg[:, :3])
    e[:, 3:] = P.compare_step(gg, fo, Ba, mp)
    return e


def fo_step(field, scheme, fo, qm, dt, atol=FO.CN_ATOL, rtol=FO.CN_RTOL, maxit=FO.CN_MAXIT):
    """the orbit's step on the model -> (records, iteration counts)"""
    if scheme == "CN":
        return A.cn_step(field, fo, qm, dt, atol=atol, rtol=rtol, maxit=maxit)
    return A.chin_step(scheme, field, fo, qm, dt), np.zeros(len(fo), dtype=np.int32)


def triplet_trace(field, grid, d, fo, gm, gg, steps, scheme, qm, mp, dt, sample_every=0, stats=None, eps=1e-12, delta=1e-12,
                  dk_maxit=30, atol=FO.CN_ATOL, rtol=FO.CN_RTOL, maxit=FO.CN_MAXIT):
    """field: analytic_trace_ref.model(...); grid: (E, B, gradB or None), or None for the grid-less pair (gg is not read,
    statistics 0 .. 2 are left alone and the analytic centre stands in the grid centre's place in 3 .. 6).
    -> Triplet; stats enters as the running maxima (None: zeros), curve[k] is the maximum over the triplets of the errors
    at step (k + 1) sample_every, accumulated from 0 by paired_trace_ref.accumulate; errors is [steps][n][7]"""
    fo = np.array(fo, dtype=np.float64).reshape(-1, 6)
    gm = np.array(gm, dtype=np.float64).reshape(-1, 6)
    n = fo.shape[0]
    j0 = 0 if grid is not None else 3
    if grid is not None:
        gg = np.array(gg, dtype=np.float64).reshape(-1, 6)
    else:
        gg = None
    stats = np.zeros((n, 7)) if stats is None else np.array(stats, dtype=np.float64).reshape(n, 7)
    curve = np.zeros((steps // sample_every, 7)) if sample_every else None
    errors = np.zeros((steps, n, 7))
    cnt = {k: np.zeros(n, dtype=np.int64) for k in ("fo_sum", "dm_total", "dg_total")}
    mx = {k: np.zeros(n, dtype=np.int32) for k in ("fo_max", "dm_max", "dg_max")}
    for k in range(1, steps + 1):
        gm, it = A.dk_push(field, gm, qm, mp, dt, eps=eps, delta=delta, maxit=dk_maxit)
        cnt["dm_total"] += it
        mx["dm_max"] = np.maximum(mx["dm_max"], it)
        if grid is not None:
            old = gg
            gg, it = DK.push(grid[0], grid[1], grid[2], d, old, qm, mp, dt, eps=eps, delta=delta, maxit=dk_maxit)
            cnt["dg_total"] += it
            mx["dg_max"] = np.maximum(mx["dg_max"], it)
        fo, it = fo_step(field, scheme, fo, qm, dt, atol, rtol, maxit)
        cnt["fo_sum"] += it
        mx["fo_max"] = np.maximum(mx["fo_max"], it)
        _, Ba, gBa = field(gm[:, :3])
        if grid is not None:
            _, Bg, gBg = DK.interpolate(grid[0], grid[1], grid[2], d, gg[:, :3], old[:, :3])
            e = compare_step(gm, gg, fo, Ba, gBa, Bg, gBg, mp)
        else:
            e = np.zeros((n, 7))
            e[:, 3:] = P.compare_step(gm, fo, Ba, mp)
        errors[k - 1] = e
        stats[:, j0:] = P.accumulate(stats[:, j0:], e[:, j0:])
        if sample_every and k % sample_every == 0:
            row = np.zeros(7)
            for q in range(n):
                row[j0:] = P.accumulate(row[j0:], e[q, j0:])
            curve[k // sample_every - 1] = row
    return Triplet(fo, gm, gg, stats, curve, errors, cnt["fo_sum"], mx["fo_max"], cnt["dm_total"], mx["dm_max"],
                   cnt["dg_total"], mx["dg_max"])
