"""The reference's two particle diagnostics restated in numpy, from a list of points and their storage cells.

* `moment(...)`  -- DistributionMoment::collect (src/diagnostics/distribution_moment.cpp:128-298) with its region rule
  (:59-108, :157-210): a particle counts iff its storage cell lies in the region; a deposit lands iff its cell lies in the
  region, after a periodic wrap on each axis the region spans in full.
* `velocity_distribution(...)` -- VelocityDistribution::collect (src/diagnostics/velocity_distribution.cpp:112-200) with
  the bin ranges of set_regions (:57-68) as written: BOTH axes start at ROUND_STEP(vx_min, dvx) and have
  ROUND_STEP(vx_max - vx_min, dvx) bins.

Points are `struct Point` records {x, y, z, vx, vy, vz}; `cells` are flat global storage cell indices (z ny + y) nx + x.
"""
import numpy as np

MOMENTS = ("density", "current", "momentum_flux", "momentum_flux_diag", "momentum_flux_cyl", "momentum_flux_diag_cyl")
DOF = {"density": 1, "current": 3, "momentum_flux": 6, "momentum_flux_diag": 3, "momentum_flux_cyl": 6,
       "momentum_flux_diag_cyl": 3}


def cround(x):
    """std::round: half away from zero (np.round rounds half to even)"""
    x = np.asarray(x, dtype=np.float64)
    t = np.trunc(x)
    return t + np.sign(x) * (np.abs(x - t) >= 0.5)


def v_cyl(pts, n, d):
    """_get_v_cyl (:260-277): about (geom_x / 2, geom_y / 2); a point on the axis keeps its Cartesian components"""
    x = pts[:, 0] - 0.5 * (n[0] * d[0])
    y = pts[:, 1] - 0.5 * (n[1] * d[1])
    r = np.hypot(x, y)
    v = pts[:, 3:6]
    with np.errstate(divide="ignore", invalid="ignore"):
        vr = (+x * v[:, 0] + y * v[:, 1]) / r
        va = (-y * v[:, 0] + x * v[:, 1]) / r
    with np.errstate(divide="ignore"):
        axis = np.isinf(1.0 / r)  # std::isinf(1.0 / r)
    vr = np.where(axis, v[:, 0], vr)
    va = np.where(axis, v[:, 1], va)
    return np.stack([vr, va, v[:, 2]], axis=1)


def moment_values(name, pts, q, m, n, d):
    """get_density ... get_momentum_flux_diag_cyl (:212-298), components in the reference's order"""
    v = pts[:, 3:6]
    if name == "density":
        return np.ones((len(pts), 1))
    if name == "current":
        return np.stack([q * v[:, 0], q * v[:, 1], q * v[:, 2]], axis=1)
    if name.endswith("_cyl"):
        v = v_cyl(pts, n, d)
    if name.startswith("momentum_flux_diag"):
        return np.stack([m * v[:, 0] * v[:, 0], m * v[:, 1] * v[:, 1], m * v[:, 2] * v[:, 2]], axis=1)
    return np.stack([m * v[:, 0] * v[:, 0], m * v[:, 0] * v[:, 1], m * v[:, 0] * v[:, 2],
                     m * v[:, 1] * v[:, 1], m * v[:, 1] * v[:, 2], m * v[:, 2] * v[:, 2]], axis=1)


def moment(name, pts, cells, q, m, n_Np, n, d, region=None):
    """-> array [nz][ny][nx][dof] over the whole box, zero outside the region.  region: (start xyz, size xyz) or None."""
    n = tuple(int(v) for v in n)
    start = np.array([0, 0, 0]) if region is None else np.asarray(region, dtype=np.int64).reshape(6)[:3]
    size = np.array(n) if region is None else np.asarray(region, dtype=np.int64).reshape(6)[3:]
    end = start + size
    full = (start == 0) & (size == np.array(n))
    dof = DOF[name]
    out = np.zeros((n[2], n[1], n[0], dof))
    cells = np.asarray(cells, dtype=np.int64)
    g = np.stack([cells % n[0], (cells // n[0]) % n[1], cells // (n[0] * n[1])], axis=1)
    keep = np.all((g >= start) & (g < end), axis=1)  # is_point_within_bounds(vg, gstart, gsize) (:179-180)
    pts = np.asarray(pts, dtype=np.float64)[keep]
    if len(pts) == 0:
        return out
    mv = moment_values(name, pts, q, m, n, d)
    pr = pts[:, :3] / np.array(d)  # Shape::make_r
    st = cround(pr - 1.0).astype(np.int64)  # Shape::make_start(p_r, shr = 1)
    w = []
    for t in range(2):
        dd = np.abs(pr - ((st + t).astype(np.float64) + 0.5))
        w.append(np.where(dd <= 1.0, 1.0 - dd, 0.0))  # spline_of_1st_order
    for i in range(8):
        ix, iy, iz = i % 2, (i // 2) % 2, i // 4
        cache = w[ix][:, 0] * w[iy][:, 1] * w[iz][:, 2]
        si = cache * n_Np
        tgt = st + np.array([ix, iy, iz])
        for a in range(3):
            if full[a]:
                tgt[:, a] %= n[a]
        ok = np.all((tgt >= start) & (tgt < end), axis=1)
        for j in range(dof):
            np.add.at(out[..., j], (tgt[ok, 2], tgt[ok, 1], tgt[ok, 0]), mv[ok, j] * si[ok])
    return out


def vsizes(vmin, vmax, dv):
    """set_regions (:57-68) as written: (vstart, vsize), the same for both axes"""
    return int(cround(vmin[0] / dv[0])), int(cround((vmax[0] - vmin[0]) / dv[0]))


def aabb(geometry, n, d):
    """VelocityDistributionBuilder (builders/velocity_distribution_builder.cpp:32-77): (start xyz, end xyz) in cells"""
    if geometry["name"] in ("box", "BoxGeometry"):
        lo, hi = np.asarray(geometry["min"], float), np.asarray(geometry["max"], float)
    else:
        c = np.asarray(geometry["center"], float)
        ext = np.array([geometry["radius"], geometry["radius"], 0.5 * geometry["height"]])
        lo, hi = c - ext, c + ext
    s = np.floor(lo / np.array(d)).astype(np.int64)
    return s, s + (np.floor(hi / np.array(d)).astype(np.int64) - s)


def within(geometry, r):
    """WithinBox / WithinCylinder (src/utils/geometries.cpp:3-19) of points r[:, 3]"""
    if geometry["name"] in ("box", "BoxGeometry"):
        lo, hi = np.asarray(geometry["min"], float), np.asarray(geometry["max"], float)
        return np.all((lo <= r) & (r < hi), axis=1)
    c = np.asarray(geometry["center"], float)
    p = r - c
    return (np.abs(p[:, 2]) < 0.5 * geometry["height"]) & ((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) <= geometry["radius"] ** 2)


def project(projector, pts, n, d):
    v = pts[:, 3:6]
    if projector == "vx_vy":
        return v[:, 0], v[:, 1]
    if projector == "vz_vxy":
        return v[:, 2], np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + 0.0 * 0.0)
    c = v_cyl(pts, n, d)
    return c[:, 0], c[:, 1]


def velocity_distribution(projector, geometry, pts, cells, n_Np, n, d, vmin=(-1.0, -1.0), vmax=(1.0, 1.0), dv=(0.1, 0.1)):
    """-> (hist [vsize][vsize], vstart)"""
    n = tuple(int(v) for v in n)
    vs, vn = vsizes(vmin, vmax, dv)
    hist = np.zeros((vn, vn))
    cells = np.asarray(cells, dtype=np.int64)
    g = np.stack([cells % n[0], (cells // n[0]) % n[1], cells // (n[0] * n[1])], axis=1)
    a0, a1 = aabb(geometry, n, d)
    keep = np.all((g >= a0) & (g < a1), axis=1)
    keep &= within(geometry, (g + 0.5) * np.array(d))  # the cell centre (:135-142)
    pts = np.asarray(pts, dtype=np.float64)[keep]
    a, b = project(projector, pts, n, d)
    bx, by = cround(a / dv[0]), cround(b / dv[1])  # ROUND_STEP
    ok = (bx >= vs) & (bx < vs + vn) & (by >= vs) & (by < vs + vn)
    np.add.at(hist, ((by[ok] - vs).astype(np.int64), (bx[ok] - vs).astype(np.int64)), n_Np)
    return hist, (vs, vs)
