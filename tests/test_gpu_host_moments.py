"""The host executable with the reference's DistributionMoment (all moments, regions) and VelocityDistribution entries:
file names and sizes as the reference writes them, contents equal to tests/moments_ref.py applied to the particles of the
SimulationBackup taken at the same step."""
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import moments_ref as M  # noqa: E402

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "xpic_amd", "host", "xpic_hip.out")
GOLD = os.path.join(ROOT, "tests", "golden")


def _f32(path):
    return np.fromfile(path, dtype=np.float32)


def _close32(got, ref):
    """equal at float32 rounding: the device's fp64 sums differ from numpy's in the last bits, a rounding may flip"""
    ref = np.asarray(ref, dtype=np.float64).ravel()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.abs(ref).max() > 0
    err = np.abs(got.astype(np.float64) - ref)
    assert np.all(err <= 2.4e-7 * np.abs(ref) + 1e-12 * np.abs(ref).max()), err.max()


def test_host_moments_and_velocity_distribution(tmp_path):
    cfg = json.load(open(os.path.join(GOLD, "ecsim_ex1", "config.json")))
    dt = cfg["Geometry"]["dt"]
    cfg["Geometry"]["t"] = 4 * dt
    cfg["Geometry"]["diagnose_period"] = 2 * dt
    cfg["OutputDirectory"] = str(tmp_path)
    cyl = {"name": "CylinderGeometry", "center": [2.5, 2.5, 2.5], "radius": 1.5, "height": 3.0}
    vd = {"dv": [0.05, 0.07], "vmin": [-0.4, -0.3], "vmax": [0.4, 0.5]}
    cfg["Diagnostics"] = [
        {"diagnostic": "DistributionMoment", "particles": "electrons", "moment": "current"},
        {"diagnostic": "DistributionMoment", "particles": "electrons", "moment": "momentum_flux_cyl",
         "region": {"type": "2D", "plane": "Z", "position": 2.25}},
        {"diagnostic": "DistributionMoment", "particles": "electrons", "moment": "density",
         "region": {"start": [1.0, 1.5, 0.5], "size": [2.5, 2.0, 3.0]}},
        dict({"diagnostic": "VelocityDistribution", "particles": "electrons", "projector": "vx_vy",
              "geometry": {"name": "BoxGeometry", "min": [0.5, 1.0, 0.0], "max": [4.0, 5.0, 3.5]}}, **vd),
        dict({"diagnostic": "VelocityDistribution", "particles": "electrons", "projector": "vz_vxy", "geometry": cyl}, **vd),
    ]
    cfg["SimulationBackup"] = {"diagnose_period": "2 [dt]"}
    path = tmp_path / "config.json"
    path.write_text(json.dumps(cfg))
    out = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]

    n = (10, 10, 10)
    d = (0.5, 0.5, 0.5)
    Np, dens, q, m = 100, 1.0, -1.0, 1.0
    vs, vn = M.vsizes(vd["vmin"], vd["vmax"], vd["dv"])
    assert (vs, vn) == (-8, 16)
    e = tmp_path / "electrons"
    for t in ("2", "4"):  # the backup keeps the last two periods
        bdir = tmp_path / "simulation_backup" / t
        (count,) = struct.unpack(">i", open(bdir / "electrons.numparts", "rb").read())
        pts = np.fromfile(bdir / "electrons", dtype=">f8").astype(np.float64).reshape(count, 6)
        g = np.floor(pts[:, :3] / np.array(d)).astype(np.int64)  # FLOOR_STEP: the storage cell after update_cells
        cells = (g[:, 2] * n[1] + g[:, 1]) * n[0] + g[:, 0]

        cur = _f32(e / "current" / t)
        assert cur.size == n[0] * n[1] * n[2] * 3
        _close32(cur, M.moment("current", pts, cells, q, m, dens / Np, n, d))

        reg = (0, 0, 4, 10, 10, 1)
        mf = _f32(e / "momentum_flux_cyl_planeZ_0004" / t)
        assert mf.size == 10 * 10 * 6
        _close32(mf, M.moment("momentum_flux_cyl", pts, cells, q, m, dens / Np, n, d, reg)[4:5])

        reg = (2, 3, 1, 5, 4, 6)
        rho = _f32(e / "density" / t)
        assert rho.size == 5 * 4 * 6
        full = M.moment("density", pts, cells, q, m, dens / Np, n, d, reg)
        _close32(rho, full[1:7, 3:7, 2:7])
        # the region rule: not a crop of the whole-box density
        whole = M.moment("density", pts, cells, q, m, dens / Np, n, d)[1:7, 3:7, 2:7]
        assert np.abs(whole - full[1:7, 3:7, 2:7]).max() > 1e-3 * np.abs(whole).max()

        for proj, geom in (("vx_vy", cfg["Diagnostics"][3]["geometry"]), ("vz_vxy", cyl)):
            h = _f32(e / proj / t)
            assert h.size == vn * vn
            ref, _ = M.velocity_distribution(proj, geom, pts, cells, dens / Np, n, d, vd["vmin"], vd["vmax"], vd["dv"])
            _close32(h, ref)
