"""The host executable with the reference's per-step commands (RemoveParticles, InjectParticles, FieldsDamping) and the
SetCoilsField setter: the energy-conservation columns in the reference's order and sum rule, the removed energy against
tests/commands_ref.py applied to the SimulationBackup of the step before, the injection schedule of the builder, and the
coils field of B0 against the restated quadrature."""
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import commands_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "xpic_amd", "host", "xpic_hip.out")
GOLD = os.path.join(ROOT, "tests", "golden")
N, D = (10, 10, 10), (0.5, 0.5, 0.5)
L = (5.0, 5.0, 5.0)
COILS = [(1.5, 1.2, 0.5), (3.5, 1.2, 0.5)]
REMOVE_CYL = {"name": "CylinderGeometry", "radius": 2.0, "height": 4.0}
INJECT = {"command": "InjectParticles", "ionized": "ions", "ejected": "electrons",
          "coordinate": {"name": "CoordinateInBox", "min": [1.0, 1.0, 1.0], "max": [4.0, 4.0, 4.0]},
          "momentum_i": {"name": "MaxwellianMomentum", "tov": True}, "momentum_e": {"name": "MaxwellianMomentum", "tov": True},
          "injection_start": 0.0, "injection_end": 3.0, "tau": 7.5}


def read_table(path):
    with open(path) as f:
        header = f.readline().split()
        rows = [[float(x) for x in line.split()] for line in f if line.strip()]
    return header, np.array(rows)


def _run(tmp_path, cfg):
    cfg["OutputDirectory"] = str(tmp_path)
    path = tmp_path / "config.json"
    path.write_text(json.dumps(cfg))
    out = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout


def _backup(tmp_path, t, sort):
    bdir = tmp_path / "simulation_backup" / t
    (count,) = struct.unpack(">i", open(bdir / (sort + ".numparts"), "rb").read())
    return np.fromfile(bdir / sort, dtype=">f8").astype(np.float64).reshape(count, 6)


def test_host_commands(tmp_path):
    cfg = json.load(open(os.path.join(GOLD, "ecsim_ex1", "config.json")))
    dt = cfg["Geometry"]["dt"]
    cfg["Geometry"]["t"] = 3 * dt
    cfg["Geometry"]["diagnose_period"] = dt
    ions = {"sort_name": "ions", "Np": 10, "n": 1.0, "q": 1.0, "m": 100.0, "T": 0.1}
    cfg["Particles"].append(ions)
    cfg["Presets"] += [
        {"command": "SetParticles", "particles": "ions",
         "coordinate": {"name": "CoordinateInCylinder", "radius": 2.0, "height": 4.0},
         "momentum": {"name": "MaxwellianMomentum", "tov": True}},
        {"command": "SetMagneticField", "field": "B0", "field_axpy": "B",
         "setter": {"name": "SetCoilsField", "coils": [{"z0": z0, "R": Rc, "I": I} for z0, Rc, I in COILS]}},
    ]
    cfg["StepPresets"] = [
        {"command": "RemoveParticles", "particles": "electrons", "geometry": REMOVE_CYL},
        INJECT,
        {"command": "FieldsDamping", "E": "E", "B": "B", "B0": "B0", "damping_coefficient": 0.5,
         "geometry": {"name": "CylinderGeometry", "radius": 2.0}},
    ]
    cfg["Diagnostics"] = [{"diagnostic": "FieldView", "field": "B0"}]
    cfg["SimulationBackup"] = {"diagnose_period": "1 [dt]"}
    _run(tmp_path, cfg)

    header, rows = read_table(tmp_path / "temporal" / "energy_conservation.txt")
    # energy.cpp:156-178: the step presets' columns in their order, before dE+dB+dK
    assert header == ["Time", "dE", "dB", "dK_electrons", "dK_ions", "Rm_electrons", "Inj_ions", "Inj_electrons",
                      "Damped(E+B)", "dE+dB+dK"]
    col = {h: rows[:, i] for i, h in enumerate(header)}
    assert list(col["Time"]) == [0, 1, 2, 3]
    # the sum rule: dF + damped, dK + removed - injected
    total = col["dE"] + col["dB"] + col["dK_electrons"] + col["dK_ions"] + col["Damped(E+B)"] + col["Rm_electrons"] \
        - col["Inj_ions"] - col["Inj_electrons"]
    scale = sum(np.abs(col[h]) for h in header[1:-1])
    assert np.all(np.abs(col["dE+dB+dK"] - total) <= 2e-6 * scale + 1e-12)
    # (E = 0 and B = B0 before the first step: nothing to damp there)
    assert np.all(col["Damped(E+B)"] >= 0) and np.all(col["Damped(E+B)"][2:] > 0) and np.all(col["Rm_electrons"][1:] > 0)

    # the removed energy of step 3 from the backup of step 2 (the state RemoveParticles sees), to print precision
    e2 = _backup(tmp_path, "2", "electrons")
    g = np.floor(e2[:, :3] / np.array(D)).astype(np.int64)  # FLOOR_STEP: the storage cell after update_cells
    cells = (g[:, 2] * N[1] + g[:, 1]) * N[0] + g[:, 0]
    geom = {"name": "cylinder", "center": (2.5, 2.5, 2.5), "radius": 2.0, "height": 4.0}
    _, k, rm = R.remove(e2, cells, geom, N, D, 1.0, 1.0 / 100)
    assert k > 0
    assert abs(col["Rm_electrons"][3] - float("%.6e" % rm)) <= 1.5e-6 * rm

    # the builder's schedule: window [0, ROUND_STEP(3.0, dt) = 2], tau = ROUND_STEP(7.5, dt) = 5, pairs per step
    # (box volume 27 * Np 10 / cell volume) / tau = 432; the ions only grow by injection
    start, end, per_step = R.inject_schedule(INJECT, 10, D, dt, L, 3)
    assert (start, end, per_step) == (0, 2, 432)
    ions0 = R.particles_number({"name": "CoordinateInCylinder", "radius": 2.0, "height": 4.0}, 10, D, L)
    assert len(_backup(tmp_path, "2", "ions")) == ions0 + 2 * per_step  # t = 1, 2
    assert len(_backup(tmp_path, "3", "ions")) == ions0 + 2 * per_step  # t = 3 is outside the window
    assert np.all(col["Inj_ions"][1:3] > 0) and col["Inj_ions"][3] == 0 and col["Inj_electrons"][3] == 0

    # B0 = the coils field (SetCoilsField into a zero B0), written as float32 by FieldView
    b0 = np.fromfile(tmp_path / "B0" / "3", dtype=np.float32).astype(np.float64)
    ref = R.coils_field(N, D, COILS).ravel()
    assert np.isfinite(ref).all() and b0.shape == ref.shape
    assert np.all(np.abs(b0 - ref) <= 2.4e-7 * np.abs(ref) + 1e-12 * np.abs(ref).max())


def test_host_without_commands_keeps_its_columns(tmp_path):
    cfg = json.load(open(os.path.join(GOLD, "ecsim_ex1", "config.json")))
    cfg["Geometry"]["t"] = 2 * cfg["Geometry"]["dt"]
    cfg["Diagnostics"] = []
    _run(tmp_path, cfg)
    header, _ = read_table(tmp_path / "temporal" / "energy_conservation.txt")
    assert header == ["Time", "dE", "dB", "dK_electrons", "dE+dB+dK"]


def test_host_rejects_zero_tau(tmp_path):
    cfg = json.load(open(os.path.join(GOLD, "ecsim_ex1", "config.json")))
    cfg["Geometry"]["t"] = cfg["Geometry"]["dt"]
    cfg["Particles"].append({"sort_name": "ions", "Np": 10, "n": 1.0, "q": 1.0, "m": 100.0, "T": 0.1})
    cfg["StepPresets"] = [dict(INJECT, tau=0.5)]  # ROUND_STEP(0.5, 1.5) = 0
    cfg["OutputDirectory"] = str(tmp_path)
    path = tmp_path / "config.json"
    path.write_text(json.dumps(cfg))
    out = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=100)
    assert out.returncode != 0 and "tau" in (out.stdout + out.stderr)
