"""SetParticles through the host executable: a "device": true entry goes through xpic_set_particles with the builder's count
and logs what tests/set_particles_ref.py gives; the same entry without the key takes the host's mt19937 path as before; a
MaxwellCosinePerturbation entry runs on both paths."""
import copy
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import set_particles_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "xpic_amd", "host", "xpic_hip.out")
N, D, L = (2, 2, 8), (0.5, 0.5, 0.5), (1.0, 1.0, 4.0)
NP, M, T = 10, 1.0, 0.1
CONFIG = {
    "Simulation": "ecsim",
    "OutputDirectory": "",
    "Geometry": {"x": L[0], "y": L[1], "z": L[2], "t": 1.5, "dx": D[0], "dy": D[1], "dz": D[2], "dt": 1.5, "diagnose_period": 1.5,
                 "da_boundary_x": "DM_BOUNDARY_PERIODIC", "da_boundary_y": "DM_BOUNDARY_PERIODIC",
                 "da_boundary_z": "DM_BOUNDARY_PERIODIC"},
    "Particles": [{"sort_name": "electrons", "Np": NP, "n": 1.0, "q": -1.0, "m": M, "T": T}],
    "Presets": [{"command": "SetParticles", "particles": "electrons", "coordinate": {"name": "CoordinateInBox"},
                 "momentum": {"name": "MaxwellianMomentum", "tov": True}}],
    "Diagnostics": [],
}
BOX = {"name": "CoordinateInBox", "min": (0.0, 0.0, 0.0), "max": L}
COSINE = {"name": "MaxwellCosinePerturbation", "amplitude": [0.5, 0.0, 0.25], "wave_number": [1.0, 0.0, 2.0]}
# (config entry, the generators as the restatement takes them)
CASES = {
    "box-maxwell": ({}, BOX, {"name": "MaxwellianMomentum", "T": (T, T, T), "tov": True}),
    "box-cosine": ({"momentum": COSINE}, BOX,
                   dict(COSINE, T=(T, T, T), min=(0.0, 0.0, 0.0), max=L)),
    "annulus-angular": (
        {"coordinate": {"name": "CoordinateOnAnnulus", "center": [0.5, 0.5, 2.0], "inner_r": 0.125, "outer_r": 0.75, "height": 3.0},
         "momentum": {"name": "AngularMomentum", "center": [0.5, 0.5, 0.0]}},
        {"name": "CoordinateOnAnnulus", "center": (0.5, 0.5, 2.0), "inner_r": 0.125, "outer_r": 0.75, "height": 3.0},
        {"name": "AngularMomentum", "T": (T, T, T), "drift": (0.0, 0.0, 0.0), "center": (0.5, 0.5, 0.0)}),
}


def run(tmp_path, entry):
    cfg = copy.deepcopy(CONFIG)
    cfg["OutputDirectory"] = str(tmp_path)
    cfg["Presets"][0].update(entry)
    path = tmp_path / "config.json"
    path.write_text(json.dumps(cfg))
    out = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout


@pytest.mark.parametrize("case", list(CASES))
def test_device_entry_logs_the_restatements_count_and_energy(tmp_path, case):
    entry, cgen, mgen = CASES[case]
    out = run(tmp_path, dict(entry, device=True, seed=7))
    count = S.particles_number(cgen, NP, D, L)
    _, _, k, e = S.set_particles(count, 0, 7, cgen, mgen, M, 1.0 / NP, N, D)
    assert 0 < k <= count and (case != "annulus-angular" or k < count)  # (the annulus reaches beyond the 1 x 1 box)
    m = re.search(r'Particles have been added into "electrons" on the device: (\d+)\n\s+energy: (\S+)', out)
    assert m, out[-2000:]
    assert int(m.group(1)) == k
    assert abs(float(m.group(2)) - e) <= 1e-12 * e
    assert "SetParticles command (device) is added" in out


def test_without_the_key_the_host_path_runs(tmp_path):
    out = run(tmp_path, {})
    assert "on the device" not in out and "(device)" not in out
    m = re.search(r'Particles have been added into "electrons": (\d+)', out)
    assert m and int(m.group(1)) == S.particles_number(BOX, NP, D, L) == NP * N[0] * N[1] * N[2]
    # "device": false is the same
    out2 = run(tmp_path, {"device": False})
    assert "on the device" not in out2 and re.search(r'added into "electrons": (\d+)', out2).group(1) == m.group(1)


def test_cosine_perturbation_runs_on_the_host_path(tmp_path):
    out = run(tmp_path, {"momentum": COSINE})
    m = re.search(r'Particles have been added into "electrons": (\d+)', out)
    assert m and int(m.group(1)) == NP * N[0] * N[1] * N[2]
    # the names only the device path has are refused on the host path
    cfg_entry = {"coordinate": CASES["annulus-angular"][0]["coordinate"]}
    cfg = copy.deepcopy(CONFIG)
    cfg["OutputDirectory"] = str(tmp_path)
    cfg["Presets"][0].update(cfg_entry)
    (tmp_path / "c2.json").write_text(json.dumps(cfg))
    bad = subprocess.run([EXE, str(tmp_path / "c2.json")], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "Unknown coordinate generator name CoordinateOnAnnulus" in bad.stdout + bad.stderr
