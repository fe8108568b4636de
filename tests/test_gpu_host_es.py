"""The host mirror's "Simulation": "electrostatic" (xpic_amd/host; include/xpic_es.h): a 6^3 config of five steps with a
device SetParticles (seeded) and a uniform external B, against the same sequence driven from Python; temporal/gauss_law.txt
from the step's own solve; the GaussLaw key (at_start honoured, every refused); and the reference's basic_ex1 config, which
must run as before (its golden tables are held by tests/test_gpu_host.py, which this change leaves alone: here its first
rows are read again after the host executable has learnt the new scheme).

Bounds.  The two runs execute the same device code on the same inputs; they differ by the order of the deposit's atomics,
which the solve's stopping rule turns into a difference of E of up to |r| / sqrt(lambda_min) per run and step (tests/
test_gpu_es.py: section 4's reasoning), carried into v by dt q/m and into r by dt, summed over the steps."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import es_ref as R
import gauss_ref as G
import test_gpu_es as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "xpic_amd", "host", "xpic_hip.out")
N, D, DT, STEPS = (6, 6, 6), (0.5, 0.5, 0.5), 0.05, 5
L = tuple(n * d for n, d in zip(N, D))
NP, TEMP, SEED, B0 = 4, 0.1, 7, (0.1, -0.2, 0.3)
RTOL = 1e-10
CONFIG = {
    "Simulation": "electrostatic",
    "OutputDirectory": "",
    "Geometry": {"x": L[0], "y": L[1], "z": L[2], "t": STEPS * DT, "dx": D[0], "dy": D[1], "dz": D[2], "dt": DT,
                 "diagnose_period": DT, "da_boundary_x": "DM_BOUNDARY_PERIODIC", "da_boundary_y": "DM_BOUNDARY_PERIODIC",
                 "da_boundary_z": "DM_BOUNDARY_PERIODIC"},
    "Particles": [{"sort_name": "electrons", "Np": NP, "n": 1.0, "q": -1.0, "m": 1.0, "T": TEMP}],
    "Presets": [{"command": "SetParticles", "particles": "electrons", "coordinate": {"name": "CoordinateInBox"},
                 "momentum": {"name": "MaxwellianMomentum", "tov": True}, "device": True, "seed": SEED},
                {"command": "SetMagneticField", "field": "B", "setter": {"name": "SetUniformField", "value": list(B0)}}],
    "Diagnostics": [],
    "SimulationBackup": {"diagnose_period": "%d [dt]" % STEPS},
    "GaussLaw": {"at_start": True, "rtol": RTOL},
}


def run(tmp_path, name, **change):
    cfg = json.loads(json.dumps(CONFIG))
    cfg.update(change)
    cfg = {k: v for k, v in cfg.items() if v is not None}  # (None drops a key)
    out_dir = tmp_path / name
    out_dir.mkdir()
    cfg["OutputDirectory"] = str(out_dir)
    (out_dir / "config.json").write_text(json.dumps(cfg))
    out = subprocess.run([EXE, str(out_dir / "config.json")], capture_output=True, text=True, timeout=120)
    return out, out_dir


def test_electrostatic_config_against_the_python_sequence(tmp_path):
    import xpic_amd as X

    out, odir = run(tmp_path, "es")
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    # the same sequence from Python
    g = X.Context("es", N, D, DT)
    s = g.add_sort(NP, 1.0, -1.0, 1.0, capacity=2 * NP * 216 + 4096)
    box = {"name": "CoordinateInBox", "min": (0.0, 0.0, 0.0), "max": L}
    count = g.particles_number(s, box)
    added, _ = g.set_particles(s, count, box, {"name": "MaxwellianMomentum", "T": (TEMP,) * 3, "tov": True}, step=0, seed=SEED)
    assert added == count == NP * 216
    g.set_field(X.B, np.zeros(g.fshape()) + np.array(B0))
    first = g.gauss_clean(X.E, rtol=RTOL, atol=0.0, maxit=10000)
    lam = G.lambda_min(N, D)
    acc, its = first.after / np.sqrt(lam), []
    for _ in range(STEPS):
        its.append(g.step())
        acc += g.gauss_info()["after"] / np.sqrt(lam)
    Ep = g.get_field(X.E)
    pp, _ = g.particles(s)

    # gauss_law.txt: the start row and one row per step, each from the solve that ran, each meeting the rule
    lines = open(odir / "temporal" / "gauss_law.txt").readlines()
    assert lines[0].split() == ["Time", "Res_before", "Res_after", "Mean_rho", "Iterations"]
    rows = np.array([[float(v) for v in ln.split()] for ln in lines[1:]])
    assert rows[:, 0].tolist() == list(range(STEPS + 1)) and len(rows[1:]) == 5
    rho_l2 = g.gauss_residual(X.E)["rho_l2"]
    print("host mirror: rows", rows.tolist(), "python iterations", first.iterations, its)
    for row in rows[1:]:  # (rho~ of a thermal load changes by per cent over five steps: the rule within 1.5 of the last one's)
        assert row[4] > 0 and row[2] <= 1.5 * max(X.ES_RTOL * rho_l2, X.ES_ATOL) * (1 + 1e-6) < row[1], row
    assert rows[0, 4] > 0 and np.allclose(rows[:, 3], -1.0, rtol=1e-6)
    assert np.abs(rows[1:, 4] - np.array(its)).max() <= 1
    assert "charge_conservation.txt" not in os.listdir(odir / "temporal")

    # the last backup against the Python run
    bdir = odir / "simulation_backup" / str(STEPS)
    assert "B0" not in os.listdir(bdir)  # (the scheme holds no B0)
    (n,) = struct.unpack(">i", open(bdir / "electrons.numparts", "rb").read())
    pts = np.fromfile(bdir / "electrons", dtype=">f8").astype(np.float64).reshape(n, 6)
    E = np.fromfile(bdir / "E", dtype=">f8", offset=8).astype(np.float64).reshape(N[2], N[1], N[0], 3)
    B = np.fromfile(bdir / "B", dtype=">f8", offset=8).astype(np.float64).reshape(N[2], N[1], N[0], 3)
    assert n == count and np.array_equal(B, np.zeros_like(B) + np.array(B0))
    bE = 2 * acc + 2 * T.K_ROUNDING * T.EPS * (T.l2(E) + T.l2(Ep))
    bV = STEPS * DT * 1.0 * bE + 4 * T.EPS * np.abs(pp[:, 3:]).max()
    bR = STEPS * DT * bV + 4 * T.EPS * max(L)
    a, b = T.canon(pts, N, D), T.canon(pp, N, D)
    print("host mirror: |dE| / bound", np.abs(E - Ep).max() / bE, "dr / bound", np.abs(a[:, :3] - b[:, :3]).max() / bR,
          "dv / bound", np.abs(a[:, 3:] - b[:, 3:]).max() / bV)
    assert np.abs(E - Ep).max() <= bE
    assert np.abs(a[:, :3] - b[:, :3]).max() <= bR and np.abs(a[:, 3:] - b[:, 3:]).max() <= bV
    g.close()


def test_gauss_law_key_on_an_electrostatic_config(tmp_path):
    # "every" is refused with a message
    out, _ = run(tmp_path, "every", GaussLaw={"at_start": True, "every": 2})
    assert out.returncode != 0 and "refused on an electrostatic simulation" in out.stdout + out.stderr
    # without the key the table is still written, and nothing cleans at the start: E = 0 does not go with the load
    out, odir = run(tmp_path, "nokey", GaussLaw=None)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    rows = np.array([[float(v) for v in ln.split()] for ln in open(odir / "temporal" / "gauss_law.txt").readlines()[1:]])
    assert rows[:, 0].tolist() == list(range(STEPS + 1))
    assert rows[0, 4] == 0 and rows[0, 1] == rows[0, 2] > 1e-3  # the start row: the residual as it stands
    assert (rows[1:, 4] > 0).all() and rows[1, 1] > 1e3 * rows[1, 2]  # the first step's solve is the electrostatic start


def test_basic_ex1_still_reproduces_its_golden_tables(tmp_path):
    gold = os.path.join(ROOT, "tests", "golden", "basic_ex1")
    cfg = json.load(open(os.path.join(gold, "config.json")))
    dt = cfg["Geometry"]["dt"]
    cfg["Geometry"]["t"] = 3 * dt
    cfg["OutputDirectory"] = str(tmp_path)
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    out = subprocess.run([EXE, str(tmp_path / "config.json")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "gauss_law.txt" not in os.listdir(tmp_path / "temporal") and "charge_conservation.txt" in os.listdir(tmp_path / "temporal")
    for table in ("energy.txt", "energy_conservation.txt"):
        mine, ref = open(tmp_path / "temporal" / table).readlines(), open(os.path.join(gold, table)).readlines()
        assert [ln.split() for ln in mine[:2]] == [ln.split() for ln in ref[:2]], table  # titles and the step-0 row, as printed
        a = np.array([[float(v) for v in ln.split()] for ln in mine[1:4]])
        b = np.array([[float(v) for v in ln.split()] for ln in ref[1:4]])
        assert np.allclose(a, b, rtol=1e-5, atol=1e-12), table  # (the full 100 steps to every digit: tests/test_gpu_host.py)
