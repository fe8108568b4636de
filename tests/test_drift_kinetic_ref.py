"""CPU checks of tests/drift_kinetic_ref.py, the model the GPU drift-kinetic kernels are tested against, with the
reference's own assertions (tests/drift_kinetic_push/drift_kinetic_grid_boris_ex1.cpp), an invariant that is exact by
construction, and the convergence of the inputs the GPU tests use."""
import ctypes
import os
import re

import numpy as np

import drift_kinetic_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DK_SYMBOLS = ("xpic_drift_kinetic_interpolate", "xpic_drift_kinetic_push", "xpic_drift_kinetic_trace")


def test_uniform_fields_match_theory():
    """drift_kinetic_grid_boris_ex1.cpp: E = (0, 1, -1), B = (0, 0, 1), q = -1, m = 1, the particle (2, 2, 2) with
    v = (0, 0.1, 0).  After T = K dt the guiding centre is at start + E x B / B^2 T + q E_par T^2 / 2 z and
    p_parallel = q E_par T, both to the reference's equal_tol of 1e-4."""
    import xpic_amd as X

    n, d = (6, 6, 6), (1.0, 1.0, 1.0)
    E0, B0 = np.array([0.0, 1.0, -1.0]), np.array([0.0, 0.0, 1.0])
    shape = (n[2], n[1], n[0], 3)
    E, B = np.zeros(shape) + E0, np.zeros(shape) + B0
    q, m, dt, K = -1.0, 1.0, 0.05, 100
    p = X.guiding_centre([[2.0, 2.0, 2.0, 0.0, 0.1, 0.0]], B0, 1.0, q / m)
    # PointByField(point, B0, 1, q / m): r - p x b / (qm |B|), |p_par|, |p_perp|, mp p_perp^2 / (2 |B|)
    assert np.allclose(p[0], [2.0 + 0.1, 2.0, 2.0, 0.0, 0.1, 0.005], rtol=0, atol=1e-15)
    start = p[0, :3].copy()
    for _ in range(K):
        p, its = R.push(E, B, None, d, p, q / m, m, dt)
        assert 1 <= its[0] < 30
    T = K * dt
    z_theory = 0.5 * q * E0[2] * T * T
    r_theory = start + np.cross(E0, B0) / B0.dot(B0) * T + np.array([0.0, 0.0, z_theory])
    assert abs(p[0, 3] - q * E0[2] * T) < 1e-4
    assert np.abs(p[0, :3] - r_theory).max() < 1e-4


def test_mirror_keeps_the_magnetic_moment():
    """B = (0, 0, 1 + 0.3 cos(2 pi z / Lz)), E = 0: update_v_perp sets p_perp = p_perp0 sqrt(|B(rn)| / |B(r0)|) with the
    B it gathered at the returned position, so p_perp^2 / |B(r)| is constant to rounding: at most ~3 roundings a step
    (the quotient, the root, the product), 20 steps, under 1e-14 relative."""
    E, B, gB = R.mirror_fields(R.N, R.D)
    rng = np.random.default_rng(1)
    n = 16
    L = np.array(R.N) * np.array(R.D)
    p = np.column_stack([rng.random((n, 3)) * L, 0.5 + rng.random(n), 0.1 + 0.4 * rng.random(n), np.zeros(n)])

    def absB(r):
        return R._len(R.interpolate(E, B, gB, R.D, r, r)[1])

    b0 = absB(p[:, :3])
    p[:, 5] = R.MP * p[:, 4] ** 2 / (2 * b0)
    inv0 = p[:, 4] ** 2 / b0
    z0 = p[:, 2].copy()
    for _ in range(20):
        p, its = R.push(E, B, gB, R.D, p, R.QM, R.MP, R.DT)
        assert its.min() >= 1 and its.max() < 30
    inv = p[:, 4] ** 2 / absB(p[:, :3])
    assert np.abs(p[:, 2] - z0).min() > 0.3  # they moved through a varying field
    assert np.abs(inv / inv0 - 1).max() <= 1e-14


def test_interpolation_returns_constants_and_the_seam_is_periodic():
    E = np.zeros((R.N[2], R.N[1], R.N[0], 3)) + np.array([0.3, -1.1, 0.7])
    B = np.zeros_like(E) + np.array([-0.2, 0.5, 0.9])
    rn, r0 = R.case_segments(max_cells=0.45)
    Ep, Bp, gBp = R.interpolate(E, B, None, R.D, rn, r0)
    assert np.abs(Ep - np.array([0.3, -1.1, 0.7])).max() < 1e-13
    assert np.abs(Bp - np.array([-0.2, 0.5, 0.9])).max() < 1e-13
    assert not gBp.any()
    # a shift by whole box lengths changes nothing but rounding
    E, B, gB = R.case_fields()
    L = np.array(R.N) * np.array(R.D)
    a = R.interpolate(E, B, gB, R.D, rn, r0)
    b = R.interpolate(E, B, gB, R.D, rn + 2 * L, r0 + 2 * L)
    for u, v in zip(a, b):
        assert np.abs(u - v).max() < 1e-12


def test_gpu_test_inputs_converge_in_the_restatement():
    """the cap of the GPU convergence test: zero unconverged particles in the restatement at DT with the default
    tolerances, and the pinned-iteration form (eps = delta = 0) does exactly maxit updates.  The particles that start
    with p_parallel = 0 exactly are left out of the convergence cases: their Vh stays small, the 1 / Vh terms make the
    Picard map expand and they run to maxit (they belong to the pinned-iteration test)."""
    E, B, gB = R.case_fields()
    p0 = R.case_particles(B, zero_par=0)
    pn, its = R.push(E, B, gB, R.D, p0, R.QM, R.MP, R.DT)
    assert its.min() >= 1 and its.max() < 30, (its.min(), its.max())
    assert np.isfinite(pn).all()
    R1, R2 = R.residuals(E, B, gB, R.D, p0, pn, R.QM, R.MP, R.DT)
    assert R1.max() < 1e-12 and R2.max() < 1e-12
    _, its = R.push(E, B, gB, R.D, p0, R.QM, R.MP, R.DT, eps=0.0, delta=0.0, maxit=2)
    assert (its == 2).all()


def test_binding_header_and_library_agree():
    import xpic_amd

    for name in DK_SYMBOLS:
        assert name in xpic_amd.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "xpic_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in DK_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert int(re.search(r"#define XPIC_DK_LAUNCH_STEPS (\d+)", hdr).group(1)) == xpic_amd.DK_LAUNCH_STEPS
    if not os.path.exists(xpic_amd.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    lib = ctypes.CDLL(xpic_amd.LIB_PATH)
    for name in DK_SYMBOLS:
        assert hasattr(lib, name), name
    # struct xpic_dk_params: five doubles and an int, padded to 48 bytes
    assert ctypes.sizeof(xpic_amd.DkParams) == 48
    for f in ("Context.drift_kinetic_interpolate", "Context.drift_kinetic_push", "Context.drift_kinetic_trace", "guiding_centre"):
        obj = xpic_amd
        for part in f.split("."):
            obj = getattr(obj, part)
        assert callable(obj)
