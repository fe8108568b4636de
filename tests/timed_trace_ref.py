"""numpy restatement of the model traces with a time envelope on the model's E (include/xpic_hip.h:
xpic_field_envelope), the model the GPU kernels of xpic_amd/csrc/model_trace.hip are tested against:

  factor(env, step, dt)     the envelope at t = float(step) * dt, one product: the reference's `t * dt` with its integer
                            loop index (tests/crank_nicolson_push/crank_nicolson_push_ex3.cpp:39-46)
  timed(field, env, ...)    a field function r -> (E * f, B, gradB) around one of analytic_trace_ref.model's; the constant
                            envelope (and None) returns the field function itself: no factor at all
  trace(...)                open_trace_ref.trace_open's loop with the pusher rebuilt at the top of every step from the
                            step's factor (step0 fixes the clock), and the running sums of ex3's two checks (ex3.cpp:51-57)
  ex3(...)                  the example itself: its constants, its table rows and its two checks

Built on analytic_trace_ref (the pushers around any field function) and open_trace_ref (the region rule).  An envelope
is a dict: {"kind": "constant"}, {"kind": "ramp", "a": .., "b": ..} or {"kind": "harmonic", "omega": .., "phase": ..}."""
import collections

import numpy as np

import analytic_trace_ref as A
import open_trace_ref as OT

TimedRef = collections.namedtuple(
    "TimedRef", "state samples exit_step alive removed iterations_sum iterations_max sums sums_abs sums_steps_abs")


def factor(env, step, dt):
    if env is None or env["kind"] == "constant":
        return np.float64(1.0)
    t = np.float64(step) * np.float64(dt)
    if env["kind"] == "ramp":
        return np.float64(env["a"]) + np.float64(env["b"]) * t
    if env["kind"] == "harmonic":
        return np.cos(np.float64(env["omega"]) * t + np.float64(env["phase"]))
    raise KeyError(env["kind"])


def timed(field, env, step, dt):
    if env is None or env["kind"] == "constant":
        return field
    f = factor(env, step, dt)

    def scaled(r):
        E, B, gB = field(r)
        return E * f, B, gB
    return scaled


def step_sums(field, p0, pn, qm, dt):
    """what one step p0 -> pn [m][6] of full orbits adds to the four sums, `field` carrying the step's factor -> [m][4]:
    0.5 (|pn.p|^2 - |p0.p|^2) - qm dt (vh . E_s) and vh.transverse_to(B_s) = vh - ((vh . B_s) B_s) / B_s^2
    (src/utils/vector3.h:195-205), with vh = 0.5 (pn.p + p0.p) and (E_s, B_s) at (r0 + rn) / 2.  Second result: the
    magnitudes of the terms each of them is made of, 0.5 |pn.p|^2 + 0.5 |p0.p|^2 + |qm dt (vh . E_s)| and
    |vh| + |parallel part|, component by component: the scale on which a sum of rounded terms can be compared (an exact
    integrator's energy balance is 0 but for rounding, so what a step adds is no scale for it)"""
    vh = 0.5 * (pn[:, 3:] + p0[:, 3:])
    Es, Bs, _ = field((p0[:, :3] + pn[:, :3]) / 2)

    def dot(a, b):
        return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]
    out, mag = np.empty((len(p0), 4)), np.empty((len(p0), 4))
    kn, k0, work = 0.5 * dot(pn[:, 3:], pn[:, 3:]), 0.5 * dot(p0[:, 3:], p0[:, 3:]), qm * dt * dot(vh, Es)
    out[:, 0] = 0.5 * (dot(pn[:, 3:], pn[:, 3:]) - dot(p0[:, 3:], p0[:, 3:])) - work
    mag[:, 0] = kn + k0 + np.abs(work)
    with np.errstate(divide="ignore", invalid="ignore"):
        par = (dot(vh, Bs)[:, None] * Bs) / dot(Bs, Bs)[:, None]
    out[:, 1:] = vh - par
    mag[:, 1:] = np.abs(vh) + np.abs(par)
    return out, mag


def trace(kind, field, env, p, steps, qm, mp, dt, geometry, d, sample_every=0, exit_step=None, step0=0, sums=None, **kw):
    """open_trace_ref.trace_open with the pusher of `kind` ("dk", "CN" or a Chin id) rebuilt for every step k from
    timed(field, env, step0 + k, dt).  geometry None: no region.  sums: None, True (zeros) or [n][4] to go on from; full
    orbits only.  sums_abs is the sum over this call's steps of the magnitudes of the terms (step_sums' second result), the
    scale a comparison of sums uses; sums_steps_abs is the sum of the magnitudes of what each step added."""
    p = np.array(p, dtype=np.float64).reshape(-1, 6)
    n = p.shape[0]
    geometry = OT.EVERYWHERE if geometry is None else geometry
    ex = np.full(n, -1, dtype=np.int64) if exit_step is None else np.array(exit_step, dtype=np.int64)
    nsamp = steps // sample_every if sample_every else 0
    samples = np.zeros((nsamp, n, 6)) if sample_every else None
    alive = np.zeros(nsamp, dtype=np.int64) if sample_every else None
    tot, mx = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32)
    if sums is not None:
        sums = np.zeros((n, 4)) if sums is True else np.array(sums, dtype=np.float64).reshape(n, 4)
    sums_abs = None if sums is None else np.zeros((n, 4))
    sums_steps_abs = None if sums is None else np.zeros((n, 4))
    removed = 0
    for k in range(steps):
        a = np.flatnonzero(ex < 0)
        out = a[~OT.keep(geometry, p[a, :3], d)]
        ex[out] = step0 + k
        removed += len(out)
        a = np.flatnonzero(ex < 0)
        if len(a):
            f = timed(field, env, step0 + k, dt)
            p0 = p[a]
            pn, its = A.pusher(kind, f, qm, mp, dt, **kw)(p0)
            p[a] = pn
            tot[a] += its
            mx[a] = np.maximum(mx[a], its)
            if sums is not None:
                added, mag = step_sums(f, p0, pn, qm, dt)
                sums[a] += added
                sums_abs[a] += mag
                sums_steps_abs[a] += np.abs(added)
        if sample_every and (k + 1) % sample_every == 0:
            samples[(k + 1) // sample_every - 1] = p
            alive[(k + 1) // sample_every - 1] = (ex < 0).sum()
    return TimedRef(p, samples, ex, alive, removed, tot, mx, sums, sums_abs, sums_steps_abs)


# ---- crank_nicolson_push_ex3.cpp: E_p = E0 * (t * dt), B_p = B0, qm = -1, from rest at the origin but for v_z = 0.1
EX3_E0, EX3_B0 = (0.0, -2.0, 0.0), (100.0, 0.0, 0.0)
EX3_MODEL = dict(E0=EX3_E0, B0=EX3_B0)
EX3_ENVELOPE = {"kind": "ramp", "a": 0.0, "b": 1.0}
EX3_QM = -1.0
EX3_START = (0.0, 0.0, 0.0, 0.0, 0.0, 0.1)
EX3_ENERGY_BOUND = 5e-10  # equal_tol(check_energy_conservation, 0.0, 5.0 * PETSC_SMALL), ex3.cpp:60
EX3_DRIFT_BOUND = 1e-6    # equal_tol(check_drift_velocity, v_drift, 1e-6), ex3.cpp:70


def ex3_run(omega_dt):
    """-> (dt, geom_nt, steps between rows): dt = omega_dt / |B0|, geom_nt = ROUND_STEP(30 000 2 pi / |B0|, dt), rows every
    geom_nt / 123 steps (ex3.cpp:24-34).  The loop makes geom_nt + 1 steps (t = 0 .. geom_nt inclusive, :39)."""
    omega = 100.0
    dt = omega_dt / omega
    nt = int(np.floor(30000 * (2.0 * np.pi / omega) / dt + 0.5))
    return dt, nt, nt // 123


def ex3_rows(start, samples, dt, every, rows):
    """the table's rows {t, r, v}: the start, then the samples (the states after every `every`-th step), `rows` in all"""
    states = np.concatenate([np.asarray(start, dtype=np.float64).reshape(1, 6), np.asarray(samples).reshape(-1, 6)])[:rows]
    return np.column_stack([np.arange(len(states)) * every * dt, states])


def ex3_checks(sums, dt, nt):
    """-> (|energy balance|, largest |drift - theory| over the components) from the undivided sums of the nt + 1 steps,
    as ex3.cpp:51-71 forms them: both sums divided by geom_nt; v_drift = v_ExB + v_pol with the time integral of the ramp"""
    E0, B0 = np.array(EX3_E0), np.array(EX3_B0)
    sums = np.asarray(sums, dtype=np.float64).reshape(4)
    E_time_int = float(nt + 1) * (0.5 * dt)
    v_ExB = np.cross(E0, B0) / B0.dot(B0) * E_time_int
    h = B0 / np.sqrt(B0.dot(B0))
    v_pol = (-1.0) * np.cross(h, np.cross(E0, h)) / B0.dot(B0)
    return abs(sums[0] / nt), np.abs(sums[1:] / nt - (v_ExB + v_pol)).max()


# ---- the inputs of tests/test_gpu_timed_trace.py: the shapes, models and batches of tests/test_gpu_model_trace.py
N, D = (9, 8, 7), (0.5, 0.4, 0.75)
NPART, NPART_CN = 3 * 256 + 7, 300
STEPS, EVERY, SPLIT = 150, 7, 70
QM, MP, DT = -1.0, 1.0, 0.05
PIN = {"CN": dict(atol=0.0, rtol=0.0, maxit=3), "dk": dict(eps=0.0, delta=0.0, maxit=4)}
KINDS = ["EB2B", "M1A", "BLF", "CN", "dk"]
MODELS = {
    "uniform": dict(E0=(0.0, 0.01, 0.02), B0=(0.2, 0.3, 1.0)),
    "linear": dict(E0=(0.0, 0.01, 0.0), B0=(0.0, 0.0, 2.0), r0=(10.0, 10.0, 20.0), g=(0.1, 0.0, 0.02)),
    "quadratic_mirror": dict(E_phi=0.003, phi=0.05, **A.QUADRATIC),
    "gaussian_mirror": dict(A.GAUSSIAN),
}
CENTRE = {"quadratic_mirror": (10.0, 10.0, 20.0), "gaussian_mirror": (5.0, 5.0, 5.0), "uniform": (10.0, 10.0, 20.0),
          "linear": (10.0, 10.0, 20.0)}
# t runs to (STEPS - 1) DT = 7.45: the ramp grows from 0.5 to 2.7, the harmonic makes two periods
ENVELOPES = {"ramp": {"kind": "ramp", "a": 0.5, "b": 0.3}, "harmonic": {"kind": "harmonic", "omega": 1.7, "phase": 0.4}}


def region(name):
    """ends 3 length units from the midplane in z, on cell corners of dz = 0.75 (the box rule is half-open)"""
    zc = CENTRE[name][2]
    return {"name": "box", "min": (-1e6, -1e6, zc - 3.0), "max": (1e6, 1e6, zc + 3.0)}


def particles(name, kind, n, seed=51):
    """within half a unit of the model's centre, three interleaved groups by the speed along z (leaves within 64 steps,
    between 64 and 150, never)"""
    rng = np.random.default_rng(seed)
    r = np.array(CENTRE[name]) + (rng.random((n, 3)) - 0.5)
    group = np.arange(n) % 3
    lo, hi = np.array([1.3, 0.5, 0.1])[group], np.array([2.0, 0.72, 0.25])[group]
    vz = (lo + (hi - lo) * rng.random(n)) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    vperp = 0.1 + 0.2 * rng.random(n)
    ang = 2 * np.pi * rng.random(n)
    if kind != "dk":
        return np.column_stack([r, vperp * np.cos(ang), vperp * np.sin(ang), vz])
    lB = np.sqrt((A.model(name, **MODELS[name])(r)[1] ** 2).sum(axis=1))
    return np.column_stack([r, vz, vperp, MP * vperp * vperp / (2.0 * lB)])
