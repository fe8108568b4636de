"""xpic_amd -- MI355X (gfx950) implementation of xpic's per-timestep hot path.

This package is a thin ctypes view of the C ABI in include/xpic_hip.h (xpic_amd/libxpic_hip.so, built from
xpic_amd/csrc/*.hip by `make` / `__graft_entry__.build()`).  There is NO CPU fallback: if the shared library
or a HIP device is missing, every entry point raises.
"""
import collections
import ctypes as C
import os

import numpy as np

from ._abi import *  # noqa: F401,F403 (the mirrors of include/xpic_hip.h; every name stays importable from here)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libxpic_hip.so")


def csrc_hash():
    """sha1 over the kernel sources (xpic_amd/csrc/*, sorted by name): the code version a PMC traffic file under
    profiles/ was taken on is stamped with it, and bench.py quotes that file only while the hash still matches."""
    import hashlib

    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
    h = hashlib.sha1()
    for name in sorted(os.listdir(d)):
        if name.endswith((".hip", ".h")):
            h.update(name.encode())
            h.update(open(os.path.join(d, name), "rb").read())
    return h.hexdigest()


class XpicError(RuntimeError):
    pass


def _geom7(geometry):
    """(kind, double[7]) of a geometry dict: {"name": "box", "min": xyz, "max": xyz} or {"name": "cylinder", "center": xyz,
    "radius": r, "height": h} ("BoxGeometry" / "CylinderGeometry" as well)"""
    kind = GEOMETRIES[geometry["name"]]
    if kind == 0:
        gp = list(geometry["min"]) + list(geometry["max"]) + [0.0]
    else:
        gp = list(geometry["center"]) + [geometry["radius"], geometry["height"], 0.0, 0.0]
    return kind, np.array(gp, dtype=np.float64)


def trace_collisions(backgrounds, strength, mass, every=1, seed=0, particle0=0):
    """The collisions of a collisional trace (include/xpic_hip.h: xpic_trace_collisions).  backgrounds: at most
    TRACE_BG_MAX dicts of q, m, n, vth (the thermal speed per component, sqrt(T / m)) and drift (three components; not
    given: at rest); strength: S of Context.collide; mass: the test particle's (its charge is qm * mass); every: collide
    after every every-th step with every * dt; particle0: the global index of the batch's first particle."""
    backgrounds = list(backgrounds)
    if len(backgrounds) > TRACE_BG_MAX:
        raise XpicError("trace_collisions: more than %d backgrounds" % TRACE_BG_MAX)
    c = TraceCollisions()
    c.nbg, c.every, c.seed, c.particle0 = len(backgrounds), int(every), int(seed), int(particle0)
    c.strength, c.mass = float(strength), float(mass)
    for i, b in enumerate(backgrounds):
        extra = set(b) - {"q", "m", "n", "vth", "drift"}
        if extra:
            raise XpicError("trace_collisions: no background parameter %r" % (sorted(extra)[0],))
        c.bg[i] = TraceBackground(float(b["q"]), float(b["m"]), float(b["n"]), float(b["vth"]),
                                  (C.c_double * 3)(*[float(x) for x in b.get("drift", (0.0, 0.0, 0.0))]))
    return c


def field_envelope(kind, **params):
    """A time envelope of a model's E (include/xpic_hip.h: xpic_field_envelope).  kind: a key of ENVELOPE_KINDS or its
    number; params: the members the kind reads -- ramp: a, b (f = a + b t); harmonic: omega, phase
    (f = cos(omega t + phase)); constant: none.  A member that is not given is 0."""
    e = FieldEnvelope()
    e.kind = int(ENVELOPE_KINDS.get(kind, kind))
    for k, v in params.items():
        if k not in ("a", "b", "omega", "phase"):
            raise XpicError("field_envelope: no parameter %r" % (k,))
        setattr(e, k, float(v))
    return e


def field_model(kind, **params):
    """An analytic field model (include/xpic_hip.h: xpic_field_model).  kind: a key of MODEL_KINDS or its number; params:
    the members the kind reads -- uniform: E0, B0; linear: E0, B0, r0, g; quadratic_mirror: B_min, B_max, W, D (and E_phi,
    phi); gaussian_mirror: B_min, B_max, L, W.  A member that is not given is 0."""
    m = FieldModel()
    m.kind = int(MODEL_KINDS.get(kind, kind))
    names = {f[0] for f in FieldModel._fields_} - {"kind", "reserved"}
    for k, v in params.items():
        if k not in names:
            raise XpicError("field_model: no parameter %r" % (k,))
        if k in ("E0", "B0", "r0", "g"):
            setattr(m, k, (C.c_double * 3)(*[float(x) for x in v]))
        else:
            setattr(m, k, float(v))
    return m


class PairedTrace(collections.namedtuple(
        "PairedTrace", "p state stats curve fo_iterations_sum fo_iterations_max dk_iterations_total dk_iterations_max")):
    """What Context.paired_trace returns: the full orbits p [n][6] and the guiding centres state [n][6] after the steps;
    stats [n][4], each pair's largest errors over the steps, and curve [steps // sample_every][4] (None without
    sample_every), the largest error over the pairs at every sample_every-th step, both with the columns PAIR_STATS; the
    iteration counters of the two closed traces."""
    __slots__ = ()


class TripletTrace(collections.namedtuple(
        "TripletTrace", "p state_model state_grid stats curve fo_iterations_sum fo_iterations_max dkm_iterations_total "
        "dkm_iterations_max dkg_iterations_total dkg_iterations_max")):
    """What Context.triplet_trace returns, PairedTrace extended: the full orbits p, the guiding centres on the model
    state_model and on the grid state_grid, [n][6] each, after the steps; stats [n][7], each triplet's largest errors over
    the steps, and curve [steps // sample_every][7] (None without sample_every), both with the columns TRIPLET_STATS; the
    iteration counters of the three closed traces.  For the grid-less pair state_grid and the dkg counters are None, and
    columns 0 .. 2 of stats and curve are what went in and 0."""
    __slots__ = ()


class OpenTrace(collections.namedtuple("OpenTrace", "state samples exit_step alive removed iterations_sum iterations_max")):
    """What Context.full_orbit_trace_open / drift_kinetic_trace_open return: the state [n][6]; samples
    [steps // sample_every][n][6] and alive [steps // sample_every] (None without sample_every); exit_step [n] (-1: alive,
    k: removed after completing k steps in total); removed, the particles this call removed; the iteration counters of the
    closed traces."""
    __slots__ = ()


class TimedTrace(collections.namedtuple(
        "TimedTrace", "state samples exit_step alive removed iterations_sum iterations_max sums")):
    """What Context.model_full_orbit_trace_timed returns: OpenTrace's fields and sums [n][4] (None when not asked for), the
    running sums of crank_nicolson_push_ex3's two checks: the energy balance and the three components of the mean
    transverse velocity, neither divided by the step count."""
    __slots__ = ()


class CollisionalTrace(collections.namedtuple(
        "CollisionalTrace", "state samples exit_step alive removed iterations_sum iterations_max coll")):
    """What Context.model_full_orbit_trace_collisional / model_drift_kinetic_trace_collisional return: OpenTrace's fields
    and coll [4] = (collisions made, skipped, sum of sigma^2, collisions with sigma^2 > 1) of the call."""
    __slots__ = ()


def guiding_centre(points6, B3, mp, qm, *, orbit_centre=False):
    """PointByField(point, Bp, mp, qm) (src/interfaces/point.h:52-58) for records {r, p} and the field B3 at each of them
    -> records {guiding centre xyz, p_parallel, p_perp, mu_p}, the particles of Context.drift_kinetic_push.

    That constructor places the centre at r - p x b / (qm |B|).  Under the force qm v x B of BorisPush (and of
    Context.full_orbit_*) a particle circles r + p x b / (qm |B|), the point on the other side of it, two Larmor radii
    away; the reference's tests compare only z, p_parallel, mu and energy between the two pushers and do not see it.
    The default keeps the constructor as it is.  orbit_centre=True returns the centre of the particle's own circle, the
    start from which a drift-kinetic trace can be laid beside a full orbit of the same particle."""
    pts = np.asarray(points6, dtype=np.float64).reshape(-1, 6)
    Bp = np.broadcast_to(np.asarray(B3, dtype=np.float64), (pts.shape[0], 3))
    r, p = pts[:, :3], pts[:, 3:]
    lB = np.sqrt((Bp * Bp).sum(axis=1))[:, None]
    b = np.divide(Bp, lB, out=np.zeros_like(p), where=lB > 0)  # Vector3::normalized
    par = (p * Bp).sum(axis=1)[:, None] * Bp / (Bp * Bp).sum(axis=1)[:, None]  # Vector3::parallel_to
    out = np.empty((pts.shape[0], 6))
    rho = np.cross(p, b) / (qm * lB)
    out[:, :3] = r + rho if orbit_centre else r - rho
    out[:, 3] = np.sqrt((par * par).sum(axis=1))
    out[:, 4] = np.sqrt(((p - par) ** 2).sum(axis=1))
    out[:, 5] = mp * out[:, 4] * out[:, 4] / (2.0 * lB[:, 0])
    return out


_lib = None


def load_library():
    """Loads libxpic_hip.so and types every entry point from PROTOTYPES, LOAD_PROTOTYPES, TRACER_PROTOTYPES,
    TRACER_MOMENT_PROTOTYPES, FIELD_LINE_PROTOTYPES, GAUSS_PROTOTYPES, ES_PROTOTYPES, POISSON_PROTOTYPES and SPECTRUM_PROTOTYPES; raises if it has not been built (no fallback path exists).  The xpic_debug_*_stamps symbols of experiment builds are not in the header and stay untyped."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise XpicError(f"{LIB_PATH} is missing: run `make` (or __graft_entry__.build()) first; "
                        "xpic_amd has no CPU fallback")
    L = C.CDLL(LIB_PATH)
    for name, (ret, args) in dict(PROTOTYPES, **LOAD_PROTOTYPES, **TRACER_PROTOTYPES, **TRACER_MOMENT_PROTOTYPES,
                                   **FIELD_LINE_PROTOTYPES, **GAUSS_PROTOTYPES, **ES_PROTOTYPES, **POISSON_PROTOTYPES,
                                   **SPECTRUM_PROTOTYPES).items():
        f = getattr(L, name)
        f.restype, f.argtypes = CTYPES[ret], [CTYPES[a] for a in args]
    if L.xpic_version() & VERSION_EXPERIMENT_BIT and os.environ.get("XPIC_ALLOW_EXPERIMENT") != "1":
        raise XpicError(f"{LIB_PATH} was built with -DXPIC_EXPERIMENT (ablation switches / in-kernel timers: its results "
                        "may be wrong by design); rebuild with `make clean all`, or set XPIC_ALLOW_EXPERIMENT=1 for a "
                        "measurement script")
    _lib = L
    return L


def _array_pointer(dtype, word):
    def pointer(a):
        """a contiguous array of the dtype as the header's pointer type; None stays None, the null pointer"""
        if a is None:
            return None
        assert a.dtype == dtype and a.flags["C_CONTIGUOUS"]
        return a.ctypes.data_as(CTYPES[word])
    return pointer


_dp = _array_pointer(np.float64, "double*")
_i64p = _array_pointer(np.int64, "int64_t*")
_i32p = _array_pointer(np.int32, "int32_t*")  # (and the header's `int*`: the same ctypes type)


def _coordinate7(coordinate):
    """(enum xpic_coordinate_kind, double[7]) of a coordinate generator's dict"""
    kind = COORDINATES[coordinate["name"]]
    if kind == 0:
        g = list(coordinate["value"]) + [0.0] * 4
    elif kind == 3:
        g = list(coordinate["center"]) + [coordinate["inner_r"], coordinate["outer_r"], coordinate["height"], 0.0]
    else:
        g = list(_geom7(dict(coordinate, name="box" if kind == 1 else "cylinder"))[1])
    return kind, np.array([float(v) for v in g], dtype=np.float64)


class LoadCommands:
    """SetParticles on the device and the builder's particle count (include/xpic_set_particles.h), as methods of Context"""

    def set_particles(self, sort, n, coordinate, momentum, step=0, seed=0, particle0=0, chunk=0):
        """SetParticles for the particles particle0 .. particle0 + n - 1 of one command -> (particles added, their energy),
        summed over the slabs.  coordinate: as inject_particles', or {"name": "CoordinateOnAnnulus", "center": xyz,
        "inner_r": r, "outer_r": r, "height": h}; momentum: as inject_particles', or {"name":
        "MaxwellCosinePerturbation", "T": (Tx, Ty, Tz), "amplitude": xyz, "wave_number": xyz, "min": xyz, "max": xyz},
        or {"name": "AngularMomentum", "T": (Tx, Ty, Tz), "drift": (px, py, pz), "center": xyz}.  chunk: particles per
        launch, 0 for the library's default."""
        p = SetParticlesParams()
        p.coordinate, g = _coordinate7(coordinate)
        p.geom[:] = list(g)
        p.momentum = MOMENTA[momentum["name"]]
        p.tov = int(bool(momentum.get("tov", False)))
        p.value[:] = [float(v) for v in (momentum["value"] if p.momentum == 0 else momentum.get("drift", (0.0, 0.0, 0.0)))]
        p.T[:] = [float(v) for v in momentum.get("T", (0.0, 0.0, 0.0))]
        p.amplitude[:] = [float(v) for v in momentum.get("amplitude", (0.0, 0.0, 0.0))]
        p.wave_number[:] = [float(v) for v in momentum.get("wave_number", (0.0, 0.0, 0.0))]
        if p.momentum == 2:
            p.box6[:] = [float(v) for v in list(momentum["min"]) + list(momentum["max"])]
        p.center[:] = [float(v) for v in momentum.get("center", (0.0, 0.0, 0.0))]
        p.seed, p.chunk = int(seed), int(chunk)
        added, energy = C.c_int64(), C.c_double()
        self._ck(self.L.xpic_set_particles(self.h, int(sort), C.byref(p), int(n), int(particle0), int(step),
                                           C.byref(added), C.byref(energy)))
        return added.value, energy.value

    def particles_number(self, sort, coordinate):
        """the number of particles the reference's builder gives a SetParticles command with this coordinate generator"""
        kind, g = _coordinate7(coordinate)
        out = C.c_int64()
        self._ck(self.L.xpic_particles_number(self.h, int(sort), kind, _dp(g), C.byref(out)))
        return out.value


class TracerState(collections.namedtuple(
        "TracerState", "state exit_step iterations_sum iterations_max steps removed alive held dropped")):
    """what TracerSet.get returns: the arrays of an OpenTrace, then the set's counts (steps done since it was created,
    particles removed, particles alive, sample rows held, sample rows dropped)"""


def _region6(region):
    """(start xyz, size xyz) in global cells, as six numbers or two triples, as the header's `const int region6[6]`"""
    if region is None:
        return None
    return (C.c_int * 6)(*[int(v) for v in np.asarray(region, dtype=np.int64).reshape(6)])


class TracerMap:
    """A map of a TracerSet (include/xpic_tracer_moments.h): made by TracerSet.map, accumulates on the device until close()"""

    def __init__(self, tracers, map_id, dof):
        self.set, self.id, self.dof = tracers, map_id, dof

    def get(self, reset=False):
        """-> (array [nz][ny][nx][dof], deposits made, particle-deposits counted, the set's step count); array / deposits
        is the time average.  reset: the map and its two counters are zeroed after the copy"""
        ctx = self.set.ctx
        out, info = np.zeros((ctx.nzl, ctx.n[1], ctx.n[0], self.dof)), np.zeros(3, dtype=np.int64)
        ctx._ck(ctx.L.xpic_tracers_map_get(ctx.h, self.set.id, self.id, _dp(out), _i64p(info), int(bool(reset))))
        return (out,) + tuple(int(v) for v in info)

    def close(self):
        if self.id is not None:
            map_id, self.id = self.id, None
            self.set.ctx._ck(self.set.ctx.L.xpic_tracers_map_destroy(self.set.ctx.h, self.set.id, map_id))


class TracerSet:
    """A tracer set of a Context (include/xpic_tracers.h): made by Context.tracers, lives on the device until close()"""

    def __init__(self, ctx, set_id, n, sample_capacity=0):
        self.ctx, self.id, self.n, self.sample_capacity = ctx, set_id, n, sample_capacity

    def advance(self, steps=1):
        """`steps` steps on the context's E and B as they stand"""
        self.ctx._ck(self.ctx.L.xpic_tracers_advance(self.ctx.h, self.id, int(steps)))

    def attach(self, on=True):
        """while attached, every Context.step advances the set by one step on the fields the step leaves behind"""
        self.ctx._ck(self.ctx.L.xpic_tracers_attach(self.ctx.h, self.id, int(bool(on))))

    def detach(self):
        self.attach(False)

    def get(self):
        """-> TracerState; the arrays are copies"""
        n = self.n
        state, ex = np.zeros((n, 6)), np.zeros(n, dtype=np.int64)
        tot, mx, info = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32), np.zeros(5, dtype=np.int64)
        self.ctx._ck(self.ctx.L.xpic_tracers_get(self.ctx.h, self.id, _dp(state), _i64p(ex), _i64p(tot), _i32p(mx), _i64p(info)))
        return TracerState(state, ex, tot, mx, *(int(v) for v in info))

    def samples(self):
        """drains the sample buffer -> (samples [rows][n][6], alive [rows]); row k of a set that has never been drained is
        the state after step (k + 1) * sample_every"""
        cap = self.sample_capacity
        samples, alive, count = np.zeros((cap, self.n, 6)), np.zeros(cap, dtype=np.int64), C.c_int64()
        self.ctx._ck(self.ctx.L.xpic_tracers_samples(self.ctx.h, self.id, _dp(samples), _i64p(alive), C.byref(count)))
        return samples[:count.value], alive[:count.value]

    def moment(self, name, q, m, weight=1.0, region=None):
        """the moment `name` (a name of Context.moment) of the set's live particles as they stand -> (array
        [nz][ny][nx][dof], particles counted).  q, m: the charge and mass of a tracer; weight: what n / Np is for a sort;
        region: None (the whole box) or (start xyz, size xyz) in cells.  A particle counts iff floor(r / d) lies in it."""
        ctx = self.ctx
        out, counted = np.zeros((ctx.nzl, ctx.n[1], ctx.n[0], MOMENT_DOF[name])), C.c_int64()
        ctx._ck(ctx.L.xpic_tracers_moment(ctx.h, self.id, MOMENTS[name], float(q), float(m), float(weight), _region6(region),
                                          _dp(out), C.byref(counted)))
        return out, counted.value

    def map(self, name, q, m, weight=1.0, region=None, every=1):
        """A map -> TracerMap: whenever the set's step count reaches a multiple of `every`, in an advance or a ride, the
        moment is added into an accumulator on the device"""
        ctx, out = self.ctx, C.c_int()
        ctx._ck(ctx.L.xpic_tracers_map_create(ctx.h, self.id, MOMENTS[name], float(q), float(m), float(weight),
                                              _region6(region), int(every), C.byref(out)))
        return TracerMap(self, out.value, MOMENT_DOF[name])

    def close(self):
        if self.id is not None:
            set_id, self.id = self.id, None
            self.ctx._ck(self.ctx.L.xpic_tracers_destroy(self.ctx.h, set_id))


class TracerCommands:
    """grad |F| of a grid vector and the tracer sets (include/xpic_tracers.h), as methods of Context"""

    def grad_abs_field(self, src, dst):
        """dst = the central differences of |src| on the nodes, every index wrapped (xpic_grad_abs_field)"""
        self._ck(self.L.xpic_grad_abs_field(self.h, int(src), int(dst)))

    def tracers(self, kind, state, *params, region=None, step0=0, compact="never", gradB_field=None, sample_every=0,
                sample_capacity=0, **tolerances):
        """A tracer set -> TracerSet.  kind "full_orbit": params = (scheme, qm, dt) and atol, rtol, maxit as
        full_orbit_trace_open's; kind "drift_kinetic": params = (qm, mp, dt) and eps, delta, maxit as
        drift_kinetic_trace_open's, gradB_field a field id, None (grad B = 0) or "auto" (the set layer computes grad |B| of
        the context's B before every advance).  region: a geometry dict or None (nothing is ever removed); step0 and
        compact as the open traces'.  sample_every 0: no samples; the buffer holds sample_capacity rows."""
        state = np.ascontiguousarray(state, dtype=np.float64).reshape(-1, 6)
        k = TRACER_KINDS[kind]
        if k == 0:
            scheme, qm, dt = params
            P = self._fo_params(scheme, qm, dt, *(tolerances.pop(w, v) for w, v in (("atol", 1e-7), ("rtol", 1e-7), ("maxit", 30))))
        else:
            qm, mp, dt = params
            P = self._dk_params(qm, mp, dt, *(tolerances.pop(w, v) for w, v in (("eps", 1e-12), ("delta", 1e-12), ("maxit", 30))))
        if tolerances:
            raise XpicError("tracers: unknown arguments %s" % sorted(tolerances))
        reg = None
        if region is not None:
            geom, gp = _geom7(region)
            reg = C.byref(TraceRegion(geom, int(COMPACT.get(compact, compact)), (C.c_double * 7)(*gp[:7]), int(step0)))
        gB = -1 if gradB_field is None else GRADB_AUTO if isinstance(gradB_field, str) and gradB_field == "auto" else int(gradB_field)
        out = C.c_int()
        self._ck(self.L.xpic_tracers_create(self.h, k, state.shape[0], C.cast(C.pointer(P), C.c_void_p), _dp(state), reg, gB,
                                            int(sample_every), int(sample_capacity), C.byref(out)))
        return TracerSet(self, out.value, state.shape[0], int(sample_capacity) if sample_every else 0)


class FieldLines(collections.namedtuple("FieldLines", "end length volume fmin smin fmax steps code samples directions")):
    """What Context.field_lines / model_field_lines return.  The raw arrays, [2][n] each with row 0 the lanes that followed
    +F and row 1 those that followed -F (end: [2][n][3]; samples: [2][n][nsamp][3] or None); a row whose direction was not
    asked for (directions: 1, 2 or 3) is zeros, with code -1.  The properties combine the directions that were."""
    __slots__ = ()

    @property
    def _rows(self):
        return [d for d in (0, 1) if self.directions & (1 << d)]

    @property
    def total_length(self):
        """the length of the whole line through each seed [n]"""
        return self.length[self._rows].sum(axis=0)

    @property
    def total_volume(self):
        """the flux-tube volume, the integral of dl / |F| along the whole line [n]"""
        return self.volume[self._rows].sum(axis=0)

    @property
    def mirror_ratio(self):
        """max |F| / min |F| over the whole line [n]"""
        return self.fmax[self._rows].max(axis=0) / self.fmin[self._rows].min(axis=0)

    @property
    def codes(self):
        """the two lanes' codes per seed [n][2] (LINE_CODES; -1: the direction was not followed)"""
        return self.code.T.copy()

    @property
    def ends(self):
        """the two end points per seed [n][2][3]"""
        return self.end.transpose(1, 0, 2).copy()


class FieldLineCommands:
    """field lines of a grid vector or of an analytic model (include/xpic_field_lines.h), as methods of Context"""

    def _field_lines(self, call, seeds, which, h, max_steps, region, directions, f_floor, close_tol, sample_every, launch_steps):
        seeds = np.ascontiguousarray(seeds, dtype=np.float64).reshape(-1, 3)
        n = seeds.shape[0]
        if h is None or max_steps is None:
            raise XpicError("field_lines: h and max_steps are required")
        d = int(LINE_DIRECTIONS.get(directions, directions))
        w = int(STAGGERS.get(which, which))
        P = LineParams(float(h), int(max_steps), float(f_floor), float(close_tol), w, d, int(launch_steps), w)
        reg = None
        if region is not None:
            geom, gp = _geom7(region)
            reg = C.byref(TraceRegion(geom, COMPACT["never"], (C.c_double * 7)(*gp[:7]), 0))
        nsamp = int(max_steps) // int(sample_every) if sample_every > 0 else 0
        end = np.zeros((2, n, 3))
        length, volume, fmin, smin, fmax = (np.zeros((2, n)) for _ in range(5))
        steps, code = np.zeros((2, n), dtype=np.int64), np.full((2, n), -1, dtype=np.int32)
        samples = np.zeros((2, n, nsamp, 3)) if sample_every > 0 else None
        self._ck(call(n, _dp(seeds), C.byref(P), reg, int(sample_every), _dp(end), _dp(length), _dp(volume), _dp(fmin), _dp(smin),
                      _dp(fmax), _i64p(steps), _i32p(code), _dp(samples)))
        return FieldLines(end, length, volume, fmin, smin, fmax, steps, code, samples, d)

    def field_lines(self, seeds, field=B, h=None, max_steps=None, region=None, directions="both", stagger=None, f_floor=0.0,
                    close_tol=0.0, sample_every=0, launch_steps=0):
        """The lines of the grid vector `field` through seeds [n][3] -> FieldLines.  h: the arc-length step; max_steps: 1 ..
        LINES_MAX_STEPS per direction; region: a geometry dict as the open traces take, or None; directions: "+", "-" or
        "both"; stagger: "B" or "E", how the vector is staggered (default: "E" for the field E, else "B"); a lane stops with
        code "null" where |F| < f_floor (or is 0), with "closed" within close_tol of its seed (0: never); sample_every k:
        every k-th point; launch_steps: steps per launch, 0 for the library's default (no result depends on it)."""
        if stagger is None:
            stagger = "E" if int(field) == E else "B"
        return self._field_lines(lambda *a: self.L.xpic_field_lines(self.h, int(field), *a), seeds, stagger, h, max_steps, region,
                                 directions, f_floor, close_tol, sample_every, launch_steps)

    def model_field_lines(self, model, seeds, h=None, max_steps=None, region=None, directions="both", component="B",
                          f_floor=0.0, close_tol=0.0, sample_every=0, launch_steps=0):
        """field_lines on B (or component="E") of an analytic model (what field_model(...) returns); any context"""
        return self._field_lines(lambda *a: self.L.xpic_model_field_lines(self.h, model, *a), seeds, component, h, max_steps,
                                 region, directions, f_floor, close_tol, sample_every, launch_steps)


class GaussClean(collections.namedtuple("GaussClean", "iterations before after mean gphi phi")):
    """One clean: CG iterations, |res|_2 before and after (the latter from the corrected field), the mean charge density
    taken out (the neutralising background), |G phi|_2, and phi [nzl][ny][nx] where it was asked for (else None)"""


class GaussCommands:
    """Gauss's law div E = rho on the device (include/xpic_gauss.h; the reference has no cleaner), as methods of Context.
    The calls use the vector W2 as scratch."""

    def gauss_background(self, rho):
        """a static charge density [nzl][ny][nx] that counts with the sorts' (None clears it)"""
        if rho is not None:
            rho = np.ascontiguousarray(rho, dtype=np.float64).reshape(self.nzl, self.n[1], self.n[0])
        self._ck(self.L.xpic_gauss_background(self.h, _dp(rho)))

    def gauss_residual(self, field=E, want_residual=False):
        """res = D F - (rho - mean rho) -> dict(l1, l2, mean, rho_l2) (+ residual [nzl][ny][nx] with want_residual)"""
        res = np.zeros((self.nzl, self.n[1], self.n[0])) if want_residual else None
        o = np.zeros(4)
        self._ck(self.L.xpic_gauss_residual(self.h, int(field), _dp(res), _dp(o)))
        out = dict(l1=o[0], l2=o[1], mean=o[2], rho_l2=o[3])
        if want_residual:
            out["residual"] = res
        return out

    def gauss_clean(self, field=E, rtol=1e-10, atol=0.0, maxit=GAUSS_MAXIT, want_phi=False):
        """F <- F - G phi with D G phi = res, by CG until |r|_2 <= max(rtol |rho - mean|_2, atol) -> GaussClean; raises
        XpicError (the field untouched) when maxit iterations do not get there"""
        phi = np.zeros((self.nzl, self.n[1], self.n[0])) if want_phi else None
        o, its = np.zeros(4), C.c_int()
        self._ck(self.L.xpic_gauss_clean(self.h, int(field), float(rtol), float(atol), int(maxit), _dp(phi), C.byref(its), _dp(o)))
        return GaussClean(its.value, o[0], o[1], o[2], o[3], phi)

    def set_gauss_clean(self, every, rtol=1e-10, atol=0.0, maxit=GAUSS_MAXIT):
        """every k > 0: each step() whose count is a multiple of k cleans E before the tracer sets ride; 0: off"""
        self._ck(self.L.xpic_set_gauss_clean(self.h, int(every), float(rtol), float(atol), int(maxit)))

    def gauss_info(self):
        o = np.zeros(6)
        self._ck(self.L.xpic_gauss_info(self.h, _dp(o)))
        return dict(cleans=int(o[0]), iterations=int(o[1]), before=o[2], after=o[3], mean=o[4], last_iterations=int(o[5]))


class EsCommands:
    """The electrostatic scheme "es" (include/xpic_es.h; the reference has none), as methods of Context: the scheme itself
    is Context("es", ...).step(), which returns the CG iterations of the step's Poisson solve."""

    def es_push(self, sort):
        """the electrostatic scheme's gather, kick, full move and charge deposit of one sort (include/xpic_es.h) -> that
        sort's rho [nzl][ny][nx] at the new positions; no re-bin (update_cells) and no field solve"""
        rho = np.zeros((self.nzl, self.n[1], self.n[0]))
        self._ck(self.L.xpic_es_push(self.h, int(sort), _dp(rho)))
        return rho


class PoissonCommands:
    """The direct Poisson solve (include/xpic_poisson.h; the reference has none), as methods of Context: which solve the
    cleans and the "es" step take, and one application of the transform solve alone."""

    def set_poisson_solver(self, kind):
        """"cg" (the default of every context) or "direct": the separable Hartley-transform solve with iterative refinement,
        on contexts without ghost planes and with extents up to POISSON_MAX_EXTENT; a clean's and a step's iterations then
        count its applications"""
        if kind not in POISSON_SOLVERS and not isinstance(kind, int):
            raise XpicError("set_poisson_solver: %r is none of %s" % (kind, sorted(POISSON_SOLVERS)))
        self._ck(self.L.xpic_set_poisson_solver(self.h, int(POISSON_SOLVERS.get(kind, kind))))

    @property
    def poisson_solver(self):
        kind = C.c_int()
        self._ck(self.L.xpic_get_poisson_solver(self.h, C.byref(kind)))
        return {v: k for k, v in POISSON_SOLVERS.items()}[kind.value]

    def poisson_apply(self, rhs):
        """one application of the transform solve to rhs - mean(rhs) [nz][ny][nx] -> the mean-free phi with D G phi = that;
        no refinement, whatever poisson_solver is"""
        rhs = np.ascontiguousarray(rhs, dtype=np.float64).reshape(self.nzl, self.n[1], self.n[0])
        phi = np.zeros_like(rhs)
        self._ck(self.L.xpic_poisson_apply(self.h, _dp(rhs), _dp(phi)))
        return phi

    def poisson_solve(self, rhs, tol=0.0, maxit=1):
        """the refinement the "direct" clean runs, on rhs - mean(rhs) [nz][ny][nx] from phi = 0 until |r|_2 <= tol ->
        (phi, applications, the last explicit |r|_2), whatever poisson_solver is.  Not converging is no error: tol = 0,
        maxit = k gives k applications while each halves the residual it was given; maxit = 1 is poisson_apply's bits"""
        rhs = np.ascontiguousarray(rhs, dtype=np.float64).reshape(self.nzl, self.n[1], self.n[0])
        phi = np.zeros_like(rhs)
        its, rn = C.c_int(), C.c_double()
        self._ck(self.L.xpic_poisson_solve(self.h, _dp(rhs), float(tol), int(maxit), _dp(phi), C.byref(its), C.byref(rn)))
        return phi, its.value, rn.value


class Spectrum(collections.namedtuple("Spectrum", "axis k_axis shell shell_count k_edges outside outside_count total")):
    """The reduced spectrum of a scalar: axis[a][i] = the sum of P over the other two indices at index i of axis a (x, y, z),
    k_axis[a][i] its folded physical wavenumber 2 pi m / (n_a d_a), m in (-n_a/2, n_a/2]; shell[j] the power and
    shell_count[j] the modes with k_edges[j] <= |k| < k_edges[j+1] (empty arrays without shells); outside, outside_count:
    the modes in no shell; total = sum_k P = sum_j x(j)^2"""


class SpectrumProbe:
    """A probe of modes that rides with Context.step() (include/xpic_spectrum.h): get() -> (steps [r], F^ [r][nmodes]
    complex, dropped), reset=True empties it afterwards; close() frees it"""

    def __init__(self, ctx, pid, nmodes):
        self.ctx, self.id, self.nmodes = ctx, pid, nmodes

    def get(self, reset=False):
        c = self.ctx
        rec, drop = C.c_int64(), C.c_int64()
        c._ck(c.L.xpic_spectrum_probe_get(c.h, self.id, 0, None, None, C.byref(rec), C.byref(drop), 0))
        steps = np.zeros(rec.value, dtype=np.int64)
        out = np.zeros((rec.value, self.nmodes, 2))
        c._ck(c.L.xpic_spectrum_probe_get(c.h, self.id, rec.value, _i64p(steps), _dp(out), C.byref(rec), C.byref(drop), int(reset)))
        return steps, out[..., 0] + 1j * out[..., 1], drop.value

    def close(self):
        if self.id is not None:
            self.ctx._ck(self.ctx.L.xpic_spectrum_probe_destroy(self.ctx.h, self.id))
            self.id = None


class SpectrumCommands:
    """Field spectra on the device (include/xpic_spectrum.h; the reference has none), as methods of Context.  source: a
    field id (comp 0, 1 or 2 is then needed), "rho" (the charge density gauss_residual deposits, the mean left in) or a
    numpy scalar [nz][ny][nx].  F^(k) = sum_j x(j) exp(-2 pi i k.j / n) / sqrt(N) on the node index of the component's own
    array (no Yee stagger); P = |F^|^2."""

    def _spectrum_source(self, source, comp):
        """(source id, comp, the host scalar or None)"""
        if isinstance(source, str):
            if source not in SPECTRUM_SOURCES or source == "host":
                raise XpicError("spectrum: %r is no source (a field id, \"rho\" or an array)" % (source,))
            return SPECTRUM_SOURCES[source], 0, None
        if isinstance(source, (int, np.integer)):
            if comp is None:
                raise XpicError("spectrum: a field source needs comp (0, 1 or 2)")
            return int(source), int(comp), None
        scalar = np.ascontiguousarray(source, dtype=np.float64).reshape(self.nzl, self.n[1], self.n[0])
        return SPECTRUM_SOURCES["host"], 0, scalar

    def spectrum_power(self, source, comp=None):
        """P [nz][ny][nx], index (kz, ky, kx), unfolded: index n - m is wavenumber -m"""
        sid, comp, scalar = self._spectrum_source(source, comp)
        out = np.zeros((self.nzl, self.n[1], self.n[0]))
        self._ck(self.L.xpic_spectrum_power(self.h, sid, comp, _dp(scalar), _dp(out)))
        return out

    def spectrum(self, source, comp=None, dk=None, nshell=0, edges=None):
        """The axis spectra, the total and shells of |k| -> Spectrum.  edges: ascending shell edges in |k| (nshell + 1 of
        them), or dk and nshell for edges = dk * arange(nshell + 1); neither: no shells"""
        sid, comp, scalar = self._spectrum_source(source, comp)
        if edges is None and dk is not None:
            edges = float(dk) * np.arange(int(nshell) + 1)
        edges = np.zeros(0) if edges is None else np.ascontiguousarray(edges, dtype=np.float64)
        ns = max(edges.size - 1, 0) if edges.size else int(nshell)
        if edges.size and not (edges >= 0.0).all():  # (a NaN too: the edges are |k|)
            raise XpicError("spectrum: the shell edges are |k| and must be finite and >= 0")
        e2 = np.ascontiguousarray(edges * edges) if edges.size else None
        axis = [np.zeros(self.n[0]), np.zeros(self.n[1]), np.zeros(self.nzl)]
        shell, count, outside, total = np.zeros(max(ns, 0)), np.zeros(max(ns, 0), dtype=np.int64), np.zeros(2), C.c_double()
        self._ck(self.L.xpic_spectrum(self.h, sid, comp, _dp(scalar), _dp(axis[0]), _dp(axis[1]), _dp(axis[2]), ns, _dp(e2),
                                      _dp(shell) if ns > 0 else None, _i64p(count) if ns > 0 else None, _dp(outside),
                                      C.byref(total)))
        k_axis = []
        for a, n in enumerate((self.n[0], self.n[1], self.nzl)):
            m = np.arange(n)
            k_axis.append(2.0 * np.pi * np.where(m <= n // 2, m, m - n) / (n * self.d[a]))
        return Spectrum(axis, k_axis, shell, count, edges, outside[0], int(outside[1]), total.value)

    def spectrum_modes(self, source, modes, comp=None):
        """F^ (complex [nmodes]) of the signed mode numbers modes [nmodes][3] = (m_x, m_y, m_z)"""
        sid, comp, scalar = self._spectrum_source(source, comp)
        modes = np.ascontiguousarray(modes, dtype=np.int32).reshape(-1, 3)
        out = np.zeros((modes.shape[0], 2))
        self._ck(self.L.xpic_spectrum_modes(self.h, sid, comp, _dp(scalar), modes.shape[0], _i32p(modes), _dp(out)))
        return out[:, 0] + 1j * out[:, 1]

    def spectrum_probe(self, source, modes, comp=None, every=1, capacity=4096):
        """A passive probe of the modes [nmodes][3] of a field component or of "rho": after every every-th step() -- after
        the riding clean and the attached tracer sets -- one row (step, F^ per mode) goes to a device buffer of `capacity`
        rows; a full buffer counts what it drops -> SpectrumProbe"""
        if not isinstance(source, (str, int, np.integer)):
            raise XpicError("spectrum_probe: an array is no probe source (a field id or \"rho\")")
        sid, comp, _ = self._spectrum_source(source, comp)
        modes = np.ascontiguousarray(modes, dtype=np.int32).reshape(-1, 3)
        pid = C.c_int()
        self._ck(self.L.xpic_spectrum_probe_create(self.h, sid, comp, modes.shape[0], _i32p(modes), int(every), int(capacity),
                                                   C.byref(pid)))
        return SpectrumProbe(self, pid.value, modes.shape[0])


class Context(LoadCommands, TracerCommands, FieldLineCommands, GaussCommands, EsCommands, PoissonCommands, SpectrumCommands):
    """One z-slab context = one `interfaces::Simulation` backend instance."""

    def __init__(self, scheme, n, d, dt, device=0, rank=0, nranks=1, self_ring=False):
        self.L = load_library()
        g = Geometry()
        g.n[:] = [int(v) for v in n]
        g.d[:] = [float(v) for v in d]
        g.dt = float(dt)
        g.periodic[:] = [1, 1, 1]
        g.rank, g.nranks, g.device, g.self_ring = rank, nranks, device, int(self_ring)
        self.n = tuple(int(v) for v in n)
        self.d = tuple(float(v) for v in d)
        self.dt = float(dt)
        self.scheme = scheme
        self.rank, self.nranks = rank, nranks
        self.nzl = self.n[2] // nranks  # planes of this z-slab
        self.z0 = rank * self.nzl
        self.h = C.c_void_p()
        self._ck(self.L.xpic_create(C.byref(g), SCHEMES[scheme], C.byref(self.h)))
        self.N = self.n[0] * self.n[1] * self.nzl  # local cells
        self.nsorts = 0
        self._cb = None

    # ---- z-slab communicator
    def comm_init_rccl(self, id128):
        buf = (C.c_char * 128).from_buffer_copy(bytes(id128))
        self._ck(self.L.xpic_comm_init_rccl(self.h, buf))

    def comm_init_callbacks(self, sendrecv, allreduce_sum):
        """sendrecv(down: bytes, up: bytes, n_from_up, n_from_down) -> (from_up: bytes, from_down: bytes);
        allreduce_sum(np.ndarray[float64]) -> reduces in place.  Used by tests (torch.distributed / gloo)."""
        def _sr(user, down, nd, up, nu, fu, nfu, fd, nfd):
            try:
                a, b = sendrecv(C.string_at(down, nd) if nd else b"", C.string_at(up, nu) if nu else b"", nfu, nfd)
                if nfu:
                    C.memmove(fu, a, nfu)
                if nfd:
                    C.memmove(fd, b, nfd)
                return 0
            except Exception as e:  # pragma: no cover
                print("xpic comm callback failed:", e, flush=True)
                return 1

        def _ar(user, buf, n):
            try:
                arr = np.ctypeslib.as_array(buf, shape=(n,))
                allreduce_sum(arr)
                return 0
            except Exception as e:  # pragma: no cover
                print("xpic comm callback failed:", e, flush=True)
                return 1

        _, (_, SR), (_, AR) = CommCallbacks._fields_
        self._cb = CommCallbacks(None, SR(_sr), AR(_ar))
        self._ck(self.L.xpic_comm_init_callbacks(self.h, C.byref(self._cb)))

    def comm_peer_export(self):
        """the blob (bytes) that tells a z-neighbour where this rank receives its matL ghost rows (copy-engine path)"""
        buf = (C.c_char * PEER_BLOB_BYTES)()
        self._ck(self.L.xpic_comm_peer_export(self.h, buf))
        return bytes(buf)

    def comm_peer_import(self, lower_blob, upper_blob):
        lo = (C.c_char * PEER_BLOB_BYTES).from_buffer_copy(bytes(lower_blob))
        up = (C.c_char * PEER_BLOB_BYTES).from_buffer_copy(bytes(upper_blob))
        self._ck(self.L.xpic_comm_peer_import(self.h, lo, up))

    def comm_size(self):
        n = C.c_int()
        self._ck(self.L.xpic_comm_size(self.h, C.byref(n)))
        return n.value

    def _ck(self, rc):
        if rc != 0:
            raise XpicError(f"xpic error {rc}: {self.L.xpic_last_error().decode()}")

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.xpic_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- particles
    def add_sort(self, Np, n, q, m, capacity):
        p = SortParams(int(Np), float(n), float(q), float(m))
        out = C.c_int()
        self._ck(self.L.xpic_add_sort(self.h, C.byref(p), int(capacity), C.byref(out)))
        self.nsorts += 1
        return out.value

    def add_particles(self, sort, pts):
        pts = np.ascontiguousarray(pts, dtype=np.float64)
        added = C.c_int64()
        self._ck(self.L.xpic_sort_add_particles(self.h, sort, pts.shape[0], _dp(pts), C.byref(added)))
        return added.value

    def count(self, sort):
        n = C.c_int64()
        self._ck(self.L.xpic_sort_count(self.h, sort, C.byref(n)))
        return n.value

    def particles(self, sort):
        n = self.count(sort)
        pts = np.zeros((n, 6))
        cells = np.zeros(n, dtype=np.int32)
        self._ck(self.L.xpic_sort_get_particles(self.h, sort, _dp(pts), _i32p(cells)))
        return pts, cells

    def clear(self, sort):
        self._ck(self.L.xpic_sort_clear(self.h, sort))

    def fill_synthetic(self, sort, ppc, vth, seed=1, regular=False):
        self._ck(self.L.xpic_sort_fill_synthetic(self.h, sort, int(ppc), vth, seed, int(regular)))

    def load_synthetic(self, sort, ppc, vth, seed=1, profile="poisson", drift=(0.0, 0.0, 0.0), param=(0.0, 0.0)):
        """fill_synthetic with a drift (MaxwellianMomentum's px, py, pz: an extension of the reference's JSON surface) and
        a density profile: "gradient" (param[0] : 1 along x) or "blob" (fraction param[0] in a Gaussian of param[1] cells)"""
        lp = LoadParams()
        lp.ppc, lp.profile, lp.vth, lp.seed = int(ppc), LOAD_PROFILES[profile], float(vth), int(seed)
        lp.drift[:] = [float(v) for v in drift]
        lp.profile_param[:] = [float(v) for v in param] + [0.0] * (4 - len(param))
        self._ck(self.L.xpic_sort_load_synthetic(self.h, sort, C.byref(lp)))

    def occupancy(self, sort):
        """dict of the cell / pencil occupancy statistics of a sort (include/xpic_hip.h: xpic_sort_occupancy)"""
        o = (C.c_int64 * 8)()
        self._ck(self.L.xpic_sort_occupancy(self.h, sort, o))
        keys = ("max_cell", "cells_over_64", "cells_over_128", "cells_over_bucket", "max_pencil", "min_pencil", "empty_cells",
                "bucket_cap")
        return dict(zip(keys, (int(v) for v in o)))

    # ---- fields
    def fshape(self):
        return (self.nzl, self.n[1], self.n[0], 3)

    def set_field(self, f, v):
        v = np.ascontiguousarray(v, dtype=np.float64).reshape(self.fshape())
        self._ck(self.L.xpic_field_set(self.h, f, _dp(v)))

    def get_field(self, f):
        v = np.zeros(self.fshape())
        self._ck(self.L.xpic_field_get(self.h, f, _dp(v)))
        return v

    def sort_current(self, sort, which):
        v = np.zeros(self.fshape())
        self._ck(self.L.xpic_sort_current_get(self.h, sort, which, _dp(v)))
        return v

    def vec_set(self, y, a):
        self._ck(self.L.xpic_vec_set(self.h, y, a))

    def vec_axpy(self, y, a, x):
        self._ck(self.L.xpic_vec_axpy(self.h, y, a, x))

    def vec_axpby(self, y, a, b, x):
        self._ck(self.L.xpic_vec_axpby(self.h, y, a, b, x))

    def vec_dot(self, x, y):
        o = C.c_double()
        self._ck(self.L.xpic_vec_dot(self.h, x, y, C.byref(o)))
        return o.value

    def vec_norm2(self, x):
        o = C.c_double()
        self._ck(self.L.xpic_vec_norm2(self.h, x, C.byref(o)))
        return o.value

    # ---- operators
    def rot_apply(self, sign, alpha, x, y, add=False):
        self._ck(self.L.xpic_rot_apply(self.h, sign, alpha, x, y, int(add)))

    def matM_apply(self, x, y, add=False):
        self._ck(self.L.xpic_matM_apply(self.h, x, y, int(add)))

    def matL_apply(self, x, y, add=False):
        self._ck(self.L.xpic_matL_apply(self.h, x, y, int(add)))

    def matA_apply(self, x, y):
        self._ck(self.L.xpic_matA_apply(self.h, x, y))

    def matL(self):
        out = np.zeros((self.N * 3, LSTENCIL))
        self._ck(self.L.xpic_matL_get(self.h, _dp(out)))
        return out

    # ---- phases
    def ecsim_first_push(self, sort):
        self._ck(self.L.xpic_ecsim_first_push(self.h, sort))

    def update_cells(self, sort):
        n = C.c_int64()
        self._ck(self.L.xpic_update_cells(self.h, sort, C.byref(n)))
        return n.value

    def ecsim_fill_current(self):
        self._ck(self.L.xpic_ecsim_fill_current(self.h))

    def ecsim_second_push(self, sort):
        self._ck(self.L.xpic_ecsim_second_push(self.h, sort))

    def basic_push(self, sort):
        self._ck(self.L.xpic_basic_push(self.h, sort))

    def ecsimcorr_first_push(self, sort):
        self._ck(self.L.xpic_ecsimcorr_first_push(self.h, sort))

    def ecsimcorr_second_push(self, sort):
        self._ck(self.L.xpic_ecsimcorr_second_push(self.h, sort))

    def ecsimcorr_final_update(self, sort):
        self._ck(self.L.xpic_ecsimcorr_final_update(self.h, sort))

    def calculate_energy(self, sort):
        o = C.c_double()
        self._ck(self.L.xpic_calculate_energy(self.h, sort, C.byref(o)))
        return o.value

    def ecsimcorr_scalars(self, sort):
        o = np.zeros(6)
        self._ck(self.L.xpic_ecsimcorr_scalars(self.h, sort, _dp(o)))
        return dict(pred_w=o[0], corr_w=o[1], lambda_dK=o[2], pred_dK=o[3], corr_dK=o[4], energy=o[5])

    def solve(self, op, rhs, x, rtol=1e-7, atol=1e-7, maxit=100):
        its, reason, rn = C.c_int(), C.c_int(), C.c_double()
        self._ck(self.L.xpic_solve(self.h, op, rhs, x, rtol, atol, maxit, C.byref(its), C.byref(reason), C.byref(rn)))
        return its.value, reason.value, rn.value

    def set_tolerances(self, rtol, atol, maxit):
        self._ck(self.L.xpic_set_tolerances(self.h, rtol, atol, maxit))

    def set_preconditioner(self, kind, degree=0):
        self._ck(self.L.xpic_set_preconditioner(self.h, int(kind), int(degree)))

    def precond_apply(self, op, r, out):
        """out = P r as the next solve(op, ...) would apply its preconditioner to a Krylov vector (test hook)"""
        self._ck(self.L.xpic_precond_apply(self.h, int(op), int(r), int(out)))

    def precond_get(self):
        """the surrogate of kinds 3 - 5 as its last build left it (test hook; include/xpic_hip.h: xpic_precond_get):
        dict of the interval, bounds, degree, flags, `abar` [3][124] and `rscale` in get_field's layout"""
        info, abar, rs = np.zeros(11), np.zeros((3, LSTENCIL + 1)), np.zeros(self.fshape())
        self._ck(self.L.xpic_precond_get(self.h, _dp(info), _dp(abar), _dp(rs)))
        return dict(lo=info[0], hi=info[1], gershgorin=info[2], degree=int(info[3]), scaled=bool(info[4]), proven=bool(info[5]),
                    valid=bool(info[6]), rmax=info[7], spread=info[8:11].copy(), abar=abar, rscale=rs)

    def comm_stats(self, reset=False):
        """(messages sent, bytes sent, all-reduces, all-reduce payload bytes) of this rank since the last reset"""
        o = (C.c_int64 * 4)()
        self._ck(self.L.xpic_comm_stats(self.h, o, int(reset)))
        return tuple(int(v) for v in o)

    def set_fill_kernel(self, kind):
        """0 (default): classic 4-wave assembly kernel; 1: warp-specialised 16-wave kernel where the grid allows (measured slower)"""
        self._ck(self.L.xpic_set_fill_kernel(self.h, int(kind)))

    def set_fused_rebin(self, on):
        """1 (default): a re-binning's scatter is left to the next kernel that reads every particle (the assembly in ecsim / ecsimcorr, the next push in basic); 2: to ecsim's second push; 0: scatter first"""
        self._ck(self.L.xpic_set_fused_rebin(self.h, int(on)))

    def fill_variant(self):
        """(power-of-two spacings, full-chunk body, warp-specialised body) of the next assembly"""
        o = (C.c_int * 3)()
        self._ck(self.L.xpic_get_fill_variant(self.h, o))
        return bool(o[0]), bool(o[1]), bool(o[2])

    def debug_set(self, what, value):
        """test hooks (include/xpic_hip.h): DEBUG_GATHER_WINDOW, DEBUG_PENCIL_LIMIT"""
        self._ck(self.L.xpic_debug_set(self.h, int(what), int(value)))

    def set_overlap(self, on):
        self._ck(self.L.xpic_set_overlap(self.h, int(on)))  # bit 0: operator halos, bit 1: matL ghost rows

    def step(self):
        """one timestep -> the step's Krylov iterations ("es": the CG iterations of its Poisson solve)"""
        its = C.c_int()
        self._ck(self.L.xpic_step(self.h, C.byref(its)))
        return its.value

    def energy(self):
        out = np.zeros(4 + 2 * self.nsorts)
        self._ck(self.L.xpic_energy(self.h, _dp(out)))
        return out

    def momentum(self):
        out = np.zeros((self.nsorts, 6))
        self._ck(self.L.xpic_momentum(self.h, _dp(out)))
        return out

    def charge_density(self, sort):
        rho = np.zeros((self.nzl, self.n[1], self.n[0]))
        self._ck(self.L.xpic_charge_density(self.h, sort, _dp(rho)))
        return rho

    def moment_density(self, sort):
        out = np.zeros((self.nzl, self.n[1], self.n[0]))
        self._ck(self.L.xpic_moment_density(self.h, sort, _dp(out)))
        return out

    def moment(self, sort, name, region=None):
        """DistributionMoment `name` of one sort (include/xpic_hip.h: xpic_moment) -> (nzl, ny, nx, dof) over this slab.
        region: None (the whole box) or (start xyz, size xyz) in global cells, as six numbers or two triples."""
        dof = MOMENT_DOF[name]
        out = np.zeros((self.nzl, self.n[1], self.n[0], dof))
        reg = None
        if region is not None:
            reg = (C.c_int * 6)(*[int(v) for v in np.asarray(region, dtype=np.int64).reshape(6)])
        self._ck(self.L.xpic_moment(self.h, sort, MOMENTS[name], reg, _dp(out)))
        return out

    def velocity_distribution(self, sort, projector, geometry, vmin=(-1.0, -1.0), vmax=(1.0, 1.0), dv=(0.1, 0.1)):
        """VelocityDistribution of one sort (include/xpic_hip.h: xpic_velocity_distribution) -> (array [vsize_y][vsize_x],
        vstart (x, y)), the whole histogram on every slab.  geometry: {"name": "box", "min": xyz, "max": xyz} or
        {"name": "cylinder", "center": xyz, "radius": r, "height": h} ("BoxGeometry" / "CylinderGeometry" as well)."""
        kind, gp = _geom7(geometry)  # (the header's `const double geom[7]`, of which this entry point reads six at most)
        vreg = np.array([vmin[0], vmin[1], vmax[0], vmax[1], dv[0], dv[1]], dtype=np.float64)
        vg = (C.c_int * 4)()  # vsize_x, vsize_y, vstart_x, vstart_y (include/xpic_hip.h)
        self._ck(self.L.xpic_velocity_distribution(self.h, sort, PROJECTORS[projector], kind, _dp(gp), _dp(vreg), vg, None))
        out = np.zeros((vg[1], vg[0]))
        self._ck(self.L.xpic_velocity_distribution(self.h, sort, PROJECTORS[projector], kind, _dp(gp), _dp(vreg), vg, _dp(out)))
        return out, (int(vg[2]), int(vg[3]))

    # ---- the per-step commands (include/xpic_hip.h: xpic_remove_particles ... xpic_set_coils_field)
    def remove_particles(self, sort, geometry):
        """RemoveParticles: empties every cell whose corner lies outside `geometry` -> (records removed, their energy),
        summed over the slabs"""
        kind, gp = _geom7(geometry)
        n, e = C.c_int64(), C.c_double()
        self._ck(self.L.xpic_remove_particles(self.h, sort, kind, _dp(gp), C.byref(n), C.byref(e)))
        return n.value, e.value

    def fields_damping(self, geometry, coefficient, E=E, B=B, B0=B0):
        """FieldsDamping of E and B - B0 outside `geometry` -> the damped energy, summed over the slabs"""
        kind, gp = _geom7(geometry)
        e = C.c_double()
        self._ck(self.L.xpic_fields_damping(self.h, E, B, B0, kind, _dp(gp), coefficient, C.byref(e)))
        return e.value

    def inject_particles(self, ionized, ejected, pairs, step, coordinate, momentum_i, momentum_e, seed=1):
        """InjectParticles of `pairs` pairs at step `step` -> (pairs added, (energy ionized, energy ejected)), summed over
        the slabs.  coordinate: {"name": "PreciseCoordinate", "value": xyz} or a CoordinateInBox / CoordinateInCylinder
        geometry dict (keys as remove_particles'); momentum_*: {"name": "PreciseMomentum", "value": xyz} or
        {"name": "MaxwellianMomentum", "T": (Tx, Ty, Tz), "drift": (px, py, pz), "tov": bool}."""
        p = InjectParams()
        p.coordinate = COORDINATES[coordinate["name"]]
        if p.coordinate == 0:
            p.geom[:] = [float(v) for v in coordinate["value"]] + [0.0] * 4
        else:
            p.geom[:] = [float(v) for v in _geom7(dict(coordinate, name="box" if p.coordinate == 1 else "cylinder"))[1]]
        for k, m in enumerate((momentum_i, momentum_e)):
            mp = p.momentum[k]
            mp.kind = MOMENTA[m["name"]]
            mp.tov = int(bool(m.get("tov", False)))
            mp.value[:] = [float(v) for v in (m["value"] if mp.kind == 0 else m.get("drift", (0.0, 0.0, 0.0)))]
            mp.T[:] = [float(v) for v in m.get("T", (0.0, 0.0, 0.0))]
        p.seed = int(seed)
        added, e2 = C.c_int64(), np.zeros(2)
        self._ck(self.L.xpic_inject_particles(self.h, ionized, ejected, C.byref(p), int(pairs), int(step),
                                              C.byref(added), _dp(e2)))
        return added.value, (float(e2[0]), float(e2[1]))

    def collide(self, sort_a, sort_b, strength, step, seed=0, dt=None):
        """Takizuka-Abe binary collisions of sort_a with sort_b (the same sort: intra-species) inside every cell
        (include/xpic_hip.h: xpic_collide; an extension, the reference has no collision operator) -> dict of the pairs
        collided, the pairs skipped (|u| == 0), the sum of sigma^2 over the collided pairs and the pairs with
        sigma^2 > 1, summed over the slabs.  dt: None for the context's."""
        return self._collide(self.L.xpic_collide, sort_a, sort_b, strength, step, seed, dt, 4)[0]

    def _collide(self, entry, sort_a, sort_b, strength, step, seed, dt, counters):
        """xpic_collide or xpic_collide_weighted -> (Context.collide's dict, the entry point's counters)"""
        p = CollisionParams(float(strength), 0.0 if dt is None else float(dt), int(seed))
        o = np.zeros(counters)
        self._ck(entry(self.h, int(sort_a), int(sort_b), C.byref(p), int(step), _dp(o)))
        return dict(pairs=int(o[0]), skipped=int(o[1]), sigma2_sum=float(o[2]), sigma2_over_1=int(o[3])), o

    def collide_weighted(self, sort_a, sort_b, strength, step, seed=0, dt=None):
        """Nanbu-Yonemura binary collisions of sort_a with sort_b, whose weights n / Np may differ (include/xpic_hip.h:
        xpic_collide_weighted; an extension): the lighter-weighted record of a pair is always updated, the
        heavier-weighted one with probability w_min / w_max -> Context.collide's dict plus the heavier-side updates made
        (heavy_updates) and rejected (heavy_rejected), summed over the slabs.  Momentum and energy are conserved in
        expectation only.  dt: None for the context's."""
        out, o = self._collide(self.L.xpic_collide_weighted, sort_a, sort_b, strength, step, seed, dt, 6)
        return dict(out, heavy_updates=int(o[4]), heavy_rejected=int(o[5]))

    def collide_info(self):
        """dict of the kernel's LDS-path limit (XPIC_COLLIDE_LDS_CELL as the library was built) and the local cells of
        the last collide() that took the second path"""
        o = (C.c_int64 * 2)()
        self._ck(self.L.xpic_collide_info(self.h, o))
        return dict(lds_cell=int(o[0]), large_cells=int(o[1]))

    def set_coils_field(self, coils, field=B0):
        """SetCoilsField: field += the field of the coils [(z0, R, I), ...]"""
        c3 = np.ascontiguousarray(np.asarray(coils, dtype=np.float64).reshape(-1, 3))
        self._ck(self.L.xpic_set_coils_field(self.h, field, int(c3.shape[0]), _dp(c3)))

    def set_mirror_field(self, D, R, I, field=B0):
        """SetApproximateMirrorField: field += the paraxial field of two coils of radius R and current I at z = -D / 2 and
        z = +D / 2, as the reference writes it (both transverse terms into the X component)"""
        self._ck(self.L.xpic_set_mirror_field(self.h, field, D, R, I))

    def cell_traversal(self, end, start, max_pts=8):
        end, start = np.ascontiguousarray(end, dtype=np.float64), np.ascontiguousarray(start, dtype=np.float64)
        n = end.shape[0]
        pts = np.zeros((n, max_pts, 3))
        counts = np.zeros(n, dtype=np.int32)
        self._ck(self.L.xpic_cell_traversal(self.h, n, _dp(end), _dp(start), max_pts, _dp(pts), _i32p(counts)))
        return pts, counts

    def implicit_esirkepov_interpolate(self, rn, r0):
        rn, r0 = np.ascontiguousarray(rn, dtype=np.float64), np.ascontiguousarray(r0, dtype=np.float64)
        Ep, Bp = np.zeros_like(rn), np.zeros_like(rn)
        self._ck(self.L.xpic_implicit_esirkepov_interpolate(self.h, rn.shape[0], _dp(rn), _dp(r0), _dp(Ep), _dp(Bp)))
        return Ep, Bp

    def implicit_esirkepov_decompose(self, alpha, v, rn, r0, field):
        alpha, v = np.ascontiguousarray(alpha, dtype=np.float64), np.ascontiguousarray(v, dtype=np.float64)
        rn, r0 = np.ascontiguousarray(rn, dtype=np.float64), np.ascontiguousarray(r0, dtype=np.float64)
        self._ck(self.L.xpic_implicit_esirkepov_decompose(self.h, rn.shape[0], _dp(alpha), _dp(v), _dp(rn), _dp(r0), field))

    # ---- drift-kinetic pusher (include/xpic_hip.h: xpic_drift_kinetic_*); particles are records {x, y, z, p_parallel,
    # p_perp, mu_p} (guiding_centre), gradB_field a field id filled with grad |B| or None
    @staticmethod
    def _dk_params(qm, mp, dt, eps, delta, maxit):
        return DkParams(float(qm), float(mp), float(dt), float(eps), float(delta), int(maxit))

    def drift_kinetic_interpolate(self, rn, r0, gradB_field=None):
        """DriftKineticEsirkepov::interpolate -> (E_p, B_p, gradB_p): E over the segment r0 -> rn, B and grad B at rn"""
        rn, r0 = np.ascontiguousarray(rn, dtype=np.float64), np.ascontiguousarray(r0, dtype=np.float64)
        Ep, Bp, gBp = np.zeros_like(rn), np.zeros_like(rn), np.zeros_like(rn)
        self._ck(self.L.xpic_drift_kinetic_interpolate(self.h, rn.shape[0], _dp(rn), _dp(r0),
                                                       -1 if gradB_field is None else int(gradB_field), _dp(Ep), _dp(Bp), _dp(gBp)))
        return Ep, Bp, gBp

    def drift_kinetic_push(self, p0, qm, mp, dt, gradB_field=None, eps=1e-12, delta=1e-12, maxit=30):
        """DriftKineticPush::process of every particle -> (pn, iterations); iterations == maxit: not converged"""
        p0 = np.ascontiguousarray(p0, dtype=np.float64).reshape(-1, 6)
        pn = np.zeros_like(p0)
        its = np.zeros(p0.shape[0], dtype=np.int32)
        P = self._dk_params(qm, mp, dt, eps, delta, maxit)
        self._ck(self.L.xpic_drift_kinetic_push(self.h, p0.shape[0], C.byref(P), -1 if gradB_field is None else int(gradB_field),
                                                _dp(p0), _dp(pn), _i32p(its)))
        return pn, its

    def drift_kinetic_trace(self, state, steps, qm, mp, dt, gradB_field=None, sample_every=0, eps=1e-12, delta=1e-12, maxit=30):
        """`steps` pushes with the particles kept on the device -> (state, samples [steps // sample_every][n][6] or None,
        iterations_total, iterations_max)"""
        state, samples, _, _, _, tot, mx = self._open_args(state, steps, sample_every, None, None, 0, "never", True)
        n = state.shape[0]
        P = self._dk_params(qm, mp, dt, eps, delta, maxit)
        self._ck(self.L.xpic_drift_kinetic_trace(self.h, n, C.byref(P), -1 if gradB_field is None else int(gradB_field),
                                                 int(steps), int(sample_every), _dp(state), _dp(samples), _i64p(tot), _i32p(mx)))
        return state, samples, tot, mx

    # ---- full-orbit pusher (include/xpic_hip.h: xpic_full_orbit_*); particles are Point records {x, y, z, px, py, pz},
    # scheme a key of FO_SCHEMES (a Chin id or "CN") or its number
    @staticmethod
    def _fo_params(scheme, qm, dt, atol, rtol, maxit):
        return FoParams(float(qm), float(dt), float(atol), float(rtol), int(FO_SCHEMES.get(scheme, scheme)), int(maxit))

    def full_orbit_push(self, p0, scheme, qm, dt, atol=1e-7, rtol=1e-7, maxit=30):
        """one step of every particle -> (pn, iterations): process_<id> of tests/boris_push/boris_push.h (iterations 0), or
        CrankNicolsonPush::process for "CN" (iterations == maxit: not converged)"""
        p0 = np.ascontiguousarray(p0, dtype=np.float64).reshape(-1, 6)
        pn = np.zeros_like(p0)
        its = np.zeros(p0.shape[0], dtype=np.int32)
        P = self._fo_params(scheme, qm, dt, atol, rtol, maxit)
        self._ck(self.L.xpic_full_orbit_push(self.h, p0.shape[0], C.byref(P), _dp(p0), _dp(pn), _i32p(its)))
        return pn, its

    def full_orbit_trace(self, state, steps, scheme, qm, dt, sample_every=0, atol=1e-7, rtol=1e-7, maxit=30):
        """`steps` pushes with the particles kept on the device -> (state, samples [steps // sample_every][n][6] or None,
        iterations_sum, iterations_max); sample k is the state after step (k + 1) * sample_every"""
        state, samples, _, _, _, tot, mx = self._open_args(state, steps, sample_every, None, None, 0, "never", True)
        n = state.shape[0]
        P = self._fo_params(scheme, qm, dt, atol, rtol, maxit)
        self._ck(self.L.xpic_full_orbit_trace(self.h, n, C.byref(P), int(steps), int(sample_every), _dp(state), _dp(samples),
                                              _i64p(tot), _i32p(mx)))
        return state, samples, tot, mx

    # ---- open-trap traces (include/xpic_hip.h: xpic_trace_region): the traces above with RemoveParticles' corner rule at
    # the top of every step.  region: a geometry dict as remove_particles'; exit_step: the array a previous call returned
    # (None: everybody alive), step0: the steps that call and its predecessors made; compact: a key of COMPACT or its number
    # ("never" by default: at 2^20 particles rebuilding the list gained 1.5 - 3.4 %, inside the +- 4 % box-to-box spread --
    # DESIGN.md 5j, "Measured")
    # keep_samples=False: alive only, no sample rows (samples is None).  _open_args builds the arrays of every trace of one
    # batch; region None: no region (XPIC_GEOM_NONE, which only the model traces take; the closed traces pass no region)
    def _open_args(self, state, steps, sample_every, region, exit_step, step0, compact, keep_samples):
        state = np.array(state, dtype=np.float64).reshape(-1, 6)  # a copy: the call works in place
        n = state.shape[0]
        nsamp = max(int(steps), 0) // int(sample_every) if sample_every else 0
        samples = np.zeros((nsamp, n, 6)) if sample_every and keep_samples else None
        alive = np.zeros(nsamp, dtype=np.int64) if sample_every else None
        ex = np.full(n, -1, dtype=np.int64) if exit_step is None else np.array(exit_step, dtype=np.int64).reshape(n)
        # (samples and alive are None exactly where the library is to get a null pointer: _dp and _i64p pass None through)
        kind, gp = (GEOM_NONE, [0.0] * 7) if region is None else _geom7(region)
        reg = TraceRegion(kind, int(COMPACT.get(compact, compact)), (C.c_double * 7)(*gp[:7]), int(step0))
        return state, samples, alive, ex, reg, np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32)

    @staticmethod
    def _trace_tail(steps, sample_every, state, samples, tot, mx, reg, ex, alive, removed):
        """the ten arguments from steps to removed that every trace with a region takes, from _open_args' arrays.  ex None:
        the closed trace, the library gets no exit_step and no removed"""
        return [int(steps), int(sample_every), _dp(state), _dp(samples), _i64p(tot), _i32p(mx), C.byref(reg), _i64p(ex),
                _i64p(alive), None if ex is None else C.byref(removed)]

    def full_orbit_trace_open(self, state, steps, scheme, qm, dt, region, sample_every=0, exit_step=None, step0=0,
                              compact="never", keep_samples=True, atol=1e-7, rtol=1e-7, maxit=30):
        """full_orbit_trace in an open system -> OpenTrace"""
        state, samples, alive, ex, reg, tot, mx = self._open_args(state, steps, sample_every, region, exit_step, step0, compact,
                                                                      keep_samples)
        P = self._fo_params(scheme, qm, dt, atol, rtol, maxit)
        removed = C.c_int64()
        self._ck(self.L.xpic_full_orbit_trace_open(
            self.h, state.shape[0], C.byref(P),
            *self._trace_tail(steps, sample_every, state, samples, tot, mx, reg, ex, alive, removed)))
        return OpenTrace(state, samples, ex, alive, removed.value, tot, mx)

    def drift_kinetic_trace_open(self, state, steps, qm, mp, dt, region, gradB_field=None, sample_every=0, exit_step=None,
                                 step0=0, compact="never", keep_samples=True, eps=1e-12, delta=1e-12, maxit=30):
        """drift_kinetic_trace in an open system -> OpenTrace"""
        state, samples, alive, ex, reg, tot, mx = self._open_args(state, steps, sample_every, region, exit_step, step0, compact,
                                                                      keep_samples)
        P = self._dk_params(qm, mp, dt, eps, delta, maxit)
        removed = C.c_int64()
        self._ck(self.L.xpic_drift_kinetic_trace_open(
            self.h, state.shape[0], C.byref(P), -1 if gradB_field is None else int(gradB_field),
            *self._trace_tail(steps, sample_every, state, samples, tot, mx, reg, ex, alive, removed)))
        return OpenTrace(state, samples, ex, alive, removed.value, tot, mx)

    def _compare_trace(self, fn, mismatch, p, centres, width, middle, steps, scheme, qm, mp, dt, sample_every, stats, atol,
                       rtol, maxit, eps, delta, dk_maxit):
        """the ctypes call of paired_trace and triplet_trace.  centres: the guiding centres in fn's order (None: an absent
        one); width: the columns of stats and curve; middle: fn's arguments between dk and steps; mismatch: the message
        for batches of different lengths -> the copies p and centres, stats, curve, and a (sum, max) pair of counters for
        p and for every centre ((None, None) for an absent one)"""
        members = [np.array(p, dtype=np.float64).reshape(-1, 6)]  # copies: the call works in place
        members += [None if c is None else np.array(c, dtype=np.float64).reshape(-1, 6) for c in centres]
        n = members[0].shape[0]
        if any(m is not None and m.shape[0] != n for m in members):
            raise XpicError(mismatch)
        stats = np.zeros((n, width)) if stats is None else np.array(stats, dtype=np.float64).reshape(n, width)
        nsamp = max(int(steps), 0) // int(sample_every) if sample_every else 0
        curve = np.zeros((nsamp, width)) if sample_every else None
        counters = [(None, None) if m is None else (np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32))
                    for m in members]
        F = self._fo_params(scheme, qm, dt, atol, rtol, maxit)
        D = self._dk_params(qm, mp, dt, eps, delta, dk_maxit)
        self._ck(fn(self.h, n, C.byref(F), C.byref(D), *middle, int(steps), int(sample_every), *[_dp(m) for m in members],
                    _dp(stats), _dp(curve), *[a for tot, mx in counters for a in (_i64p(tot), _i32p(mx))]))
        return members[0], members[1:], stats, curve, counters

    # ---- paired trace (include/xpic_hip.h: xpic_paired_trace): full_orbit_trace of p and drift_kinetic_trace of state
    # (guiding_centre(p, ..., orbit_centre=True) lays the two side by side) in lock-step, with the reference's comparison
    # of the pair (ComparisonStats, tests/drift_kinetic_push/drift_kinetic_push.h:253-329) kept on the device
    def paired_trace(self, p, state, steps, scheme, qm, mp, dt, gradB_field=None, sample_every=0, stats=None, atol=1e-7,
                     rtol=1e-7, maxit=30, eps=1e-12, delta=1e-12, dk_maxit=30):
        """-> PairedTrace.  stats: the running maxima a previous call returned (None: zeros), so that calls compose;
        sample_every: the curve's stride (0: no curve); maxit is the full orbit's (CN), dk_maxit the guiding centre's"""
        p, (state,), stats, curve, (fo, dk) = self._compare_trace(
            self.L.xpic_paired_trace, "paired_trace: p and state hold different numbers of particles", p, [state], 4,
            [-1 if gradB_field is None else int(gradB_field)], steps, scheme, qm, mp, dt, sample_every, stats, atol, rtol,
            maxit, eps, delta, dk_maxit)
        return PairedTrace(p, state, stats, curve, *fo, *dk)

    # ---- analytic field models (include/xpic_hip.h: xpic_field_model): the tracers with a closed-form field evaluated
    # on the device in the grid's place.  model: what field_model(...) returns.  region: a geometry dict as in the open
    # traces, or None for no region (the closed trace: exit_step stays -1, alive is the batch size, removed 0)
    def model_fields(self, model, r):
        """-> (E, B, gradB) of the model at the positions r [n][3]"""
        r = np.ascontiguousarray(r, dtype=np.float64).reshape(-1, 3)
        E, B, gB = np.zeros_like(r), np.zeros_like(r), np.zeros_like(r)
        self._ck(self.L.xpic_model_fields(self.h, model, r.shape[0], _dp(r), _dp(E), _dp(B), _dp(gB)))
        return E, B, gB

    def set_model_field(self, model, E_field=E, B_field=B, gradB_field=None):
        """fills the grid vectors from the model, every component of node (i, j, k) at (i dx, j dy, k dz); None: skipped"""
        ids = [-1 if f is None else int(f) for f in (E_field, B_field, gradB_field)]
        self._ck(self.L.xpic_set_model_field(self.h, model, *ids))

    _ABSENT = object()  # _model_trace: the library function has no such argument

    def _model_trace(self, fn, P, state, steps, model, region, sample_every, exit_step, step0, keep_samples,
                     envelope=_ABSENT, sums=_ABSENT, collisions=_ABSENT):
        """the ctypes call of the model traces -> the fields of TimedTrace (OpenTrace's and sums).  envelope follows
        model and sums ends the argument list where fn has them; sums as model_full_orbit_trace_timed takes it.
        collisions (what trace_collisions(...) returns, or None) and coll_4 end the list of the collisional traces:
        then the last field is coll [4]"""
        state, samples, alive, ex, reg, tot, mx = self._open_args(state, steps, sample_every, region, exit_step, step0,
                                                                      "never", keep_samples)
        n = state.shape[0]
        absent = self._ABSENT
        if sums is not absent and sums is not None:
            sums = np.zeros((n, 4)) if sums is True else np.array(sums, dtype=np.float64).reshape(n, 4)
        removed = C.c_int64()
        bare = region is None and exit_step is None  # the closed trace
        args = [self.h, n, C.byref(P), model]
        if envelope is not absent:
            args.append(envelope)
        args += self._trace_tail(steps, sample_every, state, samples, tot, mx, reg, None if bare else ex, alive, removed)
        if sums is not absent:
            args.append(_dp(sums))
        if collisions is not absent:
            coll = np.zeros(4)
            args += [collisions, _dp(coll)]
        self._ck(fn(*args))
        if collisions is not absent:
            return state, samples, ex, alive, removed.value, tot, mx, coll
        return state, samples, ex, alive, removed.value, tot, mx, None if sums is absent else sums

    def model_full_orbit_trace(self, state, steps, scheme, qm, dt, model, region=None, sample_every=0, exit_step=None,
                               step0=0, keep_samples=True, atol=1e-7, rtol=1e-7, maxit=30):
        """full_orbit_trace_open on an analytic model -> OpenTrace; steps = 1 is the one-step push"""
        return OpenTrace(*self._model_trace(
            self.L.xpic_model_full_orbit_trace, self._fo_params(scheme, qm, dt, atol, rtol, maxit), state, steps, model, region,
            sample_every, exit_step, step0, keep_samples)[:7])

    def model_drift_kinetic_trace(self, state, steps, qm, mp, dt, model, region=None, sample_every=0, exit_step=None,
                                  step0=0, keep_samples=True, eps=1e-12, delta=1e-12, maxit=30):
        """drift_kinetic_trace_open on an analytic model -> OpenTrace; steps = 1 is the one-step push"""
        return OpenTrace(*self._model_trace(
            self.L.xpic_model_drift_kinetic_trace, self._dk_params(qm, mp, dt, eps, delta, maxit), state, steps, model, region,
            sample_every, exit_step, step0, keep_samples)[:7])

    # ---- time-dependent analytic fields (include/xpic_hip.h: xpic_field_envelope): the two model traces with a time
    # envelope on the model's E.  envelope: what field_envelope(...) returns, or None (constant: the model trace itself);
    # step0 also fixes the clock, t = (step0 + k) dt
    def model_full_orbit_trace_timed(self, state, steps, scheme, qm, dt, model, envelope, region=None, sample_every=0,
                                     exit_step=None, step0=0, keep_samples=True, atol=1e-7, rtol=1e-7, maxit=30, sums=None):
        """model_full_orbit_trace with an envelope -> TimedTrace.  sums: True for sums that start at 0, or the [n][4] array a
        previous call returned, so that calls compose; None: no sums"""
        return TimedTrace(*self._model_trace(
            self.L.xpic_model_full_orbit_trace_timed, self._fo_params(scheme, qm, dt, atol, rtol, maxit), state, steps, model,
            region, sample_every, exit_step, step0, keep_samples, envelope, sums))

    def model_drift_kinetic_trace_timed(self, state, steps, qm, mp, dt, model, envelope, region=None, sample_every=0,
                                        exit_step=None, step0=0, keep_samples=True, eps=1e-12, delta=1e-12, maxit=30):
        """model_drift_kinetic_trace with an envelope -> OpenTrace"""
        return OpenTrace(*self._model_trace(
            self.L.xpic_model_drift_kinetic_trace_timed, self._dk_params(qm, mp, dt, eps, delta, maxit), state, steps, model,
            region, sample_every, exit_step, step0, keep_samples, envelope)[:7])

    # ---- collisional traces (include/xpic_hip.h: xpic_trace_collisions): the two model traces with Coulomb scattering
    # off Maxwellian backgrounds after the push.  collisions: what trace_collisions(...) returns, or None (the model trace
    # itself); step0 also fixes which steps collide and their streams
    def model_full_orbit_trace_collisional(self, state, steps, scheme, qm, dt, model, collisions, region=None,
                                           sample_every=0, exit_step=None, step0=0, keep_samples=True, atol=1e-7,
                                           rtol=1e-7, maxit=30):
        """model_full_orbit_trace with collisions -> CollisionalTrace"""
        return CollisionalTrace(*self._model_trace(
            self.L.xpic_model_full_orbit_trace_collisional, self._fo_params(scheme, qm, dt, atol, rtol, maxit), state, steps,
            model, region, sample_every, exit_step, step0, keep_samples, collisions=collisions))

    def model_drift_kinetic_trace_collisional(self, state, steps, qm, mp, dt, model, collisions, region=None,
                                              sample_every=0, exit_step=None, step0=0, keep_samples=True, eps=1e-12,
                                              delta=1e-12, maxit=30):
        """model_drift_kinetic_trace with collisions -> CollisionalTrace"""
        return CollisionalTrace(*self._model_trace(
            self.L.xpic_model_drift_kinetic_trace_collisional, self._dk_params(qm, mp, dt, eps, delta, maxit), state, steps,
            model, region, sample_every, exit_step, step0, keep_samples, collisions=collisions))

    # ---- background profiles and the collisional grid traces (include/xpic_hip.h: xpic_background_set,
    # xpic_full_orbit_trace_collisional): the open grid traces with the collisions of the collisional traces, off uniform
    # backgrounds or off the context's profiles.  A profile is n [nz][ny][nx], vth [nz][ny][nx], drift [nz][ny][nx][3]
    def _cells(self):
        return tuple(int(v) for v in self.fshape()[:3])

    def background_set(self, slot, n, vth, drift=None):
        """uploads a profile into `slot`; drift None: at rest"""
        shape = self._cells()
        n = np.ascontiguousarray(np.broadcast_to(np.asarray(n, dtype=np.float64), shape))
        vth = np.ascontiguousarray(np.broadcast_to(np.asarray(vth, dtype=np.float64), shape))
        if drift is not None:
            drift = np.ascontiguousarray(np.broadcast_to(np.asarray(drift, dtype=np.float64), shape + (3,)))
        self._ck(self.L.xpic_background_set(self.h, int(slot), _dp(n), _dp(vth), _dp(drift)))

    def background_get(self, slot):
        """-> (n, vth, drift) of a slot; an empty slot raises"""
        shape = self._cells()
        n, vth, drift = np.zeros(shape), np.zeros(shape), np.zeros(shape + (3,))
        self._ck(self.L.xpic_background_get(self.h, int(slot), _dp(n), _dp(vth), _dp(drift)))
        return n, vth, drift

    def background_clear(self, slot):
        self._ck(self.L.xpic_background_clear(self.h, int(slot)))

    def background_from_sort(self, slot, sort):
        """fills `slot` on the device from the sort's records, cell by cell: n = (n / Np) N, u = <v>,
        vth = sqrt(<|v - u|^2> / 3); the records are not changed"""
        self._ck(self.L.xpic_background_from_sort(self.h, int(slot), int(sort)))

    def _grid_trace_collisional(self, fn, P, middle, state, steps, collisions, profile, region, sample_every, exit_step,
                                step0, compact, keep_samples):
        """the ctypes call of the collisional grid traces -> the fields of CollisionalTrace.  middle: fn's arguments
        between params and steps; profile: a list of slots (-1: the uniform background of `collisions`) or None"""
        state, samples, alive, ex, reg, tot, mx = self._open_args(state, steps, sample_every, region, exit_step, step0, compact,
                                                                      keep_samples)
        removed = C.c_int64()
        bare = region is None and exit_step is None  # the closed trace
        prof = None if profile is None else (C.c_int32 * len(profile))(*[int(s) for s in profile])
        if prof is not None and collisions is not None and len(profile) != collisions.nbg:
            raise XpicError("profile: one entry per background")
        coll = np.zeros(4)
        self._ck(fn(self.h, state.shape[0], C.byref(P), *middle,
                    *self._trace_tail(steps, sample_every, state, samples, tot, mx, reg, None if bare else ex, alive, removed),
                    collisions, prof, _dp(coll)))
        return CollisionalTrace(state, samples, ex, alive, removed.value, tot, mx, coll)

    def full_orbit_trace_collisional(self, state, steps, scheme, qm, dt, collisions, profile=None, region=None,
                                     sample_every=0, exit_step=None, step0=0, compact="never", keep_samples=True, atol=1e-7,
                                     rtol=1e-7, maxit=30):
        """full_orbit_trace_open (region None: full_orbit_trace) with collisions -> CollisionalTrace"""
        return self._grid_trace_collisional(
            self.L.xpic_full_orbit_trace_collisional, self._fo_params(scheme, qm, dt, atol, rtol, maxit), [], state, steps,
            collisions, profile, region, sample_every, exit_step, step0, compact, keep_samples)

    def drift_kinetic_trace_collisional(self, state, steps, qm, mp, dt, collisions, profile=None, region=None,
                                        gradB_field=None, sample_every=0, exit_step=None, step0=0, compact="never",
                                        keep_samples=True, eps=1e-12, delta=1e-12, maxit=30):
        """drift_kinetic_trace_open (region None: drift_kinetic_trace) with collisions -> CollisionalTrace"""
        return self._grid_trace_collisional(
            self.L.xpic_drift_kinetic_trace_collisional, self._dk_params(qm, mp, dt, eps, delta, maxit),
            [-1 if gradB_field is None else int(gradB_field)], state, steps, collisions, profile, region, sample_every,
            exit_step, step0, compact, keep_samples)

    def envelope_factors(self, envelope, dt, step0, nsteps):
        """-> the factors of steps step0 .. step0 + nsteps - 1, evaluated on the device as the traces evaluate them"""
        out = np.zeros(max(int(nsteps), 0))
        self._ck(self.L.xpic_envelope_factors(self.h, envelope, float(dt), int(step0), int(nsteps), _dp(out)))
        return out

    # ---- triplet trace (include/xpic_hip.h: xpic_triplet_trace): model_drift_kinetic_trace of state_model,
    # drift_kinetic_trace of state_grid and model_full_orbit_trace of p in lock-step, with all seven maxima of the
    # reference's ComparisonStats kept on the device; the grid is the context's (set_model_field fills it from the model)
    def triplet_trace(self, p, state_model, state_grid, steps, scheme, qm, mp, dt, model, gradB_field=None, sample_every=0,
                      stats=None, atol=1e-7, rtol=1e-7, maxit=30, eps=1e-12, delta=1e-12, dk_maxit=30):
        """-> TripletTrace.  state_grid=None selects the grid-less pair (state_model beside p; gradB_field is not read).
        stats: the running maxima a previous call returned (None: zeros), so that calls compose; sample_every: the curve's
        stride (0: no curve); maxit is the full orbit's (CN), dk_maxit the guiding centres'"""
        grid = state_grid is not None
        p, (sm, sg), stats, curve, (fo, dkm, dkg) = self._compare_trace(
            self.L.xpic_triplet_trace, "triplet_trace: p, state_model and state_grid hold different numbers of particles", p,
            [state_model, state_grid], 7,
            [model, int(grid), -1 if gradB_field is None or not grid else int(gradB_field)],
            steps, scheme, qm, mp, dt, sample_every, stats, atol, rtol, maxit, eps, delta, dk_maxit)
        return TripletTrace(p, sm, sg, stats, curve, *fo, *dkm, *dkg)

    def charge_collect(self):
        self._ck(self.L.xpic_charge_collect(self.h))

    def charge_columns(self):
        out = np.zeros(2 * self.nsorts + 2)
        self._ck(self.L.xpic_charge_columns(self.h, _dp(out)))
        return out

    def synchronize(self):
        self._ck(self.L.xpic_synchronize(self.h))

    # ---- measurement
    def profile_enable(self, on=True):
        self._ck(self.L.xpic_profile_enable(self.h, int(on)))

    def profile_reset(self):
        self._ck(self.L.xpic_profile_reset(self.h))

    def profile_get(self, name):
        n, ms = C.c_int64(), C.c_double()
        self._ck(self.L.xpic_profile_get(self.h, name.encode(), C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def probe_copy_bandwidth(self, nbytes=1 << 30, reps=10):
        o = C.c_double()
        self._ck(self.L.xpic_probe_copy_bandwidth(self.h, nbytes, reps, C.byref(o)))
        return o.value


def rccl_unique_id():
    L = load_library()
    buf = (C.c_char * 128)()
    if L.xpic_comm_rccl_unique_id(buf) != 0:
        raise XpicError(L.xpic_last_error().decode())
    return bytes(buf)


def lstencil_decode(c1, k):
    L = load_library()
    c2 = C.c_int()
    d = (C.c_int * 3)()
    L.xpic_lstencil_decode(c1, k, C.byref(c2), d)
    return c2.value, (d[0], d[1], d[2])
