"""CPU-side checks of the drop-in boundary (no compute calls: there is no GPU here and no CPU fallback by design): the
library exports every symbol include/xpic_hip.h declares; the package's one table of prototypes, its struct mirrors and
its constants are the header's (tests/abi_header.py reads it); load_library() types every symbol from the table; and every
public method of Context passes its typed prototype, down to the library's own refusal of a null context."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import abi_header as H

ROOT = H.ROOT


def built_library():
    import xpic_amd

    if not os.path.exists(xpic_amd.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return C.CDLL(xpic_amd.LIB_PATH)


# ---- prototypes.  The trace families' argument lists are written out here as well, so that an edit of header and table
# in tandem does not pass unseen; the other entry points are held to the header by the table alone
TRACE_TAIL = ["int64_t", "int64_t", "double*", "double*", "int64_t*", "int*", "const xpic_trace_region*", "int64_t*",
              "int64_t*", "int64_t*"]
COLL_TAIL = ["const xpic_trace_collisions*", "double*"]
GRID_TAIL = ["const xpic_trace_collisions*", "const int32_t*", "double*"]
FO, DK = ["xpic_ctx*", "int64_t", "const xpic_fo_params*"], ["xpic_ctx*", "int64_t", "const xpic_dk_params*"]
MODEL, ENVELOPE = ["const xpic_field_model*"], ["const xpic_field_envelope*"]
LITERAL = {
    "xpic_full_orbit_trace_open": [
        "xpic_ctx*", "int64_t", "const xpic_fo_params*", "int64_t", "int64_t", "double*", "double*", "int64_t*", "int*",
        "const xpic_trace_region*", "int64_t*", "int64_t*", "int64_t*"],
    "xpic_drift_kinetic_trace_open": [
        "xpic_ctx*", "int64_t", "const xpic_dk_params*", "int", "int64_t", "int64_t", "double*", "double*", "int64_t*",
        "int*", "const xpic_trace_region*", "int64_t*", "int64_t*", "int64_t*"],
    "xpic_set_mirror_field": ["xpic_ctx*", "int", "double", "double", "double"],
    "xpic_paired_trace": [
        "xpic_ctx*", "int64_t", "const xpic_fo_params*", "const xpic_dk_params*", "int", "int64_t", "int64_t", "double*",
        "double*", "double*", "double*", "int64_t*", "int*", "int64_t*", "int*"],
    "xpic_triplet_trace": [
        "xpic_ctx*", "int64_t", "const xpic_fo_params*", "const xpic_dk_params*", "const xpic_field_model*", "int", "int",
        "int64_t", "int64_t", "double*", "double*", "double*", "double*", "double*", "int64_t*", "int*", "int64_t*", "int*",
        "int64_t*", "int*"],
    "xpic_model_fields": ["xpic_ctx*", "const xpic_field_model*", "int64_t", "const double*", "double*", "double*", "double*"],
    "xpic_set_model_field": ["xpic_ctx*", "const xpic_field_model*", "int", "int", "int"],
    "xpic_model_full_orbit_trace": FO + MODEL + TRACE_TAIL,
    "xpic_model_drift_kinetic_trace": DK + MODEL + TRACE_TAIL,
    "xpic_model_full_orbit_trace_timed": FO + MODEL + ENVELOPE + TRACE_TAIL + ["double*"],
    "xpic_model_drift_kinetic_trace_timed": DK + MODEL + ENVELOPE + TRACE_TAIL,
    "xpic_envelope_factors": ["xpic_ctx*", "const xpic_field_envelope*", "double", "int64_t", "int64_t", "double*"],
    "xpic_model_full_orbit_trace_collisional": FO + MODEL + TRACE_TAIL + COLL_TAIL,
    "xpic_model_drift_kinetic_trace_collisional": DK + MODEL + TRACE_TAIL + COLL_TAIL,
    "xpic_collide_weighted": ["xpic_ctx*", "int", "int", "const xpic_collision_params*", "int64_t", "double*"],
    "xpic_background_set": ["xpic_ctx*", "int", "const double*", "const double*", "const double*"],
    "xpic_background_get": ["xpic_ctx*", "int", "double*", "double*", "double*"],
    "xpic_background_clear": ["xpic_ctx*", "int"],
    "xpic_background_from_sort": ["xpic_ctx*", "int", "int"],
    "xpic_full_orbit_trace_collisional": FO + TRACE_TAIL + GRID_TAIL,
    "xpic_drift_kinetic_trace_collisional": DK + ["int"] + TRACE_TAIL + GRID_TAIL,
}
# the entry points that extend another one's argument list: name -> (the one extended, what follows its list)
EXTENDS = {"xpic_model_full_orbit_trace_collisional": ("xpic_model_full_orbit_trace", COLL_TAIL),
           "xpic_model_drift_kinetic_trace_collisional": ("xpic_model_drift_kinetic_trace", COLL_TAIL),
           "xpic_full_orbit_trace_collisional": ("xpic_full_orbit_trace_open", GRID_TAIL),
           "xpic_drift_kinetic_trace_collisional": ("xpic_drift_kinetic_trace_open", GRID_TAIL)}


def check_prototypes(names):
    """the header declares each of `names` with the list written out above, and with the list of the one it extends"""
    declared = H.prototypes()
    for name in names:
        assert declared[name] == ("int", LITERAL[name]), name
        if name in EXTENDS:
            base, tail = EXTENDS[name]
            assert declared[name][1] == declared[base][1] + tail, name


def check_listed_and_exported(names, methods=()):
    import xpic_amd

    lib = built_library()
    for name in names:
        assert name in xpic_amd.SYMBOLS, name
        assert hasattr(lib, name), name
    for f in methods:
        assert callable(getattr(xpic_amd.Context, f)), f


def test_header_declares_the_documented_surface():
    import xpic_amd

    assert sorted(xpic_amd.SYMBOLS) == H.symbols() == sorted(H.prototypes())
    assert xpic_amd.SYMBOLS == list(xpic_amd.PROTOTYPES)


def test_prototypes_match_the_header():
    import xpic_amd

    declared = H.prototypes()
    for name, (ret, args) in declared.items():
        assert xpic_amd.PROTOTYPES[name] == (ret, args), name
        assert ret == {"xpic_last_error": "const char*", "xpic_lstencil_decode": "void"}.get(name, "int"), name
        assert all(a in xpic_amd.CTYPES for a in args), name
    check_prototypes(LITERAL)
    for name in ("xpic_model_full_orbit_trace", "xpic_model_drift_kinetic_trace"):  # the envelope goes in after the model
        timed = declared[name + "_timed"][1]
        assert timed[:4] + timed[5:15] == declared[name][1] and timed[4] == "const xpic_field_envelope*", name


def test_library_exports_every_declared_symbol():
    lib = built_library()
    for name in H.symbols():
        assert hasattr(lib, name), name


def test_the_literal_entry_points_are_listed_and_exported():
    check_listed_and_exported(LITERAL)


def test_load_library_types_every_symbol():
    import xpic_amd as X

    built_library()
    L = X.load_library()
    for name, (ret, args) in X.PROTOTYPES.items():
        f = getattr(L, name)
        assert f.restype is X.CTYPES[ret] and list(f.argtypes) == [X.CTYPES[a] for a in args], name
    w = L.xpic_collide_weighted
    assert w.restype is C.c_int
    assert list(w.argtypes) == [C.c_void_p, C.c_int, C.c_int, C.POINTER(X.CollisionParams), C.c_int64, C.POINTER(C.c_double)]
    assert L.xpic_last_error.restype is C.c_char_p and L.xpic_lstencil_decode.restype is None
    assert X.lstencil_decode(0, 13) == (0, (0, 0, 0))  # (a pure function: the centre of the same-component block)


def test_the_package_has_the_methods_and_result_types():
    import xpic_amd as X

    for f in ("model_fields", "set_model_field", "model_full_orbit_trace", "model_drift_kinetic_trace",
              "model_full_orbit_trace_timed", "model_drift_kinetic_trace_timed", "envelope_factors",
              "model_full_orbit_trace_collisional", "model_drift_kinetic_trace_collisional", "background_set",
              "background_get", "background_clear", "background_from_sort", "full_orbit_trace_collisional",
              "drift_kinetic_trace_collisional"):
        assert callable(getattr(X.Context, f))
    assert callable(X.field_model) and callable(X.field_envelope) and callable(X.trace_collisions)
    assert X.TimedTrace._fields == X.OpenTrace._fields + ("sums",)
    assert X.PairedTrace._fields == ("p", "state", "stats", "curve", "fo_iterations_sum", "fo_iterations_max",
                                     "dk_iterations_total", "dk_iterations_max")
    assert X.TripletTrace._fields == (
        "p", "state_model", "state_grid", "stats", "curve", "fo_iterations_sum", "fo_iterations_max", "dkm_iterations_total",
        "dkm_iterations_max", "dkg_iterations_total", "dkg_iterations_max")


# ---- struct mirrors: mirror -> (the header's members, the mirror's offsets, its size), all written out
LAYOUTS = {
    "xpic_trace_region": (["int32_t geometry", "int32_t compact", "double geom[7]", "int64_t step0"], [0, 4, 8, 64], 72),
    "xpic_field_model": (
        ["int32_t kind", "int32_t reserved", "double E0[3]", "double B0[3]", "double r0[3]", "double g[3]", "double B_min",
         "double B_max", "double W", "double D", "double L", "double E_phi", "double phi"],
        [0, 4, 8, 32, 56, 80, 104, 112, 120, 128, 136, 144, 152], 160),
    "xpic_field_envelope": (["int32_t kind", "int32_t reserved", "double a", "double b", "double omega", "double phase"],
                            [0, 4, 8, 16, 24, 32], 40),
    "xpic_trace_background": (["double q", "double m", "double n", "double vth", "double drift[3]"], [0, 8, 16, 24, 32], 56),
    "xpic_trace_collisions": (
        ["int32_t nbg", "int32_t every", "uint64_t seed", "int64_t particle0", "double strength", "double mass",
         "xpic_trace_background bg[XPIC_TRACE_BG_MAX]"], [0, 4, 8, 16, 24, 32, 40], 40 + 4 * 56),
    "xpic_collision_params": (["double strength", "double dt", "uint64_t seed"], [0, 8, 16], 24),
}


def check_layouts(names):
    """the header's members, the mirror's names, offsets and size are what is written out above"""
    import xpic_amd as X

    for name in names:
        fields, offsets, size = LAYOUTS[name]
        mirror = X.MIRRORS[name]
        assert H.struct_fields(name) == fields, name
        assert [f[0] for f in mirror._fields_] == H.member_names(name), name
        assert [getattr(mirror, n).offset for n in H.member_names(name)] == offsets, name
        assert C.sizeof(mirror) == size, name
    if "xpic_trace_collisions" in names:
        assert X.TraceCollisions.bg.size == 4 * 56


def test_struct_mirrors():
    import xpic_amd as X

    assert sorted(X.MIRRORS) == sorted(H.structs())
    for name, mirror in X.MIRRORS.items():  # every struct of the header: the members' names in its order
        assert [f[0] for f in mirror._fields_] == H.member_names(name), name
    check_layouts(LAYOUTS)


# ---- constants and enums
def test_constants_and_enums():
    import xpic_amd as X

    for name, value in (("XPIC_FO_LAUNCH_STEPS", X.FO_LAUNCH_STEPS), ("XPIC_DK_LAUNCH_STEPS", X.DK_LAUNCH_STEPS),
                        ("XPIC_PAIR_LAUNCH_STEPS", X.PAIR_LAUNCH_STEPS), ("XPIC_PAIR_DK_MAXIT", X.PAIR_DK_MAXIT),
                        ("XPIC_MODEL_LAUNCH_STEPS", X.MODEL_LAUNCH_STEPS), ("XPIC_MODEL_DK_MAXIT", X.MODEL_DK_MAXIT),
                        ("XPIC_TRIPLET_LAUNCH_STEPS", X.TRIPLET_LAUNCH_STEPS), ("XPIC_TRIPLET_DK_MAXIT", X.TRIPLET_DK_MAXIT),
                        ("XPIC_TRIPLET_NSTATS", len(X.TRIPLET_STATS)), ("XPIC_TRACE_BG_MAX", X.TRACE_BG_MAX),
                        ("XPIC_GEOM_NONE", X.GEOM_NONE), ("XPIC_FO_MAXIT", X.FO_MAXIT), ("XPIC_LSTENCIL", X.LSTENCIL),
                        ("XPIC_PEER_BLOB_BYTES", X.PEER_BLOB_BYTES), ("XPIC_COLLIDE_LDS_CELL", X.COLLIDE_LDS_CELL),
                        ("XPIC_VERSION_EXPERIMENT_BIT", X.VERSION_EXPERIMENT_BIT),
                        ("XPIC_DEBUG_GATHER_WINDOW", X.DEBUG_GATHER_WINDOW), ("XPIC_DEBUG_PENCIL_LIMIT", X.DEBUG_PENCIL_LIMIT),
                        ("XPIC_DEBUG_SURROGATE_SCALE", X.DEBUG_SURROGATE_SCALE)):
        assert H.macro(name) == value, name
    assert X.TRACE_BG_MAX == 4 and X.GEOM_NONE == -1 and X.PAIR_LAUNCH_STEPS == 64
    assert X.TRIPLET_LAUNCH_STEPS == 64 and X.TRIPLET_DK_MAXIT == 1024
    assert X.PAIR_STATS == ("z", "p_parallel", "mu", "energy")
    assert X.TRIPLET_STATS == ("B", "gradB", "pos", "z", "p_parallel", "mu", "energy") and X.TRIPLET_STATS[3:] == X.PAIR_STATS
    assert H.enum("xpic_trace_compact") == {"XPIC_COMPACT_AUTO": 0, "XPIC_COMPACT_NEVER": 1, "XPIC_COMPACT_ALWAYS": 2}
    assert X.COMPACT == {"auto": 0, "never": 1, "always": 2}
    assert H.enum("xpic_model_kind") == {"XPIC_MODEL_UNIFORM": 0, "XPIC_MODEL_LINEAR": 1, "XPIC_MODEL_QUADRATIC_MIRROR": 2,
                                         "XPIC_MODEL_GAUSSIAN_MIRROR": 3, "XPIC_MODEL_NKINDS": 4}
    assert X.MODEL_KINDS == {"uniform": 0, "linear": 1, "quadratic_mirror": 2, "gaussian_mirror": 3}
    assert H.enum("xpic_envelope_kind") == {"XPIC_ENV_CONSTANT": 0, "XPIC_ENV_RAMP": 1, "XPIC_ENV_HARMONIC": 2,
                                            "XPIC_ENV_NKINDS": 3}
    assert X.ENVELOPE_KINDS == {"constant": 0, "ramp": 1, "harmonic": 2}
    # the enums the older entry points take: every package name has its enumerator, with the same number
    for enum, prefix, table in (("xpic_moment_kind", "XPIC_MOMENT_", X.MOMENTS), ("xpic_projector", "XPIC_PROJ_", X.PROJECTORS),
                                ("xpic_scheme", "XPIC_", X.SCHEMES), ("xpic_fo_scheme", "XPIC_FO_", X.FO_SCHEMES)):
        values = H.enum(enum)
        assert {prefix + k.upper(): v for k, v in table.items()}.items() <= values.items(), enum
    assert [H.enum("xpic_field")[k] for k in ("XPIC_E", "XPIC_B", "XPIC_B0", "XPIC_J", "XPIC_EP", "XPIC_EC", "XPIC_CURRI",
                                               "XPIC_CURRJE", "XPIC_W0", "XPIC_W1", "XPIC_W2")] == list(range(11))


# ---- the builders
def test_field_model_builder():
    import xpic_amd

    mm = xpic_amd.field_model("gaussian_mirror", B_min=1.0, B_max=4.0, L=5.0, W=1.0)
    assert (mm.kind, mm.B_min, mm.B_max, mm.L, mm.W, mm.D) == (3, 1.0, 4.0, 5.0, 1.0, 0.0)
    mm = xpic_amd.field_model("linear", B0=(0, 0, 2), g=(1, 0, 0))
    assert list(mm.B0) == [0.0, 0.0, 2.0] and list(mm.g) == [1.0, 0.0, 0.0] and list(mm.E0) == [0.0] * 3


def test_field_envelope_builder():
    import xpic_amd

    e = xpic_amd.field_envelope("ramp", a=0.0, b=1.0)
    assert (e.kind, e.a, e.b, e.omega, e.phase) == (1, 0.0, 1.0, 0.0, 0.0)
    e = xpic_amd.field_envelope("harmonic", omega=2.5, phase=-0.5)
    assert (e.kind, e.a, e.b, e.omega, e.phase) == (2, 0.0, 0.0, 2.5, -0.5)
    assert xpic_amd.field_envelope("constant").kind == 0 and xpic_amd.field_envelope(2).kind == 2
    with pytest.raises(xpic_amd.XpicError):
        xpic_amd.field_envelope("ramp", slope=1.0)


def test_trace_collisions_builder():
    import xpic_amd

    c = xpic_amd.trace_collisions(
        [dict(q=-1.0, m=1.0, n=2.0, vth=0.1), dict(q=1.0, m=1836.0, n=2.0, vth=0.002, drift=(0.0, 0.01, 0.02))],
        strength=1e-3, mass=4.0, every=3, seed=(1 << 63) + 5, particle0=1 << 40)
    assert (c.nbg, c.every, c.seed, c.particle0, c.strength, c.mass) == (2, 3, (1 << 63) + 5, 1 << 40, 1e-3, 4.0)
    assert (c.bg[0].q, c.bg[0].m, c.bg[0].n, c.bg[0].vth, list(c.bg[0].drift)) == (-1.0, 1.0, 2.0, 0.1, [0.0] * 3)
    assert (c.bg[1].q, c.bg[1].m, c.bg[1].vth, list(c.bg[1].drift)) == (1.0, 1836.0, 0.002, [0.0, 0.01, 0.02])
    assert (c.bg[2].m, c.bg[3].n) == (0.0, 0.0)
    d = xpic_amd.trace_collisions([], strength=0.0, mass=1.0)
    assert (d.nbg, d.every, d.seed, d.particle0) == (0, 1, 0, 0)
    with pytest.raises(xpic_amd.XpicError):
        xpic_amd.trace_collisions([dict(q=1.0, m=1.0, n=1.0, vth=0.0)] * 5, strength=1.0, mass=1.0)
    with pytest.raises(xpic_amd.XpicError):
        xpic_amd.trace_collisions([dict(q=1.0, m=1.0, n=1.0, vth=0.0, nonsense=1)], strength=1.0, mass=1.0)


def test_collide_weighted_returns_the_six_keys():
    """Context.collide_weighted on a stand-in library"""
    import xpic_amd as X

    seen = {}

    def fake(h, a, b, p, step, out):
        params = C.cast(p, C.POINTER(X.CollisionParams)).contents
        seen.update(h=h, a=a, b=b, step=step, strength=params.strength, dt=params.dt, seed=params.seed)
        for k, v in enumerate((7.0, 1.0, 0.25, 2.0, 5.0, 2.0)):
            out[k] = v
        return 0

    ctx = object.__new__(X.Context)
    ctx.L = types.SimpleNamespace(xpic_collide_weighted=fake)
    ctx.h = C.c_void_p(0)
    out = ctx.collide_weighted(0, 1, 2e-3, 11, seed=5, dt=0.7)
    assert out == dict(pairs=7, skipped=1, sigma2_sum=0.25, sigma2_over_1=2, heavy_updates=5, heavy_rejected=2)
    assert list(out) == ["pairs", "skipped", "sigma2_sum", "sigma2_over_1", "heavy_updates", "heavy_rejected"]
    assert all(isinstance(out[k], int) for k in out if k != "sigma2_sum") and isinstance(out["sigma2_sum"], float)
    assert (seen["a"], seen["b"], seen["step"], seen["strength"], seen["dt"], seen["seed"]) == (0, 1, 11, 2e-3, 0.7, 5)
    assert ctx.collide_weighted(1, 0, 1e-3, 0)["pairs"] == 7 and seen["dt"] == 0.0  # (dt None: the context's)
    ctx.h = None  # (nothing to destroy)


def test_the_header_says_what_is_there():
    txt = " ".join(open(os.path.join(ROOT, "include", "xpic_hip.h")).read().split())
    assert "the grid traces and the paired and triplet traces have * no collisional form" not in txt
    for letter in "abcdef":
        assert "(%s)" % letter in txt.split("collisional grid traces:")[1]


# ---- the null-handle sweep: every public method of Context on a context that was never created.  Each call must pass the
# typed prototype (no ctypes.ArgumentError, no TypeError) and come back as the library's own refusal.  The library refuses
# at its null check, before it reads another argument: the sweep shows that ctypes takes what every wrapper passes, in
# both forms of its optional arguments, and nothing about the values; that an accepted value arrives as the C type the
# header names is what argtypes == table == header, above, stand for
NO_CONTEXT = {"xpic_last_error", "xpic_version", "xpic_create", "xpic_destroy", "xpic_comm_rccl_unique_id",
              "xpic_lstencil_decode"}  # take no context, or create or destroy one: the sweep need not reach them
NO_CALL = {"fshape", "close"}  # methods that make no library call on a null handle


class Recorder:
    """the library, remembering which symbols were asked of it"""

    def __init__(self, lib):
        self.lib, self.seen = lib, set()

    def __getattr__(self, name):
        self.seen.add(name)
        return getattr(self.lib, name)


def sweep_cases(X):
    """(method, args, kwargs) with small valid arguments, both forms where an optional argument changes the argument list"""
    p = np.array([[1.0, 1.0, 1.0, 0.1, 0.0, 0.0], [2.0, 1.5, 1.0, 0.0, 0.1, 0.0], [1.5, 2.0, 2.5, 0.0, 0.0, 0.1]])
    r0, rn, field = p[:, :3].copy(), p[:, :3] + 0.3, np.zeros((4, 4, 4, 3))
    box = {"name": "box", "min": (0.0, 0.0, 0.0), "max": (4.0, 4.0, 4.0)}
    cyl = {"name": "cylinder", "center": (2.0, 2.0, 2.0), "radius": 1.5, "height": 3.0}
    model, env = X.field_model("uniform", B0=(0.0, 0.0, 1.0)), X.field_envelope("ramp", a=0.0, b=1.0)
    coll = X.trace_collisions([dict(q=-1.0, m=1.0, n=1.0, vth=0.1)], strength=1e-3, mass=1.0)
    fo, dk, pair, ex = ("EB2B", -1.0, 0.5), (-1.0, 1.0, 0.5), ("EB2B", -1.0, 1.0, 0.5), np.array([-1, 2, -1])
    maxwell = {"name": "MaxwellianMomentum", "T": (1.0, 1.0, 1.0), "tov": True}
    # the optional arguments of the traces: samples, a region with an exit_step (where the region is optional), a grad B
    forms = [{}, dict(sample_every=1), dict(sample_every=2, keep_samples=False, exit_step=ex, step0=4)]
    region = [{}, dict(region=box, sample_every=1), dict(exit_step=ex), dict(region=cyl, exit_step=ex, step0=4)]
    gradB = [{}, dict(gradB_field=X.W0)]

    def c(name, *args, **kwargs):
        return name, args, kwargs
    cases = [
        c("comm_init_rccl", bytes(128)), c("comm_init_callbacks", lambda *a: (b"", b""), lambda a: None),
        c("comm_peer_export"), c("comm_peer_import", bytes(X.PEER_BLOB_BYTES), bytes(X.PEER_BLOB_BYTES)), c("comm_size"),
        c("add_sort", 8, 1.0, -1.0, 1.0, 100), c("add_particles", 0, p), c("count", 0), c("particles", 0), c("clear", 0),
        c("fill_synthetic", 0, 4, 0.1), c("fill_synthetic", 1, 4, 0.1, seed=(1 << 64) - 1, regular=True),
        c("load_synthetic", 0, 4, 0.1, profile="blob", drift=(0.1, 0.0, 0.0), param=(0.5, 2.0)), c("occupancy", 0),
        c("set_field", X.E, field), c("get_field", X.B), c("sort_current", 0, X.J), c("vec_set", X.W0, 1.5),
        c("vec_set", X.W0, 2), c("vec_axpy", X.W0, 2.0, X.W1), c("vec_axpby", X.W0, 2.0, 0.5, X.W1), c("vec_dot", X.W0, X.W1),
        c("vec_norm2", X.W0), c("rot_apply", 1, 0.5, X.E, X.W0), c("rot_apply", -1, 0.5, X.B, X.W0, add=True),
        c("matM_apply", X.E, X.W0), c("matL_apply", X.E, X.W0, add=True), c("matA_apply", X.E, X.W0), c("matL"),
        c("ecsim_first_push", 0), c("update_cells", 0), c("ecsim_fill_current"), c("ecsim_second_push", 0),
        c("basic_push", 0), c("ecsimcorr_first_push", 0), c("ecsimcorr_second_push", 0), c("ecsimcorr_final_update", 0),
        c("calculate_energy", 0), c("ecsimcorr_scalars", 0), c("solve", X.OP_MATA_GMRES, X.W0, X.W1),
        c("solve", X.OP_MATM_CG, X.W0, X.W1, rtol=1e-9, atol=0, maxit=7), c("set_tolerances", 1e-7, 1e-7, 100),
        c("set_preconditioner", 5), c("set_preconditioner", 2, degree=3), c("precond_apply", X.OP_MATA_GMRES, X.W0, X.W1),
        c("precond_get"), c("comm_stats"), c("comm_stats", reset=True), c("set_fill_kernel", 0), c("set_fused_rebin", 1),
        c("fill_variant"), c("debug_set", X.DEBUG_GATHER_WINDOW, 150), c("set_overlap", 0), c("step"), c("energy"),
        c("momentum"), c("charge_density", 0), c("moment_density", 0), c("moment", 0, "current"),
        c("moment", 0, "density", region=((0, 0, 0), (2, 2, 2))), c("velocity_distribution", 0, "vx_vy", box),
        c("velocity_distribution", 0, "vr_vphi", cyl), c("remove_particles", 0, box), c("remove_particles", 0, cyl),
        c("fields_damping", box, 0.5), c("fields_damping", cyl, 1),
        c("inject_particles", 0, 1, 3, 0, {"name": "PreciseCoordinate", "value": (1.0, 1.0, 1.0)},
          {"name": "PreciseMomentum", "value": (0.1, 0.0, 0.0)}, maxwell),
        c("inject_particles", 0, 1, 3, 1 << 40, dict(box, name="CoordinateInBox"), maxwell, maxwell, seed=7),
        c("collide", 0, 0, 1e-3, 0), c("collide", 0, 1, 1e-3, 1 << 40, seed=5, dt=0.5), c("collide_weighted", 0, 1, 1e-3, 0),
        c("collide_weighted", 0, 1, 1e-3, 1 << 40, seed=5, dt=0.5), c("collide_info"),
        c("set_coils_field", [(1.0, 2.0, 3.0)]), c("set_mirror_field", 2.0, 1.0, 1.0), c("set_mirror_field", 2, 1, 1, field=X.B),
        c("cell_traversal", rn, r0), c("implicit_esirkepov_interpolate", rn, r0),
        c("implicit_esirkepov_decompose", np.ones(3), rn, rn, r0, X.J), c("model_fields", model, r0),
        c("set_model_field", model), c("set_model_field", model, gradB_field=X.W0),
        c("background_set", 0, 1.0, 0.1), c("background_set", 1, 1.0, 0.1, drift=(0.0, 0.0, 0.1)), c("background_get", 0),
        c("background_clear", 0), c("background_from_sort", 0, 0), c("envelope_factors", env, 0.5, 0, 3),
        c("envelope_factors", None, 0.5, 1 << 40, 3), c("charge_collect"), c("charge_columns"), c("synchronize"),
        c("profile_enable"), c("profile_reset"), c("profile_get", "fill_current"), c("probe_copy_bandwidth", 1 << 33, 2),
    ]
    for g in gradB:
        cases += [c("drift_kinetic_interpolate", rn, r0, **g), c("drift_kinetic_push", p, *dk, **g)]
        cases += [c("drift_kinetic_trace", p, 3, *dk, **g, **f) for f in forms[:2]]
        cases += [c("drift_kinetic_trace_open", p, 3, *dk, box, **g, **f) for f in forms]
        cases += [c("paired_trace", p, p, 3, *pair, **g, **f) for f in forms[:2]]
        cases += [c("paired_trace", p, p, 3, *pair, stats=np.zeros((3, 4)), **g)]
        cases += [c("triplet_trace", p, p, sg, 3, *pair, model, **g, **f) for f in forms[:2] for sg in (p, None)]
        cases += [c("drift_kinetic_trace_collisional", p, 3, *dk, coll, profile=prof, compact="auto", **g, **f)
                  for f in region for prof in (None, [-1])]
    cases += [c("full_orbit_push", p, *fo), c("full_orbit_push", p, "CN", -1.0, 0.5, maxit=5)]
    cases += [c("full_orbit_trace", p, 3, *fo, **f) for f in forms[:2]]
    cases += [c("full_orbit_trace_open", p, 3, *fo, box, **f) for f in forms]
    cases += [c("full_orbit_trace_collisional", p, 3, *fo, coll, profile=prof, **f) for f in region for prof in (None, [-1])]
    for f in region:
        cases += [c("model_full_orbit_trace", p, 3, *fo, model, **f), c("model_drift_kinetic_trace", p, 3, *dk, model, **f)]
        cases += [c("model_full_orbit_trace_timed", p, 3, *fo, model, e, sums=s, **f)
                  for e in (env, None) for s in (None, True, np.zeros((3, 4)))]
        cases += [c("model_drift_kinetic_trace_timed", p, 3, *dk, model, e, **f) for e in (env, None)]
        cases += [c(m, p, 3, *a, model, k, **f) for k in (coll, None)
                  for m, a in (("model_full_orbit_trace_collisional", fo), ("model_drift_kinetic_trace_collisional", dk))]
    return cases


def test_null_handle_sweep():
    import xpic_amd as X

    built_library()
    ctx = object.__new__(X.Context)
    ctx.L, ctx.h = Recorder(X.load_library()), C.c_void_p(0)
    ctx.n, ctx.d, ctx.dt, ctx.nzl, ctx.N, ctx.nsorts = (4, 4, 4), (1.0, 1.0, 1.0), 0.5, 4, 64, 2
    swept, messages = set(), set()
    for name, args, kwargs in sweep_cases(X):
        if name == "particles":  # count() comes first and is refused: stand in for it, so that the read-back is reached
            ctx.count = lambda sort: 3
        with pytest.raises(X.XpicError) as e:
            getattr(ctx, name)(*args, **kwargs)
        ctx.__dict__.pop("count", None)
        assert re.fullmatch(r"xpic error [1-9]\d*: .+", str(e.value)), (name, kwargs, str(e.value))  # the library's own words
        messages.add(str(e.value))
        swept.add(name)
    public = {k for k, v in vars(X.Context).items() if callable(v) and not k.startswith("_")}
    assert swept == public - NO_CALL
    reached = ctx.L.seen & set(X.PROTOTYPES)
    assert reached >= set(X.PROTOTYPES) - NO_CONTEXT, sorted(set(X.PROTOTYPES) - NO_CONTEXT - reached)
    print("the sweep reached %d of %d symbols through %d calls: %s" % (
        len(reached), len(X.PROTOTYPES), len(sweep_cases(X)), sorted(messages)))
    assert ctx.nsorts == 2 and ctx.h.value is None  # (a refused add_sort adds nothing; close() has nothing to destroy)
    ctx.close()


def test_library_is_not_an_experiment_build():
    """xpic_version() carries bit 30 when any object was compiled with -DXPIC_EXPERIMENT (FILL_EXP / ESK_EXP ablations
    and in-kernel stamps, some of which compute garbage on purpose): such a library must not pass as the product."""
    lib = built_library()
    v = lib.xpic_version()
    assert v & 0x40000000 == 0, "libxpic_hip.so is an XPIC_EXPERIMENT build: make clean all"
    assert v == H.macro("XPIC_VERSION")
    # the ablation switches refuse to compile without the experiment switch
    src = open(os.path.join(ROOT, "xpic_amd", "csrc", "common.h")).read()
    assert "#error" in src and "XPIC_EXPERIMENT" in src


def test_no_cpu_fallback_without_a_device():
    """Without a HIP device xpic_create must fail loudly (never route to a CPU path)."""
    import torch
    import xpic_amd

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(xpic_amd.XpicError):
        xpic_amd.Context("ecsim", (8, 8, 8), (0.5, 0.5, 0.5), 1.0)


def test_product_does_not_reference_the_oracle():
    """Nothing under xpic_amd/ or include/ may import, link or mention the oracle."""
    for base in ("xpic_amd", "include"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, base)):
            for f in files:
                if f.endswith((".so", ".o", ".pyc")):
                    continue
                txt = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "oracle" not in txt.lower(), os.path.join(dirpath, f)


def test_host_mirror_selftest(tmp_path):
    """Host logic of the C++ mirror (JSON reader, Builder::parse_value units, TableDiagnostic text format against
    literal lines of the reference's golden tables) -- runs without a GPU."""
    import subprocess

    exe = os.path.join(ROOT, "xpic_amd", "host", "xpic_hip.out")
    if not os.path.exists(exe):
        import __graft_entry__

        __graft_entry__.build()
    out = subprocess.run([exe, "--selftest", str(tmp_path)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "selftest ok" in out.stdout, out.stdout + out.stderr


def test_host_mirror_fails_loudly_without_gpu(tmp_path):
    import json
    import subprocess

    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    exe = os.path.join(ROOT, "xpic_amd", "host", "xpic_hip.out")
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "ecsim_ex1", "config.json")))
    cfg["OutputDirectory"] = str(tmp_path)
    (tmp_path / "c.json").write_text(json.dumps(cfg))
    out = subprocess.run([exe, str(tmp_path / "c.json")], capture_output=True, text=True, timeout=60)
    assert out.returncode != 0 and "no ROCm-capable device" in (out.stdout + out.stderr)
