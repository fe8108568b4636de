"""The mirrors of include/xpic_hip.h: its constants, enums and structs, and PROTOTYPES, the one table of its entry points.
load_library() types every symbol from the table; tests/test_abi.py holds table, structs and constants to the header."""
import ctypes as C

E, B, B0, J, EP, EC, CURRI, CURRJE, W0, W1, W2 = range(11)
BASIC, ECSIM, ECSIMCORR, ES = 0, 1, 2, 3
OP_MATA_GMRES, OP_MATM_GMRES, OP_MATM_CG = 0, 1, 2
LSTENCIL = 123
SCHEMES = {"basic": BASIC, "ecsim": ECSIM, "ecsimcorr": ECSIMCORR, "es": ES}


class Geometry(C.Structure):
    _fields_ = [("n", C.c_int32 * 3), ("d", C.c_double * 3), ("dt", C.c_double), ("periodic", C.c_int32 * 3),
                ("rank", C.c_int32), ("nranks", C.c_int32), ("device", C.c_int32), ("self_ring", C.c_int32)]


# enum xpic_moment_kind (the reference's order) and the components of each moment
MOMENTS = {"density": 0, "current": 1, "momentum_flux": 2, "momentum_flux_diag": 3, "momentum_flux_cyl": 4,
           "momentum_flux_diag_cyl": 5}
MOMENT_DOF = {"density": 1, "current": 3, "momentum_flux": 6, "momentum_flux_diag": 3, "momentum_flux_cyl": 6,
              "momentum_flux_diag_cyl": 3}
PROJECTORS = {"vx_vy": 0, "vz_vxy": 1, "vr_vphi": 2}  # enum xpic_projector
GEOMETRIES = {"box": 0, "BoxGeometry": 0, "cylinder": 1, "CylinderGeometry": 1}  # enum xpic_vgeometry

# enum xpic_coordinate_kind, enum xpic_momentum_kind; inject_particles takes the first three and the first two
COORDINATES = {"PreciseCoordinate": 0, "CoordinateInBox": 1, "CoordinateInCylinder": 2, "CoordinateOnAnnulus": 3}
MOMENTA = {"PreciseMomentum": 0, "MaxwellianMomentum": 1, "MaxwellCosinePerturbation": 2, "AngularMomentum": 3}


class MomentumParams(C.Structure):
    _fields_ = [("kind", C.c_int32), ("tov", C.c_int32), ("value", C.c_double * 3), ("T", C.c_double * 3)]


class InjectParams(C.Structure):
    _fields_ = [("coordinate", C.c_int32), ("reserved", C.c_int32), ("geom", C.c_double * 7),
                ("momentum", MomentumParams * 2), ("seed", C.c_uint64)]


class SetParticlesParams(C.Structure):
    _fields_ = [("coordinate", C.c_int32), ("momentum", C.c_int32), ("tov", C.c_int32), ("reserved", C.c_int32),
                ("geom", C.c_double * 7), ("value", C.c_double * 3), ("T", C.c_double * 3), ("amplitude", C.c_double * 3),
                ("wave_number", C.c_double * 3), ("box6", C.c_double * 6), ("center", C.c_double * 3), ("seed", C.c_uint64),
                ("chunk", C.c_int64)]


SET_PARTICLES_CHUNK = 1 << 24  # XPIC_SET_PARTICLES_CHUNK


class CollisionParams(C.Structure):
    _fields_ = [("strength", C.c_double), ("dt", C.c_double), ("seed", C.c_uint64)]


COLLIDE_LDS_CELL = 256  # XPIC_COLLIDE_LDS_CELL (Context.collide_info reads the library's own)
DEBUG_GATHER_WINDOW, DEBUG_PENCIL_LIMIT, DEBUG_SURROGATE_SCALE = 0, 1, 2  # xpic_debug_set
PEER_BLOB_BYTES = 256  # XPIC_PEER_BLOB_BYTES
VERSION_EXPERIMENT_BIT = 0x40000000  # XPIC_VERSION_EXPERIMENT_BIT


class LoadParams(C.Structure):
    _fields_ = [("ppc", C.c_int32), ("profile", C.c_int32), ("vth", C.c_double), ("drift", C.c_double * 3),
                ("profile_param", C.c_double * 4), ("seed", C.c_uint64)]


LOAD_PROFILES = {"poisson": 0, "uniform": 0, "regular": 1, "gradient": 2, "blob": 3}  # XPIC_LOAD_*


class SortParams(C.Structure):
    _fields_ = [("Np", C.c_int32), ("n", C.c_double), ("q", C.c_double), ("m", C.c_double)]


class DkParams(C.Structure):
    _fields_ = [("qm", C.c_double), ("mp", C.c_double), ("dt", C.c_double), ("eps", C.c_double), ("delta", C.c_double),
                ("maxit", C.c_int32)]


DK_LAUNCH_STEPS = 64  # XPIC_DK_LAUNCH_STEPS


class FoParams(C.Structure):
    _fields_ = [("qm", C.c_double), ("dt", C.c_double), ("atol", C.c_double), ("rtol", C.c_double), ("scheme", C.c_int32),
                ("maxit", C.c_int32)]


# enum xpic_fo_scheme -- the 17 Chin ids of tests/boris_push/boris_push.h, then Crank-Nicolson
FO_SCHEMES = {name: i for i, name in enumerate(
    ["M1A", "M1B", "MLF", "B1A", "B1B", "BLF", "C1A", "C1B", "CLF", "M2A", "M2B", "C2A", "B2B", "EB1A", "EB1B", "EBLF",
     "EB2B", "CN"])}
FO_LAUNCH_STEPS = 64  # XPIC_FO_LAUNCH_STEPS
FO_MAXIT = 64         # XPIC_FO_MAXIT


class TraceRegion(C.Structure):
    _fields_ = [("geometry", C.c_int32), ("compact", C.c_int32), ("geom", C.c_double * 7), ("step0", C.c_int64)]


COMPACT = {"auto": 0, "never": 1, "always": 2}  # enum xpic_trace_compact
PAIR_LAUNCH_STEPS = 64  # XPIC_PAIR_LAUNCH_STEPS
PAIR_DK_MAXIT = 1024    # XPIC_PAIR_DK_MAXIT
PAIR_STATS = ("z", "p_parallel", "mu", "energy")  # the columns of stats_4 and curve_4 (xpic_paired_trace)


class FieldModel(C.Structure):
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("E0", C.c_double * 3), ("B0", C.c_double * 3),
                ("r0", C.c_double * 3), ("g", C.c_double * 3), ("B_min", C.c_double), ("B_max", C.c_double), ("W", C.c_double),
                ("D", C.c_double), ("L", C.c_double), ("E_phi", C.c_double), ("phi", C.c_double)]


MODEL_KINDS = {"uniform": 0, "linear": 1, "quadratic_mirror": 2, "gaussian_mirror": 3}  # enum xpic_model_kind
GEOM_NONE = -1             # XPIC_GEOM_NONE
MODEL_LAUNCH_STEPS = 64    # XPIC_MODEL_LAUNCH_STEPS
MODEL_DK_MAXIT = 1024      # XPIC_MODEL_DK_MAXIT
TRIPLET_LAUNCH_STEPS = 64  # XPIC_TRIPLET_LAUNCH_STEPS
TRIPLET_DK_MAXIT = 1024    # XPIC_TRIPLET_DK_MAXIT
# the columns of stats_7 and curve_7 (xpic_triplet_trace), XPIC_TRIPLET_NSTATS of them: ComparisonStats' order
TRIPLET_STATS = ("B", "gradB", "pos", "z", "p_parallel", "mu", "energy")


class FieldEnvelope(C.Structure):
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("a", C.c_double), ("b", C.c_double), ("omega", C.c_double),
                ("phase", C.c_double)]


# enum xpic_envelope_kind; "harmonic" is an extension, the reference has no such callback
ENVELOPE_KINDS = {"constant": 0, "ramp": 1, "harmonic": 2}
TRACE_BG_MAX = 4  # XPIC_TRACE_BG_MAX


class TraceBackground(C.Structure):
    _fields_ = [("q", C.c_double), ("m", C.c_double), ("n", C.c_double), ("vth", C.c_double), ("drift", C.c_double * 3)]


class TraceCollisions(C.Structure):
    _fields_ = [("nbg", C.c_int32), ("every", C.c_int32), ("seed", C.c_uint64), ("particle0", C.c_int64),
                ("strength", C.c_double), ("mass", C.c_double), ("bg", TraceBackground * TRACE_BG_MAX)]


class CommCallbacks(C.Structure):
    _fields_ = [("user", C.c_void_p),
                ("sendrecv", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                         C.c_size_t, C.c_void_p, C.c_size_t)),
                ("allreduce_sum", C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int))]


# every struct the header defines (all typedefs but the opaque xpic_ctx) and its mirror
MIRRORS = {"xpic_geometry": Geometry, "xpic_sort_params": SortParams, "xpic_load_params": LoadParams,
           "xpic_momentum_params": MomentumParams, "xpic_inject_params": InjectParams,
           "xpic_set_particles_params": SetParticlesParams,
           "xpic_collision_params": CollisionParams, "xpic_dk_params": DkParams, "xpic_fo_params": FoParams,
           "xpic_trace_region": TraceRegion, "xpic_field_model": FieldModel, "xpic_field_envelope": FieldEnvelope,
           "xpic_trace_background": TraceBackground, "xpic_trace_collisions": TraceCollisions,
           "xpic_comm_callbacks": CommCallbacks}

c_dp = C.POINTER(C.c_double)
# the header's argument and return types in ctypes.  Where the prototype has a pointer, ctypes takes None (NULL), a
# pointer or array of that type, byref() of the pointee or the pointee itself; void* takes any pointer, array or byref()
# (const or not is one ctypes type)
CTYPES = {"void": None, "int": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "double": C.c_double,
          "const char*": C.c_char_p, "void*": C.c_void_p, "const void*": C.c_void_p, "xpic_ctx*": C.c_void_p,
          "xpic_ctx**": C.POINTER(C.c_void_p)}
for _word, _pointee in dict(MIRRORS, int=C.c_int, int32_t=C.c_int32, int64_t=C.c_int64, double=C.c_double).items():
    CTYPES[_word + "*"] = CTYPES["const " + _word + "*"] = C.POINTER(_pointee)

# entry point -> (return type, argument types), in the header's order and words with the parameter names dropped (an array
# parameter such as `double out6[6]` is `double*`).  _STEPS .. _GRID are the runs of arguments the trace families share:
# steps, sample_every, the state, samples and the two iteration counters; region, exit_step, alive, removed; the collisions
# and coll_4 of the collisional model traces; collisions, profile and coll_4 of the collisional grid traces
_STEPS = ["int64_t", "int64_t", "double*", "double*", "int64_t*", "int*"]
_OPEN = _STEPS + ["const xpic_trace_region*", "int64_t*", "int64_t*", "int64_t*"]
_COLL = ["const xpic_trace_collisions*", "double*"]
_GRID = ["const xpic_trace_collisions*", "const int32_t*", "double*"]
_FO = ["xpic_ctx*", "int64_t", "const xpic_fo_params*"]
_DK = ["xpic_ctx*", "int64_t", "const xpic_dk_params*"]
_MODEL, _ENVELOPE = ["const xpic_field_model*"], ["const xpic_field_envelope*"]
PROTOTYPES = {
    "xpic_last_error": ("const char*", []),
    "xpic_version": ("int", []),
    "xpic_create": ("int", ["const xpic_geometry*", "int", "xpic_ctx**"]),
    "xpic_destroy": ("int", ["xpic_ctx*"]),
    "xpic_synchronize": ("int", ["xpic_ctx*"]),
    "xpic_add_sort": ("int", ["xpic_ctx*", "const xpic_sort_params*", "int64_t", "int*"]),
    "xpic_sort_add_particles": ("int", ["xpic_ctx*", "int", "int64_t", "const double*", "int64_t*"]),
    "xpic_sort_count": ("int", ["xpic_ctx*", "int", "int64_t*"]),
    "xpic_sort_get_particles": ("int", ["xpic_ctx*", "int", "double*", "int32_t*"]),
    "xpic_sort_clear": ("int", ["xpic_ctx*", "int"]),
    "xpic_sort_fill_synthetic": ("int", ["xpic_ctx*", "int", "int", "double", "uint64_t", "int"]),
    "xpic_sort_load_synthetic": ("int", ["xpic_ctx*", "int", "const xpic_load_params*"]),
    "xpic_sort_occupancy": ("int", ["xpic_ctx*", "int", "int64_t*"]),
    "xpic_field_set": ("int", ["xpic_ctx*", "int", "const double*"]),
    "xpic_field_get": ("int", ["xpic_ctx*", "int", "double*"]),
    "xpic_sort_current_get": ("int", ["xpic_ctx*", "int", "int", "double*"]),
    "xpic_vec_set": ("int", ["xpic_ctx*", "int", "double"]),
    "xpic_vec_axpy": ("int", ["xpic_ctx*", "int", "double", "int"]),
    "xpic_vec_axpby": ("int", ["xpic_ctx*", "int", "double", "double", "int"]),
    "xpic_vec_dot": ("int", ["xpic_ctx*", "int", "int", "double*"]),
    "xpic_vec_norm2": ("int", ["xpic_ctx*", "int", "double*"]),
    "xpic_rot_apply": ("int", ["xpic_ctx*", "int", "double", "int", "int", "int"]),
    "xpic_matM_apply": ("int", ["xpic_ctx*", "int", "int", "int"]),
    "xpic_matL_apply": ("int", ["xpic_ctx*", "int", "int", "int"]),
    "xpic_matA_apply": ("int", ["xpic_ctx*", "int", "int"]),
    "xpic_matL_get": ("int", ["xpic_ctx*", "double*"]),
    "xpic_lstencil_decode": ("void", ["int", "int", "int*", "int*"]),
    "xpic_ecsim_first_push": ("int", ["xpic_ctx*", "int"]),
    "xpic_update_cells": ("int", ["xpic_ctx*", "int", "int64_t*"]),
    "xpic_ecsim_fill_current": ("int", ["xpic_ctx*"]),
    "xpic_ecsim_second_push": ("int", ["xpic_ctx*", "int"]),
    "xpic_basic_push": ("int", ["xpic_ctx*", "int"]),
    "xpic_ecsimcorr_first_push": ("int", ["xpic_ctx*", "int"]),
    "xpic_ecsimcorr_second_push": ("int", ["xpic_ctx*", "int"]),
    "xpic_ecsimcorr_final_update": ("int", ["xpic_ctx*", "int"]),
    "xpic_calculate_energy": ("int", ["xpic_ctx*", "int", "double*"]),
    "xpic_ecsimcorr_scalars": ("int", ["xpic_ctx*", "int", "double*"]),
    "xpic_solve": ("int", ["xpic_ctx*", "int", "int", "int", "double", "double", "int", "int*", "int*", "double*"]),
    "xpic_set_tolerances": ("int", ["xpic_ctx*", "double", "double", "int"]),
    "xpic_set_preconditioner": ("int", ["xpic_ctx*", "int", "int"]),
    "xpic_precond_apply": ("int", ["xpic_ctx*", "int", "int", "int"]),
    "xpic_precond_get": ("int", ["xpic_ctx*", "double*", "double*", "double*"]),
    "xpic_set_fill_kernel": ("int", ["xpic_ctx*", "int"]),
    "xpic_set_fused_rebin": ("int", ["xpic_ctx*", "int"]),
    "xpic_get_fill_variant": ("int", ["xpic_ctx*", "int*"]),
    "xpic_debug_set": ("int", ["xpic_ctx*", "int", "int64_t"]),
    "xpic_set_overlap": ("int", ["xpic_ctx*", "int"]),
    "xpic_step": ("int", ["xpic_ctx*", "int*"]),
    "xpic_energy": ("int", ["xpic_ctx*", "double*"]),
    "xpic_momentum": ("int", ["xpic_ctx*", "double*"]),
    "xpic_charge_density": ("int", ["xpic_ctx*", "int", "double*"]),
    "xpic_moment_density": ("int", ["xpic_ctx*", "int", "double*"]),
    "xpic_moment": ("int", ["xpic_ctx*", "int", "int", "const int*", "double*"]),
    "xpic_velocity_distribution": ("int", ["xpic_ctx*", "int", "int", "int", "const double*", "const double*", "int*",
                                           "double*"]),
    "xpic_remove_particles": ("int", ["xpic_ctx*", "int", "int", "const double*", "int64_t*", "double*"]),
    "xpic_fields_damping": ("int", ["xpic_ctx*", "int", "int", "int", "int", "const double*", "double", "double*"]),
    "xpic_inject_particles": ("int", ["xpic_ctx*", "int", "int", "const xpic_inject_params*", "int64_t", "int64_t",
                                      "int64_t*", "double*"]),
    "xpic_collide": ("int", ["xpic_ctx*", "int", "int", "const xpic_collision_params*", "int64_t", "double*"]),
    "xpic_collide_info": ("int", ["xpic_ctx*", "int64_t*"]),
    "xpic_collide_weighted": ("int", ["xpic_ctx*", "int", "int", "const xpic_collision_params*", "int64_t", "double*"]),
    "xpic_set_coils_field": ("int", ["xpic_ctx*", "int", "int", "const double*"]),
    "xpic_set_mirror_field": ("int", ["xpic_ctx*", "int", "double", "double", "double"]),
    "xpic_charge_collect": ("int", ["xpic_ctx*"]),
    "xpic_charge_columns": ("int", ["xpic_ctx*", "double*"]),
    "xpic_cell_traversal": ("int", ["xpic_ctx*", "int64_t", "const double*", "const double*", "int", "double*", "int*"]),
    "xpic_implicit_esirkepov_interpolate": ("int", ["xpic_ctx*", "int64_t", "const double*", "const double*", "double*",
                                                    "double*"]),
    "xpic_implicit_esirkepov_decompose": ("int", ["xpic_ctx*", "int64_t", "const double*", "const double*", "const double*",
                                                  "const double*", "int"]),
    "xpic_drift_kinetic_interpolate": ("int", ["xpic_ctx*", "int64_t", "const double*", "const double*", "int", "double*",
                                               "double*", "double*"]),
    "xpic_drift_kinetic_push": ("int", _DK + ["int", "const double*", "double*", "int*"]),
    "xpic_drift_kinetic_trace": ("int", _DK + ["int"] + _STEPS),
    "xpic_full_orbit_push": ("int", _FO + ["const double*", "double*", "int*"]),
    "xpic_full_orbit_trace": ("int", _FO + _STEPS),
    "xpic_full_orbit_trace_open": ("int", _FO + _OPEN),
    "xpic_drift_kinetic_trace_open": ("int", _DK + ["int"] + _OPEN),
    "xpic_paired_trace": ("int", _FO + ["const xpic_dk_params*", "int", "int64_t", "int64_t", "double*", "double*", "double*",
                                        "double*", "int64_t*", "int*", "int64_t*", "int*"]),
    "xpic_model_fields": ("int", ["xpic_ctx*", "const xpic_field_model*", "int64_t", "const double*", "double*", "double*",
                                  "double*"]),
    "xpic_set_model_field": ("int", ["xpic_ctx*", "const xpic_field_model*", "int", "int", "int"]),
    "xpic_model_full_orbit_trace": ("int", _FO + _MODEL + _OPEN),
    "xpic_model_drift_kinetic_trace": ("int", _DK + _MODEL + _OPEN),
    "xpic_model_full_orbit_trace_timed": ("int", _FO + _MODEL + _ENVELOPE + _OPEN + ["double*"]),
    "xpic_model_drift_kinetic_trace_timed": ("int", _DK + _MODEL + _ENVELOPE + _OPEN),
    "xpic_envelope_factors": ("int", ["xpic_ctx*", "const xpic_field_envelope*", "double", "int64_t", "int64_t", "double*"]),
    "xpic_model_full_orbit_trace_collisional": ("int", _FO + _MODEL + _OPEN + _COLL),
    "xpic_model_drift_kinetic_trace_collisional": ("int", _DK + _MODEL + _OPEN + _COLL),
    "xpic_background_set": ("int", ["xpic_ctx*", "int", "const double*", "const double*", "const double*"]),
    "xpic_background_get": ("int", ["xpic_ctx*", "int", "double*", "double*", "double*"]),
    "xpic_background_clear": ("int", ["xpic_ctx*", "int"]),
    "xpic_background_from_sort": ("int", ["xpic_ctx*", "int", "int"]),
    "xpic_full_orbit_trace_collisional": ("int", _FO + _OPEN + _GRID),
    "xpic_drift_kinetic_trace_collisional": ("int", _DK + ["int"] + _OPEN + _GRID),
    "xpic_triplet_trace": ("int", _FO + ["const xpic_dk_params*", "const xpic_field_model*", "int", "int", "int64_t",
                                         "int64_t", "double*", "double*", "double*", "double*", "double*", "int64_t*", "int*",
                                         "int64_t*", "int*", "int64_t*", "int*"]),
    "xpic_comm_rccl_unique_id": ("int", ["void*"]),
    "xpic_comm_init_rccl": ("int", ["xpic_ctx*", "const void*"]),
    "xpic_comm_init_callbacks": ("int", ["xpic_ctx*", "const xpic_comm_callbacks*"]),
    "xpic_comm_peer_export": ("int", ["xpic_ctx*", "void*"]),
    "xpic_comm_peer_import": ("int", ["xpic_ctx*", "const void*", "const void*"]),
    "xpic_comm_size": ("int", ["xpic_ctx*", "int*"]),
    "xpic_comm_stats": ("int", ["xpic_ctx*", "int64_t*", "int"]),
    "xpic_profile_enable": ("int", ["xpic_ctx*", "int"]),
    "xpic_profile_reset": ("int", ["xpic_ctx*"]),
    "xpic_profile_get": ("int", ["xpic_ctx*", "const char*", "int64_t*", "double*"]),
    "xpic_probe_copy_bandwidth": ("int", ["xpic_ctx*", "int64_t", "int", "double*"]),
}
SYMBOLS = list(PROTOTYPES)  # every symbol include/xpic_hip.h declares
# the entry points of include/xpic_set_particles.h, typed by load_library() as PROTOTYPES' are; tests/test_abi_set_particles.py
# holds them to that header
LOAD_PROTOTYPES = {
    "xpic_set_particles": ("int", ["xpic_ctx*", "int", "const xpic_set_particles_params*", "int64_t", "int64_t", "int64_t",
                                   "int64_t*", "double*"]),
    "xpic_particles_number": ("int", ["xpic_ctx*", "int", "int", "const double*", "int64_t*"]),
}
# the entry points of include/xpic_tracers.h, typed by load_library() as PROTOTYPES' are; tests/test_abi_tracers.py holds them
# to that header
TRACER_PROTOTYPES = {
    "xpic_grad_abs_field": ("int", ["xpic_ctx*", "int", "int"]),
    "xpic_tracers_create": ("int", ["xpic_ctx*", "int", "int64_t", "const void*", "const double*", "const xpic_trace_region*",
                                    "int", "int64_t", "int64_t", "int*"]),
    "xpic_tracers_advance": ("int", ["xpic_ctx*", "int", "int64_t"]),
    "xpic_tracers_attach": ("int", ["xpic_ctx*", "int", "int"]),
    "xpic_tracers_get": ("int", ["xpic_ctx*", "int", "double*", "int64_t*", "int64_t*", "int*", "int64_t*"]),
    "xpic_tracers_samples": ("int", ["xpic_ctx*", "int", "double*", "int64_t*", "int64_t*"]),
    "xpic_tracers_destroy": ("int", ["xpic_ctx*", "int"]),
}
# the entry points of include/xpic_tracer_moments.h, typed by load_library() as PROTOTYPES' are;
# tests/test_abi_tracer_moments.py holds them to that header
TRACER_MOMENT_PROTOTYPES = {
    "xpic_tracers_moment": ("int", ["xpic_ctx*", "int", "int", "double", "double", "double", "const int*", "double*",
                                    "int64_t*"]),
    "xpic_tracers_map_create": ("int", ["xpic_ctx*", "int", "int", "double", "double", "double", "const int*", "int64_t",
                                        "int*"]),
    "xpic_tracers_map_get": ("int", ["xpic_ctx*", "int", "int", "double*", "int64_t*", "int"]),
    "xpic_tracers_map_destroy": ("int", ["xpic_ctx*", "int", "int"]),
}
TRACERS_MAX_MAPS = 4  # XPIC_TRACERS_MAX_MAPS
DEBUG_TRACER_MOMENT_LDS = 3  # XPIC_DEBUG_TRACER_MOMENT_LDS (xpic_debug_set)
TRACERS_MAX_SETS = 8  # XPIC_TRACERS_MAX_SETS
TRACER_KINDS = {"full_orbit": 0, "drift_kinetic": 1}  # XPIC_TRACERS_FULL_ORBIT, XPIC_TRACERS_DRIFT_KINETIC
GRADB_AUTO = -2  # XPIC_GRADB_AUTO


# include/xpic_field_lines.h: its struct (that header's, so not one of MIRRORS, which are xpic_hip.h's), its constants and its
# entry points, typed by load_library() as PROTOTYPES' are; tests/test_abi_field_lines.py holds them to that header
class LineParams(C.Structure):
    _fields_ = [("h", C.c_double), ("max_steps", C.c_int64), ("f_floor", C.c_double), ("close_tol", C.c_double),
                ("stagger", C.c_int32), ("directions", C.c_int32), ("launch_steps", C.c_int32), ("component", C.c_int32)]


CTYPES["const xpic_line_params*"] = C.POINTER(LineParams)
_LINES = ["int64_t", "const double*", "const xpic_line_params*", "const xpic_trace_region*", "int64_t", "double*", "double*",
          "double*", "double*", "double*", "double*", "int64_t*", "int32_t*", "double*"]
FIELD_LINE_PROTOTYPES = {
    "xpic_field_lines": ("int", ["xpic_ctx*", "int"] + _LINES),
    "xpic_model_field_lines": ("int", ["xpic_ctx*", "const xpic_field_model*"] + _LINES),
}
LINES_LAUNCH_STEPS = 256    # XPIC_LINES_LAUNCH_STEPS
LINES_MAX_STEPS = 1 << 24   # XPIC_LINES_MAX_STEPS
STAGGERS = {"B": 0, "E": 1}  # XPIC_STAGGER_B, XPIC_STAGGER_E
LINE_DIRECTIONS = {"+": 1, "-": 2, "both": 3}
LINE_CODES = {"maxsteps": 0, "left": 1, "null": 2, "closed": 3}  # XPIC_LINE_*

# the entry points of include/xpic_gauss.h (Gauss's law: its residual and the cleaner), typed by load_library() as PROTOTYPES'
# are; tests/test_abi_gauss.py holds them to that header
GAUSS_PROTOTYPES = {
    "xpic_gauss_background": ("int", ["xpic_ctx*", "const double*"]),
    "xpic_gauss_residual": ("int", ["xpic_ctx*", "int", "double*", "double*"]),
    "xpic_gauss_clean": ("int", ["xpic_ctx*", "int", "double", "double", "int", "double*", "int*", "double*"]),
    "xpic_set_gauss_clean": ("int", ["xpic_ctx*", "int", "double", "double", "int"]),
    "xpic_gauss_info": ("int", ["xpic_ctx*", "double*"]),
}
GAUSS_MAXIT = 10000  # the package's default iteration limit of a clean

# the entry point of include/xpic_es.h (the electrostatic scheme's particle phase alone), typed by load_library() as
# PROTOTYPES' are; tests/test_abi_es.py holds it to that header
ES_PROTOTYPES = {
    "xpic_es_push": ("int", ["xpic_ctx*", "int", "double*"]),
}
ES_RTOL, ES_ATOL, ES_MAXIT = 1e-10, 1e-14, 10000  # the tolerances an "es" context is created with (xpic_es.h)

# the entry points of include/xpic_poisson.h (the direct Poisson solve and the choice between it and CG), typed by
# load_library() as PROTOTYPES' are; tests/test_abi_poisson.py holds them to that header
POISSON_PROTOTYPES = {
    "xpic_set_poisson_solver": ("int", ["xpic_ctx*", "int"]),
    "xpic_get_poisson_solver": ("int", ["xpic_ctx*", "int*"]),
    "xpic_poisson_apply": ("int", ["xpic_ctx*", "const double*", "double*"]),
    "xpic_poisson_solve": ("int", ["xpic_ctx*", "const double*", "double", "int", "double*", "int*", "double*"]),
}
POISSON_SOLVERS = {"cg": 0, "direct": 1}  # enum xpic_poisson_solver
POISSON_MAX_EXTENT = 1024  # XPIC_POISSON_MAX_EXTENT

# the entry points of include/xpic_spectrum.h (field spectra: power, axis and shell sums, single modes, the probe that rides
# with the step), typed by load_library() as PROTOTYPES' are; tests/test_abi_spectrum.py holds them to that header
_SOURCE = ["xpic_ctx*", "int", "int", "const double*"]
SPECTRUM_PROTOTYPES = {
    "xpic_spectrum_power": ("int", _SOURCE + ["double*"]),
    "xpic_spectrum": ("int", _SOURCE + ["double*", "double*", "double*", "int", "const double*", "double*", "int64_t*", "double*",
                                        "double*"]),
    "xpic_spectrum_modes": ("int", _SOURCE + ["int", "const int32_t*", "double*"]),
    "xpic_spectrum_probe_create": ("int", ["xpic_ctx*", "int", "int", "int", "const int32_t*", "int", "int64_t", "int*"]),
    "xpic_spectrum_probe_get": ("int", ["xpic_ctx*", "int", "int64_t", "int64_t*", "double*", "int64_t*", "int64_t*", "int"]),
    "xpic_spectrum_probe_destroy": ("int", ["xpic_ctx*", "int"]),
}
SPECTRUM_SOURCES = {"host": 100, "rho": 101}  # enum xpic_spectrum_source (a field id is a source too)
SPECTRUM_MAX_SHELLS = 2048  # XPIC_SPECTRUM_MAX_SHELLS
SPECTRUM_MAX_PROBES = 16    # XPIC_SPECTRUM_MAX_PROBES
