"""The C boundary of the collisional grid traces and the background profiles (no compute calls: these run without a GPU):
the library exports the new symbols, include/xpic_hip.h declares them with the argument types written here, the package
lists them and has their methods, and the header no longer says that the grid traces have no collisional form."""
import ctypes
import os

import test_abi_collisional_trace as T

ROOT = T.ROOT
GRID_TAIL = ["const xpic_trace_collisions*", "const int32_t*", "double*"]
PROTOTYPES = {
    "xpic_background_set": ["xpic_ctx*", "int", "const double*", "const double*", "const double*"],
    "xpic_background_get": ["xpic_ctx*", "int", "double*", "double*", "double*"],
    "xpic_background_clear": ["xpic_ctx*", "int"],
    "xpic_background_from_sort": ["xpic_ctx*", "int", "int"],
    "xpic_full_orbit_trace_collisional": ["xpic_ctx*", "int64_t", "const xpic_fo_params*"] + T.TRACE_TAIL + GRID_TAIL,
    "xpic_drift_kinetic_trace_collisional":
        ["xpic_ctx*", "int64_t", "const xpic_dk_params*", "int"] + T.TRACE_TAIL + GRID_TAIL,
}
# the open grid traces' lists, which the collisional ones extend
OPEN = {"xpic_full_orbit_trace_collisional": "xpic_full_orbit_trace_open",
        "xpic_drift_kinetic_trace_collisional": "xpic_drift_kinetic_trace_open"}


def test_prototypes_match_the_header():
    for name, types in PROTOTYPES.items():
        assert T.declared_types(name) == types, name
    for name, base in OPEN.items():
        assert T.declared_types(name) == T.declared_types(base) + GRID_TAIL, name


def test_library_exports_the_new_symbols():
    import xpic_amd

    if not os.path.exists(xpic_amd.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    lib = ctypes.CDLL(xpic_amd.LIB_PATH)
    for name in PROTOTYPES:
        assert name in xpic_amd.SYMBOLS, name
        assert hasattr(lib, name), name
    for f in ("background_set", "background_get", "background_clear", "background_from_sort",
              "full_orbit_trace_collisional", "drift_kinetic_trace_collisional"):
        assert callable(getattr(xpic_amd.Context, f))


def test_the_header_says_what_is_there():
    txt = " ".join(open(os.path.join(ROOT, "include", "xpic_hip.h")).read().split())
    assert "the grid traces and the paired and triplet traces have * no collisional form" not in txt
    for letter in "abcdef":
        assert "(%s)" % letter in txt.split("collisional grid traces:")[1]
