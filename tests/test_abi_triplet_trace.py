"""The C boundary of the triplet trace (no compute calls: these run without a GPU): the library exports the symbol,
include/xpic_hip.h declares it with the argument types written here, the package lists it, and the constants the Python
side quotes are the header's."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = {
    "xpic_triplet_trace": [
        "xpic_ctx*", "int64_t", "const xpic_fo_params*", "const xpic_dk_params*", "const xpic_field_model*", "int", "int",
        "int64_t", "int64_t", "double*", "double*", "double*", "double*", "double*", "int64_t*", "int*", "int64_t*", "int*",
        "int64_t*", "int*"],
}


def header():
    txt = open(os.path.join(ROOT, "include", "xpic_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def declared_types(name):
    """the argument types of `int name(...);` in the header, names stripped"""
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header())
    assert m, name
    types = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        t = re.match(r"^(.*?)(\w+)$", arg).group(1).strip()  # drop the parameter's name
        types.append(t.replace(" *", "*"))
    return types


def test_prototype_matches_the_header():
    for name, types in PROTOTYPES.items():
        assert declared_types(name) == types, name


def test_library_exports_the_symbol():
    import xpic_amd

    if not os.path.exists(xpic_amd.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    lib = ctypes.CDLL(xpic_amd.LIB_PATH)
    for name in PROTOTYPES:
        assert name in xpic_amd.SYMBOLS, name
        assert hasattr(lib, name), name


def test_constants():
    import xpic_amd

    for macro, value in (("XPIC_TRIPLET_LAUNCH_STEPS", xpic_amd.TRIPLET_LAUNCH_STEPS),
                         ("XPIC_TRIPLET_DK_MAXIT", xpic_amd.TRIPLET_DK_MAXIT),
                         ("XPIC_TRIPLET_NSTATS", len(xpic_amd.TRIPLET_STATS))):
        assert int(re.search(r"#define %s (\d+)" % macro, header()).group(1)) == value
    assert xpic_amd.TRIPLET_LAUNCH_STEPS == 64 and xpic_amd.TRIPLET_DK_MAXIT == 1024
    assert xpic_amd.TRIPLET_STATS == ("B", "gradB", "pos", "z", "p_parallel", "mu", "energy")
    assert xpic_amd.TRIPLET_STATS[3:] == xpic_amd.PAIR_STATS
    assert xpic_amd.TripletTrace._fields == (
        "p", "state_model", "state_grid", "stats", "curve", "fo_iterations_sum", "fo_iterations_max", "dkm_iterations_total",
        "dkm_iterations_max", "dkg_iterations_total", "dkg_iterations_max")
