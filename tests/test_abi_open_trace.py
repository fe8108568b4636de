"""The C boundary of the open-trap traces and the mirror field (no compute calls: these run without a GPU): the library
exports the new symbols, include/xpic_hip.h declares them with the argument types written here, the package lists them,
and the ctypes mirror of xpic_trace_region has the header's layout."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = {
    "xpic_full_orbit_trace_open": [
        "xpic_ctx*", "int64_t", "const xpic_fo_params*", "int64_t", "int64_t", "double*", "double*", "int64_t*", "int*",
        "const xpic_trace_region*", "int64_t*", "int64_t*", "int64_t*"],
    "xpic_drift_kinetic_trace_open": [
        "xpic_ctx*", "int64_t", "const xpic_dk_params*", "int", "int64_t", "int64_t", "double*", "double*", "int64_t*",
        "int*", "const xpic_trace_region*", "int64_t*", "int64_t*", "int64_t*"],
    "xpic_set_mirror_field": ["xpic_ctx*", "int", "double", "double", "double"],
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


def test_prototypes_match_the_header():
    for name, types in PROTOTYPES.items():
        assert declared_types(name) == types, name


def test_library_exports_the_new_symbols():
    import xpic_amd

    if not os.path.exists(xpic_amd.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    lib = ctypes.CDLL(xpic_amd.LIB_PATH)
    for name in PROTOTYPES:
        assert name in xpic_amd.SYMBOLS, name
        assert hasattr(lib, name), name


def test_trace_region_layout():
    import xpic_amd

    m = re.search(r"typedef struct xpic_trace_region \{(.*?)\} xpic_trace_region;", header(), flags=re.S)
    fields = [" ".join(f.split()) for f in m.group(1).split(";") if f.strip()]
    assert fields == ["int32_t geometry", "int32_t compact", "double geom[7]", "int64_t step0"]
    T = xpic_amd.TraceRegion
    assert [f[0] for f in T._fields_] == ["geometry", "compact", "geom", "step0"]
    assert (T.geometry.offset, T.compact.offset, T.geom.offset, T.step0.offset) == (0, 4, 8, 64)
    assert ctypes.sizeof(T) == 72
    enum = re.search(r"enum xpic_trace_compact \{(.*?)\};", header(), flags=re.S).group(1)
    values = dict(re.findall(r"(XPIC_COMPACT_\w+) = (\d+)", enum))
    assert values == {"XPIC_COMPACT_AUTO": "0", "XPIC_COMPACT_NEVER": "1", "XPIC_COMPACT_ALWAYS": "2"}
    assert xpic_amd.COMPACT == {"auto": 0, "never": 1, "always": 2}
    # the launch lengths the Python side quotes
    for macro, value in (("XPIC_FO_LAUNCH_STEPS", xpic_amd.FO_LAUNCH_STEPS), ("XPIC_DK_LAUNCH_STEPS", xpic_amd.DK_LAUNCH_STEPS)):
        assert int(re.search(r"#define %s (\d+)" % macro, header()).group(1)) == value
