"""The C boundary of the collisional traces (no compute calls: these run without a GPU): the library exports the new
symbols, include/xpic_hip.h declares them with the argument types written here, the package lists them, and the ctypes
mirrors of xpic_trace_background and xpic_trace_collisions have the header's layout and constant."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TRACE_TAIL = ["int64_t", "int64_t", "double*", "double*", "int64_t*", "int*", "const xpic_trace_region*", "int64_t*",
              "int64_t*", "int64_t*"]
COLL_TAIL = ["const xpic_trace_collisions*", "double*"]
PROTOTYPES = {
    "xpic_model_full_orbit_trace_collisional":
        ["xpic_ctx*", "int64_t", "const xpic_fo_params*", "const xpic_field_model*"] + TRACE_TAIL + COLL_TAIL,
    "xpic_model_drift_kinetic_trace_collisional":
        ["xpic_ctx*", "int64_t", "const xpic_dk_params*", "const xpic_field_model*"] + TRACE_TAIL + COLL_TAIL,
}
# the model traces' lists, which the collisional ones extend
MODEL = {"xpic_model_full_orbit_trace_collisional": "xpic_model_full_orbit_trace",
         "xpic_model_drift_kinetic_trace_collisional": "xpic_model_drift_kinetic_trace"}


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
        assert declared_types(name) == declared_types(MODEL[name]) + COLL_TAIL, name


def test_library_exports_the_new_symbols():
    import xpic_amd

    if not os.path.exists(xpic_amd.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    lib = ctypes.CDLL(xpic_amd.LIB_PATH)
    for name in PROTOTYPES:
        assert name in xpic_amd.SYMBOLS, name
        assert hasattr(lib, name), name
    for f in ("model_full_orbit_trace_collisional", "model_drift_kinetic_trace_collisional"):
        assert callable(getattr(xpic_amd.Context, f))
    assert callable(xpic_amd.trace_collisions)


def struct_fields(name):
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header(), flags=re.S)
    assert m, name
    out = []
    for decl in m.group(1).split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        typ, rest = decl.split(" ", 1)
        out += ["%s %s" % (typ, v.strip()) for v in rest.split(",")]  # `double q, m, n` declares three members
    return out


def test_struct_layouts_and_the_constant():
    import xpic_amd

    assert int(re.search(r"#define XPIC_TRACE_BG_MAX (\d+)", header()).group(1)) == xpic_amd.TRACE_BG_MAX == 4
    fields = struct_fields("xpic_trace_background")
    assert fields == ["double q", "double m", "double n", "double vth", "double drift[3]"]
    B = xpic_amd.TraceBackground
    names = [f.split()[-1].split("[")[0] for f in fields]
    assert [f[0] for f in B._fields_] == names
    assert [getattr(B, n).offset for n in names] == [0, 8, 16, 24, 32]
    assert ctypes.sizeof(B) == 56
    fields = struct_fields("xpic_trace_collisions")
    assert fields == ["int32_t nbg", "int32_t every", "uint64_t seed", "int64_t particle0", "double strength", "double mass",
                      "xpic_trace_background bg[XPIC_TRACE_BG_MAX]"]
    T = xpic_amd.TraceCollisions
    names = [f.split()[-1].split("[")[0] for f in fields]
    assert [f[0] for f in T._fields_] == names
    assert [getattr(T, n).offset for n in names] == [0, 4, 8, 16, 24, 32, 40]
    assert ctypes.sizeof(T) == 40 + 4 * 56
    assert T.bg.size == 4 * 56


def test_the_builder():
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
