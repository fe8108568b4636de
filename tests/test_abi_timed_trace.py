"""The C boundary of the time-dependent analytic fields (no compute calls: these run without a GPU): the library exports
the new symbols, include/xpic_hip.h declares them with the argument types written here, the package lists them, and the
ctypes mirror of xpic_field_envelope has the header's layout and constants."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TRACE_TAIL = ["int64_t", "int64_t", "double*", "double*", "int64_t*", "int*", "const xpic_trace_region*", "int64_t*",
              "int64_t*", "int64_t*"]
PROTOTYPES = {
    "xpic_model_full_orbit_trace_timed": ["xpic_ctx*", "int64_t", "const xpic_fo_params*", "const xpic_field_model*",
                                          "const xpic_field_envelope*"] + TRACE_TAIL + ["double*"],
    "xpic_model_drift_kinetic_trace_timed": ["xpic_ctx*", "int64_t", "const xpic_dk_params*", "const xpic_field_model*",
                                             "const xpic_field_envelope*"] + TRACE_TAIL,
    "xpic_envelope_factors": ["xpic_ctx*", "const xpic_field_envelope*", "double", "int64_t", "int64_t", "double*"],
}
# the entry points these extend keep their prototypes
UNCHANGED = {
    "xpic_model_full_orbit_trace": ["xpic_ctx*", "int64_t", "const xpic_fo_params*", "const xpic_field_model*"] + TRACE_TAIL,
    "xpic_model_drift_kinetic_trace": ["xpic_ctx*", "int64_t", "const xpic_dk_params*", "const xpic_field_model*"] + TRACE_TAIL,
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
    for name, types in list(PROTOTYPES.items()) + list(UNCHANGED.items()):
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
    for f in ("model_full_orbit_trace_timed", "model_drift_kinetic_trace_timed", "envelope_factors"):
        assert callable(getattr(xpic_amd.Context, f))
    assert callable(xpic_amd.field_envelope)
    assert xpic_amd.TimedTrace._fields == xpic_amd.OpenTrace._fields + ("sums",)


def test_field_envelope_layout_and_constants():
    import xpic_amd

    m = re.search(r"typedef struct xpic_field_envelope \{(.*?)\} xpic_field_envelope;", header(), flags=re.S)
    fields = [" ".join(f.split()) for f in m.group(1).split(";") if f.strip()]
    assert fields == ["int32_t kind", "int32_t reserved", "double a", "double b", "double omega", "double phase"]
    T = xpic_amd.FieldEnvelope
    names = [f.split()[-1] for f in fields]
    assert [f[0] for f in T._fields_] == names
    assert [getattr(T, n).offset for n in names] == [0, 4, 8, 16, 24, 32]
    assert ctypes.sizeof(T) == 40
    enum = re.search(r"enum xpic_envelope_kind \{(.*?)\};", header(), flags=re.S).group(1)
    values = dict(re.findall(r"(XPIC_ENV_\w+) = (\d+)", enum))
    assert values == {"XPIC_ENV_CONSTANT": "0", "XPIC_ENV_RAMP": "1", "XPIC_ENV_HARMONIC": "2", "XPIC_ENV_NKINDS": "3"}
    assert xpic_amd.ENVELOPE_KINDS == {"constant": 0, "ramp": 1, "harmonic": 2}
    e = xpic_amd.field_envelope("ramp", a=0.0, b=1.0)
    assert (e.kind, e.a, e.b, e.omega, e.phase) == (1, 0.0, 1.0, 0.0, 0.0)
    e = xpic_amd.field_envelope("harmonic", omega=2.5, phase=-0.5)
    assert (e.kind, e.a, e.b, e.omega, e.phase) == (2, 0.0, 0.0, 2.5, -0.5)
    assert xpic_amd.field_envelope("constant").kind == 0 and xpic_amd.field_envelope(2).kind == 2
    try:
        xpic_amd.field_envelope("ramp", slope=1.0)
    except xpic_amd.XpicError:
        pass
    else:
        raise AssertionError("an unknown parameter was accepted")
