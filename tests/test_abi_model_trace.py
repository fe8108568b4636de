"""The C boundary of the analytic field models (no compute calls: these run without a GPU): the library exports the new
symbols, include/xpic_hip.h declares them with the argument types written here, the package lists them, and the ctypes
mirror of xpic_field_model has the header's layout and constants."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TRACE_TAIL = ["int64_t", "int64_t", "double*", "double*", "int64_t*", "int*", "const xpic_trace_region*", "int64_t*",
              "int64_t*", "int64_t*"]
PROTOTYPES = {
    "xpic_model_fields": ["xpic_ctx*", "const xpic_field_model*", "int64_t", "const double*", "double*", "double*", "double*"],
    "xpic_set_model_field": ["xpic_ctx*", "const xpic_field_model*", "int", "int", "int"],
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
    for f in ("model_fields", "set_model_field", "model_full_orbit_trace", "model_drift_kinetic_trace"):
        assert callable(getattr(xpic_amd.Context, f))
    assert callable(xpic_amd.field_model)


def test_field_model_layout_and_constants():
    import xpic_amd

    m = re.search(r"typedef struct xpic_field_model \{(.*?)\} xpic_field_model;", header(), flags=re.S)
    fields = [" ".join(f.split()) for f in m.group(1).split(";") if f.strip()]
    assert fields == ["int32_t kind", "int32_t reserved", "double E0[3]", "double B0[3]", "double r0[3]", "double g[3]",
                      "double B_min", "double B_max", "double W", "double D", "double L", "double E_phi", "double phi"]
    T = xpic_amd.FieldModel
    names = [f.split()[-1].split("[")[0] for f in fields]
    assert [f[0] for f in T._fields_] == names
    offsets = [getattr(T, n).offset for n in names]
    assert offsets == [0, 4, 8, 32, 56, 80, 104, 112, 120, 128, 136, 144, 152]
    assert ctypes.sizeof(T) == 160
    enum = re.search(r"enum xpic_model_kind \{(.*?)\};", header(), flags=re.S).group(1)
    values = dict(re.findall(r"(XPIC_MODEL_\w+) = (\d+)", enum))
    assert values == {"XPIC_MODEL_UNIFORM": "0", "XPIC_MODEL_LINEAR": "1", "XPIC_MODEL_QUADRATIC_MIRROR": "2",
                      "XPIC_MODEL_GAUSSIAN_MIRROR": "3", "XPIC_MODEL_NKINDS": "4"}
    assert xpic_amd.MODEL_KINDS == {"uniform": 0, "linear": 1, "quadratic_mirror": 2, "gaussian_mirror": 3}
    assert int(re.search(r"#define XPIC_GEOM_NONE \((-?\d+)\)", header()).group(1)) == xpic_amd.GEOM_NONE == -1
    for macro, value in (("XPIC_MODEL_LAUNCH_STEPS", xpic_amd.MODEL_LAUNCH_STEPS), ("XPIC_MODEL_DK_MAXIT", xpic_amd.MODEL_DK_MAXIT)):
        assert int(re.search(r"#define %s (\d+)" % macro, header()).group(1)) == value
    mm = xpic_amd.field_model("gaussian_mirror", B_min=1.0, B_max=4.0, L=5.0, W=1.0)
    assert (mm.kind, mm.B_min, mm.B_max, mm.L, mm.W, mm.D) == (3, 1.0, 4.0, 5.0, 1.0, 0.0)
    mm = xpic_amd.field_model("linear", B0=(0, 0, 2), g=(1, 0, 0))
    assert list(mm.B0) == [0.0, 0.0, 2.0] and list(mm.g) == [1.0, 0.0, 0.0] and list(mm.E0) == [0.0] * 3
