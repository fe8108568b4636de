"""The C boundary of the field-line tracer (no GPU): include/xpic_field_lines.h against the package's FIELD_LINE_PROTOTYPES
by the rules tests/test_abi_tracers.py holds include/xpic_tracers.h to -- the table is the header's, the library exports
the symbols, load_library() types them, the struct and the constants are the package's, and every method passes its typed
prototype down to the library's own refusal of a null context."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import abi_header as H
import test_abi as A

_TAIL = ["int64_t", "const double*", "const xpic_line_params*", "const xpic_trace_region*", "int64_t", "double*", "double*",
         "double*", "double*", "double*", "double*", "int64_t*", "int32_t*", "double*"]
LITERAL = {
    "xpic_field_lines": ["xpic_ctx*", "int"] + _TAIL,
    "xpic_model_field_lines": ["xpic_ctx*", "const xpic_field_model*"] + _TAIL,
}


def declared(monkeypatch):
    """include/xpic_field_lines.h as abi_header's own parser reads a header"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(H.ROOT, "include", "xpic_field_lines.h")).read(), flags=re.S)
    monkeypatch.setattr(H, "header", lambda: text)


def test_the_table_is_the_header(monkeypatch):
    import xpic_amd as X

    declared(monkeypatch)
    symbols, prototypes = H.symbols(), H.prototypes()
    assert symbols == sorted(LITERAL) == sorted(prototypes) == sorted(X.FIELD_LINE_PROTOTYPES)
    for name in LITERAL:
        assert prototypes[name] == X.FIELD_LINE_PROTOTYPES[name] == ("int", LITERAL[name]), name
        assert all(a in X.CTYPES for a in LITERAL[name]), name
        assert name not in X.PROTOTYPES and name not in X.LOAD_PROTOTYPES and name not in X.TRACER_PROTOTYPES
    # the struct: the header's members in its order, the offsets and the size written out
    assert H.structs() == ["xpic_line_params"] and "xpic_line_params" not in X.MIRRORS
    assert H.struct_fields("xpic_line_params") == ["double h", "int64_t max_steps", "double f_floor", "double close_tol",
                                                   "int32_t stagger", "int32_t directions", "int32_t launch_steps",
                                                   "int32_t component"]
    names = H.member_names("xpic_line_params")
    assert [f[0] for f in X.LineParams._fields_] == names
    assert [getattr(X.LineParams, n).offset for n in names] == [0, 8, 16, 24, 32, 36, 40, 44] and C.sizeof(X.LineParams) == 48
    assert X.CTYPES["const xpic_line_params*"] is C.POINTER(X.LineParams)
    assert H.macro("XPIC_LINES_LAUNCH_STEPS") == X.LINES_LAUNCH_STEPS == 256
    assert H.macro("XPIC_LINES_MAX_STEPS") == X.LINES_MAX_STEPS == 1 << 24
    assert {"B": H.macro("XPIC_STAGGER_B"), "E": H.macro("XPIC_STAGGER_E")} == X.STAGGERS
    assert {k: H.macro("XPIC_LINE_" + k.upper()) for k in X.LINE_CODES} == X.LINE_CODES == {
        "maxsteps": 0, "left": 1, "null": 2, "closed": 3}
    assert H.macro("XPIC_LINE_RUNNING") == -1 and X.LINE_DIRECTIONS == {"+": 1, "-": 2, "both": 3}
    assert '#include "xpic_field_lines.h"' in open(os.path.join(H.ROOT, "include", "xpic_hip.h")).read()


def test_library_exports_and_types_the_symbols():
    import xpic_amd as X

    lib = A.built_library()
    L = X.load_library()
    for name in LITERAL:
        assert hasattr(lib, name), name
        f = getattr(L, name)
        assert f.restype is C.c_int and list(f.argtypes) == [X.CTYPES[a] for a in LITERAL[name]], name
    for f in ("field_lines", "model_field_lines"):
        assert callable(getattr(X.Context, f)), f
    assert X.FieldLines._fields == ("end", "length", "volume", "fmin", "smin", "fmax", "steps", "code", "samples", "directions")
    for f in ("total_length", "total_volume", "mirror_ratio", "codes", "ends"):
        assert isinstance(getattr(X.FieldLines, f), property), f


def test_null_handle_sweep():
    """every method, in the forms of its optional arguments, on a context that was never created"""
    import xpic_amd as X

    A.built_library()
    ctx = object.__new__(X.Context)
    ctx.L, ctx.h = A.Recorder(X.load_library()), C.c_void_p(0)
    seeds = np.array([[1.0, 1.0, 1.0], [2.0, 1.5, 1.0]])
    box = {"name": "box", "min": (0.0, 0.0, 0.0), "max": (4.0, 4.0, 4.0)}
    cyl = {"name": "cylinder", "center": (2.0, 2.0, 2.0), "radius": 1.5, "height": 3.0}
    model = X.field_model("gaussian_mirror", B_min=1.0, B_max=4.0, L=5.0, W=1.0)
    refused = pytest.raises(X.XpicError, match=r"xpic error [1-9]\d*: .+")
    forms = ({}, dict(region=box, directions="+"), dict(region=cyl, directions="-", sample_every=2, launch_steps=7),
             dict(f_floor=0.1, close_tol=0.05, directions=3))
    for kw in forms:
        for field, stagger in ((X.B, None), (X.E, None), (X.W0, "E"), (X.B0, "B")):
            with refused:
                ctx.field_lines(seeds, field=field, h=0.1, max_steps=5, stagger=stagger, **kw)
        for component in ("B", "E"):
            with refused:
                ctx.model_field_lines(model, seeds, h=0.1, max_steps=5, component=component, **kw)
    with refused:
        ctx.field_lines(np.zeros((0, 3)), h=0.1, max_steps=5)
    with pytest.raises(X.XpicError, match="h and max_steps are required"):
        ctx.field_lines(seeds)
    assert ctx.L.seen >= set(LITERAL)
    ctx.h = None  # (nothing to destroy)
