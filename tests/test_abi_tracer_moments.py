"""The C boundary of the tracer-set moments (no GPU): include/xpic_tracer_moments.h against the package's
TRACER_MOMENT_PROTOTYPES by the rules tests/test_abi_field_lines.py holds include/xpic_field_lines.h to -- the table is the
header's, the library exports the symbols, load_library() types them, the constants are the package's, and every method
passes its typed prototype down to the library's own refusal of a null context."""
import ctypes as C
import os
import re

import pytest

import abi_header as H
import test_abi as A

_SPEC = ["int", "double", "double", "double", "const int*"]
LITERAL = {
    "xpic_tracers_moment": ["xpic_ctx*", "int"] + _SPEC + ["double*", "int64_t*"],
    "xpic_tracers_map_create": ["xpic_ctx*", "int"] + _SPEC + ["int64_t", "int*"],
    "xpic_tracers_map_get": ["xpic_ctx*", "int", "int", "double*", "int64_t*", "int"],
    "xpic_tracers_map_destroy": ["xpic_ctx*", "int", "int"],
}


def declared(monkeypatch):
    """include/xpic_tracer_moments.h as abi_header's own parser reads a header"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(H.ROOT, "include", "xpic_tracer_moments.h")).read(), flags=re.S)
    monkeypatch.setattr(H, "header", lambda: text)


def test_the_table_is_the_header(monkeypatch):
    import xpic_amd as X

    declared(monkeypatch)
    symbols, prototypes = H.symbols(), H.prototypes()
    assert symbols == sorted(LITERAL) == sorted(prototypes) == sorted(X.TRACER_MOMENT_PROTOTYPES)
    for name in LITERAL:
        assert prototypes[name] == X.TRACER_MOMENT_PROTOTYPES[name] == ("int", LITERAL[name]), name
        assert all(a in X.CTYPES for a in LITERAL[name]), name
        for table in (X.PROTOTYPES, X.LOAD_PROTOTYPES, X.TRACER_PROTOTYPES, X.FIELD_LINE_PROTOTYPES):
            assert name not in table
    assert H.structs() == []
    assert H.macro("XPIC_TRACERS_MAX_MAPS") == X.TRACERS_MAX_MAPS == 4
    assert H.macro("XPIC_DEBUG_TRACER_MOMENT_LDS") == X.DEBUG_TRACER_MOMENT_LDS == 3
    assert X.DEBUG_TRACER_MOMENT_LDS not in (X.DEBUG_GATHER_WINDOW, X.DEBUG_PENCIL_LIMIT, X.DEBUG_SURROGATE_SCALE)
    hip = open(os.path.join(H.ROOT, "include", "xpic_hip.h")).read()
    assert hip.index('#include "xpic_tracers.h"') < hip.index('#include "xpic_tracer_moments.h"')


def test_library_exports_and_types_the_symbols():
    import xpic_amd as X

    lib = A.built_library()
    L = X.load_library()
    for name in LITERAL:
        assert hasattr(lib, name), name
        f = getattr(L, name)
        assert f.restype is C.c_int and list(f.argtypes) == [X.CTYPES[a] for a in LITERAL[name]], name
    for f in ("moment", "map"):
        assert callable(getattr(X.TracerSet, f)), f
    for f in ("get", "close"):
        assert callable(getattr(X.TracerMap, f)), f


def test_null_handle_sweep():
    """every method, in the forms of its optional arguments, on a context that was never created"""
    import xpic_amd as X

    A.built_library()
    ctx = object.__new__(X.Context)
    ctx.L, ctx.h = A.Recorder(X.load_library()), C.c_void_p(0)
    ctx.n, ctx.nzl = (6, 5, 4), 4
    refused = pytest.raises(X.XpicError, match=r"xpic error [1-9]\d*: .+")
    s = X.TracerSet(ctx, 0, 2)
    forms = ({}, dict(weight=0.5), dict(region=(1, 1, 0, 4, 3, 3)), dict(weight=2.0, region=((0, 1, 1), (6, 3, 2))))
    for name in X.MOMENTS:
        for kw in forms:
            with refused:
                s.moment(name, -1.0, 1.0, **kw)
            with refused:
                s.map(name, -1.0, 1.0, **kw)
            with refused:
                s.map(name, -1.0, 1.0, every=3, **kw)
    m = X.TracerMap(s, 0, 3)
    for call in (m.get, lambda: m.get(reset=True), m.close):
        with refused:
            call()
    with pytest.raises(KeyError):
        s.moment("pressure", 1.0, 1.0)
    assert ctx.L.seen >= set(LITERAL)
    ctx.h = None  # (nothing to destroy)
