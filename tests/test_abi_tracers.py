"""The C boundary of the tracer sets (no GPU): include/xpic_tracers.h against the package's TRACER_PROTOTYPES by the rules
tests/test_abi.py holds include/xpic_hip.h and PROTOTYPES to -- the table is the header's, the library exports the symbols,
load_library() types them, the constants are the package's numbers, and every method passes its typed prototype down to
the library's own refusal of a null context."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import abi_header as H
import test_abi as A

LITERAL = {
    "xpic_grad_abs_field": ["xpic_ctx*", "int", "int"],
    "xpic_tracers_create": ["xpic_ctx*", "int", "int64_t", "const void*", "const double*", "const xpic_trace_region*", "int",
                            "int64_t", "int64_t", "int*"],
    "xpic_tracers_advance": ["xpic_ctx*", "int", "int64_t"],
    "xpic_tracers_attach": ["xpic_ctx*", "int", "int"],
    "xpic_tracers_get": ["xpic_ctx*", "int", "double*", "int64_t*", "int64_t*", "int*", "int64_t*"],
    "xpic_tracers_samples": ["xpic_ctx*", "int", "double*", "int64_t*", "int64_t*"],
    "xpic_tracers_destroy": ["xpic_ctx*", "int"],
}


def declared(monkeypatch):
    """(symbols, prototypes) of include/xpic_tracers.h, read by abi_header's own parser"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(H.ROOT, "include", "xpic_tracers.h")).read(), flags=re.S)
    monkeypatch.setattr(H, "header", lambda: text)
    return H.symbols(), H.prototypes()


def test_the_table_is_the_header(monkeypatch):
    import xpic_amd as X

    symbols, prototypes = declared(monkeypatch)
    assert symbols == sorted(LITERAL) == sorted(prototypes) == sorted(X.TRACER_PROTOTYPES)
    for name in LITERAL:
        assert prototypes[name] == X.TRACER_PROTOTYPES[name] == ("int", LITERAL[name]), name
        assert all(a in X.CTYPES for a in LITERAL[name]), name
        assert name not in X.PROTOTYPES and name not in X.LOAD_PROTOTYPES
    assert H.macro("XPIC_TRACERS_MAX_SETS") == X.TRACERS_MAX_SETS == 8
    assert H.macro("XPIC_GRADB_AUTO") == X.GRADB_AUTO == -2
    assert {"full_orbit": H.macro("XPIC_TRACERS_FULL_ORBIT"), "drift_kinetic": H.macro("XPIC_TRACERS_DRIFT_KINETIC")} == X.TRACER_KINDS
    assert '#include "xpic_tracers.h"' in open(os.path.join(H.ROOT, "include", "xpic_hip.h")).read()


def test_library_exports_and_types_the_symbols():
    import xpic_amd as X

    lib = A.built_library()
    L = X.load_library()
    for name in LITERAL:
        assert hasattr(lib, name), name
        f = getattr(L, name)
        assert f.restype is C.c_int and list(f.argtypes) == [X.CTYPES[a] for a in LITERAL[name]], name
    for f in ("grad_abs_field", "tracers"):
        assert callable(getattr(X.Context, f)), f
    for f in ("advance", "attach", "detach", "get", "samples", "close"):
        assert callable(getattr(X.TracerSet, f)), f


def test_null_handle_sweep():
    """every method, in the forms of its optional arguments, on a context that was never created"""
    import xpic_amd as X

    A.built_library()
    ctx = object.__new__(X.Context)
    ctx.L, ctx.h = A.Recorder(X.load_library()), C.c_void_p(0)
    p = np.array([[1.0, 1.0, 1.0, 0.1, 0.0, 0.0], [2.0, 1.5, 1.0, 0.0, 0.1, 0.0]])
    box = {"name": "box", "min": (0.0, 0.0, 0.0), "max": (4.0, 4.0, 4.0)}
    cyl = {"name": "cylinder", "center": (2.0, 2.0, 2.0), "radius": 1.5, "height": 3.0}
    refused = pytest.raises(X.XpicError, match=r"xpic error [1-9]\d*: .+")
    with refused:
        ctx.grad_abs_field(X.B, X.W0)
    for kw in ({}, dict(region=box, sample_every=2, sample_capacity=5), dict(region=cyl, step0=1 << 40, compact="always")):
        with refused:
            ctx.tracers("full_orbit", p, "EB2B", -1.0, 0.5, **kw)
        with refused:
            ctx.tracers("full_orbit", p, "CN", -1.0, 0.5, maxit=5, atol=0.0, rtol=0.0, **kw)
        for gradB in (None, X.W0, "auto"):
            with refused:
                ctx.tracers("drift_kinetic", p, -1.0, 1.0, 0.5, gradB_field=gradB, maxit=7, **kw)
    with pytest.raises(X.XpicError, match="unknown arguments"):
        ctx.tracers("full_orbit", p, "EB2B", -1.0, 0.5, eps=1.0)
    s = X.TracerSet(ctx, 0, 2)
    for call in (s.advance, lambda: s.advance(3), s.attach, s.detach, s.get, s.samples, s.close):
        with refused:
            call()
    assert ctx.L.seen >= set(LITERAL)
    ctx.h = None  # (nothing to destroy)
