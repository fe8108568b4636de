"""The C boundary of the Gauss-law cleaner (no GPU): include/xpic_gauss.h against the package's GAUSS_PROTOTYPES by the
rules tests/test_abi_field_lines.py holds include/xpic_field_lines.h to -- the table is the header's, the library exports
the symbols, load_library() types them, and every method passes its typed prototype down to the library's own refusal of
a null context."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import abi_header as H
import test_abi as A

LITERAL = {
    "xpic_gauss_background": ["xpic_ctx*", "const double*"],
    "xpic_gauss_residual": ["xpic_ctx*", "int", "double*", "double*"],
    "xpic_gauss_clean": ["xpic_ctx*", "int", "double", "double", "int", "double*", "int*", "double*"],
    "xpic_set_gauss_clean": ["xpic_ctx*", "int", "double", "double", "int"],
    "xpic_gauss_info": ["xpic_ctx*", "double*"],
}


def declared(monkeypatch):
    """include/xpic_gauss.h as abi_header's own parser reads a header"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(H.ROOT, "include", "xpic_gauss.h")).read(), flags=re.S)
    monkeypatch.setattr(H, "header", lambda: text)


def test_the_table_is_the_header(monkeypatch):
    import xpic_amd as X

    declared(monkeypatch)
    symbols, prototypes = H.symbols(), H.prototypes()
    assert symbols == sorted(LITERAL) == sorted(prototypes) == sorted(X.GAUSS_PROTOTYPES)
    for name in LITERAL:
        assert prototypes[name] == X.GAUSS_PROTOTYPES[name] == ("int", LITERAL[name]), name
        assert all(a in X.CTYPES for a in LITERAL[name]), name
        for table in (X.PROTOTYPES, X.LOAD_PROTOTYPES, X.TRACER_PROTOTYPES, X.TRACER_MOMENT_PROTOTYPES, X.FIELD_LINE_PROTOTYPES):
            assert name not in table, name
    assert H.structs() == []
    assert '#include "xpic_gauss.h"' in open(os.path.join(H.ROOT, "include", "xpic_hip.h")).read()
    # the header says what it must: the scratch vector, the extension, the slabs
    raw = open(os.path.join(H.ROOT, "include", "xpic_gauss.h")).read()
    assert "XPIC_W2" in raw and "unpinned on distinct ranks" in raw and "the reference has no Gauss-law cleaner" in raw


def test_library_exports_and_types_the_symbols():
    import xpic_amd as X

    lib = A.built_library()
    L = X.load_library()
    for name in LITERAL:
        assert hasattr(lib, name), name
        f = getattr(L, name)
        assert f.restype is C.c_int and list(f.argtypes) == [X.CTYPES[a] for a in LITERAL[name]], name
    for f in ("gauss_background", "gauss_residual", "gauss_clean", "set_gauss_clean", "gauss_info"):
        assert callable(getattr(X.Context, f)), f
    assert X.GaussClean._fields == ("iterations", "before", "after", "mean", "gphi", "phi")


def test_null_handle_sweep():
    """every method, in the forms of its optional arguments, on a context that was never created"""
    import xpic_amd as X

    A.built_library()
    ctx = object.__new__(X.Context)
    ctx.L, ctx.h = A.Recorder(X.load_library()), C.c_void_p(0)
    ctx.n, ctx.nzl = (3, 2, 2), 2
    refused = pytest.raises(X.XpicError, match=r"xpic error [1-9]\d*: .+")
    for rho in (None, np.ones((2, 2, 3))):
        with refused:
            ctx.gauss_background(rho)
    for field in (X.E, X.EP, X.W0):
        for want in (False, True):
            with refused:
                ctx.gauss_residual(field, want_residual=want)
            with refused:
                ctx.gauss_clean(field, rtol=1e-9, atol=1e-30, maxit=7, want_phi=want)
    with refused:
        ctx.gauss_clean()
    for every in (0, 2):
        with refused:
            ctx.set_gauss_clean(every, rtol=1e-8)
    with refused:
        ctx.gauss_info()
    assert ctx.L.seen >= set(LITERAL)
    ctx.h = None  # (nothing to destroy)
