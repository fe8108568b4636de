"""The C boundary of the electrostatic scheme (no GPU): include/xpic_es.h against the package's ES_PROTOTYPES by the rules
tests/test_abi_gauss.py holds include/xpic_gauss.h to -- the table is the header's, the library exports the symbol,
load_library() types it, the method passes its typed prototype down to the library's own refusal of a null context --
and XPIC_ES in enum xpic_scheme against the package's SCHEMES."""
import ctypes as C
import os
import re

import pytest

import abi_header as H
import test_abi as A

LITERAL = {"xpic_es_push": ["xpic_ctx*", "int", "double*"]}


def declared(monkeypatch):
    """include/xpic_es.h as abi_header's own parser reads a header"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(H.ROOT, "include", "xpic_es.h")).read(), flags=re.S)
    monkeypatch.setattr(H, "header", lambda: text)


def test_the_scheme_is_in_the_enum():
    import xpic_amd as X

    assert H.enum("xpic_scheme") == {"XPIC_BASIC": 0, "XPIC_ECSIM": 1, "XPIC_ECSIMCORR": 2, "XPIC_ES": 3}
    assert X.SCHEMES == {"basic": 0, "ecsim": 1, "ecsimcorr": 2, "es": 3} and X.ES == 3


def test_the_table_is_the_header(monkeypatch):
    import xpic_amd as X

    declared(monkeypatch)
    symbols, prototypes = H.symbols(), H.prototypes()
    assert symbols == sorted(LITERAL) == sorted(prototypes) == sorted(X.ES_PROTOTYPES)
    for name in LITERAL:
        assert prototypes[name] == X.ES_PROTOTYPES[name] == ("int", LITERAL[name]), name
        assert all(a in X.CTYPES for a in LITERAL[name]), name
        for table in (X.PROTOTYPES, X.LOAD_PROTOTYPES, X.TRACER_PROTOTYPES, X.TRACER_MOMENT_PROTOTYPES, X.FIELD_LINE_PROTOTYPES,
                      X.GAUSS_PROTOTYPES):
            assert name not in table, name
    assert H.structs() == []
    assert '#include "xpic_es.h"' in open(os.path.join(H.ROOT, "include", "xpic_hip.h")).read()
    # the header says what it must: the staggering, the defaults, the refusals, the extension
    raw = open(os.path.join(H.ROOT, "include", "xpic_es.h")).read()
    for words in ("v^{n-1/2}", "rtol = 1e-10, atol = 1e-14, maxit = 10000", "xpic_set_gauss_clean", "at least 6 cells",
                  "the reference has no electrostatic scheme", "unpinned"):
        assert words in raw, words
    assert (X.ES_RTOL, X.ES_ATOL, X.ES_MAXIT) == (1e-10, 1e-14, 10000)


def test_library_exports_and_types_the_symbol():
    import xpic_amd as X

    lib = A.built_library()
    L = X.load_library()
    for name in LITERAL:
        assert hasattr(lib, name), name
        f = getattr(L, name)
        assert f.restype is C.c_int and list(f.argtypes) == [X.CTYPES[a] for a in LITERAL[name]], name
    assert callable(X.Context.es_push)


def test_null_handle():
    import xpic_amd as X

    A.built_library()
    ctx = object.__new__(X.Context)
    ctx.L, ctx.h = A.Recorder(X.load_library()), C.c_void_p(0)
    ctx.n, ctx.nzl = (6, 6, 6), 6
    with pytest.raises(X.XpicError, match=r"xpic error [1-9]\d*: .+"):
        ctx.es_push(0)
    assert ctx.L.seen >= set(LITERAL)
    ctx.h = None  # (nothing to destroy)
