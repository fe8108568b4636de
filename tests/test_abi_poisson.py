"""The C boundary of the direct Poisson solve (no GPU): include/xpic_poisson.h against the package's POISSON_PROTOTYPES by
the rules tests/test_abi_es.py holds include/xpic_es.h to -- the table is the header's, the library exports the symbols,
load_library() types them, every method passes its typed prototype down to the library's own refusal of a null context --
and enum xpic_poisson_solver and the cap against the package's POISSON_SOLVERS and POISSON_MAX_EXTENT."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import abi_header as H
import test_abi as A

LITERAL = {
    "xpic_set_poisson_solver": ["xpic_ctx*", "int"],
    "xpic_get_poisson_solver": ["xpic_ctx*", "int*"],
    "xpic_poisson_apply": ["xpic_ctx*", "const double*", "double*"],
    "xpic_poisson_solve": ["xpic_ctx*", "const double*", "double", "int", "double*", "int*", "double*"],
}


def declared(monkeypatch):
    """include/xpic_poisson.h as abi_header's own parser reads a header"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(H.ROOT, "include", "xpic_poisson.h")).read(), flags=re.S)
    monkeypatch.setattr(H, "header", lambda: text)


def test_the_table_is_the_header(monkeypatch):
    import xpic_amd as X

    declared(monkeypatch)
    symbols, prototypes = H.symbols(), H.prototypes()
    assert symbols == sorted(LITERAL) == sorted(prototypes) == sorted(X.POISSON_PROTOTYPES)
    for name in LITERAL:
        assert prototypes[name] == X.POISSON_PROTOTYPES[name] == ("int", LITERAL[name]), name
        assert all(a in X.CTYPES for a in LITERAL[name]), name
        for table in (X.PROTOTYPES, X.LOAD_PROTOTYPES, X.TRACER_PROTOTYPES, X.TRACER_MOMENT_PROTOTYPES, X.FIELD_LINE_PROTOTYPES,
                      X.GAUSS_PROTOTYPES, X.ES_PROTOTYPES):
            assert name not in table, name
    assert H.structs() == []
    assert H.enum("xpic_poisson_solver") == {"XPIC_POISSON_CG": 0, "XPIC_POISSON_DIRECT": 1}
    assert X.POISSON_SOLVERS == {"cg": 0, "direct": 1}
    assert H.macro("XPIC_POISSON_MAX_EXTENT") == X.POISSON_MAX_EXTENT == 1024
    assert '#include "xpic_poisson.h"' in open(os.path.join(H.ROOT, "include", "xpic_hip.h")).read()
    # the header says what it must: the formula, the tables, the count's meaning, the refusals, the extension
    raw = " ".join(open(os.path.join(H.ROOT, "include", "xpic_poisson.h")).read().replace(" * ", " ").split())
    for words in ("H_n[k][j] = (cos(2 pi k j / n) + sin(2 pi k j / n)) / sqrt(n)", "lam_a[k] = -4 sin^2(pi k / n_a) / d_a^2",
                  "the library builds H_n per distinct extent", "in long double, k j reduced modulo n in integers",
                  "counts the applications", "single-slab contexts only", "XPIC_POISSON_MAX_EXTENT = 1024",
                  "the reference has no such solver"):
        assert words in raw, words


def test_the_makefile_builds_and_tracks_it():
    mk = open(os.path.join(H.ROOT, "Makefile")).read()
    assert "$(CSRC)/poisson.hip" in mk.split("SRCS :=")[1].splitlines()[0]
    assert mk.count("include/xpic_poisson.h") == 2  # HDRS and the host executable's dependencies
    assert "-lrccl -Wl" in mk and mk.count(" -l") == 2  # the link lines: rccl for the library, the library for the host mirror


def test_library_exports_and_types_the_symbols():
    import xpic_amd as X

    lib = A.built_library()
    L = X.load_library()
    for name in LITERAL:
        assert hasattr(lib, name), name
        f = getattr(L, name)
        assert f.restype is C.c_int and list(f.argtypes) == [X.CTYPES[a] for a in LITERAL[name]], name
    for f in ("set_poisson_solver", "poisson_apply", "poisson_solve"):
        assert callable(getattr(X.Context, f)), f
    assert isinstance(X.Context.poisson_solver, property)


def test_null_handle_sweep():
    import xpic_amd as X

    A.built_library()
    ctx = object.__new__(X.Context)
    ctx.L, ctx.h = A.Recorder(X.load_library()), C.c_void_p(0)
    ctx.n, ctx.nzl = (3, 2, 2), 2
    refused = pytest.raises(X.XpicError, match=r"xpic error [1-9]\d*: .+")
    for kind in ("cg", "direct", 1):
        with refused:
            ctx.set_poisson_solver(kind)
    with refused:
        ctx.poisson_solver
    with refused:
        ctx.poisson_apply(np.ones((2, 2, 3)))
    with refused:
        ctx.poisson_solve(np.ones((2, 2, 3)), tol=0.0, maxit=2)
    with pytest.raises(X.XpicError, match="none of"):  # (the package's own refusal of a name it does not know)
        ctx.set_poisson_solver("fft")
    assert ctx.L.seen >= set(LITERAL)
    ctx.h = None  # (nothing to destroy)
