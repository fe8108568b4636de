"""The C boundary of the field spectra (no GPU): include/xpic_spectrum.h against the package's SPECTRUM_PROTOTYPES by the rules
tests/test_abi_poisson.py holds include/xpic_poisson.h to -- the table is the header's, the Makefile builds and tracks the
source and the header, the library exports the symbols, load_library() types them, every method passes its typed prototype
down to the library's own refusal of a null context -- and enum xpic_spectrum_source and the caps against the package's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import abi_header as H
import test_abi as A

_SOURCE = ["xpic_ctx*", "int", "int", "const double*"]
LITERAL = {
    "xpic_spectrum_power": _SOURCE + ["double*"],
    "xpic_spectrum": _SOURCE + ["double*", "double*", "double*", "int", "const double*", "double*", "int64_t*", "double*", "double*"],
    "xpic_spectrum_modes": _SOURCE + ["int", "const int32_t*", "double*"],
    "xpic_spectrum_probe_create": ["xpic_ctx*", "int", "int", "int", "const int32_t*", "int", "int64_t", "int*"],
    "xpic_spectrum_probe_get": ["xpic_ctx*", "int", "int64_t", "int64_t*", "double*", "int64_t*", "int64_t*", "int"],
    "xpic_spectrum_probe_destroy": ["xpic_ctx*", "int"],
}


def declared(monkeypatch):
    """include/xpic_spectrum.h as abi_header's own parser reads a header"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(H.ROOT, "include", "xpic_spectrum.h")).read(), flags=re.S)
    monkeypatch.setattr(H, "header", lambda: text)


def test_the_table_is_the_header(monkeypatch):
    import xpic_amd as X

    declared(monkeypatch)
    symbols, prototypes = H.symbols(), H.prototypes()
    assert symbols == sorted(LITERAL) == sorted(prototypes) == sorted(X.SPECTRUM_PROTOTYPES)
    for name in LITERAL:
        assert prototypes[name] == X.SPECTRUM_PROTOTYPES[name] == ("int", LITERAL[name]), name
        assert all(a in X.CTYPES for a in LITERAL[name]), name
        for table in (X.PROTOTYPES, X.LOAD_PROTOTYPES, X.TRACER_PROTOTYPES, X.TRACER_MOMENT_PROTOTYPES, X.FIELD_LINE_PROTOTYPES,
                      X.GAUSS_PROTOTYPES, X.ES_PROTOTYPES, X.POISSON_PROTOTYPES):
            assert name not in table, name
    assert H.structs() == []
    assert H.enum("xpic_spectrum_source") == {"XPIC_SPECTRUM_HOST": 100, "XPIC_SPECTRUM_RHO": 101}
    assert X.SPECTRUM_SOURCES == {"host": 100, "rho": 101}
    assert min(X.SPECTRUM_SOURCES.values()) > max(X.E, X.B, X.W2)  # no field id is a special source
    assert H.macro("XPIC_SPECTRUM_MAX_SHELLS") == X.SPECTRUM_MAX_SHELLS == 2048
    assert H.macro("XPIC_SPECTRUM_MAX_PROBES") == X.SPECTRUM_MAX_PROBES == 16
    assert '#include "xpic_spectrum.h"' in open(os.path.join(H.ROOT, "include", "xpic_hip.h")).read()
    # the header says what it must: the identity, the stagger, the shell rule, the order of the riders, the extension
    raw = " ".join(open(os.path.join(H.ROOT, "include", "xpic_spectrum.h")).read().replace(" * ", " ").split())
    for words in ("H(k) = 1/2 [ T(r_x k) + T(r_y k) + T(r_z k) - T(r_xyz k) ]", "P(k) = |F^(k)|^2 = (H(k)^2 + H(-k)^2) / 2",
                  "the Yee stagger is not applied", "s = kx2[x] + ky2[y] + kz2[z]", "edges2[j] <= s < edges2[j+1]",
                  "then the attached tracer sets, then the probes in creation order", "XPIC_SPECTRUM_HOST is not a probe source",
                  "the reference has no spectral diagnostic"):
        assert words in raw, words


def test_the_makefile_builds_and_tracks_it():
    mk = open(os.path.join(H.ROOT, "Makefile")).read()
    assert "$(CSRC)/spectrum.hip" in mk.split("SRCS :=")[1].splitlines()[0]
    assert mk.count("include/xpic_spectrum.h") == 2  # HDRS and the host executable's dependencies
    assert "-lrccl -Wl" in mk and mk.count(" -l") == 2  # the link lines are as they were


def test_library_exports_and_types_the_symbols():
    import xpic_amd as X

    lib = A.built_library()
    L = X.load_library()
    for name in LITERAL:
        assert hasattr(lib, name), name
        f = getattr(L, name)
        assert f.restype is C.c_int and list(f.argtypes) == [X.CTYPES[a] for a in LITERAL[name]], name
    for f in ("spectrum_power", "spectrum", "spectrum_modes", "spectrum_probe"):
        assert callable(getattr(X.Context, f)), f
    for f in ("get", "close"):
        assert callable(getattr(X.SpectrumProbe, f)), f


def test_null_handle_sweep():
    import xpic_amd as X

    A.built_library()
    ctx = object.__new__(X.Context)
    ctx.L, ctx.h = A.Recorder(X.load_library()), C.c_void_p(0)
    ctx.n, ctx.nzl, ctx.d = (3, 2, 2), 2, (0.5, 0.5, 0.5)
    refused = pytest.raises(X.XpicError, match=r"xpic error [1-9]\d*: .+")
    x = np.ones((2, 2, 3))
    for source, comp in ((x, None), ("rho", None), (X.E, 1)):
        with refused:
            ctx.spectrum_power(source, comp)
        with refused:
            ctx.spectrum(source, comp, dk=0.5, nshell=3)
        with refused:
            ctx.spectrum_modes(source, [(1, 0, 0)], comp)
    with refused:
        ctx.spectrum_probe(X.E, [(1, 0, 0)], comp=0)
    probe = X.SpectrumProbe(ctx, 0, 1)
    with refused:
        probe.get()
    with refused:
        probe.close()
    # the package's own refusals: a name that is no source, a field without its component, an array as a probe source
    with pytest.raises(X.XpicError, match="no source"):
        ctx.spectrum_power("phi")
    with pytest.raises(X.XpicError, match="needs comp"):
        ctx.spectrum_power(X.E)
    with pytest.raises(X.XpicError, match="no probe source"):
        ctx.spectrum_probe(x, [(1, 0, 0)])
    assert ctx.L.seen >= set(LITERAL)
    ctx.h = None  # (nothing to destroy)
