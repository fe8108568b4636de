"""The C boundary of SetParticles on the device (no GPU): include/xpic_set_particles.h against the package's
LOAD_PROTOTYPES by the rules tests/test_abi.py holds include/xpic_hip.h and PROTOTYPES to -- the table is the header's, the
library exports the symbols, load_library() types them, the struct mirror has the header's layout, the enumerators are the
package's numbers, and both methods pass their typed prototypes down to the library's own refusal of a null context."""
import ctypes as C
import os
import re

import pytest

import abi_header as H
import test_abi as A

NAMES = ("xpic_set_particles", "xpic_particles_number")
LITERAL = {
    "xpic_set_particles": ["xpic_ctx*", "int", "const xpic_set_particles_params*", "int64_t", "int64_t", "int64_t", "int64_t*",
                           "double*"],
    "xpic_particles_number": ["xpic_ctx*", "int", "int", "const double*", "int64_t*"],
}


def declared(monkeypatch):
    """(symbols, prototypes) of include/xpic_set_particles.h, read by abi_header's own parser"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(H.ROOT, "include", "xpic_set_particles.h")).read(), flags=re.S)
    monkeypatch.setattr(H, "header", lambda: text)
    return H.symbols(), H.prototypes()


def test_the_table_is_the_header(monkeypatch):
    import xpic_amd as X

    symbols, prototypes = declared(monkeypatch)
    assert symbols == sorted(NAMES) == sorted(prototypes) == sorted(X.LOAD_PROTOTYPES)
    for name in NAMES:
        assert prototypes[name] == X.LOAD_PROTOTYPES[name] == ("int", LITERAL[name]), name
        assert all(a in X.CTYPES for a in LITERAL[name]), name
        assert name not in X.PROTOTYPES
    assert '#include "xpic_set_particles.h"' in open(os.path.join(H.ROOT, "include", "xpic_hip.h")).read()


def test_library_exports_and_types_the_symbols():
    import xpic_amd as X

    lib = A.built_library()
    L = X.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name
        f = getattr(L, name)
        assert f.restype is C.c_int and list(f.argtypes) == [X.CTYPES[a] for a in LITERAL[name]], name
    assert L.xpic_set_particles.argtypes[2] is C.POINTER(X.SetParticlesParams)
    for f in ("set_particles", "particles_number"):
        assert callable(getattr(X.Context, f)), f


def test_struct_mirror_and_constants():
    import xpic_amd as X

    name = "xpic_set_particles_params"
    assert H.struct_fields(name) == [
        "int32_t coordinate", "int32_t momentum", "int32_t tov", "int32_t reserved", "double geom[7]", "double value[3]",
        "double T[3]", "double amplitude[3]", "double wave_number[3]", "double box6[6]", "double center[3]", "uint64_t seed",
        "int64_t chunk"]
    mirror = X.MIRRORS[name]
    assert mirror is X.SetParticlesParams and [f[0] for f in mirror._fields_] == H.member_names(name)
    assert [getattr(mirror, n).offset for n in H.member_names(name)] == [0, 4, 8, 12, 16, 72, 96, 120, 144, 168, 216, 240, 248]
    assert C.sizeof(mirror) == 256
    # the new enumerators follow the old ones, which keep their numbers
    assert H.enum("xpic_coordinate_kind") == {"XPIC_COORD_PRECISE": 0, "XPIC_COORD_IN_BOX": 1, "XPIC_COORD_IN_CYLINDER": 2,
                                              "XPIC_COORD_ON_ANNULUS": 3}
    assert H.enum("xpic_momentum_kind") == {"XPIC_MOMENTUM_PRECISE": 0, "XPIC_MOMENTUM_MAXWELLIAN": 1,
                                            "XPIC_MOMENTUM_COSINE_PERTURBATION": 2, "XPIC_MOMENTUM_ANGULAR": 3}
    assert X.COORDINATES == {"PreciseCoordinate": 0, "CoordinateInBox": 1, "CoordinateInCylinder": 2, "CoordinateOnAnnulus": 3}
    assert X.MOMENTA == {"PreciseMomentum": 0, "MaxwellianMomentum": 1, "MaxwellCosinePerturbation": 2, "AngularMomentum": 3}
    assert H.macro("XPIC_SET_PARTICLES_CHUNK") == X.SET_PARTICLES_CHUNK == 1 << 24
    # the structs inject_particles takes are as they were
    assert C.sizeof(X.InjectParams) == 8 + 56 + 2 * 56 + 8 and C.sizeof(X.MomentumParams) == 56


def test_null_handle_sweep():
    """both methods, in every dict form they take, on a context that was never created"""
    import xpic_amd as X

    A.built_library()
    ctx = object.__new__(X.Context)
    ctx.L, ctx.h = A.Recorder(X.load_library()), C.c_void_p(0)
    box = {"name": "CoordinateInBox", "min": (0.0, 0.0, 0.0), "max": (4.0, 4.0, 4.0)}
    cyl = {"name": "CoordinateInCylinder", "center": (2.0, 2.0, 2.0), "radius": 1.5, "height": 3.0}
    ann = {"name": "CoordinateOnAnnulus", "center": (2.0, 2.0, 2.0), "inner_r": 0.5, "outer_r": 1.5, "height": 3.0}
    point = {"name": "PreciseCoordinate", "value": (1.0, 1.0, 1.0)}
    momenta = [{"name": "PreciseMomentum", "value": (0.1, 0.0, 0.0)},
               {"name": "MaxwellianMomentum", "T": (1.0, 1.0, 1.0), "tov": True},
               {"name": "MaxwellCosinePerturbation", "T": (1.0, 1.0, 1.0), "amplitude": (0.1, 0, 0), "wave_number": (1, 0, 0),
                "min": (0, 0, 0), "max": (4, 4, 4)},
               {"name": "AngularMomentum", "T": (1.0, 1.0, 1.0), "drift": (0.1, 0.1, 0), "center": (2, 2, 0)}]
    for coord in (box, cyl, ann, point):
        with pytest.raises(X.XpicError, match=r"xpic error [1-9]\d*: .+"):
            ctx.particles_number(0, coord)
        for mom in momenta:
            for kwargs in ({}, dict(step=1 << 40, seed=(1 << 64) - 1, particle0=1 << 40, chunk=64)):
                with pytest.raises(X.XpicError, match=r"xpic error [1-9]\d*: .+"):
                    ctx.set_particles(0, 3, coord, mom, **kwargs)
    assert ctx.L.seen >= set(NAMES)
    ctx.h = None  # (nothing to destroy)
