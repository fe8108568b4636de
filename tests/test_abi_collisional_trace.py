"""The C boundary of the collisional traces, under the test names it has had since the feature.  What is asserted -- the
argument lists, the model traces' lists plus the two collision arguments, the exports, the layouts of
xpic_trace_background and xpic_trace_collisions, the builder -- is written once, in tests/test_abi.py."""
import abi_header as H
import test_abi as A
from test_abi import test_trace_collisions_builder as test_the_builder  # noqa: F401

NAMES = ("xpic_model_full_orbit_trace_collisional", "xpic_model_drift_kinetic_trace_collisional")


def test_prototypes_match_the_header():
    A.check_prototypes(NAMES)


def test_library_exports_the_new_symbols():
    import xpic_amd

    A.check_listed_and_exported(NAMES, ("model_full_orbit_trace_collisional", "model_drift_kinetic_trace_collisional"))
    assert callable(xpic_amd.trace_collisions)


def test_struct_layouts_and_the_constant():
    import xpic_amd

    assert H.macro("XPIC_TRACE_BG_MAX") == xpic_amd.TRACE_BG_MAX == 4
    A.check_layouts(("xpic_trace_background", "xpic_trace_collisions"))
