"""The C boundary of the collisional grid traces and the background profiles, under the test names it has had since the
feature.  What is asserted -- the argument lists, the open grid traces' lists plus the three collision arguments, the
exports and methods, the header's text -- is written once, in tests/test_abi.py."""
import test_abi as A
from test_abi import test_the_header_says_what_is_there  # noqa: F401

NAMES = ("xpic_background_set", "xpic_background_get", "xpic_background_clear", "xpic_background_from_sort",
         "xpic_full_orbit_trace_collisional", "xpic_drift_kinetic_trace_collisional")


def test_prototypes_match_the_header():
    A.check_prototypes(NAMES)


def test_library_exports_the_new_symbols():
    A.check_listed_and_exported(NAMES, ("background_set", "background_get", "background_clear", "background_from_sort",
                                        "full_orbit_trace_collisional", "drift_kinetic_trace_collisional"))
