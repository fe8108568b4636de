"""xpic_set_mirror_field against SetApproximateMirrorField::operator() (src/commands/set_magnetic_field.cpp:142-191)
restated here node by node, as written: B0(z, s) = I R^2 / 2 / (R^2 + (z + s D / 2)^2)^1.5 and B1(z, s) = (z + s D / 2) /
(R^2 + (z + s D / 2)^2) for s = +1, -1; both transverse terms, B0 B1 1.5 (x dx - geom_x / 2) and B0 B1 1.5 (y dy -
geom_y / 2) at (z + 1/2) dz, go to the X component, nothing to Y, B0 at z dz to Z.  The comparison and its tolerance are
those of test_coils_matches_ref in tests/test_gpu_commands.py."""
import math

import numpy as np
import pytest

import open_trace_ref as O

pytestmark = pytest.mark.gpu


def get_B0(z, sign, D, R, I):
    return 0.5 * I * (R * R) / math.pow(R * R + (z + 0.5 * sign * D) ** 2, 1.5)


def get_B1(z, sign, D, R):
    return (z + 0.5 * sign * D) / (R * R + (z + 0.5 * sign * D) ** 2)


def mirror_ref(n, d, D, R, I):
    out = np.zeros((n[2], n[1], n[0], 3))
    geom_x, geom_y = n[0] * d[0], n[1] * d[1]
    for z in range(n[2]):
        for y in range(n[1]):
            for x in range(n[0]):
                a = out[z, y, x]
                sz = (z + 0.5) * d[2]
                sm = 1.5 * (x * d[0] - 0.5 * geom_x)
                a[0] += get_B0(sz, +1.0, D, R, I) * sm * get_B1(sz, +1.0, D, R)
                a[0] += get_B0(sz, -1.0, D, R, I) * sm * get_B1(sz, -1.0, D, R)
                sz = (z + 0.5) * d[2]
                sm = 1.5 * (y * d[1] - 0.5 * geom_y)
                a[0] += get_B0(sz, +1.0, D, R, I) * sm * get_B1(sz, +1.0, D, R)
                a[0] += get_B0(sz, -1.0, D, R, I) * sm * get_B1(sz, -1.0, D, R)
                sz = z * d[2]
                a[2] += get_B0(sz, +1.0, D, R, I)
                a[2] += get_B0(sz, -1.0, D, R, I)
    return out


@pytest.mark.parametrize("n,d,coil", [((8, 8, 8), (1.0, 1.0, 1.0), (8.0, 3.0, 2.0)),
                                      ((6, 8, 10), (0.5, 0.4, 0.75), (5.0, 1.3, -0.7))], ids=["cubic", "6x8x10"])
def test_mirror_matches_ref(n, d, coil):
    import xpic_amd as X

    D, R, I = coil
    g = X.Context("ecsim", n, d, 0.7)
    base = np.random.default_rng(5).normal(size=g.fshape())
    g.set_field(X.B0, base)
    g.set_mirror_field(D, R, I)  # into B0, its default, ADDED to what the vector held
    add = mirror_ref(n, d, D, R, I)
    ref = base + add
    got = g.get_field(X.B0)
    assert np.isfinite(ref).all()
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.array_equal(got[..., 1], base[..., 1])  # the Y component is not touched
    # what was added, on its own scale (the base is O(1), the field may be smaller)
    assert np.abs((got - base) - add).max() <= 1e-12 * np.abs(ref).max()
    assert np.abs(add[..., 0]).max() > 0 and np.abs(add[..., 2]).min() > 0
    # a second call adds again; another vector is addressed by its id
    g.set_mirror_field(D, R, I)
    assert np.abs(g.get_field(X.B0) - (base + 2 * add)).max() <= 1e-12 * np.abs(ref).max()
    g.set_field(X.B, np.zeros(g.fshape()))
    g.set_mirror_field(D, R, I, field=X.B)
    assert np.abs(g.get_field(X.B) - add).max() <= 1e-12 * np.abs(add).max()
    # the vectorised restatement the trace tests build their field from says the same
    assert np.abs(O.mirror_field(n, d, D, R, I) - add).max() <= 1e-14 * np.abs(add).max()


def test_mirror_argument_checks():
    import xpic_amd as X

    g = X.Context("ecsim", (8, 8, 8), (1.0, 1.0, 1.0), 0.7)
    with pytest.raises(X.XpicError):
        g.set_mirror_field(8.0, 3.0, 2.0, field=99)
