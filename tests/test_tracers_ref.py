"""tracers_ref.grad_abs is a gradient (an analytic |B| on a fine grid), it is open_trace_ref.grad_abs at unit spacings, and
each bug the device test (tests/test_gpu_tracers.py) is there to catch changes the result on that test's own grids."""
import numpy as np
import pytest

import open_trace_ref as O
import tracers_ref as T


def periodic_field(n, d):
    """B = (a(x) sin, ...) with |B| = 2 + sin(kx x) cos(ky y) + 0.5 sin(kz z), periodic in the box: B = |B| (0.6, 0, 0.8)"""
    L = [n[a] * d[a] for a in range(3)]
    z, y, x = np.meshgrid(*(np.arange(n[a]) * d[a] for a in (2, 1, 0)), indexing="ij")
    k = [2 * np.pi / L[a] for a in range(3)]
    mag = 2.0 + np.sin(k[0] * x) * np.cos(k[1] * y) + 0.5 * np.sin(k[2] * z)
    grad = np.stack([k[0] * np.cos(k[0] * x) * np.cos(k[1] * y), -k[1] * np.sin(k[0] * x) * np.sin(k[1] * y),
                     0.5 * k[2] * np.cos(k[2] * z)], axis=-1)
    return mag[..., None] * np.array([0.6, 0.0, 0.8]), grad


def test_it_is_a_gradient():
    """central differences of a smooth periodic |B|: the error is (k h)^2 / 6 of the derivative's amplitude"""
    n, d = (64, 48, 40), (0.05, 0.1, 0.2)
    B, grad = periodic_field(n, d)
    g = T.grad_abs(B, d)
    for c in range(3):
        kh = 2 * np.pi / n[c]
        assert np.abs(g[..., c] - grad[..., c]).max() <= 1.01 * (kh * kh / 6.0) * np.abs(grad[..., c]).max() + 1e-12, c
    assert np.abs(g).max() > 0.1


def test_unit_spacings_are_the_open_trace_fixture():
    _, B, gB = O.fields()
    assert np.array_equal(T.grad_abs(B, O.D), gB) and np.array_equal(T.grad_abs(B, O.D), O.grad_abs(B))


def test_folded_axes_are_exactly_zero():
    rng = np.random.default_rng(5)
    B = rng.normal(size=(3, 2, 2, 3))
    g = T.grad_abs(B, (0.5, 0.25, 2.0))
    assert np.all(g[..., 0] == 0.0) and np.all(g[..., 1] == 0.0) and np.abs(g[..., 2]).min() > 0.0


# the grids of the device test: 8 x 6 x 5 nodes with three spacings, and 2 x 2 x 3
@pytest.mark.parametrize("bug", T.BUGS)
def test_planted_bugs_are_visible(bug):
    rng = np.random.default_rng(11)
    n, d = (8, 6, 5), (0.5, 0.25, 2.0)
    B = rng.normal(size=(n[2], n[1], n[0], 3)) + np.array([0.0, 0.0, 3.0])
    good, bad = T.grad_abs(B, d), T.grad_abs_bugged(B, d, bug)
    assert np.array_equal(T.grad_abs_bugged(B, d, None), good)
    for c in range(3):  # every component of the result shows it: the device test compares all three bit for bit
        assert not np.array_equal(good[..., c], bad[..., c]), (bug, c)
    if bug == "no_wrap":  # and it shows only on the faces: the interior is right
        assert np.array_equal(good[1:-1, 1:-1, 1:-1], bad[1:-1, 1:-1, 1:-1])
