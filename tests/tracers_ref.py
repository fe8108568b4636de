"""numpy statement of xpic_grad_abs_field (include/xpic_tracers.h): grad |B| on the nodes by central differences, every
index wrapped, with one spacing per axis.  open_trace_ref.grad_abs is the same statement for unit spacings.

  grad_abs(B, d)              the statement the device kernel must return bit for bit
  grad_abs_bugged(B, d, bug)  the same with one planted bug, for tests/test_tracers_ref.py: each must be visible to the
                              comparison the device test makes
"""
import numpy as np

BUGS = ("one_sided", "no_wrap", "wrong_axis_spacing", "abs_after_difference")


def abs_field(B):
    """|B| of an (nz, ny, nx, 3) array, summed in the kernel's order: (Bx Bx + By By) + Bz Bz"""
    B = np.asarray(B, dtype=np.float64)
    return np.sqrt((B[..., 0] * B[..., 0] + B[..., 1] * B[..., 1]) + B[..., 2] * B[..., 2])


def grad_abs(B, d):
    """g[z, y, x, c] = (|B|(node + e_c) - |B|(node - e_c)) / (2 d[c]); component c runs along array axis 2 - c"""
    lB = abs_field(B)
    g = np.zeros(lB.shape + (3,))
    for c, axis in enumerate((2, 1, 0)):
        g[..., c] = (np.roll(lB, -1, axis=axis) - np.roll(lB, 1, axis=axis)) / (2.0 * float(d[c]))
    return g


def grad_abs_bugged(B, d, bug):
    B = np.asarray(B, dtype=np.float64)
    lB = abs_field(B)
    g = np.zeros(lB.shape + (3,))
    for c, axis in enumerate((2, 1, 0)):
        up, down = np.roll(lB, -1, axis=axis), np.roll(lB, 1, axis=axis)
        h = 2.0 * float(d[c])
        if bug == "one_sided":
            down, h = lB, float(d[c])
        elif bug == "no_wrap":  # the neighbour beyond an edge is the edge node itself
            n = lB.shape[axis]
            idx = np.arange(n)
            up = np.take(lB, np.minimum(idx + 1, n - 1), axis=axis)
            down = np.take(lB, np.maximum(idx - 1, 0), axis=axis)
        elif bug == "wrong_axis_spacing":
            h = 2.0 * float(d[(c + 1) % 3])
        elif bug == "abs_after_difference":
            diff = (np.roll(B, -1, axis=axis) - np.roll(B, 1, axis=axis)) / h
            g[..., c] = abs_field(diff)
            continue
        elif bug is not None:
            raise ValueError(bug)
        g[..., c] = (up - down) / h
    return g
