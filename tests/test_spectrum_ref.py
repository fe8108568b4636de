"""The numpy restatement of the field spectra against itself (no GPU, no library): tests/spectrum_ref.py's route -- the
separable Hartley passes and the four-term identity -- against numpy.fft.fftn within the rounding bound, Parseval, the
bitwise symmetry P(k) == P(-k), the planted bugs at least 1e6 bounds away, the measured constant behind K_SPEC, and the tie
condition of every shape and edge set the device tests use."""
import numpy as np
import pytest

import spectrum_ref as S

EPS = S.EPS
CPU_SHAPES = ["2x3x5", "5x4x3", "1x4x6", "6x7x9", "18x17x20"]


@pytest.fixture(scope="module")
def inputs():
    return S.inputs()


@pytest.mark.parametrize("name", CPU_SHAPES)
def test_route_equals_fftn(inputs, name):
    n, d, x = inputs[name]
    ref = S.dft(x)
    f, p = S.fourier(x, n), S.power(x, n)
    p_ref = np.abs(ref) ** 2
    print(name, "|dF| / bound", np.abs(f - ref).max() / S.mode_bound(x), "|dP| / bound", (np.abs(p - p_ref) / S.power_bound(p_ref, x)).max())
    assert np.abs(f - ref).max() <= S.mode_bound(x)
    assert (np.abs(p - p_ref) <= S.power_bound(p_ref, x)).all()
    # Parseval, within N eps of the sum
    assert abs(p.sum() - (x ** 2).sum()) <= x.size * EPS * (x ** 2).sum()
    # P(k) == P(-k), the same bits
    rx, ry, rz = S.reflections(n)
    assert np.array_equal(p, p[np.ix_(rz, ry, rx)])
    hk, hm = S.route(x, n)
    assert np.array_equal(hm, hk[np.ix_(rz, ry, rx)])


def test_the_identity_at_5x4x7():
    """the issue's own check: 5x4x7 against fftn to 3e-15"""
    x = np.random.default_rng(1).normal(0.0, 1.0, (7, 4, 5))
    assert np.abs(S.fourier(x, (5, 4, 7)) - S.dft(x)).max() <= 3e-15


def test_axis_sums_and_shells_against_fftn(inputs):
    for name in CPU_SHAPES:
        n, d, x = inputs[name]
        p, p_ref = S.power(x, n), np.abs(S.dft(x)) ** 2
        bound = S.power_bound(p_ref, x)
        for a, b, c in zip(S.axis_sums(p), S.axis_sums(p_ref), S.axis_sums(bound)):
            assert (np.abs(a - b) <= c + x.size * EPS * b).all()
        for which in ("dk", "offset"):
            edges = S.shell_edges(n, d, which)
            sh, cnt, out, nout = S.shells(p, n, d, edges)
            sh_ref, cnt_ref, out_ref, nout_ref = S.shells(p_ref, n, d, edges)
            assert np.array_equal(cnt, cnt_ref) and nout == nout_ref and cnt.sum() + nout == x.size
            assert abs(sh.sum() + out - p.sum()) <= x.size * EPS * p.sum()
            # the shell rule against |k| itself, from the folded mode numbers
            kk = np.sqrt(sum(np.asarray(k).reshape(s) ** 2 for k, s in zip(
                [2 * np.pi * S.fold(n[a]) / (n[a] * d[a]) for a in range(3)], [(1, 1, -1), (1, -1, 1), (-1, 1, 1)])))
            for j in range(S.NSHELL):
                assert cnt[j] == int(((kk >= edges[j]) & (kk < edges[j + 1])).sum())
        assert nout > 0  # the offset set leaves mode 0 and the highest modes outside


@pytest.mark.parametrize("bug", ["plus_triple", "no_mod", "two_axes", "im_sign", "unfolded"])
def test_planted_bugs_lie_far_outside_the_bound(inputs, bug):
    """each on at least one input at least 1e6 bounds away"""
    worst = 0.0
    for name in CPU_SHAPES:
        n, d, x = inputs[name]
        if bug == "unfolded":
            p = S.power(x, n)
            edges = S.shell_edges(n, d, "dk")
            good, bad = S.shells(p, n, d, edges), S.shells(p, n, d, edges, mutate="unfolded")
            bound = S.power_bound(p, x).sum() + x.size * EPS * p.sum()
            worst = max(worst, np.abs(good[0] - bad[0]).max() / bound)
        elif bug == "im_sign":
            worst = max(worst, np.abs(S.fourier(x, n, mutate=bug) - S.dft(x)).max() / S.mode_bound(x))
        else:
            p_ref = np.abs(S.dft(x)) ** 2
            worst = max(worst, (np.abs(S.power(x, n, mutate=bug) - p_ref) / S.power_bound(p_ref, x)).max())
    print(bug, "bounds away:", worst)
    assert worst >= 1e6


def test_k_spec_is_what_was_measured():
    """K_SPEC = 8 x the largest float64-vs-long-double ratio over every input of the device tests"""
    df, dp = S.measure()
    assert max(df, dp) <= S.MEASURED_RATIO and max(df, dp) >= 0.98 * S.MEASURED_RATIO
    assert S.K_SPEC == 8 * S.MEASURED_RATIO


def test_no_mode_sits_on_a_shell_edge():
    """no s within a relative 1e-9 of a squared edge, on every shape and edge set of the device tests"""
    for name, (n, d) in dict(S.SHAPES, special=(S.SPECIAL_N, S.SPECIAL_D)).items():
        for which in ("dk", "offset"):
            m = S.tie_margin(n, d, S.shell_edges(n, d, which))
            assert m > 1e-9, (name, which, m)
