"""CPU checks of tests/open_trace_ref.py, which tests/test_gpu_open_trace.py takes its inputs and its rule from: run around
the numpy pushers (full_orbit_ref, drift_kinetic_ref), the restated open trace splits the test batch into the three
groups the GPU tests count on -- removed within the first launch, removed later, never removed -- and composes: 150
steps are 70 steps followed by 80 with step0 = 70 and the first call's exit_step."""
import numpy as np
import pytest

import commands_ref as C
import open_trace_ref as O

KINDS = ["EB2B", "CN", "dk"]


@pytest.fixture(scope="module")
def fields():
    return O.fields()


@pytest.fixture(scope="module", params=KINDS)
def run(request, fields):
    kind = request.param
    E, B, gB = fields
    p = O.particles("dk" if kind == "dk" else "fo", B)
    push = O.numpy_push(kind, E, B, gB)
    return kind, p, push, O.trace_open(push, p, O.STEPS, O.REGION, O.D, sample_every=O.EVERY)


def test_field_is_never_zero(fields):
    _, B, gB = fields
    assert np.sqrt((B * B).sum(axis=-1)).min() >= 1.0  # the mirror part only adds to Bz
    assert np.ptp(B[..., 2]) > 0.2 and np.abs(gB).max() > 0.05  # and it is not uniform


def test_three_groups(run):
    kind, p, _, full = run
    first, later, never = O.groups(full.exit_step)
    print(kind, "removed within 64 steps:", first, "later:", later, "never:", never)
    assert first + later + never == O.NPART == len(p)
    assert min(first, later, never) >= O.NPART // 5
    assert full.removed == first + later
    # every particle starts inside, so nobody is removed before taking a step
    assert full.exit_step[full.exit_step >= 0].min() >= 1 and full.exit_step.max() < O.STEPS
    # fewer than half are alive after the second launch, more than half after the first: the default policy compacts once
    assert O.compactions(full.exit_step, O.STEPS, 0) == 1 and O.compactions(full.exit_step, O.STEPS, 2) == 2
    assert O.compactions(full.exit_step, O.STEPS, 1) == 0
    taken = np.where(full.exit_step < 0, O.STEPS, full.exit_step)
    if kind == "CN":
        assert np.array_equal(full.iterations_sum, 3 * taken) and (full.iterations_max == 3).all()
    if kind == "dk":
        assert full.iterations_max.max() < 30 and (full.iterations_sum >= taken).all()  # every step converged


def test_samples_and_alive(run):
    _, p, _, full = run
    assert full.samples.shape == (O.STEPS // O.EVERY, O.NPART, 6)
    ex = full.exit_step
    for k in range(full.samples.shape[0]):
        step = (k + 1) * O.EVERY
        assert full.alive[k] == ((ex < 0) | (ex >= step)).sum()
        frozen = (ex >= 0) & (ex < step)  # removed at the top of step ex + 1 <= step
        assert np.array_equal(full.samples[k][frozen], full.state[frozen])
    assert full.alive[-1] >= O.groups(ex)[2]
    # a removed particle's cell is one of the two planes outside the region, and it was not there one step earlier
    gone = ex >= 0
    cz = O.corner(full.state[gone, :3], O.D)[:, 2]
    assert np.isin(cz, (0.0, 7.0)).all()
    assert O.keep(O.REGION, full.state[~gone, :3], O.D).sum() >= (~gone).sum() - 1  # (the final state is not tested)


def test_composition(run):
    _, p, push, full = run
    a = O.trace_open(push, p, O.SPLIT, O.REGION, O.D, sample_every=O.EVERY)
    b = O.trace_open(push, a.state, O.STEPS - O.SPLIT, O.REGION, O.D, sample_every=O.EVERY, exit_step=a.exit_step,
                     step0=O.SPLIT)
    assert np.array_equal(b.state, full.state) and np.array_equal(b.exit_step, full.exit_step)
    assert np.array_equal(np.concatenate([a.samples, b.samples]), full.samples)
    assert np.array_equal(np.concatenate([a.alive, b.alive]), full.alive)
    assert a.removed + b.removed == full.removed
    assert np.array_equal(a.iterations_sum + b.iterations_sum, full.iterations_sum)
    assert np.array_equal(np.maximum(a.iterations_max, b.iterations_max), full.iterations_max)


def test_cylinder_probes():
    """the outcomes the GPU test expects of its four probes, from commands_ref.within at their cells' corners"""
    p = O.with_cylinder_probes(np.zeros((4, 6)))
    c = O.corner(p[:, :3], O.D)
    assert np.array_equal(c, [(7.0, 4.0, 4.0), (7.0, 5.0, 4.0), (4.0, 4.0, 1.0), (1.0, 4.0, 6.0)])
    assert list(C.within(O.CYLINDER, c[:, 0], c[:, 1], c[:, 2])) == [True, False, False, True]
    assert list(O.keep(O.CYLINDER, p[:, :3], O.D)) == [True, False, False, True]


def test_corner_of_positions_outside_the_box():
    r = np.array([[-0.25, 8.5, -1.0], [7.999, 0.0, 16.3]])
    assert np.array_equal(O.corner(r, (0.5, 0.5, 0.5)), [(-0.5, 8.5, -1.0), (7.5, 0.0, 16.0)])
    assert list(O.keep(O.REGION, r, O.D)) == [False, False]
