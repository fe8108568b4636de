"""The particle kernels on lattice-aligned positions and exact moves (tests/lattice_cases.py), through the C ABI against the
CPU oracle: particles ON cell faces and half-cell planes, moves of exactly 0, 1/4, 1/2 and 1 cell, landings on the planes,
on 0 and on L, crossings of the periodic edge.  Those are the values at which the kernels branch: floor(x / dx) and
floor(x / dx - 1/2) of the CIC weights and the assembly's half-cell octant, the bucket cell against floor(r / d) where the
move happens inside the consuming kernel, round(pr - 1.5) and the 4-node limit of the Esirkepov box, the periodic fold.

Tolerances are the suite's own (test_gpu_ecsim.py): integers exact; deposits within 1e-12 of the oracle's largest entry; r
and v as the random-input test of the same phase holds them.  On the exact grid (power-of-two spacings and dt) every plane
is hit bit for bit on both sides, so there the zeros are compared too: an entry of currI / matL that is exactly 0 in the
oracle is exactly 0 on the device.  On the general grid (dy = 0.4) a tie is an ulp wide; which side of a vanishing weight
was taken shows as agreement within the tolerance.  After every re-binning the storage cell of every particle is
floor(r / d) of the position the device itself returns -- on both grids, no oracle needed."""
import numpy as np
import pytest

import lattice_cases as LC
from test_gpu_ecsim import canon, make_pair
from test_gpu_schemes import by_position
from test_lattice_cases_ref import continuity_residual

pytestmark = pytest.mark.gpu

DT = 0.5         # ecsim, ecsimcorr: a power of two
DT_BASIC = 0.125  # basic: a power of two inside the explicit scheme's stability limit on these grids
FAMS = {g: LC.families(n, d) for g, (n, d) in LC.GRIDS.items()}
FAMS2 = {g: LC.families(n, d, seed=1) for g, (n, d) in LC.GRIDS.items()}  # the second species' draw of the same classes
NAMES = list(FAMS["p2fx"])
COORD = [f for f in NAMES if f.split("_")[0] in ("node", "half", "near", "still")]
LANDING = [f for f in NAMES if f.split("_")[0] in ("land", "edge", "cross", "unit", "halfmove")]
MOVES = [f for f in NAMES if f != "overflow"]
# with random fields the kick comes on top of the family's move: the classes that stay below half a cell, so that the
# reference's 4-node box holds the pair of positions.  node / half / near / quarter START on the planes and one ulp off
# them (where the ecsimcorr second push gathers), mid puts the MID-STEP position there (where basic_push gathers).
GATHER = [f for f in NAMES if f.split("_")[0] in ("node", "half", "near", "still", "quarter", "mid")]


def cases(names):
    return pytest.mark.parametrize("grid,fam", [(g, f) for g in LC.GRIDS for f in names],
                                   ids=["%s-%s" % (g, f) for g in LC.GRIDS for f in names])


PUSH_CASES = [(g, f, "zero") for g in LC.GRIDS for f in MOVES] + [(g, f, "random") for g in LC.GRIDS for f in GATHER]
push_cases = pytest.mark.parametrize("grid,fam,fields", PUSH_CASES, ids=["%s-%s-%s" % c for c in PUSH_CASES])


def pair(oracle, scheme, grid, dt, species, fields="random", background=0, B0=(0.0, 0.0, 0.0)):
    """oracle + context on one of the two grids holding the same species [(q, m, points)] and fields; `background` random
    particles per cell go into species 0 in front of the family"""
    import xpic_amd as X

    n, d = LC.GRIDS[grid]
    bg = [(4, 1.0, species[0][0], species[0][1])] if background else []
    o, g = make_pair(oracle, scheme, n, d, dt, bg, seed=3, ppc=background, vth=0.2 * min(d) / dt, B0=B0)
    for k, (q, m, pts) in enumerate(species):
        if not (background and k == 0):
            assert o.add_sort(4, 1.0, q, m) == g.add_sort(4, 1.0, q, m, capacity=8192) == k
        assert o.add_particles(k, pts) == g.add_particles(k, pts)
    if fields == "zero":
        for name, fid in (("E", X.E), ("B", X.B), ("B0", X.B0)):
            o.set_field(name, np.zeros(o.fshape()))
            g.set_field(fid, np.zeros(o.fshape()))
    for sim in (o, g):
        sim.set_tolerances(1e-12, 1e-50, 400)
    return o, g


def close(a, b, tol=1e-12):
    return np.abs(a - b).max() <= tol * np.abs(a).max()


def stored_in_own_cell(g, sort, grid):
    n, d = LC.GRIDS[grid]
    pts, cells = g.particles(sort)
    return np.array_equal(cells, LC.storage_cell(pts, n, d)) and np.all(np.diff(cells) >= 0)


def same_zeros(ref, dev, grid):
    """exact grid: what is exactly 0 in the oracle is exactly 0 on the device"""
    return grid != "p2fx" or not dev[ref == 0].any()


# ---- a. the assembly, scatter-first, positions on the planes
@cases(COORD)
def test_assembly_on_the_planes(oracle, grid, fam):
    import xpic_amd as X

    n, d = LC.GRIDS[grid]
    sp = [(-1.0, 1.0, LC.points(FAMS[grid][fam], d, DT)), (+1.0, 100.0, LC.points(FAMS2[grid][fam], d, DT))]
    o, g = pair(oracle, "ecsim", grid, DT, sp, B0=(0.3, -0.2, 0.9))
    oracle.lib().orc_ecsim_fill_current(o.h)
    Lo, ci_o = o.matL(), o.get_field("currI")
    x = np.random.default_rng(8).normal(0, 1, o.fshape())
    ref = o.matL_apply(x)
    ran = []
    for kind in (0, 1):
        g.set_fill_kernel(kind)
        if g.fill_variant()[2] != bool(kind):
            continue  # (the warp-specialised kernel needs nx % 4 == 0)
        ran.append(kind)
        g.ecsim_fill_current()
        ci_g, Lg = g.get_field(X.CURRI), g.matL()
        assert close(ci_o, ci_g) and same_zeros(ci_o, ci_g, grid), kind
        for s in range(2):
            a, b = o.sort_current(s, "currI"), g.sort_current(s, X.CURRI)
            assert close(a, b) and same_zeros(a, b, grid), (kind, s)
        assert np.abs(Lo).max() > 0 and close(Lo, Lg) and same_zeros(Lo, Lg, grid), kind
        g.set_field(X.W0, x)
        g.matL_apply(X.W0, X.W1)
        assert close(ref, g.get_field(X.W1)), kind
    assert ran == [0, 1]  # nx = 12 on both grids


# ---- b. the assembly behind the fused first push: the move lands on the planes inside the consuming kernel
@cases(LANDING)
def test_fused_first_push_lands_on_the_planes(oracle, grid, fam):
    """xpic_set_fused_rebin 1 and 2 against 0 and the oracle, and once more with the gather window cut to 150 slots.  The
    deferred forms exist inside xpic_step only (the phase calls scatter first), so the move, the re-binning and the
    assembly run as the first half of one step: positions and cells bit for bit in every form, currI and matL within 1e-12
    of the oracle's, the bucket cell of a particle that lands on a face is floor(r / d)."""
    import xpic_amd as X

    n, d = LC.GRIDS[grid]
    sp = [(-1.0, 1.0, LC.points(FAMS[grid][fam], d, DT)), (+1.0, 30.0, LC.points(FAMS2[grid][fam], d, DT))]
    o, g = pair(oracle, "ecsim", grid, DT, sp, background=3, B0=(0.1, 0.0, 0.3))
    start = [o.particles(s)[0] for s in range(2)]  # (with the background)
    fields = [(fid, o.get_field(name)) for name, fid in (("E", X.E), ("B", X.B), ("B0", X.B0))]
    assert o.step() >= 0
    Lo, ci_o, parts = o.matL(), o.get_field("currI"), [canon(*o.particles(s)) for s in range(2)]
    control = None
    for mode, window in ((0, None), (1, None), (2, None), (1, 150), (2, 150)):
        if control is not None:  # a fresh context with the same particles and fields
            g = X.Context("ecsim", n, d, DT)
            g.set_preconditioner(0)
            g.set_tolerances(1e-12, 1e-50, 400)
            for s, (q, m, _) in enumerate(sp):
                assert g.add_sort(4, 1.0, q, m, capacity=16384) == s
                assert g.add_particles(s, start[s]) == len(start[s])
            for fid, F in fields:
                g.set_field(fid, F)
        g.set_fused_rebin(mode)
        if window:
            g.debug_set(X.DEBUG_GATHER_WINDOW, window)  # the 64-bit-address arm of the gather sees the same particles
        g.step()
        Lg, ci_g = g.matL(), g.get_field(X.CURRI)
        assert close(Lo, Lg) and close(ci_o, ci_g), (mode, window)
        assert same_zeros(Lo, Lg, grid) and same_zeros(ci_o, ci_g, grid), (mode, window)
        for s in range(2):
            assert stored_in_own_cell(g, s, grid), (mode, window, s)
            pg, cg = canon(*g.particles(s))
            po, co = parts[s]
            assert np.array_equal(cg, co), (mode, window, s)            # dropped at s == L, kept at s == 0, as the oracle
            assert np.array_equal(pg[:, :3], po[:, :3]), (mode, window, s)  # r + v dt: the same bits in every form
            assert np.abs(pg - po).max() <= 1e-9, (mode, window, s)
        if control is None:
            control = Lg, ci_g
        else:  # the deferred forms against scatter-first
            assert close(control[0], Lg) and close(control[1], ci_g), (mode, window)


# ---- c. ecsim_second_push from the planes (the CIC gather at vanishing weights), then a full step
@cases(COORD)
def test_second_push_and_step_from_the_planes(oracle, grid, fam):
    import xpic_amd as X

    n, d = LC.GRIDS[grid]
    o, g = pair(oracle, "ecsim", grid, DT, [(-1.0, 1.0, LC.points(FAMS[grid][fam], d, DT))], background=3, B0=(0.1, 0.2, -0.6))
    Ep = np.random.default_rng(3).normal(0, 0.1, o.fshape())
    o.set_field("Ep", Ep)
    g.set_field(X.EP, Ep)
    oracle.lib().orc_ecsim_second_push(o.h, 0)
    g.ecsim_second_push(0)
    po, co = canon(*o.particles(0))
    pg, cg = canon(*g.particles(0))
    assert np.array_equal(co, cg) and np.array_equal(po[:, :3], pg[:, :3])
    assert np.abs(po[:, 3:] - pg[:, 3:]).max() <= 1e-14
    assert o.step() >= 0
    g.step()
    assert o.count(0) == g.count(0)
    assert np.array_equal(np.bincount(o.particles(0)[1], minlength=o.N), np.bincount(g.particles(0)[1], minlength=o.N))
    assert stored_in_own_cell(g, 0, grid)  # (the second push binned these records for the next step: its keys too)


# ---- d. Esirkepov MODE 0
@push_cases
def test_basic_push_on_the_planes(oracle, grid, fam, fields):
    """E = B = 0: old, mid-step and new position are the generator's, every move class; the gather multiplies zeros.
    Random fields: the 2nd-order gather sits at the mid-step position u + w / 2, which is on a plane or one ulp off it, one
    axis at a time, in the mid_ families (and in `still`); the other random-field families start on the planes and gather
    at generic positions.  The new position is the field's."""
    import xpic_amd as X

    n, d = LC.GRIDS[grid]
    dt = DT_BASIC
    sp = [(-1.0, 1.0, LC.points(FAMS[grid][fam], d, dt)), (+1.0, 4.0, LC.points(FAMS2[grid][fam], d, dt))]
    o, g = pair(oracle, "basic", grid, dt, sp, fields=fields, B0=(0.2, -0.1, 0.7) if fields == "random" else (0.0, 0.0, 0.0))
    rho0 = [o.charge_density(s) for s in range(2)]
    assert oracle.lib().orc_basic_push(o.h) == 0
    g.vec_set(X.J, 0.0)
    for s in range(2):
        g.basic_push(s)
    for s in range(2):
        po, pg = by_position(o.particles(s)[0]), by_position(g.particles(s)[0])
        assert np.abs(po - pg).max() <= 1e-13, s
        a, b = o.sort_current(s, "J"), g.sort_current(s, X.J)
        if fam == "still" and fields == "zero":
            assert not a.any() and not b.any(), s  # no move: identically zero on both sides
            continue
        assert np.abs(a).max() > 0 and close(a, b), s
        # continuity on the device: its J against the reference's charge density at its own new positions
        o1 = oracle.OracleSim("basic", n, d, dt)
        o1.add_sort(4, 1.0, sp[s][0], sp[s][1])
        res, scale = continuity_residual(oracle, o1, g.particles(s)[0], rho0[s], b, dt)
        assert res <= 1e-11 * max(scale, 1e-30), (s, res, scale)
    a, b = o.get_field("J"), g.get_field(X.J)
    assert np.abs(a - b).max() <= 1e-12 * max(np.abs(a).max(), 1e-300)


@pytest.mark.parametrize("grid", list(LC.GRIDS))
def test_pushes_refuse_the_overflow_family(oracle, grid):
    """from k + 1/2 by exactly one cell: a box of 5 nodes.  The reference would overflow Shape::shape; the oracle's
    pushes return 1 and the device raises."""
    import xpic_amd as X

    n, d = LC.GRIDS[grid]
    L = oracle.lib()
    f = FAMS[grid]["overflow"]
    o, g = pair(oracle, "basic", grid, DT_BASIC, [(-1.0, 1.0, LC.points(f, d, DT_BASIC))], fields="zero")
    assert L.orc_basic_push(o.h) == 1
    with pytest.raises(X.XpicError):
        g.basic_push(0)
    for phase in ("first", "second"):
        o, g = pair(oracle, "ecsimcorr", grid, DT, [(-1.0, 1.0, LC.points(f, d, DT / 2))], fields="zero")
        g.set_field(X.EP, np.zeros(o.fshape()))
        assert getattr(L, "orc_ecsimcorr_%s_push" % phase)(o.h, 0) == 1
        with pytest.raises(X.XpicError):
            getattr(g, "ecsimcorr_%s_push" % phase)(0)


# ---- e. Esirkepov MODE 1 and MODE 2
def corr_fields(o, g, fields):
    import xpic_amd as X

    rng = np.random.default_rng(11)
    Ep = rng.normal(0, 0.05, o.fshape()) * (fields == "random")
    Ec = rng.normal(0, 0.05, o.fshape())
    for name, fid, F in (("Ep", X.EP, Ep), ("Ec", X.EC, Ec)):
        o.set_field(name, F)
        g.set_field(fid, F)


def corr_second_push_and_update(oracle, o, g, grid, fields, moved):
    """second push (rc == 0 on the oracle), final_update and re-binning, compared as test_ecsimcorr_phases_match_oracle does"""
    import xpic_amd as X

    L = oracle.lib()
    assert L.orc_ecsimcorr_second_push(o.h, 0) == 0
    g.ecsimcorr_second_push(0)
    a, b = o.sort_current(0, "currJe"), g.sort_current(0, X.CURRJE)
    if not moved:
        assert not a.any() and not b.any()
        return  # (no kinetic energy: the reference's own lambda is 0 / 0)
    assert np.abs(a).max() > 0 and close(a, b)
    assert np.isclose(o.ecsimcorr_scalars(0)["pred_w"], g.ecsimcorr_scalars(0)["pred_w"], rtol=1e-11, atol=1e-300)
    po, pg = by_position(o.particles(0)[0]), by_position(g.particles(0)[0])
    assert np.abs(po - pg).max() <= 1e-13
    L.orc_ecsimcorr_final_update(o.h, 0)
    g.ecsimcorr_final_update(0)
    so, sg = o.ecsimcorr_scalars(0), g.ecsimcorr_scalars(0)
    # In zero fields the velocities stay: pred_dK, corr_dK and lambda_dK are then differences of the SAME kinetic energy K
    # summed over the N <= 400 particles in another order on either side, N eps K < 1e-13 K of round-off and nothing else.
    # With fields they are compared as the random-input test compares them.
    atol = 1e-16 + (1e-12 * abs(so["energy"]) if fields == "zero" else 0.0)
    for k in so:
        assert np.isclose(so[k], sg[k], rtol=1e-10, atol=atol), k
    L.orc_update_cells(o.h, 0)
    assert g.update_cells(0) == o.count(0)
    assert stored_in_own_cell(g, 0, grid)
    po, co = canon(*o.particles(0))
    pg, cg = canon(*g.particles(0))
    assert np.array_equal(co, cg) and np.abs(po - pg).max() <= 1e-12


@push_cases
def test_ecsimcorr_second_push_from_the_planes(oracle, grid, fam, fields):
    """MODE 2 called on the families as they are: the CIC gather out of the bucket cell's neighbourhood and the old
    position of the deposit are ON the planes (node, half, quarter, halfmove, unit, still) or one ulp off them (near), the
    move is the family's in zero fields and the field's on top of it with random ones.  The reference accepts every case.
    (The `table` switch of test_esirkepov_rounds_ragged_pencils composes the rounds of a pencil, not the path of a
    particle inside its round: one mode here.)"""
    import xpic_amd as X

    n, d = LC.GRIDS[grid]
    o, g = pair(oracle, "ecsimcorr", grid, DT, [(-1.0, 1.0, LC.points(FAMS[grid][fam], d, DT / 2))], fields=fields,
                B0=(0.1, 0.0, 0.4) if fields == "random" else (0.0, 0.0, 0.0))
    corr_fields(o, g, fields)
    assert np.isclose(oracle.lib().orc_calculate_energy(o.h, 0), g.calculate_energy(0), rtol=1e-13)
    g.vec_set(X.CURRJE, 0.0)
    corr_second_push_and_update(oracle, o, g, grid, fields, moved=not (fam == "still" and fields == "zero"))


@cases(MOVES)
def test_ecsimcorr_first_push_then_second(oracle, grid, fam):
    """MODE 1 (half a step, no gather) on every move class, the re-binning, and MODE 2 from where the first push left the
    particles -- on the faces and half-cell planes for the landing families -- in zero fields, so the second move is the
    first again.  Each family is cut to the particles whose second move fits the reference's 4-node box as well and that
    the re-binning keeps (lattice_cases.moves_twice; the cut keeps 8 on every plane, test_lattice_cases_ref.py): the
    reference accepts both pushes of every case.  What leaves at s == L is test_update_cells_on_the_landings'."""
    import xpic_amd as X

    n, d = LC.GRIDS[grid]
    L = oracle.lib()
    f = FAMS[grid][fam]
    pts = LC.points(f, d, DT / 2)[LC.moves_twice(f, n, d)]
    o, g = pair(oracle, "ecsimcorr", grid, DT, [(-1.0, 1.0, pts)], fields="zero")
    corr_fields(o, g, "zero")
    assert np.isclose(L.orc_calculate_energy(o.h, 0), g.calculate_energy(0), rtol=1e-13)
    assert L.orc_ecsimcorr_first_push(o.h, 0) == 0
    g.ecsimcorr_first_push(0)
    L.orc_update_cells(o.h, 0)
    assert g.update_cells(0) == o.count(0) == len(pts)
    assert stored_in_own_cell(g, 0, grid)
    po, co = canon(*o.particles(0))
    pg, cg = canon(*g.particles(0))
    assert np.array_equal(co, cg) and np.abs(po - pg).max() <= 1e-13
    g.vec_set(X.CURRJE, 0.0)
    corr_second_push_and_update(oracle, o, g, grid, "zero", moved=fam != "still")


# ---- f. update_cells on the landings
@cases(LANDING)
def test_update_cells_on_the_landings(oracle, grid, fam):
    n, d = LC.GRIDS[grid]
    pts = LC.points(FAMS[grid][fam], d, DT)
    o, g = pair(oracle, "ecsim", grid, DT, [(-1.0, 1.0, pts)])
    oracle.lib().orc_ecsim_first_push(o.h, 0)
    g.ecsim_first_push(0)
    oracle.lib().orc_update_cells(o.h, 0)
    assert g.update_cells(0) == o.count(0) == g.count(0)
    if fam.startswith("edge"):
        assert 0 < g.count(0) < len(pts)  # onto s == L: not folded, outside; onto s == 0: kept
    po, co = canon(*o.particles(0))
    pg, cg = canon(*g.particles(0))
    assert np.array_equal(co, cg) and np.array_equal(po, pg)
    assert stored_in_own_cell(g, 0, grid)


# ---- g. the densities
@cases(COORD)
def test_densities_on_the_planes(oracle, grid, fam):
    n, d = LC.GRIDS[grid]
    o, g = pair(oracle, "basic", grid, DT_BASIC, [(-1.0, 1.0, LC.points(FAMS[grid][fam], d, DT_BASIC))])
    for ref, dev in ((o.charge_density(0), g.charge_density(0)), (o.moment_density(0), g.moment_density(0))):
        assert np.abs(ref).max() > 0 and close(ref, dev)


# ---- h. three steps of each scheme from a lattice quiet start
@pytest.mark.parametrize("scheme", ["basic", "ecsim", "ecsimcorr"])
@pytest.mark.parametrize("grid", list(LC.GRIDS))
def test_steps_from_a_lattice_quiet_start(oracle, grid, scheme):
    """One particle on every node and in every cell centre, two cold beams drifting by exactly +-1/4 cell per step along all
    three axes.  The beams are heavy (m = 2^100: the fields, which they drive, do not turn them within three steps), so on
    the exact grid every particle is on a quarter-cell lattice after every step and on a plane after the second -- where
    the upper beam's last half-cell layer sits on s == L and leaves the box, as in the reference.  Fields within the
    bounds of the random-input multi-step tests, cells and counts exactly."""
    import xpic_amd as X

    n, d = LC.GRIDS[grid]
    dt = DT_BASIC if scheme == "basic" else DT
    sp = [(-1.0, 2.0 ** 100, LC.quiet_start(n, d, dt, +1)), (+1.0, 2.0 ** 100, LC.quiet_start(n, d, dt, -1))]
    o, g = pair(oracle, scheme, grid, dt, sp, B0=(0.0, 0.0, 0.2))
    tol = 1e-11 if scheme == "basic" else 1e-6
    for t in range(3):
        assert o.step() >= 0
        g.step()
        for name, fid in (("E", X.E), ("B", X.B)):
            a, b = o.get_field(name), g.get_field(fid)
            assert np.abs(a - b).max() <= tol * np.abs(a).max(), (t, name)
        for s in range(2):
            assert o.count(s) == g.count(s), (t, s)
            assert stored_in_own_cell(g, s, grid), (t, s)
            po, co = canon(*o.particles(s))
            pg, cg = canon(*g.particles(s))
            assert np.array_equal(co, cg) and np.abs(po - pg).max() <= 1e-12, (t, s)
            if grid == "p2fx":
                assert np.array_equal(pg, po) and np.all(pg[:, :3] / np.array(d) * 4 == np.floor(pg[:, :3] / np.array(d) * 4)), (t, s)
    assert g.count(0) < len(sp[0][2]) and g.count(1) == len(sp[1][2])  # s == L leaves, s == 0 stays
