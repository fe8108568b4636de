"""The lattice case generator (tests/lattice_cases.py) does what it says, checked against the CPU oracle alone: the
reference accepts every family but `overflow`, every tie class sits bit-exactly on its plane at the place it is meant
for, the oracle's Esirkepov current of every family satisfies the discrete continuity equation, and no move is no current."""
import numpy as np
import pytest

import lattice_cases as LC

DT = 0.5  # a power of two: tau v is exact on the exact grid
FAMS = {g: LC.families(n, d) for g, (n, d) in LC.GRIDS.items()}
NAMES = list(FAMS["p2fx"])
CASES = [(g, f) for g in LC.GRIDS for f in NAMES]
IDS = ["%s-%s" % c for c in CASES]


def test_grids_are_the_suites():
    import test_gpu_ecsim as T

    assert LC.EXACT == T.GRID_P2FX[:2] and LC.GENERAL == T.GRID[:2]
    assert list(FAMS["general"]) == NAMES and "overflow" in NAMES and "still" in NAMES
    for g in FAMS:
        for f in FAMS[g].values():
            assert 8 <= len(f.u) <= 400 and f.u.shape == f.w.shape == (len(f.u), 3), f.name


def sim(oracle, scheme, grid, fam, tau):
    n, d = LC.GRIDS[grid]
    o = oracle.OracleSim(scheme, n, d, DT)
    o.add_sort(4, 1.0, -1.0, 1.0)
    pts = LC.points(FAMS[grid][fam], d, tau)
    assert o.add_particles(0, pts) == len(pts)
    return o, pts


@pytest.mark.parametrize("grid,fam", CASES, ids=IDS)
def test_reference_accepts_all_but_the_overflow_family(oracle, grid, fam):
    """Shape::shape holds 4 nodes per axis: the three Esirkepov pushes return 0, and 1 for the family with one such particle"""
    L = oracle.lib()
    want = FAMS[grid][fam].overflow
    o, _ = sim(oracle, "basic", grid, fam, DT)
    assert L.orc_basic_push(o.h) == want
    o, _ = sim(oracle, "ecsimcorr", grid, fam, DT / 2)
    assert L.orc_ecsimcorr_first_push(o.h, 0) == want
    o, _ = sim(oracle, "ecsimcorr", grid, fam, DT / 2)
    assert L.orc_ecsimcorr_second_push(o.h, 0) == want  # E = B = 0: the velocity stays


@pytest.mark.parametrize("fam", NAMES)
def test_exact_grid_hits_every_plane_bit_for_bit(fam):
    """On the exact grid r / d, (r + v tau / 2) / d and (r + v tau) / d computed with the kernels' operations ARE u, u + w / 2
    and u + w wherever those have few bits, and each (class, axis, place) the family is built for holds >= 8 particles
    exactly on a face, and as many exactly on a half-cell plane, where it is built for both; the edge families hold 8 on 0
    and 8 on L."""
    n, d = LC.EXACT
    f = FAMS["p2fx"][fam]
    for tau in (DT, DT / 2):
        pts = LC.points(f, d, tau)
        few = np.all((f.u * 2048 == np.floor(f.u * 2048)) & (f.w * 2048 == np.floor(f.w * 2048)), axis=1)
        assert few.sum() >= 8 or fam.startswith("near")
        for place, frac in (("old", 0.0), ("mid", 0.5), ("new", 1.0)):
            x = LC.scaled(pts, d, tau, place)
            assert np.array_equal(x[few], (f.u + f.w * frac)[few]), (place, tau)
        for a, place, kind in f.ties:
            hits = int(LC.on_plane(LC.scaled(pts, d, tau, place)[:, a], kind).sum())
            assert hits >= 8, (fam, a, place, kind, hits)
        if fam.startswith("edge"):
            a = f.ties[0][0]
            x = LC.scaled(pts, d, tau, "new")[:, a]
            assert (x == 0).sum() >= 8 and (x == n[a]).sum() >= 8, fam


def test_tie_classes_cover_every_axis_and_place():
    tied = {t for f in FAMS["p2fx"].values() if f.name != "still" for t in f.ties}  # one axis at a time
    assert tied == {(a, p, kind) for a in range(3) for p in ("old", "mid", "new") for kind in ("face", "half")}


@pytest.mark.parametrize("grid,fam", [c for c in CASES if c[1] != "overflow"], ids=[i for i in IDS if "overflow" not in i])
def test_two_moves_in_a_row_fit_where_the_generator_says(oracle, grid, fam):
    """LC.moves_twice: first push, re-binning and second push in zero fields are accepted by the reference, nothing leaves
    the box, and on the exact grid the landing families still put >= 8 particles on a face and 8 on a half-cell plane
    under the second push (all 8 on s == 0 for the edge families)."""
    n, d = LC.GRIDS[grid]
    f = FAMS[grid][fam]
    keep = LC.moves_twice(f, n, d)
    pts = LC.points(f, d, DT / 2)[keep]
    o = oracle.OracleSim("ecsimcorr", n, d, DT)
    o.add_sort(4, 1.0, -1.0, 1.0)
    assert o.add_particles(0, pts) == len(pts) >= 8
    L = oracle.lib()
    assert L.orc_ecsimcorr_first_push(o.h, 0) == 0
    L.orc_update_cells(o.h, 0)
    assert o.count(0) == len(pts)
    assert L.orc_ecsimcorr_second_push(o.h, 0) == 0
    if grid == "p2fx":
        for a, place, kind in f.ties:
            if place == "new" and not (fam.startswith("edge") and kind == "half"):
                assert LC.on_plane(LC.scaled(pts, d, DT / 2, "new")[:, a], kind).sum() >= 8, (fam, a, kind)


def continuity_residual(oracle, o, pts_new, rho0, J, dt):
    """(rho1 - rho0) / dt + div J with the reference's own charge density of the moved particles (folded into the box:
    s == L is the node at 0) -- test_esirkepov_continuity_on_device's statement"""
    L = np.array(o.n) * np.array(o.d)
    r = pts_new[:, :3]
    r = np.where(r < 0, r + L, np.where(r >= L, r - L, r))
    o.clear(0)
    assert o.add_particles(0, np.hstack([r, pts_new[:, 3:]])) == len(r)
    rho1 = o.charge_density(0)
    div = np.zeros(rho0.shape)
    oracle.lib().orc_div_neg(o.h, oracle._dp(np.ascontiguousarray(J)), oracle._dp(div))
    return np.abs((rho1 - rho0) / dt + div).max(), np.abs(div).max()


@pytest.mark.parametrize("grid,fam", [c for c in CASES if c[1] != "overflow"], ids=[i for i in IDS if "overflow" not in i])
def test_oracle_current_is_charge_conserving_on_every_family(oracle, grid, fam):
    o, pts = sim(oracle, "basic", grid, fam, DT)
    rho0 = o.charge_density(0)
    assert oracle.lib().orc_basic_push(o.h) == 0
    J = o.get_field("J")
    if fam == "still":
        assert not J.any()  # no move: identically zero, not round-off
        return  # (nothing to balance: the two densities are the same particles summed in another order)
    res, scale = continuity_residual(oracle, o, o.particles(0)[0], rho0, J, DT)
    assert res <= 1e-11 * max(scale, 1e-30), (res, scale)
