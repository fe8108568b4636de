"""The grid operators, the reductions and the Krylov drivers on the device against tests/krylov_ref.py: explicit float64
matrices on the project's node ordering and a direct solve on them (tests/test_krylov_ref.py checks that restatement on
the CPU and plants the bugs these assertions are there for).  Parity with a second GMRES cannot see a wrong dot product
or a stale basis vector -- the method converges to its own operator's answer; a direct solve does.

Tolerances: SURVEY 8d's 1e-14 (rot), 1e-13 (matM), 1e-12 (matL products) of the largest reference entry; reductions
inside krylov_ref.dot_bound of math.fsum; solves as krylov_ref.solve_figures states them.  Iteration counts come from the
textbook methods of krylov_ref, never from the device.

Found by these tests: a right-hand side holding an inf passed for converged (|b| = inf <= rtol |b|), the solve returned
x = 0 with a positive reason; both drivers now refuse a |b|^2 that is not finite."""
import functools
import threading

import numpy as np
import pytest
import scipy.sparse as sp

import krylov_ref as K

pytestmark = pytest.mark.gpu


def load(ctx, sorts, B, B0, z0=0, nzl=None):
    import xpic_amd as X

    nzl = B.shape[0] if nzl is None else nzl
    for par, pts in sorts:
        s = ctx.add_sort(*par, capacity=2 * len(pts) + 1024)
        ctx.add_particles(s, pts)  # (a slab keeps what lies in it)
    ctx.set_field(X.B, B[z0:z0 + nzl])
    ctx.set_field(X.B0, (np.zeros_like(B) + np.array(B0))[z0:z0 + nzl])


def put(g, f, v):
    g.set_field(f, v)
    return v


def close_to(got, ref, rel):
    return np.abs(got - ref).max() <= rel * np.abs(ref).max()


@pytest.fixture(scope="module", autouse=True)
def contexts_closed_at_the_end():
    """the contexts op_case and solve_case keep for the module's tests are closed with it"""
    yield
    for cache, ctx in ((op_case, lambda v: v[0]), (solve_case, lambda v: v.g)):
        for v in KEPT.pop(cache.__name__, []):
            ctx(v).close()
        cache.cache_clear()


KEPT = {}


def kept(fn):
    """lru_cache that also lists what it made, for contexts_closed_at_the_end"""
    @functools.lru_cache(maxsize=None)
    def cached(*args, **kw):
        v = fn(*args, **kw)
        KEPT.setdefault(fn.__name__, []).append(v)
        return v
    cached.__name__ = fn.__name__
    return cached


# ---- a. operators against the matrices ----------------------------------------------------------------------------------
@kept
def op_case(name):
    import xpic_amd as X

    n, zs, _ = K.SHAPES[name]
    i = list(K.SHAPES).index(name)
    d, dt = K.D_GENERAL, K.DT
    sorts, B, x, y = K.build_load(n, d, 200 + i, ppc=2 + i % 3)
    g = X.Context("ecsim", n, d, dt)
    load(g, sorts, B, K.B0)
    g.ecsim_fill_current()
    mats = dict(Rp=K.rot_matrix(n, d, True), Rm=K.rot_matrix(n, d, False), M=K.matM_matrix(n, d, dt),
                L=K.matL_matrix(g.matL(), n))
    return g, mats, x, y


@pytest.mark.parametrize("name", list(K.SHAPES))
def test_operators_match_the_matrices(name):
    import xpic_amd as X

    n, zs, _ = K.SHAPES[name]
    assert K.row_split(n[1], n[2]) == zs  # the shape takes the split it is here for
    g, m, x, y = op_case(name)
    assert abs(m["L"]).max() > 0
    g.set_field(X.W0, x)
    for sign, R in ((+1, m["Rp"]), (-1, m["Rm"])):
        Rx = K.apply(R, x)
        for alpha in (0.37, 0.0, -2.0):
            for add in (False, True):
                g.set_field(X.W1, y)
                g.rot_apply(sign, alpha, X.W0, X.W1, add)
                assert close_to(g.get_field(X.W1), alpha * Rx + (y if add else 0.0), 1e-14), (sign, alpha, add)
    Mx, Lx = K.apply(m["M"], x), K.apply(m["L"], x)
    for add in (False, True):
        g.set_field(X.W1, y)
        g.matM_apply(X.W0, X.W1, add)
        assert close_to(g.get_field(X.W1), Mx + (y if add else 0.0), 1e-13), add
        g.set_field(X.W1, y)
        g.matL_apply(X.W0, X.W1, add)
        assert close_to(g.get_field(X.W1), Lx + (y if add else 0.0), 1e-12), add
    g.set_field(X.W1, y)
    g.matA_apply(X.W0, X.W1)
    assert close_to(g.get_field(X.W1), Mx + Lx, 1e-12)


@pytest.mark.parametrize("name", ["2x2x2", "two-bands"])
def test_operator_identities_on_the_device(name):
    """<rot+ x, y> = <x, rot- y> and <matM x, y> = <x, matM y> through vec_dot.  Bound: dot_bound with the operator's
    entries and the vectors in absolute value, n eps sum (|R| |x|)_i |y_i| on either side -- it covers the summation (any
    order) and, for n of 24 and more, the dozen roundings of the operator itself.  matM against its composition from
    rot_apply: 1e-13 of the largest entry."""
    import xpic_amd as X

    g, m, x, y = op_case(name)
    dt = g.dt
    g.set_field(X.W0, x)
    g.set_field(X.W1, y)
    aRp, aRm = abs(m["Rp"]), abs(m["Rm"])
    aM = 2.0 * sp.identity(x.size) + 0.5 * dt * dt * (aRm @ aRp)
    g.rot_apply(+1, 1.0, X.W0, X.W2)
    lhs = g.vec_dot(X.W2, X.W1)
    g.rot_apply(-1, 1.0, X.W1, X.W2)
    rhs = g.vec_dot(X.W0, X.W2)
    bound = K.dot_bound(K.apply(aRp, np.abs(x)), y) + K.dot_bound(x, K.apply(aRm, np.abs(y)))
    print(name, "rot", lhs, rhs, bound)
    assert abs(lhs - rhs) <= bound
    g.matM_apply(X.W0, X.W2)
    Mx = g.get_field(X.W2)
    lhs = g.vec_dot(X.W2, X.W1)
    g.matM_apply(X.W1, X.W2)
    rhs = g.vec_dot(X.W0, X.W2)
    bound = K.dot_bound(K.apply(aM, np.abs(x)), y) + K.dot_bound(x, K.apply(aM, np.abs(y)))
    print(name, "matM", lhs, rhs, bound)
    assert abs(lhs - rhs) <= bound
    g.rot_apply(+1, 1.0, X.W0, X.W2)
    g.rot_apply(-1, 0.5 * dt * dt, X.W2, X.E)
    g.vec_axpy(X.E, 2.0, X.W0)
    assert close_to(g.get_field(X.E), Mx, 1e-13)


# ---- b. reductions --------------------------------------------------------------------------------------------------------
RED_GRIDS = {"8-nodes": (2, 2, 2), "1025-nodes": (41, 5, 5), "cap": (72, 72, 72)}


def contents(kind, shape, rng):
    if kind == "smooth":
        return rng.normal(0, 1.0, shape)
    if kind == "alternating":
        v = np.where(np.arange(int(np.prod(shape))) % 2 == 0, 1e8, -1e8) + 1e-8 * rng.normal(size=int(np.prod(shape)))
        return v.reshape(shape)
    v = np.zeros(shape)
    v[-1, -1, -1, 2] = 3.25  # the last owned node of the last component
    return v


def fma(a, x, y):
    """a x + y rounded once, elementwise: the product's rounding error from Veltkamp's split and Dekker's product, the
    sum's from Knuth's two-sum, both added to the sum in one last operation"""
    a = np.float64(a)
    p = a * x
    sa, sx = 134217729.0 * a, 134217729.0 * x
    ah, xh = sa - (sa - a), sx - (sx - x)
    al, xl = a - ah, x - xh
    e = ((ah * xh - p) + ah * xl + al * xh) + al * xl
    s = p + y
    bb = s - p
    t = (p - (s - bb)) + (y - bb)
    return s + (t + e)


def same_bits(got, candidates):
    print("elements off, per candidate:", [int(np.count_nonzero(got != c)) for c in candidates])
    return any(np.array_equal(got, c) for c in candidates)


@pytest.mark.parametrize("grid", list(RED_GRIDS))
def test_reductions_inside_the_summation_bound(grid):
    """vec_dot and vec_norm2 against math.fsum inside dot_bound, below a wave (8 nodes), one node past a multiple of the
    1024 nodes of a reduction block (1025 = 41 x 5 x 5) and with red_grid at its cap of kRedBlocks / 3 = 341 blocks per
    component (72^3 = 373248 > 341 x 1024 nodes; a `basic` context, seven vectors and no matrix); there also vec_axpy and
    vec_axpby against numpy bit for bit: the whole array equals the unfused result or one of the fused ones."""
    import xpic_amd as X

    n = RED_GRIDS[grid]
    nown = n[0] * n[1] * n[2]
    assert (K.red_blocks(nown) == K.RED_CAP and nown > K.RED_CAP * 4 * K.KBLOCK) if grid == "cap" else K.red_blocks(nown) < K.RED_CAP
    assert grid != "1025-nodes" or nown % (4 * K.KBLOCK) == 1
    g = X.Context("basic" if grid == "cap" else "ecsim", n, K.D_GENERAL, K.DT)  # (basic needs extents of 4 and more)
    rng = np.random.default_rng(17)
    shape = g.fshape()
    y = put(g, X.B, rng.normal(0, 1.0, shape))
    for kind in ("smooth", "alternating", "single"):
        x = put(g, X.E, contents(kind, shape, rng))
        got, ref, bound = g.vec_dot(X.E, X.B), K.dot_exact(x, y), K.dot_bound(x, y)
        print(grid, kind, "dot", got, ref, bound)
        assert abs(got - ref) <= bound, (kind, got, ref, bound)
        got, ref2, bound2 = g.vec_norm2(X.E), K.dot_exact(x, x), K.dot_bound(x, x)
        print(grid, kind, "norm2", got * got, ref2, bound2)
        assert abs(got * got - ref2) <= bound2 + 4.0 * K.EPS * ref2, (kind, got, ref2)  # (the root and its square: 4 eps)
        if kind == "single":
            assert g.vec_dot(X.E, X.B) == x[-1, -1, -1, 2] * y[-1, -1, -1, 2] and got == 3.25
    if grid == "cap":
        x = put(g, X.E, contents("smooth", shape, rng))
        g.set_field(X.W0, y)
        g.vec_axpy(X.W0, -0.37, X.E)
        assert same_bits(g.get_field(X.W0), [y + -0.37 * x, fma(-0.37, x, y)])
        g.set_field(X.W0, y)
        g.vec_axpby(X.W0, 1.5, -0.25, X.E)  # W0 = 1.5 E - 0.25 W0
        assert same_bits(g.get_field(X.W0), [1.5 * x + -0.25 * y, fma(1.5, x, -0.25 * y), fma(-0.25, y, 1.5 * x)])
    g.close()


# ---- c. solves against the direct solve -----------------------------------------------------------------------------------
class Case:
    pass


@kept
def solve_case(name, scheme="ecsim", particles=True):
    import xpic_amd as X

    n, d, dt, seed, B0 = K.SOLVE_CASES[name]
    sorts, B, rhs, _ = K.build_load(n, d, seed, B0=B0)
    c = Case()
    c.g = X.Context(scheme, n, d, dt)
    c.M = K.matM_matrix(n, d, dt)
    c.A = c.M
    if particles:
        load(c.g, sorts, B, B0)
        c.g.ecsim_fill_current()
        c.A = (c.M + K.matL_matrix(c.g.matL(), n)).tocsr()
    c.rhs, c.n = rhs, n
    c.mat = {0: c.A, 1: c.M, 2: c.M}
    c.kappa = {0: K.cond2(c.A), 1: K.cond2(c.M)}
    c.kappa[2] = c.kappa[1]
    c.xstar = {0: K.direct_solve(c.A, rhs), 1: K.direct_solve(c.M, rhs)}
    c.xstar[2] = c.xstar[1]
    return c


@functools.lru_cache(maxsize=None)
def ref_count(name, op, rtol, atol=1e-50, scheme="ecsim", particles=True):
    c = solve_case(name, scheme, particles)
    return (K.cg if op == 2 else K.gmres)(c.mat[op], c.rhs, rtol, atol, 400)[1]


def run(c, op, kind, rtol, atol=1e-50, maxit=300, rhs=None):
    import xpic_amd as X

    c.g.set_preconditioner(kind)
    c.g.set_field(X.E, c.rhs if rhs is None else rhs)
    c.g.vec_set(X.W2, 7.0)
    its, reason, rn = c.g.solve(op, X.E, X.W2, rtol, atol, maxit)
    return c.g.get_field(X.W2), its, reason, rn


def check(c, op, got, rtol, atol=1e-50, its_ref=None, explicit=False, where=None):
    x, its, reason, rn = got
    assert reason > 0, where
    f = K.solve_figures(c.mat[op], c.rhs, x, its, rn, rtol, atol, c.xstar[op], c.kappa[op], its_ref, explicit)
    print(where, "its", its, f)
    assert not K.failed(f), (where, K.failed(f), f)


KINDS = {0: (0, 1, 2, 3, 4, 5), 1: (0, 1, 2), 2: (0,)}


@pytest.mark.parametrize("name", ["6x5x4", "8x8x6"])
@pytest.mark.parametrize("op", [0, 1, 2])
def test_solves_match_the_direct_solve(name, op):
    c = solve_case(name)
    try:
        plain = None
        for kind in KINDS[op]:
            got = run(c, op, kind, 1e-7)
            check(c, op, got, 1e-7, its_ref=ref_count(name, op, 1e-7) if kind == 0 else None, where=(name, op, kind))
            if kind == 0:
                plain = got[1]
            else:
                assert got[1] <= plain, (kind, got[1], plain)
    finally:
        c.g.set_preconditioner(5)


def test_the_correct_solve_on_an_ecsimcorr_context():
    c = solve_case("6x5x4", "ecsimcorr", False)
    try:
        plain = run(c, 1, 0, 1e-7)
        check(c, 1, plain, 1e-7, its_ref=ref_count("6x5x4", 1, 1e-7, scheme="ecsimcorr", particles=False), where="plain")
        for kind in (1, 2):
            got = run(c, 1, kind, 1e-7)
            check(c, 1, got, 1e-7, where=kind)
            assert got[1] <= plain[1]
    finally:
        c.g.set_preconditioner(5)


@pytest.mark.parametrize("rtol", [1e-5, 1e-7, 1e-8, 1.01e-8, 0.99e-8, 1e-11])
def test_tolerances_across_both_switches(rtol):
    """rtol on both sides of 1e-6 |b| (where the one-reduction norm gives way) and of 1e-8 |b| (below: every norm
    explicit).  At 1e-5 the reductions are counted as test_one_reduction_per_gmres_iteration counts them: the w . w row
    read from the wrong place sends every norm through a second reduction and shows nowhere else."""
    c = solve_case("8x8x6")
    try:
        for op in (0, 1, 2):
            if op != 0 and rtol not in (1e-5, 1e-11):
                continue
            c.g.profile_enable(True)
            c.g.profile_reset()
            got = run(c, op, 0, rtol)
            nred = c.g.profile_get("allreduce")[0]
            c.g.profile_enable(False)
            check(c, op, got, rtol, its_ref=ref_count("8x8x6", op, rtol), explicit=rtol == 1e-11, where=(op, rtol))
            if rtol == 1e-5 and op != 2:
                assert nred <= got[1] + 3 + (got[1] - 1) // 30, (op, got[1], nred)
    finally:
        c.g.profile_enable(False)
        c.g.set_preconditioner(5)


def test_zero_right_hand_side():
    c = solve_case("6x5x4")
    try:
        for op in (0, 1, 2):
            for kind in KINDS[op][:2]:
                x, its, reason, rn = run(c, op, kind, 1e-7, 0.0, rhs=np.zeros_like(c.rhs))  # (0 <= 0: the stop is <=)
                assert its == 0 and reason > 0 and rn == 0.0 and not x.any(), (op, kind, its, reason)
    finally:
        c.g.set_preconditioner(5)


def test_eigenvector_right_hand_side_and_the_solve_after_it():
    """No particles: matL = 0, and rot of a constant field is 0, so A b = 2 b: the next Hessenberg entry vanishes, one
    iteration, x = b / 2.  With the polynomial in fp64 (kind 2; kind 1 rounds it to fp32, and b would no longer be an
    eigenvector of what the Arnoldi step sees).  An ordinary solve afterwards still matches the direct one."""
    c = solve_case("6x5x4", "ecsim", False)
    b = np.zeros_like(c.rhs) + np.array([0.5, -1.25, 2.0])
    try:
        for op in (0, 1, 2):
            for kind in (0, 2) if op != 2 else (0,):
                x, its, reason, rn = run(c, op, kind, 1e-7, rhs=b)
                print(op, kind, its, rn, np.abs(x - 0.5 * b).max())
                assert its == 1 and reason > 0, (op, kind, its)
                assert np.abs(x - 0.5 * b).max() <= 1e-15 * np.abs(b).max(), (op, kind)
                check(c, op, run(c, op, kind, 1e-7), 1e-7, its_ref=ref_count("6x5x4", op, 1e-7, particles=False) if kind == 0 else None,
                      where=("after", op, kind))
    finally:
        c.g.set_preconditioner(5)


def test_absolute_tolerance_decides():
    """atol >= |b|: no iteration.  atol at the geometric mean of the restated GMRES's residuals after 5 and 6 iterations
    (rtol = 0): the solve stops at 6, +- 1; CG likewise."""
    c = solve_case("6x5x4")
    bn = float(np.linalg.norm(c.rhs))
    try:
        for op in (0, 2):
            x, its, reason, rn = run(c, op, 0, 1e-7, 1.5 * bn)
            assert its == 0 and reason > 0 and not x.any()
            hist = (K.cg if op == 2 else K.gmres)(c.mat[op], c.rhs, 1e-12, 0.0, 300)[2]
            k = 5
            atol = float(np.sqrt(hist[k - 1] * hist[k]))
            assert hist[k] < atol < hist[k - 1]
            got = run(c, op, 0, 0.0, atol)
            assert abs(got[1] - (k + 1)) <= 1, (op, got[1])
            check(c, op, got, 0.0, atol, where=("atol", op))
    finally:
        c.g.set_preconditioner(5)


def test_iteration_limit_exactly_at_the_count():
    import xpic_amd as X

    c = solve_case("6x5x4")
    try:
        for op in (0, 2):
            x, k, reason, rn = run(c, op, 0, 1e-7)
            x2, k2, reason2, _ = run(c, op, 0, 1e-7, maxit=k)
            assert (k2, reason2 > 0) == (k, True) and np.array_equal(x, x2)
            for maxit in (k - 1, 0):
                with pytest.raises(X.XpicError, match="did not converge"):
                    run(c, op, 0, 1e-7, maxit=maxit)
    finally:
        c.g.set_preconditioner(5)


def test_solve_across_two_restarts():
    """8 x 8 x 6, d = 0.25, dt = 1.5 (krylov_ref.RESTART_DT): cond2(A) = 108 and the restated GMRES(30) takes 89
    iterations to 1e-9 (76 at dt = 1.25, 60 at dt = 1, 127 at dt = 2; measured on the CPU with the oracle's matL) and 70
    to 1e-7.  At 1e-9 every norm is explicit; at 1e-7 the norms above 1e-6 |b| come out of the one reduction, the
    recurrence drifts over a cycle and b - A x at the restart is what brings it back: a restart norm taken from the
    recurrence costs 9 iterations there and leaves 3.7 tol of true residual (tests/test_krylov_ref.py).  A limit
    of 30, 31 or 60 iterations ends on, one past and on a restart: the solve raises, and the x it leaves has the residual
    the restated method has after as many iterations, within the 1e-8 |b| of the recurrence."""
    import xpic_amd as X

    c = solve_case("restart")
    ref = ref_count("restart", 0, 1e-9)
    assert 60 < ref < 120
    bn = float(np.linalg.norm(c.rhs))
    try:
        got = run(c, 0, 0, 1e-9)
        assert got[1] > 60
        check(c, 0, got, 1e-9, its_ref=ref, where="restart")
        ref7 = ref_count("restart", 0, 1e-7)
        assert 60 < ref7 < 120
        got = run(c, 0, 0, 1e-7)
        assert got[1] > 60
        check(c, 0, got, 1e-7, its_ref=ref7, where="restart, 1e-7")
        hist = K.gmres(c.A, c.rhs, 1e-9, 0.0, 60)[2]
        for maxit in (30, 31, 60):
            with pytest.raises(X.XpicError, match="did not converge: %d iterations" % maxit):
                run(c, 0, 0, 1e-9, maxit=maxit)
            res = K.true_residual(c.A, c.g.get_field(X.W2), c.rhs)
            print(maxit, res, hist[maxit - 1])
            assert abs(res - hist[maxit - 1]) <= 1e-8 * bn, maxit
    finally:
        c.g.set_preconditioner(5)


def test_strongly_nonsymmetric_operator():
    c = solve_case("nonsymmetric")
    skew = lambda A: abs(A - A.T).max() / abs(A).max()  # noqa: E731
    print("asymmetry", skew(c.A), "ordinary case", skew(solve_case("6x5x4").A))
    # premise only: the skew part (matL's rotation terms, odd in B) is larger than in the same grid's ordinary case with
    # its weaker field and dt = 0.7, also relative to a matM that has grown with dt^2
    assert skew(c.A) > skew(solve_case("6x5x4").A)
    try:
        for kind in (0, 1, 2):
            got = run(c, 0, kind, 1e-7)
            check(c, 0, got, 1e-7, its_ref=ref_count("nonsymmetric", 0, 1e-7) if kind == 0 else None, where=kind)
    finally:
        c.g.set_preconditioner(5)


def test_a_right_hand_side_that_is_not_finite_raises():
    import xpic_amd as X

    c = solve_case("6x5x4", "ecsim", False)
    b = c.rhs.copy()
    b[1, 2, 3, 1] = np.inf
    try:
        for op in (0, 1, 2):
            with pytest.raises(X.XpicError):
                run(c, op, 0, 1e-7, maxit=5, rhs=b)
        check(c, 0, run(c, 0, 0, 1e-7), 1e-7, where="after")  # the context still solves
    finally:
        c.g.set_preconditioner(5)


def test_solves_repeat_bit_for_bit():
    c = solve_case("8x8x6")
    try:
        for op, kind in ((0, 0), (0, 5), (1, 1), (2, 0)):
            a, b = run(c, op, kind, 1e-7), run(c, op, kind, 1e-7)
            assert a[1] == b[1] and a[3] == b[3] and np.array_equal(a[0], b[0]), (op, kind)
    finally:
        c.g.set_preconditioner(5)


# ---- d. two z-slabs in one process -------------------------------------------------------------------------------------------
def test_two_slabs_apply_and_solve_like_one_context():
    """6 x 5 x 12 in two slabs of 6 planes (threads of this process, the callback transport): matA_apply and the solves
    of ops 0 and 2, whose operator runs split into interior and boundary planes beside the halo exchange, against the
    matrix of the whole box inside the bounds of sections a and c, and against the single context."""
    import xpic_amd as X
    from xpic_amd.parallel import ThreadRing

    n, d, dt, nr = (6, 5, 12), K.D_GENERAL, K.DT, 2
    sorts, B, rhs, x = K.build_load(n, d, 310)
    one = X.Context("ecsim", n, d, dt)
    load(one, sorts, B, K.B0)
    one.ecsim_fill_current()
    one.set_preconditioner(0)
    A = (K.matM_matrix(n, d, dt) + K.matL_matrix(one.matL(), n)).tocsr()
    M = K.matM_matrix(n, d, dt)
    ring = ThreadRing(nr)
    res, errs = [None] * nr, []

    def work(ctx, sl):
        ctx.set_preconditioner(0)
        ctx.set_field(X.W0, x[sl])
        ctx.matA_apply(X.W0, X.W1)
        out = dict(matL=ctx.matL(), Ax=ctx.get_field(X.W1))
        ctx.set_field(X.E, rhs[sl])
        for op in (0, 2):
            out[op] = ctx.solve(op, X.E, X.W2, 1e-7, 1e-50, 300) + (ctx.get_field(X.W2),)
        return out

    def rank_main(rk):
        try:
            ctx = X.Context("ecsim", n, d, dt, rank=rk, nranks=nr)
            load(ctx, sorts, B, K.B0, ctx.z0, ctx.nzl)
            ring.attach(ctx, rk)
            ctx.ecsim_fill_current()
            res[rk] = work(ctx, slice(ctx.z0, ctx.z0 + ctx.nzl))
            ctx.close()
        except BaseException as e:  # noqa: BLE001 -- release the other rank, report below
            errs.append((rk, repr(e)))
            ring.bar.abort()

    th = [threading.Thread(target=rank_main, args=(rk,)) for rk in range(nr)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not errs and all(r is not None for r in res), errs
    whole = work(one, slice(None))
    Ax = np.concatenate([r["Ax"] for r in res], axis=0)
    ref = K.apply(A, x)
    assert close_to(Ax, ref, 1e-12) and close_to(whole["Ax"], ref, 1e-12)
    for op, mat in ((0, A), (2, M)):
        xs, kappa = K.direct_solve(mat, rhs), K.cond2(mat)
        its_ref = (K.cg if op == 2 else K.gmres)(mat, rhs, 1e-7, 1e-50, 300)[1]
        assert res[0][op][:3] == res[1][op][:3]  # every slab reports the same solve
        its, reason, rn = res[0][op][:3]
        xg = np.concatenate([r[op][3] for r in res], axis=0)
        for who, (i, rs, r_, xx) in (("slabs", (its, reason, rn, xg)), ("one", whole[op])):
            assert rs > 0
            f = K.solve_figures(mat, rhs, xx, i, r_, 1e-7, 1e-50, xs, kappa, its_ref)
            print(who, op, i, f)
            assert not K.failed(f), (who, op, f)
    one.close()
