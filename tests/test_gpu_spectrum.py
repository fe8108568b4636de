"""Field spectra on the device (include/xpic_spectrum.h, xpic_amd/csrc/spectrum.hip) against tests/spectrum_ref.py's numpy
restatement: the power, the axis and shell sums and the total, single modes, special inputs, the bits, the field and
charge sources, the refusals, and the probe that rides with the step.

Shapes (spectrum_ref.SHAPES): the small ones but 1x4x6 (xpic_create takes extents >= 2; that shape stays with the CPU tests);
2x2x2 (reflection is the identity); 15 / 16 / 17 and 63 / 64 / 65
along each axis in turn -- odd and even extents differ in the self-conjugate Nyquist plane, 63 / 64 / 65 sit on both sides
of the 64-lane x tile of the combine kernel, 15 / 16 / 17 of its 16 rows per workgroup --, 66x65x67 (two x tiles, five
row groups, several workgroups per reduction) and 6x6x129.
The bound is spectrum_ref's: |dP(k)| <= K_SPEC eps (2 sqrt(P_ref) |x| + eps |x|^2), |dF^| <= K_SPEC eps |x|, reduced outputs
in addition terms * eps * their own value; K_SPEC = 8 x 1.354 (measured on the CPU, tests/test_spectrum_ref.py)."""
import numpy as np
import pytest

import spectrum_ref as S
import test_gpu_es as TE
import test_gpu_gauss as TG

pytestmark = pytest.mark.gpu
EPS = S.EPS


@pytest.fixture(scope="module")
def X():
    import xpic_amd

    return xpic_amd


@pytest.fixture(scope="module")
def refs():
    """name -> (n, d, x, P of the restatement): computed once on demand, read by every test"""
    inputs, cache = S.inputs(), {}

    def get(name):
        if name not in cache:
            n, d, x = inputs[name]
            p = S.power(x, n)
            p.setflags(write=False)
            cache[name] = (n, d, x, p)
        return cache[name]
    return get


def all_modes(n):
    z, y, x = np.meshgrid(np.arange(n[2]), np.arange(n[1]), np.arange(n[0]), indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)


def check_reduced(label, got, p_ref, x, mask):
    """a sum of P over the modes of `mask` against the restatement's"""
    want, terms = p_ref[mask].sum(), int(mask.sum())
    bound = S.power_bound(p_ref, x)[mask].sum() + terms * EPS * want
    assert abs(got - want) <= bound, (label, got, want, bound)
    return abs(got - want) / bound if bound > 0 else 0.0


# ---- 1. power, axis, shells, total and modes against the restatement --------------------------------------------------------
@pytest.mark.parametrize("name", list(S.SHAPES))
def test_spectrum_matches_the_restatement(X, refs, name):
    n, d, x, p_ref = refs(name)
    g = X.Context("ecsim", n, d, 0.5)
    p = g.spectrum_power(x)
    bound = S.power_bound(p_ref, x)
    used = [(np.abs(p - p_ref) / bound).max()]
    assert (np.abs(p - p_ref) <= bound).all()
    rx, ry, rz = S.reflections(n)
    assert np.array_equal(p, p[np.ix_(rz, ry, rx)])  # P(k) == P(-k), the same bits
    assert np.array_equal(g.spectrum_power(x), p)    # the same bits twice
    assert abs(p.sum() - (x ** 2).sum()) <= x.size * EPS * (x ** 2).sum()  # Parseval
    # modes: every mode of the box, against the restatement and against the power
    f_ref = S.fourier(x, n)
    modes = all_modes(n)
    f = g.spectrum_modes(x, modes).reshape(p.shape)
    used.append(np.abs(f - f_ref).max() / S.mode_bound(x))
    assert np.abs(f - f_ref).max() <= S.mode_bound(x)
    assert np.array_equal(g.spectrum_modes(x, modes).reshape(p.shape), f)
    # (Re^2 + Im^2 = (H(k)^2 + H(-k)^2) / 2 from the same H(+-k): four roundings apart)
    assert (np.abs(f.real ** 2 + f.imag ** 2 - p) <= 8 * EPS * p).all()
    assert np.array_equal(f[np.ix_(rz, ry, rx)], np.conj(f))  # H(k) and H(-k) change places: the conjugate, bit for bit
    # the bits of H(+-k) are those of the power's route: at a self-conjugate mode H(k) and H(-k) are one expression, so
    # Re = (H + H) / 2 = H, Im = 0 and P = (H^2 + H^2) / 2 = fl(H^2), all exact: P == Re * Re bit for bit
    own = (rz[:, None, None] == np.arange(n[2])[:, None, None]) & (ry[None, :, None] == np.arange(n[1])[None, :, None]) & \
        (rx[None, None, :] == np.arange(n[0])[None, None, :])
    assert own.sum() >= 1 and np.array_equal((f.real * f.real)[own], p[own]) and not f.imag[own].any()
    # signed and folded mode numbers agree
    nn = np.array(n)
    assert np.array_equal(g.spectrum_modes(x, modes - nn), f.ravel()) and np.array_equal(g.spectrum_modes(x, modes + 2 * nn), f.ravel())
    # the reduced form, with both edge sets
    ones = np.ones(p.shape, dtype=bool)
    for which in ("dk", "offset"):
        edges = S.shell_edges(n, d, which)
        sp = g.spectrum(x, dk=edges[1], nshell=S.NSHELL) if which == "dk" else g.spectrum(x, edges=edges)
        again = g.spectrum(x, edges=edges)
        for a in range(3):
            assert np.array_equal(sp.axis[a], again.axis[a])  # the same bits twice
            for i in range(n[a]):
                mask = np.zeros(p.shape, dtype=bool)
                mask[tuple(i if 2 - a == ax else slice(None) for ax in range(3))] = True
                used.append(check_reduced("axis", sp.axis[a][i], p_ref, x, mask))
            assert np.allclose(sp.k_axis[a], 2 * np.pi * S.fold(n[a]) / (n[a] * d[a]), rtol=4 * EPS, atol=0)
            used.append(check_reduced("sum axis", sp.axis[a].sum(), p_ref, x, ones))
        assert sp.total == again.total
        used.append(check_reduced("total", sp.total, p_ref, x, ones))
        sh, cnt, out, nout = S.shells(p_ref, n, d, edges)
        assert np.array_equal(sp.shell_count, cnt) and sp.outside_count == nout  # exact
        s = S.s_of(n, d)
        e2 = edges ** 2
        for j in range(S.NSHELL):
            used.append(check_reduced("shell", sp.shell[j], p_ref, x, (s >= e2[j]) & (s < e2[j + 1])))
        used.append(check_reduced("outside", sp.outside, p_ref, x, ~((s >= e2[0]) & (s < e2[-1]))))
        used.append(check_reduced("shells + outside", sp.shell.sum() + sp.outside, p_ref, x, ones))
        assert np.array_equal(sp.k_edges, edges)
    none = g.spectrum(x)
    assert none.shell.size == 0 and none.outside_count == x.size and none.outside == none.total == sp.total
    print(name, "largest share of the bound used:", max(used))
    assert g.poisson_solver == "cg" and g.gauss_info()["cleans"] == 0
    g.close()


# ---- 2. special inputs ------------------------------------------------------------------------------------------------------
def test_special_inputs(X):
    n, d = S.SPECIAL_N, S.SPECIAL_D
    nx, ny, nz = n
    N = nx * ny * nz
    g = X.Context("ecsim", n, d, 0.5)
    modes = all_modes(n)
    kj = lambda j: 2 * np.pi * (modes[:, 0] * j[2] / nx + modes[:, 1] * j[1] / ny + modes[:, 2] * j[0] / nz)  # noqa: E731
    for name, x in S.special_inputs().items():
        p, f = g.spectrum_power(x), g.spectrum_modes(x, modes)
        theory = None
        if name == "constant":
            theory = np.zeros(N, dtype=complex)
            theory[0] = 1.5 * np.sqrt(N)
        elif name.startswith("delta"):
            j = {"delta_origin": (0, 0, 0), "delta_last": (nz - 1, ny - 1, nx - 1), "delta_centre": (nz // 2, ny // 2, nx // 2)}[name]
            theory = np.exp(-1j * kj(j)) / np.sqrt(N)
        elif name.startswith("cos") or name != "sin_%d" % (nx // 2):
            m = int(name.split("_")[1])
            theory = np.zeros((nz, ny, nx), dtype=complex)
            amp = 0.5 * np.sqrt(N) * (1.0 if name.startswith("cos") else -1j)
            theory[0, 0, m] += amp
            theory[0, 0, (nx - m) % nx] += np.conj(amp)
            theory = theory.ravel()
        # the closed form of a cosine or a sine is that of the exact function, the input is its rounded samples: |dx| <= eps/2
        # per node, so |dF^| <= eps/2 sqrt(N) <= eps |x| (|x|^2 = N / 2) on top of the bound, and 2 sqrt(P) times that for P;
        # the constant and the deltas are exact in float64, and fftn sees the very x the device sees: no allowance
        trig = name.startswith(("cos", "sin"))
        for ref, slack in ([(theory, EPS * S.l2(x) if trig else 0.0)] if theory is not None else []) + [(S.dft(x).ravel(), 0.0)]:
            assert np.abs(f - ref).max() <= S.mode_bound(x) + slack, name
            p_ref = np.abs(ref.reshape(p.shape)) ** 2
            assert (np.abs(p - p_ref) <= S.power_bound(p_ref, x) + 2 * np.sqrt(p_ref) * slack).all(), name
        if name.startswith("delta"):
            assert np.abs(p - 1.0 / N).max() <= S.power_bound(np.full(p.shape, 1.0 / N), x).max()  # flat
    g.close()


# ---- 3. field sources -------------------------------------------------------------------------------------------------------
def test_field_component_is_the_host_scalar_bit_for_bit(X):
    n, d = (17, 9, 7), (0.25, 0.125, 0.5)
    g = X.Context("ecsim", n, d, 0.5)
    rng = np.random.default_rng(31)
    modes = all_modes(n)[::7]
    edges = S.shell_edges(n, d, "offset")
    for fid in (X.E, X.B):
        F = rng.normal(0.0, 2.0, (n[2], n[1], n[0], 3))
        g.set_field(fid, F)
        for c in range(3):
            x = np.ascontiguousarray(F[..., c])
            assert np.array_equal(g.spectrum_power(fid, c), g.spectrum_power(x))
            assert np.array_equal(g.spectrum_modes(fid, modes, c), g.spectrum_modes(x, modes))
            a, b = g.spectrum(fid, c, edges=edges), g.spectrum(x, edges=edges)
            assert all(np.array_equal(a.axis[i], b.axis[i]) for i in range(3)) and a.total == b.total
            assert np.array_equal(a.shell_count, b.shell_count)
        assert np.array_equal(g.get_field(fid), F)  # read in place, not written
    g.close()


def test_rho_is_the_residuals_charge(X):
    g, E, bg = TG.build(X, "17x9x7", 3, background=True, field="zero")
    n, d, _ = TG.GRIDS["17x9x7"]
    r = g.gauss_residual(X.E, want_residual=True)
    x = -r["residual"]  # = rho - mean at E = 0
    p_rho, p_host = g.spectrum_power("rho"), g.spectrum_power(x)
    rho = x + r["mean"]
    bound = S.power_bound(p_host, rho)
    diff = np.abs(p_rho - p_host)
    diff[0, 0, 0] = 0.0
    print("rho: share of the bound", (diff / bound).max())
    assert (diff <= bound).all()
    N = x.size
    # P(0) = N mean^2; the residual's single-pass mean of N values is within N eps mean|rho| of the exact one
    dmean = N * EPS * np.abs(rho).mean()
    assert abs(p_rho[0, 0, 0] - N * r["mean"] ** 2) <= 2 * N * abs(r["mean"]) * dmean + S.power_bound(N * r["mean"] ** 2, rho)
    f = g.spectrum_modes("rho", [(1, 0, 0), (0, -2, 3)])
    assert np.abs(f - g.spectrum_modes(x, [(1, 0, 0), (0, -2, 3)])).max() <= S.mode_bound(rho)
    assert np.array_equal(g.spectrum_power("rho"), p_rho)
    g.close()


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(X):
    n, d = (6, 5, 4), (0.5, 0.4, 0.6)
    g = X.Context("ecsim", n, d, 0.5)
    x = np.random.default_rng(5).normal(size=(4, 5, 6))
    sid, L = X.SPECTRUM_SOURCES, g.L
    refused = lambda words: pytest.raises(X.XpicError, match=words)  # noqa: E731
    with refused("unknown source"):
        g.spectrum_power(57, 0)
    with refused("unknown source"):
        g.spectrum_modes(-1, [(1, 0, 0)], 0)
    with refused("XPIC_W2 is the charge deposit's scratch"):
        g.spectrum_power(X.W2, 0)
    with refused("must be finite and >= 0"):  # (the package's own: the edges are |k|)
        g.spectrum(x, edges=[-1.0, 0.5, 1.0])
    for comp in (-1, 3):
        with refused("comp must be"):
            g.spectrum_power(X.E, comp)
        with refused("comp must be"):
            g.spectrum_probe(X.E, [(1, 0, 0)], comp=comp)
    bad = x.copy()
    bad[1, 2, 3] = np.nan
    for call in (lambda: g.spectrum_power(bad), lambda: g.spectrum(bad), lambda: g.spectrum_modes(bad, [(0, 0, 1)])):
        with refused("not finite"):
            call()
    with refused("nshell must be"):
        g.spectrum(x, nshell=-1)
    with refused("nshell must be"):
        g.spectrum(x, dk=0.01, nshell=X.SPECTRUM_MAX_SHELLS + 1)
    with refused("needs edges2"):
        g.spectrum(x, nshell=3)
    with refused("strictly ascending"):
        g.spectrum(x, edges=[0.0, 1.0, 1.0, 2.0])
    with refused("strictly ascending"):
        g.spectrum(x, edges=[0.0, 2.0, 1.0])
    with refused("edges2 is not finite"):
        g.spectrum(x, edges=[0.0, np.inf])
    with refused("must be finite and >= 0"):
        g.spectrum(x, edges=[0.0, np.nan])
    with refused("nmodes must be"):
        g.spectrum_modes(x, np.zeros((0, 3)))
    with refused("nmodes must be"):
        g.spectrum_probe(X.E, np.zeros((0, 3)), comp=0)
    with refused("every must be"):
        g.spectrum_probe(X.E, [(1, 0, 0)], comp=0, every=0)
    with refused("capacity must be"):
        g.spectrum_probe(X.E, [(1, 0, 0)], comp=0, capacity=0)
    m = np.array([[1, 0, 0]], dtype=np.int32)
    pid = X.C.c_int(-7)
    with refused("not a probe source"):
        g._ck(L.xpic_spectrum_probe_create(g.h, sid["host"], 0, 1, m.ctypes.data_as(X.CTYPES["const int32_t*"]), 1, 4, X.C.byref(pid)))
    assert pid.value == -7
    with refused("unknown or destroyed probe id"):
        X.SpectrumProbe(g, 0, 1).get()
    probe = g.spectrum_probe(X.E, [(1, 0, 0)], comp=0)
    stale = X.SpectrumProbe(g, probe.id, 1)
    probe.close()
    probe.close()  # (the handle knows it is closed)
    with refused("unknown or destroyed probe id"):
        stale.get()
    with refused("unknown or destroyed probe id"):
        stale.close()
    with refused("unknown or destroyed probe id"):
        X.SpectrumProbe(g, 99, 1).get()
    fresh = g.spectrum_probe(X.E, [(1, 0, 0)], comp=0)
    assert fresh.id != stale.id  # an id is never given twice: the stale handle stays refused
    with refused("unknown or destroyed probe id"):
        stale.get()
    fresh.close()
    assert g.poisson_solver == "cg" and g.gauss_info()["cleans"] == 0  # the kind and the counters are untouched
    g.close()
    ring, _, _ = TG.build(X, "17x9x7", 5, background=True, self_ring=True)
    for call in (lambda: ring.spectrum_power(X.E, 0), lambda: ring.spectrum("rho"), lambda: ring.spectrum_probe(X.E, [(1, 0, 0)], comp=0)):
        with refused("single-slab"):
            call()
    ring.close()
    long = X.Context("ecsim", (X.POISSON_MAX_EXTENT + 1, 2, 2), (0.5, 0.5, 0.5), 0.5)
    with refused("extents up to 1024"):
        long.spectrum_power(X.E, 0)
    long.close()


def test_a_cg_clean_after_spectrum_calls_returns_a_fresh_contexts_bits(X):
    def run(with_spectrum):
        g, E, bg = TG.build(X, "17x9x7", 2, background=True)
        if with_spectrum:
            g.spectrum_power(X.E, 1)
            g.spectrum("rho", dk=0.5, nshell=4)
            g.spectrum_modes(np.ones((7, 9, 17)), [(1, 2, 3)])
        c = g.gauss_clean(X.E, rtol=1e-10, want_phi=True)
        out = (c.iterations, c.before, c.after, c.mean, c.gphi, c.phi, g.get_field(X.E), g.gauss_info())
        g.close()
        return out
    a, b = run(False), run(True)
    assert a[:5] == b[:5] and np.array_equal(a[5], b[5]) and np.array_equal(a[6], b[6]) and a[7] == b[7]


# ---- 5. the probe -----------------------------------------------------------------------------------------------------------
MODES = [(1, 0, 0), (0, 1, 0), (-1, 2, 1), (2, 0, -1)]


# The loads: one particle per sort.  With many particles the deposits' floating-point atomics meet at shared nodes in an order
# that is not pinned, and two runs of the same input differ in their last bits before any probe has run (measured: max |dE|
# 6.7e-16 on test_gpu_es.py's load, 9.7e-17 on test_gpu_gauss.py's thermal one, after one step); a single particle's deposit
# writes every node once, and the sorts are deposited one launch after the other, so a run is reproducible bit for bit and
# a twin can be compared that way -- the rule tests/test_gpu_tracers.py and test_gpu_tracer_moments.py follow with their
# unloaded sorts.  The particles move, E and rho change every step.
LONE = [np.array([[1.30, 0.90, 0.60, 0.30, -0.20, 0.10]]), np.array([[2.10, 1.70, 1.10, -0.10, 0.25, -0.15]])]


def es_context(X):
    n, d = TE.GRIDS["6x6x6"]
    _, E, B = TE.load(n, d)
    return TE.context(X, n, d, LONE, E, B)


def ecsim_context(X):
    """test_gpu_gauss.py's riding context with the lone particles: started clean, the clean rides with every step"""
    g = X.Context("ecsim", TG.RIDE_N, TG.RIDE_D, TG.RIDE_DT)
    for (q, m), pts in zip(((-1.0, 1.0), (1.0, 16.0)), LONE):
        s = g.add_sort(4, 1.0, q, m, capacity=64)
        assert g.add_particles(s, pts) == 1
    shape = (TG.RIDE_N[2], TG.RIDE_N[1], TG.RIDE_N[0])
    g.set_field(X.B, np.zeros(shape + (3,)) + np.array([0.1, -0.2, 0.3]))
    g.set_tolerances(1e-12, 1e-50, 400)
    g.gauss_clean(X.E, rtol=TG.RIDE_RTOL)
    g.set_gauss_clean(1, rtol=TG.RIDE_RTOL)
    return g


def state(g, X):
    """the fields, and the particles of both sorts in a canonical order (the binning's arrival order is not pinned)"""
    out = [g.get_field(X.E), g.get_field(X.B)]
    for s in range(2):
        p = g.particles(s)[0]
        out.append(p[np.lexsort(p.T[::-1])])
    return out


@pytest.mark.parametrize("make", [es_context, ecsim_context], ids=["es", "ecsim"])
def test_probe_rides_and_leaves_the_run_alone(X, make):
    """rows equal spectrum_modes by hand on a twin, and the probed run equals the unprobed twin -- fields, particles,
    iterations, xpic_gauss_info -- bit for bit"""
    probed, twin = make(X), make(X)
    pe = probed.spectrum_probe(X.E, MODES, comp=0, every=2)
    pr = probed.spectrum_probe("rho", MODES[:2], every=3)
    small = probed.spectrum_probe(X.E, MODES, comp=2, every=2, capacity=2)
    by_hand = {}
    for step in range(1, 7):
        ia, ib = probed.step(), twin.step()
        assert ia == ib
        assert probed.gauss_info() == twin.gauss_info()
        if step % 2 == 0:
            by_hand[("E0", step)] = twin.spectrum_modes(X.E, MODES, 0)
            by_hand[("E2", step)] = twin.spectrum_modes(X.E, MODES, 2)
        if step % 3 == 0:
            by_hand[("rho", step)] = twin.spectrum_modes("rho", MODES[:2])
    for a, b in zip(state(probed, X), state(twin, X)):
        assert np.array_equal(a, b)  # the probed run is the unprobed one, bit for bit
    steps, f, dropped = pe.get()
    assert list(steps) == [2, 4, 6] and dropped == 0 and f.shape == (3, len(MODES))
    for i, s in enumerate(steps):
        assert np.array_equal(f[i], by_hand[("E0", s)])
    steps, f, dropped = pr.get()
    assert list(steps) == [3, 6] and dropped == 0
    for i, s in enumerate(steps):
        assert np.array_equal(f[i], by_hand[("rho", s)])
    steps, f, dropped = small.get(reset=True)
    assert list(steps) == [2, 4] and dropped == 1
    for i, s in enumerate(steps):
        assert np.array_equal(f[i], by_hand[("E2", s)])
    steps, f, dropped = small.get()
    assert steps.size == 0 and dropped == 0 and f.shape == (0, len(MODES))
    pe.close()
    probed.step(); twin.step()  # step 7: nothing records
    probed.step(); twin.step()  # step 8: the small probe records again, the closed one is gone
    steps, f, dropped = small.get()
    assert list(steps) == [8] and np.array_equal(f[0], twin.spectrum_modes(X.E, MODES, 2))
    assert np.array_equal(probed.get_field(X.E), twin.get_field(X.E))
    probed.close(); twin.close()


def test_probe_rows_on_a_load_whose_deposits_collide(X):
    """test_gpu_es.py's load, thousands of particles whose deposits meet at shared nodes: no twin of such a run is bit for
    bit, so the rows of E are held to spectrum_modes taken by hand on the probed context itself after each step -- the same
    state, the same kernels, the same bits --, those of "rho" within the deposit's own reordering, and the step counts of the run to those of an unprobed twin"""
    n, d = TE.GRIDS["7x6x9"]
    pts, E, B = TE.load(n, d)
    g, twin = TE.context(X, n, d, pts, E, B), TE.context(X, n, d, pts, E, B)
    pe = g.spectrum_probe(X.E, MODES, comp=1)
    pr = g.spectrum_probe("rho", MODES, every=2)
    hand_e, hand_r = [], []
    for step in range(1, 5):
        g.step(); twin.step()
        hand_e.append(g.spectrum_modes(X.E, MODES, 1))
        if step % 2 == 0:
            hand_r.append(g.spectrum_modes("rho", MODES))
    steps, f, dropped = pe.get()
    assert list(steps) == [1, 2, 3, 4] and dropped == 0 and np.array_equal(f, np.array(hand_e))
    steps, f, dropped = pr.get()
    # "rho" deposits afresh for every call, with the same unordered atomics: a node's sum of at most count(s) terms of one
    # sign moves by count(s) eps |rho_s(node)| at the most, and F^ is unitary: |dF^| <= eps sum_s count(s) |rho_s|_2
    rho_s = [g.charge_density(s) for s in range(2)]
    order = EPS * sum(g.count(s) * S.l2(rho_s[s]) for s in range(2))
    assert list(steps) == [2, 4] and dropped == 0
    assert np.abs(f - np.array(hand_r)).max() <= order + 2 * S.mode_bound(rho_s[0] + rho_s[1])
    # against the twin: the runs differ by the deposits' unordered atomics alone, and F^ is unitary: |dF^| <= |dE|_2
    dE = S.l2(g.get_field(X.E)[..., 1] - twin.get_field(X.E)[..., 1])
    assert np.abs(hand_e[-1] - twin.spectrum_modes(X.E, MODES, 1)).max() <= dE + 2 * S.mode_bound(g.get_field(X.E)[..., 1])
    assert g.count(0) == twin.count(0) and g.count(1) == twin.count(1)
    g.close(); twin.close()


# ---- 6. the host mirror's "FieldSpectrum" diagnostic ---------------------------------------------------------------------------
def test_host_mirror_field_spectrum(X, tmp_path):
    """tests/test_gpu_tracers.py's host configuration: ecsim on 8 x 8 x 8 with a sort that is never loaded and a coils field in
    B alone, so rot B drives E, both fields change every step and the executable's run and the same run made here agree bit
    for bit.  The files equal the Python calls on the same state; a config without the key writes none of them."""
    import json
    import os
    import subprocess

    exe = os.path.join(os.path.dirname(os.path.abspath(X.__file__)), "host", "xpic_hip.out")
    n, d, dt, nt, period = (8, 8, 8), 0.5, 0.5, 4, 2
    coils = [{"z0": 1.0, "R": 1.5, "I": 2.0}, {"z0": 3.0, "R": 1.5, "I": 2.0}]
    modes = [[1, 0, 0], [0, -1, 2], [3, 1, -1]]
    dk, nshell = 0.61, 5
    diags = [{"diagnostic": "FieldSpectrum", "field": "B", "comp": 2, "modes": modes, "dk": dk, "nshell": nshell},
             {"diagnostic": "FieldSpectrum", "field": "E", "comp": 0, "name": "ex", "modes": modes[:1]},
             {"diagnostic": "FieldSpectrum", "field": "rho", "name": "rho", "dk": dk, "nshell": nshell}]

    def run(sub, diagnostics):
        out = tmp_path / sub
        out.mkdir()
        cfg = {
            "Simulation": "ecsim", "OutputDirectory": str(out),
            "Geometry": {"x": 4.0, "y": 4.0, "z": 4.0, "t": nt * dt, "dx": d, "dy": d, "dz": d, "dt": dt, "diagnose_period": period * dt,
                         "da_boundary_x": "DM_BOUNDARY_PERIODIC", "da_boundary_y": "DM_BOUNDARY_PERIODIC",
                         "da_boundary_z": "DM_BOUNDARY_PERIODIC"},
            "Particles": [{"sort_name": "electrons", "Np": 1, "n": 1.0, "q": -1.0, "m": 1.0, "T": 0.0}],
            "Presets": [{"command": "SetMagneticField", "field": "B", "setter": {"name": "SetCoilsField", "coils": coils}}],
            "Diagnostics": diagnostics,
        }
        (out / "config.json").write_text(json.dumps(cfg))
        r = subprocess.run([exe, str(out / "config.json")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return out

    out = run("with", diags)
    g = X.Context("ecsim", n, (d, d, d), dt)
    g.add_sort(1, 1.0, -1.0, 1.0, capacity=1 << 16)
    g.set_coils_field([(c["z0"], c["R"], c["I"]) for c in coils], field=X.B)
    rows = {"": [], "_ex": []}
    for t in range(0, nt + 1):
        if t:
            g.step()
        if t % period:
            continue
        for suffix, source, comp, shells in (("", X.B, 2, True), ("_ex", X.E, 0, False), ("_rho", "rho", None, True)):
            sp = g.spectrum(source, comp, dk=dk, nshell=nshell) if shells else g.spectrum(source, comp)
            want = np.concatenate(sp.axis + [sp.shell])
            got = np.fromfile(out / ("field_spectrum" + suffix) / str(t), dtype=np.float64)
            assert got.shape == want.shape and np.array_equal(got, want), (suffix, t)
        rows[""].append((t, g.spectrum_modes(X.B, modes, 2)))
        rows["_ex"].append((t, g.spectrum_modes(X.E, modes[:1], 0)))
    assert np.abs(g.get_field(X.E)).max() > 0.0  # the fields did move
    for suffix, want in rows.items():
        table = np.loadtxt(out / "temporal" / ("field_modes%s.txt" % suffix), ndmin=2)
        assert table.shape == (len(want), 1 + 2 * len(want[0][1]))
        for line, (t, f) in zip(table, want):
            assert line[0] == t and np.array_equal(line[1:], np.column_stack([f.real, f.imag]).ravel()), (suffix, t)
    assert not (out / "temporal" / "field_modes_rho.txt").exists()  # (no "modes": no table)
    assert sorted(os.listdir(out / "field_spectrum")) == ["0", "2", "4"]
    g.close()
    # a config without the key runs as before: the same files but the diagnostic's
    plain = run("without", [])
    assert not any(p.startswith("field_") for p in os.listdir(plain)) and not (plain / "temporal" / "field_modes.txt").exists()
    assert sorted(os.listdir(plain / "temporal")) == sorted(f for f in os.listdir(out / "temporal") if not f.startswith("field_modes"))
    for f in os.listdir(plain / "temporal"):
        assert (plain / "temporal" / f).read_bytes() == (out / "temporal" / f).read_bytes(), f


# ---- 7. physics: the two-stream mode by the probe ---------------------------------------------------------------------------
def test_two_stream_seeded_mode_grows_at_the_theory_rate(X):
    """tests/test_gpu_es.py::test_two_stream_growth_rate's run -- the same load, steps and fitting window -- read off a
    probe on E_x instead of the field energy: |E^(MODE, 0, 0)|^2 grows at 2 gamma, every other (m, 0, 0) stays below it"""
    import two_stream as TS

    bm, n, d, k = TS.beams()
    g = X.Context("es", n, d, TS.DT)
    for pts in bm:
        s = g.add_sort(TS.PPC_BEAM, 0.5, -1.0, 1.0, capacity=2 * pts.shape[0])
        assert g.add_particles(s, pts) == pts.shape[0]
    g.gauss_clean(rtol=TE.RTOL, atol=1e-12)
    ms = list(range(1, n[0] // 2 + 1))
    probe = g.spectrum_probe(X.E, [(m, 0, 0) for m in ms], comp=0, capacity=700)
    for it in range(700):
        g.step()
    steps, f, dropped = probe.get()
    assert list(steps) == list(range(1, 701)) and dropped == 0
    t, w = steps * TS.DT, np.abs(f) ** 2
    seeded = w[:, ms.index(TS.MODE)]
    rate, npts = TS.fit_growth(t, seeded, 1e-6, 1e-2)
    theory = TS.gamma_theory(k)
    print("two-stream by the probe: rate", rate, "theory", theory, "points", npts)
    assert seeded.max() > 1e8 * seeded[0] and npts >= 100
    assert abs(rate - theory) <= 0.10 * theory, (rate, theory)
    i_sat = int(np.argmax(seeded))
    window = [i for i in range(i_sat) if 1e-6 * seeded[i_sat] <= seeded[i] <= 1e-2 * seeded[i_sat]]
    others = np.delete(w, ms.index(TS.MODE), axis=1)
    print("two-stream by the probe: largest other mode / seeded in the window", (others[window].max(axis=1) / seeded[window]).max())
    assert (others[window].max(axis=1) < seeded[window]).all()
    g.close()
