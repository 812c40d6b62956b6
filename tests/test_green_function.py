"""The lattice Green's function and local impurities on k meshes -- tb_model.green_function_mesh, impurity_t_matrix_mesh and
impurity_ldos_mesh -- against the NumPy restatement in gf_ref.py, the resolvent of the torus of the mesh and the identities of G.

Bounds.  G: (1e-10 + 1e-12 W / eta) max|reference|, W the width of the reference spectrum -- 1e-10 is the project's bound for the
density matrix, the second term its 1e-12 eigenvalue parity passed through 1 / (z - E)^2.  T, det and ldos0 + dldos: 1e-10 kappa
max|reference|, kappa = cond(1 - g V) from the reference, asserted to be at most 100.  The measured errors are in DESIGN.md section 30."""
import numpy as np
import pytest

import dm_ref as dmr
import gf_ref as gfr
import helpers as hp
from helpers import quiet
from test_density_matrix import NPERIOD, build, haldane, r_list

import pythtb_amd as tb

ETA = 0.05
FREQ_BLOCK = 4                                                # frequencies per workgroup of the kernels (GF_WB of tbk_gf.h)
MODELS = ["square_1", "haldane_2a", "haldane_2b", "chain3_3", "kane_mele_4", "cubic16_16", "haldane3x3_18", "haldane4x4_32",
          "chain3x11_33"]


def close(what, got, want, bound):
    scale = np.max(np.abs(want))
    err = np.max(np.abs(got - want))
    print("%s: max abs error / max |reference| = %.3e (bound %.3e)" % (what, err / scale, bound))
    assert err <= bound * scale, (what, err / scale)


def g_bound(ev, eta):
    return 1e-10 + 1e-12 * (ev.max() - ev.min()) / eta


def three_sites(m):
    n = m._nsta
    return [(0, [0] * m._dim_k), (n - 1, [1] + [0] * (m._dim_k - 1)), (1 % n, [-1] + [2] * (m._dim_k - 1))]


def hermitian(rng, ns, scale):
    a = rng.normal(size=(ns, ns)) + 1j * rng.normal(size=(ns, ns))
    return scale * (a + a.conj().T)


# ---------------------------------------------------------------- CPU: argument errors
def test_argument_errors_without_gpu():
    m = haldane()
    flat = quiet(tb.tb_model, 0, 2, hp.LAT, hp.ORB)
    site, v = [(0, [0, 0])], [1.0]
    calls = (lambda mm, mesh, w=0.1, eta=0.1, **kw: mm.green_function_mesh(mesh, w, eta, **kw),
             lambda mm, mesh, w=0.1, eta=0.1, **kw: mm.impurity_t_matrix_mesh(mesh, w, eta, site, v),
             lambda mm, mesh, w=0.1, eta=0.1, **kw: mm.impurity_ldos_mesh(mesh, w, eta, site, v, **kw))
    for call in calls:
        with pytest.raises(Exception, match="dim_k"):
            call(flat, [4])
        for bad in ([8], [8, 0], [8, 8, 8], [-3, 4]):
            with pytest.raises(Exception, match="[Mm]esh"):
                call(m, bad)
        for bad in ([], [[0.1, 0.2]], [0.1, np.nan], np.nan, [np.inf], np.zeros(65537), "x"):
            with pytest.raises(Exception, match="omega"):
                call(m, [4, 4], w=bad)
        for bad in (0.0, -0.1, np.nan, np.inf, "x", [0.1, 0.2]):
            with pytest.raises(Exception, match="eta"):
                call(m, [4, 4], eta=bad)
    for call in (calls[0], calls[2]):
        for bad in ([0.5, 0.0], [[0, 0], [1, 0.25]], [np.nan, 0], [0], [[0, 0, 0]], [[[0, 0]]], np.zeros((0, 2), dtype=int), [2 ** 30, 0],
                    [[0, -2 ** 30]], np.zeros((4097, 2), dtype=int), "ab", [[0, 1j]]):
            with pytest.raises(Exception, match="R_list"):
                call(m, [4, 4], R_list=bad)
        for bad in ([0, 0], [0, 2], [-3], [], [[0]], [0.0], list(range(33))):
            with pytest.raises(Exception, match="states"):
                call(m, [4, 4], states=bad)
    big = quiet(haldane().make_supercell, [[16, 0], [0, 16]])               # 512 states
    with pytest.raises(Exception, match="split omega or R_list"):
        big.green_function_mesh([2, 2], np.zeros(17), 0.1)
    with pytest.raises(Exception, match="states"):
        big.green_function_mesh([2, 2], 0.0, 0.1, states=list(range(33)))
    with pytest.raises(Exception, match="split omega or R_list"):
        m.green_function_mesh([4, 4], np.zeros(257), 0.1, R_list=np.zeros((4096, 2), dtype=int))
    with pytest.raises(Exception, match="states"):
        big.impurity_ldos_mesh([2, 2], 0.0, 0.1, site, v)                    # all 512 states as probes
    # sites and potential
    for call in (lambda s, p: m.impurity_t_matrix_mesh([4, 4], 0.1, 0.1, s, p), lambda s, p: m.impurity_ldos_mesh([4, 4], 0.1, 0.1, s, p)):
        for bad in ([], [(0, [0, 0])] * 2, [(0, [0, 0]), (0, [4, -8])], [(0, [0])], [(0, [0, 0, 0])], [(2, [0, 0])], [(0.5, [0, 0])],
                    [(0, [0.5, 0])], [(0, [2 ** 30, 0])], [(a % 2, [a // 2, 0]) for a in range(17)], 3, [0, 1]):
            with pytest.raises(Exception, match="sites"):
                call(bad, np.ones(len(bad)) if isinstance(bad, list) and len(bad) else [1.0])
        two = [(0, [0, 0]), (1, [1, 0])]
        for bad in ([[0.0, 1.0], [0.5, 0.0]], [[0.0, 1j], [1j, 0.0]], [1.0], [1.0, 2.0, 3.0], [1.0, np.nan], [[1.0, 0.0], [0.0, np.inf]],
                    [1.0, 1j], np.zeros((2, 2, 2)), "x"):
            with pytest.raises(Exception, match="potential"):
                call(two, bad)
    # the cap of the internal problem of the LDOS: a 64 x 64 map has 8191 probe-site differences, 4 entries each, at 300 frequencies
    grid = np.array([[a, b] for a in range(64) for b in range(64)])
    with pytest.raises(Exception, match="split omega or R_list"):
        m.impurity_ldos_mesh([256, 256], np.zeros(300), 0.1, site, v, R_list=grid)


# ---------------------------------------------------------------- CPU: the reference's own identities
REF_CASES = ((lambda: haldane(), [4, 5]), (lambda: hp.kane_mele(tb.tb_model), [3, 4]), (lambda: hp.chain3(tb.tb_model, -1.3, 2.0, 0.3), [7]))
REF_Z = np.array([0.3 + 0.05j, -1.1 + 0.2j])


def test_numpy_green_is_the_torus_inverse():
    """inv(z - H_T)[(0, i), (R, j)] = G_ij(R, z) for every cell R of the torus.  Bound 1e-12: two complex float64 sums of at most 60
    terms of size O(1 / eta) stay near 1e-14 (the worst seen when this was written: 2e-15)."""
    for make, mesh in REF_CASES:
        m = make()
        n, cs = m._nsta, gfr.cells(mesh)
        g = gfr.green(m, mesh, REF_Z, cs)
        ht = gfr.torus_hamiltonian(m, mesh)
        for w, z in enumerate(REF_Z):
            inv = np.linalg.inv(z * np.identity(len(ht)) - ht)
            err = max(np.max(np.abs(inv[:n, r * n:(r + 1) * n] - g[w, r])) for r in range(len(cs)))
            print("mesh %s z=%s: %.3e" % (mesh, z, err))
            assert err <= 1e-12


def test_numpy_dyson_on_the_torus():
    """Three sites with a random Hermitian V: ldos0 + dldos is the diagonal of inv(z - H_T - V) at every (cell, state), to 1e-12 of
    its largest value (a 3 x 3 solve of a matrix of condition number below 10; the worst seen: 2e-15)."""
    rng = np.random.default_rng(3)
    for make, mesh in REF_CASES:
        m = make()
        n, cs = m._nsta, gfr.cells(mesh)
        sites = [(0, cs[0]), (n - 1, cs[1]), (1 % n, cs[-1])]
        v = hermitian(rng, 3, 0.5)
        assert np.all(gfr.t_matrix(m, mesh, REF_Z, sites, v)[2] <= 10.0)
        l0, dl = gfr.impurity_ldos(m, mesh, REF_Z, sites, v, cs)
        hv = gfr.torus_with_impurity(m, mesh, sites, v)
        for w, z in enumerate(REF_Z):
            want = (-np.imag(np.diag(np.linalg.inv(z * np.identity(len(hv)) - hv))) / np.pi).reshape(len(cs), n)
            err = np.max(np.abs(l0[w][None, :] + dl[w] - want)) / np.max(np.abs(want))
            print("mesh %s z=%s: %.3e" % (mesh, z, err))
            assert err <= 1e-12


def lorentz_dos(ev, w, eta):
    """(1 / N_k) sum_{k,n} (eta / pi) / ((w - E)^2 + eta^2), (nw,)."""
    w = np.atleast_1d(w)
    return (eta / np.pi / ((w[:, None] - ev.ravel()[None, :]) ** 2 + eta ** 2)).sum(axis=1) / ev.shape[0]


def test_numpy_ldos_trace_and_conjugate_symmetry():
    for make, mesh in REF_CASES:
        m = make()
        ev = dmr.levels(m, mesh)
        w = np.array([0.3, -1.1, 2.0])
        g = gfr.green(m, mesh, w + 1j * ETA)[:, 0]
        tr = -np.imag(np.trace(g, axis1=1, axis2=2)) / np.pi
        assert np.max(np.abs(tr - lorentz_dos(ev, w, ETA))) <= 1e-12 * np.max(tr)
        rs = r_list(mesh)[:-NPERIOD]
        up = gfr.green(m, mesh, w + 1j * ETA, rs)
        dn = gfr.green(m, mesh, w - 1j * ETA, -rs)
        assert np.max(np.abs(np.conj(up) - np.transpose(dn, (0, 1, 3, 2)))) <= 1e-13 * np.max(np.abs(up))


# ---------------------------------------------------------------- GPU: against gf_ref
@pytest.mark.gpu
@pytest.mark.parametrize("name", MODELS)
def test_models(name):
    m, mesh, _ = build(name)
    pairs = gfr.eigenpairs(m, mesh)
    ev = pairs[1]
    lo, width = ev.min(), ev.max() - ev.min()
    rs = r_list(mesh)
    n = m._nsta
    one = (m._norb, 2, m._norb, 2) if m._nspin == 2 else (n, n)
    bound = g_bound(ev, ETA)
    for nw in (1, 3, FREQ_BLOCK + 1):
        if nw == 3:
            w = lo + width * np.array([0.7, 0.2, 0.7])          # out of order, with a repeat
        else:
            w = lo + width * np.linspace(-0.1, 1.05, nw + 1)[1:]
        got = m.green_function_mesh(mesh, w, ETA, rs)
        assert got.dtype == complex and got.shape == (nw, len(rs)) + one
        got = got.reshape(nw, len(rs), n, n)
        close("%s nw=%d G" % (name, nw), got, gfr.green(m, mesh, w + 1j * ETA, rs, None, pairs), bound)
        for r in range(len(rs) - NPERIOD, len(rs)):            # an R equal to a mesh period is R = 0, to the last bit
            np.testing.assert_array_equal(got[:, r], got[:, 0])
        if nw == 3:
            np.testing.assert_array_equal(got[0], got[2])
            assert m.green_function_mesh(mesh, w[1], ETA).shape == one       # a scalar omega, R_list=None: no leading axes
            np.testing.assert_array_equal(m.green_function_mesh(mesh, w[1], ETA, rs[4]).reshape(n, n), got[1, 4])
            np.testing.assert_array_equal(m.green_function_mesh(mesh, w, ETA, rs).reshape(got.shape), got)   # two calls


@pytest.mark.gpu
def test_two_chunks_tiled():
    """40 states on 37 x 37: 1310 points per chunk, then a ragged second one of 59 -- fewer points than the 164 k-groups.  Two
    frequencies and 14 lattice vectors: the partial sums of one launch hold one frequency, so every chunk takes two launches."""
    m = quiet(haldane().make_supercell, [[5, 0], [0, 4]])
    mesh = [37, 37]
    assert m._nsta == 40
    rs = np.array([[0, 0], [1, 0], [-1, 2], [37, 0]] + [[a, b] for a in (-2, 3) for b in (-1, 0, 1, 2, 40)])
    assert len(rs) == 14
    pairs = gfr.eigenpairs(m, mesh)
    w = np.array([0.2, -1.3])
    got = m.green_function_mesh(mesh, w, ETA, rs)
    close("40 states, two chunks: G", got, gfr.green(m, mesh, w + 1j * ETA, rs, None, pairs), g_bound(pairs[1], ETA))
    np.testing.assert_array_equal(got[:, 3], got[:, 0])
    np.testing.assert_array_equal(got[1, 13], m.green_function_mesh(mesh, w[1], ETA, rs[13]))   # the second launch's, alone
    np.testing.assert_array_equal(got[0, 13], m.green_function_mesh(mesh, w[0], ETA, rs[13]))


@pytest.mark.gpu
def test_two_chunks_lds():
    """32 states on 46 x 46: 2048 points per chunk, then 68; 512 k-groups of four one-point batches, then 68 groups with a point and
    444 without."""
    m = quiet(haldane().make_supercell, [[4, 0], [0, 4]])
    mesh = [46, 46]
    rs = np.array([[0, 0], [0, -1], [47, 3], [0, 46], [1, 1]])
    pairs = gfr.eigenpairs(m, mesh)
    w = np.array([0.4, -2.1])
    got = m.green_function_mesh(mesh, w, ETA, rs)
    close("32 states, two chunks: G", got, gfr.green(m, mesh, w + 1j * ETA, rs, None, pairs), g_bound(pairs[1], ETA))
    np.testing.assert_array_equal(got[:, 3], got[:, 0])
    np.testing.assert_array_equal(got[1, 4], m.green_function_mesh(mesh, w[1], ETA, rs[4]))


@pytest.mark.gpu
@pytest.mark.parametrize("name,states", [("kane_mele_4", [3, 0, -2]), ("cubic16_16", [11, 2, 15, 7, 0]), ("chain3x11_33", [32, 5, -16, 0, 20])])
def test_selection(name, states):
    """A subset of the states in scrambled order (one negative index): the block of the full matrix, the same bits alone and inside
    longer omega and R lists, and no spin axes."""
    m, mesh, _ = build(name)
    n = m._nsta
    pairs = gfr.eigenpairs(m, mesh)
    ev = pairs[1]
    w = ev.min() + (ev.max() - ev.min()) * np.array([0.6, 0.15, 0.9, 0.4, 0.35, 0.05])
    rs = r_list(mesh)[:-NPERIOD]
    got = m.green_function_mesh(mesh, w, ETA, rs, states=states)
    na = len(states)
    assert got.shape == (len(w), len(rs), na, na)
    bound = g_bound(ev, ETA)
    close("%s selection against the reference" % name, got, gfr.green(m, mesh, w + 1j * ETA, rs, states, pairs), bound)
    idx = np.array(states) % n
    full = m.green_function_mesh(mesh, w, ETA, rs).reshape(len(w), len(rs), n, n)[:, :, idx][:, :, :, idx]
    close("%s selection against the block of the full call" % name, got, full, bound)
    alone = m.green_function_mesh(mesh, w[4], ETA, rs[2], states=states)
    assert alone.shape == (na, na)
    np.testing.assert_array_equal(alone, got[4, 2])
    np.testing.assert_array_equal(m.green_function_mesh(mesh, w[1:3], ETA, rs[3:], states=states), got[1:3, 3:])
    one = m.green_function_mesh(mesh, w[0], ETA, states=states[1:2])
    assert one.shape == (1, 1)
    close("%s one state" % name, one, gfr.green(m, mesh, w[0] + 1j * ETA, None, states[1:2], pairs)[0, 0], bound)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["haldane_2a", "kane_mele_4", "chain3x11_33"])
def test_green_function_properties(name):
    m, mesh, _ = build(name)
    n = m._nsta
    ev = np.asarray(m.solve_all(dmr.mesh_points(m, mesh))).T                 # the device's own eigenvalues, (nk, n)
    lo, width = ev.min(), ev.max() - ev.min()
    w = lo + width * np.linspace(-0.2, 1.2, 9)
    g = m.green_function_mesh(mesh, w, ETA).reshape(len(w), n, n)
    ldos = -np.imag(np.einsum("wii->wi", g)) / np.pi
    assert np.all(ldos > 0.0)
    want = lorentz_dos(ev, w, ETA)
    err = np.max(np.abs(ldos.sum(axis=1) - want)) / np.max(want)
    print("%s: trace of the LDOS against the Lorentzian sum: %.3e" % (name, err))
    assert err <= 1e-10
    # far outside the spectrum: z G(0) -> 1 and z G(R != 0) -> 0, to O(|E|_max / |z|)
    emax = np.max(np.abs(ev))
    rs = r_list(mesh)[:-NPERIOD]
    for far in (1e3 * emax, -1e4 * emax):
        z = far + 1j * ETA
        zg = z * m.green_function_mesh(mesh, far, ETA, rs).reshape(len(rs), n, n)
        tol = 2.0 * emax / abs(z)
        assert np.max(np.abs(zg[0] - np.identity(n))) <= tol and np.max(np.abs(zg[1:])) <= tol


# ---------------------------------------------------------------- GPU: the impurity
def impurity_cases():
    rng = np.random.default_rng(11)
    for name, make, mesh in (("haldane", lambda: haldane(), [6, 5]), ("kane_mele", lambda: hp.kane_mele(tb.tb_model), [3, 4])):
        m = make()
        yield name + " one site", m, mesh, [(0, [0, 0])], np.array([1.5])
        yield name + " three sites, on-site", m, mesh, three_sites(m), np.array([1.5, -0.7, 0.4])
        yield name + " three sites, Hermitian", m, mesh, three_sites(m), hermitian(rng, 3, 0.4)


@pytest.mark.gpu
def test_t_matrix_and_ldos():
    eta = 0.1
    for what, m, mesh, sites, v in impurity_cases():
        n = m._nsta
        pairs = gfr.eigenpairs(m, mesh)
        ev = pairs[1]
        w = np.array([ev.min() + 0.3 * (ev.max() - ev.min()), ev.max() + 0.5, 0.5 * (ev.min() + ev.max())])
        t_ref, det_ref, kappa = gfr.t_matrix(m, mesh, w + 1j * eta, sites, v, pairs)
        assert np.all(kappa <= 100.0), kappa
        bound = 1e-10 * kappa.max()
        t, det = m.impurity_t_matrix_mesh(mesh, w, eta, sites, v, return_det=True)
        assert t.shape == (3, len(sites), len(sites)) and det.shape == (3,)
        close(what + ": T", t, t_ref, bound)
        close(what + ": det", det, det_ref, bound)
        np.testing.assert_array_equal(m.impurity_t_matrix_mesh(mesh, w[1], eta, sites, v), t[1])
        cs = gfr.cells(mesh)
        l0, dl = m.impurity_ldos_mesh(mesh, w, eta, sites, v, R_list=cs)
        assert l0.shape == (3, n) and dl.shape == (3, len(cs), n) and l0.dtype == float and dl.dtype == float
        assert np.all(l0 > 0.0)
        hv = gfr.torus_with_impurity(m, mesh, sites, v)
        want = np.array([(-np.imag(np.diag(np.linalg.inv(z * np.identity(len(hv)) - hv))) / np.pi).reshape(len(cs), n) for z in w + 1j * eta])
        close(what + ": ldos0 + dldos on the torus", l0[:, None, :] + dl, want, bound)
        assert np.all(l0[:, None, :] + dl > 0.0)
        # probe states in scrambled order, one cell, a scalar frequency
        sel = [n - 1, 0]
        l1, d1 = m.impurity_ldos_mesh(mesh, w[2], eta, sites, v, R_list=cs[7], states=sel)
        assert l1.shape == (2,) and d1.shape == (2,)
        close(what + ": selected probes", l1 + d1, want[2, 7, sel], bound)


@pytest.mark.gpu
def test_impurity_on_the_tiled_form():
    """33 states on a mesh of 5: the impurity calls on the tiled kernel, whose internal selection is the probe states followed by
    the site states not among them (here 33 of them: three tiles per side)."""
    m, mesh, _ = build("chain3x11_33")
    n, eta = m._nsta, 0.1
    pairs = gfr.eigenpairs(m, mesh)
    ev = pairs[1]
    sites = [(0, [0]), (n - 1, [1]), (17, [-2])]
    v = hermitian(np.random.default_rng(11), 3, 0.4)
    w = np.array([ev.min() + 0.3 * (ev.max() - ev.min()), ev.max() + 0.5, 0.5 * (ev.min() + ev.max())])
    t_ref, det_ref, kappa = gfr.t_matrix(m, mesh, w + 1j * eta, sites, v, pairs)
    assert np.all(kappa <= 100.0), kappa
    bound = 1e-10 * kappa.max()
    t, det = m.impurity_t_matrix_mesh(mesh, w, eta, sites, v, return_det=True)
    close("33 states: T", t, t_ref, bound)
    close("33 states: det", det, det_ref, bound)
    cs = gfr.cells(mesh)
    sel = [s for s in range(n) if s != 17][::-1]                             # 32 probe states, scrambled; 0 and 32 are sites too
    l0, dl = m.impurity_ldos_mesh(mesh, w, eta, sites, v, R_list=cs, states=sel)
    assert l0.shape == (3, 32) and dl.shape == (3, len(cs), 32) and np.all(l0 > 0.0)
    hv = gfr.torus_with_impurity(m, mesh, sites, v)
    want = np.array([(-np.imag(np.diag(np.linalg.inv(z * np.identity(len(hv)) - hv))) / np.pi).reshape(len(cs), n) for z in w + 1j * eta])
    close("33 states: ldos0 + dldos on the torus", l0[:, None, :] + dl, want[:, :, sel], bound)


@pytest.mark.gpu
def test_gap_state():
    """Gapped Haldane with one strong on-site impurity: |det(1 - g V)| over a scan of the gap is smallest where the torus with V has
    its in-gap eigenvalue, to within the scan step."""
    m, mesh, u = hp.haldane(tb.tb_model, delta=0.7), [12, 10], 5.0
    s = np.sort(dmr.levels(m, mesh).ravel())
    j = int(np.argmax(np.diff(s)))
    lo, hi = s[j], s[j + 1]
    assert hi - lo > 0.3
    sites = [(0, [0, 0])]
    e = np.linalg.eigvalsh(gfr.torus_with_impurity(m, mesh, sites, [u]))
    inside = e[(e > lo + 1e-9) & (e < hi - 1e-9)]
    assert len(inside) == 1
    scan = np.linspace(lo, hi, 43)[1:-1]
    _, det = m.impurity_t_matrix_mesh(mesh, scan, 1e-3, sites, [u], return_det=True)
    at = scan[int(np.argmin(np.abs(det)))]
    print("bound state at %.6f, |det| smallest at %.6f, scan step %.6f" % (inside[0], at, scan[1] - scan[0]))
    assert abs(at - inside[0]) <= scan[1] - scan[0]
