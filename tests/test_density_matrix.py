"""The occupied states on k meshes -- tb_model.thermodynamics_mesh, fermi_level_mesh and density_matrix_mesh -- against the NumPy
restatement in dm_ref.py, the closed forms of the one-band square lattice and the identities of the density matrix.

Measured on an MI355X (max abs error / max |reference|; the bounds are 1e-10 for N, E, S and D, 1e-12 of the spectrum's width
for the Fermi level and the edges at kT = 0, 1e-8 absolute for the occupations of the mean-field loop): see DESIGN.md section 27."""
import numpy as np
import pytest

import dm_ref as dmr
import helpers as hp
from helpers import quiet

import pythtb_amd as tb

KT = 0.07


def haldane(delta=0.2):
    return hp.haldane(tb.tb_model, delta=delta)


def square(t=-1.0):
    """One orbital on the square lattice, on a lattice point: E = 2 t (cos 2 pi k_x + cos 2 pi k_y)."""
    m = quiet(tb.tb_model, 2, 2, [[1.0, 0.0], [0.0, 1.0]], [[0.0, 0.0]])
    m.set_hop(t, 0, 0, [1, 0])
    m.set_hop(t, 0, 0, [0, 1])
    return m


def honeycomb_spinful(t=-1.0):
    m = quiet(tb.tb_model, 2, 2, hp.LAT, hp.ORB, nspin=2)
    m.set_hop(t, 0, 1, [0, 0])
    m.set_hop(t, 1, 0, [1, 0])
    m.set_hop(t, 1, 0, [0, 1])
    return m


def safe_mu(ev, target):
    """The midpoint of the two reference levels around `target`: a gap of at least 2e-6, asserted, so that no kT = 0 occupation
    hangs on the last bits of an eigenvalue."""
    s = np.unique(ev.ravel())
    j = int(np.searchsorted(s, target))
    if j == 0:
        return s[0] - 1.0
    if j == len(s):
        return s[-1] + 1.0
    assert s[j] - s[j - 1] >= 2e-6
    return 0.5 * (s[j - 1] + s[j])


def widest_gap(ev):
    """The middle of the widest gap between consecutive levels of the whole mesh."""
    s = np.sort(ev.ravel())
    j = int(np.argmax(np.diff(s)))
    assert s[j + 1] - s[j] > 0.05
    return 0.5 * (s[j] + s[j + 1])


def r_list(mesh):
    """0, nearest neighbours, negative entries, an R beyond the mesh period -- and, LAST, three R equal to a mesh period."""
    d = len(mesh)
    unit = [[1 if a == b else 0 for b in range(d)] for a in range(d)]
    rs = [[0] * d] + unit + [[-x for x in u] for u in unit[:1]]
    rs.append([(-1) ** a * (1 + a) for a in range(d)])                       # (1, -2, 3)
    rs.append([mesh[0] + 1] + [-2] * (d - 1))                                # beyond the period
    rs.append([mesh[a] if a == 0 else 0 for a in range(d)])                  # periods
    rs.append([-2 * mesh[a] if a == d - 1 else 0 for a in range(d)])
    rs.append([(-1) ** a * mesh[a] for a in range(d)])
    return np.array(rs, dtype=int)


NPERIOD = 3


def close(what, got, want, rel=1e-10):
    scale = np.max(np.abs(want))
    if scale == 0.0:
        assert np.all(got == 0.0)
        return
    err = np.max(np.abs(got - want))
    print("%s: max abs error / max |reference| = %.3e" % (what, err / scale))
    assert err <= rel * scale, (what, err / scale)


# ---------------------------------------------------------------- CPU: argument errors
def test_argument_errors_without_gpu():
    m = haldane()
    flat = quiet(tb.tb_model, 0, 2, hp.LAT, hp.ORB)
    for call in (lambda mm, mesh: mm.thermodynamics_mesh(mesh, [0.0]), lambda mm, mesh: mm.fermi_level_mesh(mesh, 1.0),
                 lambda mm, mesh: mm.density_matrix_mesh(mesh, 0.0)):
        with pytest.raises(Exception, match="dim_k"):
            call(flat, [4])
        for bad in ([8], [8, 0], [8, 8, 8], [-3, 4]):
            with pytest.raises(Exception):
                call(m, bad)
    for kT in (-1e-3, np.inf, np.nan, "x"):
        with pytest.raises(Exception, match="kT"):
            m.thermodynamics_mesh([4, 4], [0.0], kT)
        with pytest.raises(Exception, match="kT"):
            m.fermi_level_mesh([4, 4], 1.0, kT)
        with pytest.raises(Exception, match="kT"):
            m.density_matrix_mesh([4, 4], 0.0, kT)
    for bad in ([], [[0.1, 0.2]], [0.1, np.nan], [np.inf], np.zeros(8193), np.nan):
        with pytest.raises(Exception, match="fermi_levels"):
            m.thermodynamics_mesh([4, 4], bad)
    for bad in (np.nan, np.inf, [0.0, 0.1], "x"):
        with pytest.raises(Exception, match="fermi_level"):
            m.density_matrix_mesh([4, 4], bad)
    # fillings: shape, range, a non-integer count at kT = 0
    for bad in ([], [[1.0]], np.ones(65), np.nan, [1.0, np.inf]):
        with pytest.raises(Exception, match="n_electrons"):
            m.fermi_level_mesh([4, 4], bad)
    for bad in (0.0, 2.0, -0.5, 2.5, 1.0 + 1e-3, 1.03125 + 1e-5, [1.0, 0.3]):    # 16 points: 1.03125 is 16.5 / 16
        with pytest.raises(Exception, match="n_electrons"):
            m.fermi_level_mesh([4, 4], bad)
    for bad in (0.0, 2.0, -0.1, 2.1, [1.0, 2.0]):
        with pytest.raises(Exception, match="n_electrons"):
            m.fermi_level_mesh([4, 4], bad, kT=0.05)
    with pytest.raises(Exception, match="return_edges"):
        m.fermi_level_mesh([4, 4], 1.0, kT=0.05, return_edges=True)
    # lattice vectors: shape, integers, size, the cap on the result
    for bad in ([0.5, 0.0], [[0, 0], [1, 0.25]], [np.nan, 0], [0], [[0, 0, 0]], [[[0, 0]]], np.zeros((0, 2), dtype=int), [2 ** 30, 0],
                [[0, -2 ** 30]], np.zeros((4097, 2), dtype=int), "ab", [[0, 1j]]):
        with pytest.raises(Exception, match="R_list"):
            m.density_matrix_mesh([4, 4], 0.0, R_list=bad)
    big = quiet(haldane().make_supercell, [[16, 0], [0, 16]])               # 512 states: 16 R at most
    with pytest.raises(Exception, match="nR"):
        big.density_matrix_mesh([2, 2], 0.0, R_list=np.zeros((17, 2), dtype=int))


# ---------------------------------------------------------------- CPU: the reference's own identities and closed forms
def ref_identities(m, mesh, mu, kT):
    table = dmr.hopping_table(m)
    rs = np.array([r for r, _ in table] + [[-x for x in r] for r, _ in table])
    d = dmr.density_matrix(m, mesh, mu, kT, rs)
    nt = len(table)
    n_e_s = dmr.thermodynamics(m, mesh, mu, kT)[:, 0]
    zero = [i for i, (r, _) in enumerate(table) if not any(r)][0]
    assert abs(np.trace(d[zero]).real - n_e_s[0]) <= 1e-13 * d.shape[1] and abs(np.trace(d[zero]).imag) <= 1e-13
    for i in range(nt):
        assert np.max(np.abs(d[nt + i] - d[i].conj().T)) <= 1e-13           # D_ji(-R) = conj D_ij(R)
    scale = sum(np.abs(t).sum() for _, t in table)
    assert abs(dmr.energy_from_density_matrix(table, d[:nt]) - n_e_s[1]) <= 1e-13 * scale


def test_numpy_trace_hermiticity_energy():
    for m, mesh in ((haldane(), [4, 5]), (hp.kane_mele(tb.tb_model), [3, 4]), (hp.chain3(tb.tb_model, -1.3, 2.0, 0.3), [7])):
        ev = dmr.levels(m, mesh)
        ref_identities(m, mesh, safe_mu(ev, widest_gap(ev)), 0.0)
        ref_identities(m, mesh, safe_mu(ev, ev.mean() - 0.4), 0.0)            # inside a band
        ref_identities(m, mesh, 0.13, KT)


def test_numpy_idempotent_on_the_torus():
    """Gapped Haldane on 4 x 5 at kT = 0: D is a projector on the torus of the mesh, sum_{R', l} D_il(R') D_lj(R - R') = D_ij(R)."""
    m, mesh = haldane(), [4, 5]
    ev = dmr.levels(m, mesh)
    cells = np.array([[a, b] for a in range(mesh[0]) for b in range(mesh[1])])
    d = dmr.density_matrix(m, mesh, safe_mu(ev, widest_gap(ev)), 0.0, cells).reshape(mesh[0], mesh[1], 2, 2)
    for R in cells:
        acc = np.zeros((2, 2), dtype=complex)
        for Rp in cells:
            q = (R - Rp) % np.array(mesh)
            acc += d[Rp[0], Rp[1]] @ d[q[0], q[1]]
        assert np.max(np.abs(acc - d[R[0], R[1]])) <= 1e-13


def test_numpy_square_lattice_closed_forms():
    """Half filling on 8 x 8: the Fermi level cuts the degenerate group at E = 0 (14 mesh points of the nested Fermi surface), so both
    edges are 0; and D(0) = 1/2 at kT > 0 by particle-hole symmetry."""
    m, mesh = square(), [8, 8]
    mu, (lo, hi) = dmr.fermi_level(m, mesh, 0.5, 0.0)
    assert abs(mu) <= 1e-12 and abs(lo) <= 1e-12 and abs(hi) <= 1e-12
    assert dmr.thermodynamics(m, mesh, 1e-9, 0.0)[0, 0] > 0.5                # the whole group is counted
    d = dmr.density_matrix(m, mesh, 0.0, 0.3)
    assert d.shape == (1, 1, 1) and abs(d[0, 0, 0] - 0.5) <= 1e-14
    assert abs(dmr.fermi_level(m, mesh, 0.5, 0.3)[0]) <= 1e-13


# ---------------------------------------------------------------- GPU: against dm_ref
def build(name):
    """(model, mesh, target of the Fermi level; None: the middle of the widest gap)."""
    if name == "square_1":                                    # 63 points: ragged against the 64 points of a batch
        return square(), [7, 9], 0.3
    if name == "haldane_2a":
        return haldane(), [12, 10], 0.0
    if name == "haldane_2b":
        return haldane(), [13, 5], -1.1
    if name == "chain3_3":
        return hp.chain3(tb.tb_model, -1.3, 2.0, 0.3), [41], None
    if name == "kane_mele_4":
        return hp.kane_mele(tb.tb_model), [6, 7], None
    if name == "cubic16_16":
        return hp.cubic16(tb.tb_model), [3, 4, 5], 0.0
    if name == "haldane3x3_18":                               # 324 elements of P(k): two per lane of the LDS kernel
        return quiet(haldane().make_supercell, [[3, 0], [0, 3]]), [3, 2], None
    if name == "haldane4x4_32":                               # the last size of the LDS kernel (four elements per lane)
        return quiet(haldane().make_supercell, [[4, 0], [0, 4]]), [3, 2], None
    if name == "chain3x11_33":                                # the first size of the tiled kernel; 33 = 2 x 16 + 1
        return quiet(hp.chain3(tb.tb_model, -1.3, 2.0, 0.3).make_supercell, [[11]]), [5], None
    raise KeyError(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["square_1", "haldane_2a", "haldane_2b", "chain3_3", "kane_mele_4", "cubic16_16", "haldane3x3_18",
                                  "haldane4x4_32", "chain3x11_33"])
def test_models(name):
    m, mesh, target = build(name)
    ev = dmr.levels(m, mesh)
    if target is None:
        target = widest_gap(ev)
    rs = r_list(mesh)
    n = m._nsta
    for kT, mu in ((0.0, safe_mu(ev, target)), (KT, target + 0.11)):
        got = m.thermodynamics_mesh(mesh, [mu], kT)
        close("%s kT=%g N E S" % (name, kT), got, dmr.thermodynamics(m, mesh, [mu], kT, ev))
        want = dmr.density_matrix(m, mesh, mu, kT, rs)
        got = m.density_matrix_mesh(mesh, mu, kT, rs)
        assert got.dtype == complex
        one = (m._norb, 2, m._norb, 2) if m._nspin == 2 else (n, n)
        assert got.shape == (len(rs),) + one
        assert m.density_matrix_mesh(mesh, mu, kT).shape == one   # R_list=None: R = 0, no leading axis
        got = got.reshape(len(rs), n, n)
        close("%s kT=%g D" % (name, kT), got, want)
        for r in range(len(rs) - NPERIOD, len(rs)):            # an R equal to a mesh period is R = 0
            assert np.max(np.abs(got[r] - got[0])) <= 1e-13
        assert np.max(np.abs(got[0] - got[0].conj().T)) <= 1e-13


@pytest.mark.gpu
def test_two_chunks_tiled():
    """40 states on 37 x 37: 32 MiB / (40^2 16 B) = 1310 points per chunk, then a ragged second one of 59 -- fewer points than
    the 164 k-groups.  14 lattice vectors: 12 fit the partial sums of one launch, so every chunk takes two."""
    m = quiet(haldane().make_supercell, [[5, 0], [0, 4]])
    mesh = [37, 37]
    assert m._nsta == 40
    rs = np.array([[0, 0], [1, 0], [-1, 2], [37, 0]] + [[a, b] for a in (-2, 3) for b in (-1, 0, 1, 2, 40)])
    assert len(rs) == 14
    mu, kT = 0.2, KT
    got = m.density_matrix_mesh(mesh, mu, kT, rs)
    close("40 states, two chunks: D", got, dmr.density_matrix(m, mesh, mu, kT, rs))
    assert np.max(np.abs(got[3] - got[0])) <= 1e-13
    np.testing.assert_array_equal(got[13], m.density_matrix_mesh(mesh, mu, kT, rs[13]))   # the second launch's R, alone
    close("40 states: N E S", m.thermodynamics_mesh(mesh, mu, kT), dmr.thermodynamics(m, mesh, mu, kT)[:, 0])


@pytest.mark.gpu
def test_two_chunks_lds():
    """32 states on 46 x 46: 2048 points per chunk, then 68; 512 k-groups of four one-point batches, then 68 groups with a point
    and 444 without."""
    m = quiet(haldane().make_supercell, [[4, 0], [0, 4]])
    mesh = [46, 46]
    rs = np.array([[0, 0], [0, -1], [47, 3], [0, 46], [1, 1]])
    ev = dmr.levels(m, mesh)
    mu = safe_mu(ev, widest_gap(ev))
    got = m.density_matrix_mesh(mesh, mu, 0.0, rs)
    close("32 states, two chunks: D", got, dmr.density_matrix(m, mesh, mu, 0.0, rs))
    assert np.max(np.abs(got[3] - got[0])) <= 1e-13


@pytest.mark.gpu
def test_thermodynamics_levels():
    m, mesh = haldane(), [12, 10]
    ev = dmr.levels(m, mesh)
    lo, hi = ev.min() - 1.0, ev.max() + 1.0
    rng = np.random.default_rng(5)
    for kT in (0.0, KT):
        for nmu in (1, 3, 300):
            mus = rng.uniform(lo, hi, nmu)
            if nmu >= 3:
                mus[0], mus[1] = hi, lo                       # above and below the whole spectrum, out of order
            if nmu == 300:
                mus[7] = mus[200] = mus[50]                   # repeated levels
            if kT == 0.0:
                mus = np.array([safe_mu(ev, x) if lo < x < hi else x for x in mus])
            got = m.thermodynamics_mesh(mesh, mus, kT)
            assert got.shape == (3, nmu) and got.dtype == float
            want = dmr.thermodynamics(m, mesh, mus, kT, ev)
            for c, nm in enumerate("NES"):
                close("kT=%g nmu=%d %s" % (kT, nmu, nm), got[c], want[c])
            if kT == 0.0:
                assert np.all(got[2] == 0.0)                  # S is exactly 0
                np.testing.assert_array_equal(got[0], want[0])   # N: an integer count / N_k
                if nmu >= 3:
                    assert got[0, 0] == 2.0 and got[0, 1] == 0.0 and got[1, 1] == 0.0
            if nmu == 300:
                assert np.all(got[:, 7] == got[:, 50]) and np.all(got[:, 200] == got[:, 50])
            one = m.thermodynamics_mesh(mesh, mus[-1], kT)    # a scalar drops the axis: the level's own value
            assert one.shape == (3,)
            np.testing.assert_array_equal(one, got[:, -1])
            np.testing.assert_array_equal(got, m.thermodynamics_mesh(mesh, mus, kT))


@pytest.mark.gpu
def test_fermi_level_zero_temperature():
    m = haldane()
    for mesh in ([12, 10], [13, 5]):
        ev = dmr.levels(m, mesh)
        nk = ev.shape[0]
        s = np.sort(ev.ravel())
        width = s[-1] - s[0]
        inside = next(c for c in range(nk // 3, nk) if s[c] - s[c - 1] >= 2e-6)   # inside the lower band
        assert s[nk] - s[nk - 1] > 0.05
        cs = [nk, inside]
        for c in cs:
            mu, edges = m.fermi_level_mesh(mesh, c / nk, return_edges=True)
            want_mu, want_edges = dmr.fermi_level(m, mesh, c / nk, 0.0, ev)
            print("c=%d: mu error / width %.3e, edges %.3e" % (c, abs(mu - want_mu) / width, np.max(np.abs(edges - want_edges)) / width))
            assert isinstance(mu, float) and edges.shape == (2,)
            assert abs(mu - want_mu) <= 1e-12 * width and np.max(np.abs(edges - np.array(want_edges))) <= 1e-12 * width
            assert mu == 0.5 * (edges[0] + edges[1]) and edges[0] < edges[1]
            assert m.thermodynamics_mesh(mesh, mu, 0.0)[0] == c / nk             # exactly c levels
            assert m.fermi_level_mesh(mesh, c / nk) == mu
        both, e2 = m.fermi_level_mesh(mesh, [c / nk for c in cs], return_edges=True)
        assert both.shape == (2,) and e2.shape == (2, 2)
        assert both[0] == m.fermi_level_mesh(mesh, cs[0] / nk) and both[1] == m.fermi_level_mesh(mesh, cs[1] / nk)


@pytest.mark.gpu
def test_fermi_level_cuts_a_degenerate_group():
    """The half-filled square lattice on 8 x 8: equal edges, and the count at that mu is more than c."""
    m, mesh = square(), [8, 8]
    mu, edges = m.fermi_level_mesh(mesh, 0.5, return_edges=True)
    assert abs(mu) <= 1e-12 * 8.0 and np.max(np.abs(edges)) <= 1e-12 * 8.0
    count = m.thermodynamics_mesh(mesh, mu, 0.0)[0]
    print("levels at or below mu: %g of 64 (c = 32)" % (count * 64))
    assert count >= 0.5                                       # (more than c where the group's levels are equal to the last bit)
    d = m.density_matrix_mesh(mesh, 0.0, 0.3)
    assert d.shape == (1, 1) and abs(d[0, 0] - 0.5) <= 1e-10
    assert abs(m.fermi_level_mesh(mesh, 0.5, kT=0.3)) <= 1e-10


@pytest.mark.gpu
def test_fermi_level_thermal():
    m, mesh, kT = haldane(), [12, 10], 0.05
    ev = dmr.levels(m, mesh)
    n = m._nsta
    count = lambda mu: dmr.thermodynamics(m, mesh, mu, kT, ev)[0, 0]
    for nel, metallic in ((0.7, True), (1.0, False)):
        mu = m.fermi_level_mesh(mesh, nel, kT=kT)
        print("n=%g: |N_ref(mu) - n| = %.3e" % (nel, abs(count(mu) - nel)))
        assert isinstance(mu, float) and abs(count(mu) - nel) <= 1e-12 * n
        if metallic:
            want = dmr.fermi_level(m, mesh, nel, kT, ev)[0]
            print("n=%g: mu - reference root = %.3e" % (nel, mu - want))
            assert abs(mu - want) <= 1e-10
        assert mu == m.fermi_level_mesh(mesh, nel, kT=kT)
    fills = np.array([0.3, 1.0, 0.7, 1.9, 1.25])
    mus = m.fermi_level_mesh(mesh, fills, kT=kT)
    assert mus.shape == (5,)
    for j, nel in enumerate(fills):
        assert mus[j] == m.fermi_level_mesh(mesh, nel, kT=kT)                    # bit for bit
        assert abs(count(mus[j]) - nel) <= 1e-12 * n


# ---------------------------------------------------------------- GPU: properties of the density matrix
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["haldane_2a", "kane_mele_4", "chain3x11_33"])
def test_density_matrix_properties(name):
    m, mesh, _ = build(name)
    n = m._nsta
    ev = dmr.levels(m, mesh)
    table = dmr.hopping_table(m)
    nt = len(table)
    rs = np.array([r for r, _ in table] + [[-x for x in r] for r, _ in table])
    zero = [i for i, (r, _) in enumerate(table) if not any(r)][0]
    scale = sum(np.abs(t).sum() for _, t in table)
    for kT, mu in ((0.0, safe_mu(ev, ev.mean() - 0.3)), (KT, 0.13)):
        d = m.density_matrix_mesh(mesh, mu, kT, rs).reshape(len(rs), n, n)
        n_e_s = m.thermodynamics_mesh(mesh, mu, kT)
        tr = np.trace(d[zero])
        print("%s kT=%g: trace - N = %.3e" % (name, kT, abs(tr - n_e_s[0])))
        assert abs(tr - n_e_s[0]) <= 1e-10 * n
        for i in range(nt):
            assert np.max(np.abs(d[nt + i] - d[i].conj().T)) <= 1e-12
        e = dmr.energy_from_density_matrix(table, d[:nt])
        print("%s kT=%g: energy identity %.3e of sum |t|" % (name, kT, abs(e - n_e_s[1]) / scale))
        assert abs(e - n_e_s[1]) <= 1e-10 * scale
        np.testing.assert_array_equal(d, m.density_matrix_mesh(mesh, mu, kT, rs).reshape(d.shape))   # two calls
    # below and above the whole spectrum at kT = 0
    rs = r_list(mesh)[:-NPERIOD]
    assert np.all(m.density_matrix_mesh(mesh, ev.min() - 1.0, 0.0, rs) == 0.0)
    full = m.density_matrix_mesh(mesh, ev.max() + 1.0, 0.0, rs).reshape(len(rs), n, n)
    assert np.max(np.abs(full[0] - np.identity(n))) <= 1e-12 and np.max(np.abs(full[1:])) <= 1e-12
    # the same R alone and inside a list of 9
    nine = np.array([rs[i % len(rs)] + (i // len(rs)) for i in range(9)])
    many = m.density_matrix_mesh(mesh, 0.13, KT, nine)
    for i in (0, 3, 4, 8):
        alone = m.density_matrix_mesh(mesh, 0.13, KT, nine[i])
        assert alone.shape == many.shape[1:]
        np.testing.assert_array_equal(alone, many[i])


# ---------------------------------------------------------------- GPU: a mean-field loop
@pytest.mark.gpu
def test_hubbard_mean_field_loop():
    """Spinful honeycomb, U = 3 |t|, 12 x 12, kT = 0.05, two electrons per cell, a staggered start, exactly 8 Hartree iterations --
    set_onsite, fermi_level_mesh, density_matrix_mesh at R = 0 -- against the same loop in NumPy.  A map of slope O(U chi0) <~ 3
    can amplify 1e-12 per step to about 1e-8 over 8 steps: that is the bound."""
    mesh, U, kT, nel = [12, 12], 3.0, 0.05, 2.0
    occ0 = [[0.8, 0.2], [0.2, 0.8]]
    dev = dmr.hartree_loop(honeycomb_spinful(), mesh, U, kT, nel, occ0, 8,
                           lambda m: m.fermi_level_mesh(mesh, nel, kT=kT), lambda m, mu: m.density_matrix_mesh(mesh, mu, kT))
    ref = dmr.hartree_loop(honeycomb_spinful(), mesh, U, kT, nel, occ0, 8,
                           lambda m: dmr.fermi_level(m, mesh, nel, kT)[0], lambda m, mu: dmr.density_matrix(m, mesh, mu, kT)[0])
    print("occupations, max deviation per iteration:", np.max(np.abs(dev - ref), axis=(1, 2)))
    assert np.max(np.abs(dev - ref)) <= 1e-8
    moment = dev[-1, 0, 0] - dev[-1, 0, 1] - dev[-1, 1, 0] + dev[-1, 1, 1]
    print("staggered moment after 8 iterations: %.6f" % moment)
    assert abs(moment) > 0.1 and abs(dev[-1].sum() - nel) <= 1e-10
