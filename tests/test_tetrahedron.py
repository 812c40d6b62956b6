"""The linear tetrahedron method on k meshes -- tb_model.tetrahedron_dos_mesh, tetrahedron_weights_mesh and
tetrahedron_fermi_level_mesh -- against the NumPy restatement in tetra_ref.py, and tetra_ref.py itself against sampled integrals,
centred differences and the 1 / N^2 convergence of N(E) on the square lattice.

Bounds: 1e-10 of max |reference| for idos, the weights (plain, corrected, derivative), dos and pdos; 1e-12 of the scale for the
identities on the device alone.  Every energy is asserted to lie at least 1e-9 of the spectrum's width from every reference level,
so no branch hangs on the last bits of an eigenvalue.

Measured on an MI355X (max abs error / max |reference| over the cases below): idos 4e-15, dos 4.5e-14 (cubic16), pdos 8e-14
(cubic16), weights 1.9e-14, derivative weights 1.3e-13 (the chain on [41]), corrected weights 9e-15.  No model needed more than
1e-10 for dos or pdos, so no allowance from a perturbation of the reference's eigenvalues is applied."""
import functools

import numpy as np
import pytest

import helpers as hp
import tetra_ref as tr
from helpers import quiet

import pythtb_amd as tb


def square(t=-1.0):
    m = quiet(tb.tb_model, 2, 2, [[1.0, 0.0], [0.0, 1.0]], [[0.0, 0.0]])
    m.set_hop(t, 0, 0, [1, 0])
    m.set_hop(t, 0, 0, [0, 1])
    return m


def flat_band():
    """One orbital with on-site energy 0.5 and no hopping."""
    m = quiet(tb.tb_model, 2, 2, [[1.0, 0.0], [0.0, 1.0]], [[0.0, 0.0]])
    m.set_onsite([0.5])
    return m


CASES = {
    "chain41": (lambda: hp.chain3(tb.tb_model, -1.3, 2.0, 0.3), [41]),
    "chain2": (lambda: hp.chain3(tb.tb_model, -1.3, 2.0, 0.3), [2]),
    "chain1": (lambda: hp.chain3(tb.tb_model, -1.3, 2.0, 0.3), [1]),
    "haldane": (lambda: hp.haldane(tb.tb_model, delta=0.2), [12, 10]),
    "graphene": (lambda: hp.graphene(tb.tb_model), [12, 12]),
    "square": (square, [8, 8]),
    "kane_mele": (lambda: hp.kane_mele(tb.tb_model), [8, 6]),
    "cubic16": (lambda: hp.cubic16(tb.tb_model), [5, 4, 3]),
    "random3d": (lambda: hp.random_model(tb.tb_model, 3, 3, 1, 11), [6, 5, 4]),
    "random34": (lambda: hp.random_model(tb.tb_model, 34, 2, 1, 12), [6, 6]),
    "big40": (lambda: hp.random_model(tb.tb_model, 40, 2, 1, 13), [40, 36]),
}
DOS_CASES = [c for c in CASES if c != "big40"]
PDOS_CASES = {"haldane": None, "cubic16": None, "random3d": None, "big40": [3, 17, 39, 0]}   # None: every state


@functools.lru_cache(maxsize=None)
def case(name):
    """(model, mesh, E (N_k, n), u (N_k, n, n), energies) of a case; the reference is computed once and left unchanged."""
    build, mesh = CASES[name]
    m = build()
    ev, u = tr.eigenpairs(m, mesh)
    ev.setflags(write=False)
    u.setflags(write=False)
    en = energies_for(ev, 12 if name == "big40" else 39)
    en.setflags(write=False)
    return m, mesh, ev, u, en


def energies_for(ev, count):
    """`count` energies from below the spectrum to above it, unsorted, and the fourth one again; each at least 1e-9 of the width from
    every level."""
    lo, hi = float(ev.min()), float(ev.max())
    width = hi - lo
    en = lo - 0.07 * width + 1.14 * width * (np.arange(count) + 0.3718) / count
    np.random.default_rng(5).shuffle(en)
    en = np.append(en, en[3])
    assert margin(ev, en) >= 1e-9 * width
    assert en.min() < lo and en.max() > hi
    return en


def margin(ev, en):
    s = np.unique(ev.ravel())
    j = np.clip(np.searchsorted(s, en), 1, len(s) - 1) if len(s) > 1 else np.zeros(len(en), dtype=int)
    return float(np.min(np.minimum(np.abs(en - s[j - 1]), np.abs(en - s[j]))))


@functools.lru_cache(maxsize=None)
def reference_dos(name):
    _, mesh, ev, _, en = case(name)
    g, big = tr.dos(ev, mesh, en)
    g.setflags(write=False)
    big.setflags(write=False)
    return g, big


def inner_energy(name):
    """The energy of the case's list inside the spectrum where the reference's total DOS is largest: a Fermi level that cuts bands
    (where the DOS vanishes everywhere, as on a single mesh point: one that leaves bands on both sides)."""
    _, _, ev, _, en = case(name)
    g, big = reference_dos(name)
    if g.any():
        return float(en[np.argmax(g.sum(axis=0))])
    return float(en[np.argmin(np.abs(big.sum(axis=0) - 0.5 * ev.shape[1]))])


def close(what, got, want, rel=1e-10):
    scale = np.max(np.abs(want))
    err = np.max(np.abs(got - want))
    print("%s: max abs error %.3e, max |reference| %.3e, ratio %.3e" % (what, err, scale, err / scale if scale else 0.0))
    assert err <= rel * scale, (what, err, scale)


# ---------------------------------------------------------------- CPU: argument errors
def test_argument_errors_without_gpu():
    m = hp.haldane(tb.tb_model, delta=0.2)
    flat = quiet(tb.tb_model, 0, 2, hp.LAT, hp.ORB)
    cube = hp.random_model(tb.tb_model, 3, 3, 1, 11)
    calls = (lambda mm, mesh: mm.tetrahedron_dos_mesh(mesh, [0.0]), lambda mm, mesh: mm.tetrahedron_weights_mesh(mesh, 0.0),
             lambda mm, mesh: mm.tetrahedron_fermi_level_mesh(mesh, 1.0))
    for call in calls:
        with pytest.raises(Exception, match="dim_k"):
            call(flat, [4])
        for bad in ([8], [8, 0], [8, 8, 8], [-3, 4], [65536, 32768]):
            with pytest.raises(Exception):
                call(m, bad)
    for bad in ([], [[0.1, 0.2]], [0.1, np.nan], [np.inf], np.zeros(65537), 0.3, "x"):
        with pytest.raises(Exception, match="energies"):
            m.tetrahedron_dos_mesh([4, 4], bad)
    for bad in ([], [0, 0], [2], [-1], [0.5], [[0]], np.arange(17)):
        with pytest.raises(Exception, match="states"):
            m.tetrahedron_dos_mesh([4, 4], [0.0], states=bad)
    big = quiet(hp.haldane(tb.tb_model, delta=0.2).make_supercell, [[16, 0], [0, 16]])      # 512 states
    with pytest.raises(Exception, match="2\\*\\*22"):
        big.tetrahedron_dos_mesh([2, 2], np.zeros(8193), per_band=True)
    with pytest.raises(Exception, match="2\\*\\*22"):
        big.tetrahedron_dos_mesh([2, 2], np.zeros(8192), per_band=True, states=[0, 1])
    with pytest.raises(Exception, match="2\\*\\*22"):
        big.tetrahedron_dos_mesh([2, 2], np.zeros(65536), states=np.arange(16) * 3, per_band=True)
    for bad in (np.nan, np.inf, [0.0, 0.1], "x"):
        with pytest.raises(Exception, match="fermi_level"):
            m.tetrahedron_weights_mesh([4, 4], bad)
    with pytest.raises(Exception, match="correction"):
        m.tetrahedron_weights_mesh([4, 4], 0.0, correction=True)
    with pytest.raises(Exception, match="correction"):
        cube.tetrahedron_weights_mesh([4, 4, 4], 0.0, correction=True, derivative=True)
    for bad in (np.nan, np.inf, 0.0, 2.0, -0.5, 2.5, [1.0, 0.5], "x"):
        with pytest.raises(Exception, match="n_electrons"):
            m.tetrahedron_fermi_level_mesh([4, 4], bad)


# ---------------------------------------------------------------- CPU: tetra_ref against things that do not depend on it
def random_simplices(rng, dim, count):
    return np.sort(rng.uniform(-1.0, 1.0, (count, dim + 1)), axis=1)


def closed_sums(e, E):
    """(N_T, g_T) of sorted simplices of volume 1 strictly inside a branch, from the closed forms for the sums."""
    dim = e.shape[1] - 1
    if dim == 1:
        t = (E - e[:, 0]) / (e[:, 1] - e[:, 0])
        return t, 1.0 / (e[:, 1] - e[:, 0])
    if dim == 2:
        e1, e2, e3 = e.T
        lowb = E < e2
        n1, g1 = (E - e1) ** 2 / ((e2 - e1) * (e3 - e1)), 2.0 * (E - e1) / ((e2 - e1) * (e3 - e1))
        n2, g2 = 1.0 - (e3 - E) ** 2 / ((e3 - e1) * (e3 - e2)), 2.0 * (e3 - E) / ((e3 - e1) * (e3 - e2))
        return np.where(lowb, n1, n2), np.where(lowb, g1, g2)
    e1, e2, e3, e4 = e.T
    e21, e31, e41, e32, e42, e43 = e2 - e1, e3 - e1, e4 - e1, e3 - e2, e4 - e2, e4 - e3
    n1, g1 = (E - e1) ** 3 / (e21 * e31 * e41), 3.0 * (E - e1) ** 2 / (e21 * e31 * e41)
    x = E - e2
    n2 = (e21 ** 2 + 3.0 * e21 * x + 3.0 * x ** 2 - (e31 + e42) * x ** 3 / (e32 * e42)) / (e31 * e41)
    g2 = (3.0 * e21 + 6.0 * x - 3.0 * (e31 + e42) * x ** 2 / (e32 * e42)) / (e31 * e41)
    n3, g3 = 1.0 - (e4 - E) ** 3 / (e41 * e42 * e43), 3.0 * (e4 - E) ** 2 / (e41 * e42 * e43)
    b1, b2 = E < e2, (E >= e2) & (E < e3)
    return np.where(b1, n1, np.where(b2, n2, n3)), np.where(b1, g1, np.where(b2, g2, g3))


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_ref_weights_sum_to_the_closed_forms_in_every_branch(dim):
    rng = np.random.default_rng(100 + dim)
    e = random_simplices(rng, dim, 400)
    for branch in range(dim):
        E = e[:, branch] + rng.uniform(0.05, 0.95, len(e)) * (e[:, branch + 1] - e[:, branch])
        for i in range(len(e)):
            # slots in a random order: the result follows the slots
            perm = rng.permutation(dim + 1)
            w, d = tr.simplex_weights(e[i:i + 1, perm], E[i])
            ws, ds = tr.simplex_weights(e[i:i + 1], E[i])
            assert np.array_equal(w[0], ws[0, perm]) and np.array_equal(d[0], ds[0, perm])
            nt, gt = closed_sums(e[i:i + 1], E[i])
            assert abs(ws.sum() - nt[0]) <= 1e-12 and abs(ds.sum() - gt[0]) <= 1e-11 * max(1.0, abs(gt[0]))
            assert np.all(ws >= -1e-15) and np.all(ds.sum() >= 0.0)


@pytest.mark.parametrize("dim", [2, 3])
def test_ref_weights_are_continuous_across_the_inner_corners(dim):
    rng = np.random.default_rng(200 + dim)
    e = random_simplices(rng, dim, 200)
    for j in range(1, dim):
        for i in range(len(e)):
            below, _ = tr.simplex_weights(e[i:i + 1], np.nextafter(e[i, j], -np.inf))
            at, _ = tr.simplex_weights(e[i:i + 1], e[i, j])
            assert np.max(np.abs(below - at)) <= 1e-12


@pytest.mark.parametrize("dim", [2, 3])
def test_ref_weights_against_a_sampled_integral(dim):
    rng = np.random.default_rng(300 + dim)
    nsamp = 400000
    lam = rng.dirichlet(np.ones(dim + 1), nsamp)                     # uniform on the simplex
    for _ in range(4):
        e = rng.uniform(-1.0, 1.0, dim + 1)
        x = rng.uniform(-1.0, 1.0, dim + 1)
        for E in np.sort(e)[:-1] + 0.5 * np.diff(np.sort(e)):
            f = (lam @ e <= E) * (lam @ x)
            w, _ = tr.simplex_weights(e[None, :], E)
            err = abs(float(w[0] @ x) - f.mean())
            assert err <= 5.0 * f.std() / np.sqrt(nsamp) + 1e-12, (e, x, E, err)


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_ref_dos_weights_against_a_centred_difference(dim):
    rng = np.random.default_rng(400 + dim)
    e = random_simplices(rng, dim, 200)
    h = 1e-6
    for branch in range(dim):
        gap = e[:, branch + 1] - e[:, branch]
        ok = gap > 0.05                                              # (the centred difference's own error grows with 1 / gap^3)
        E = e[:, branch] + rng.uniform(0.1, 0.9, len(e)) * gap
        for i in np.flatnonzero(ok):
            _, d = tr.simplex_weights(e[i:i + 1], E[i])
            wp, _ = tr.simplex_weights(e[i:i + 1], E[i] + h)
            wm, _ = tr.simplex_weights(e[i:i + 1], E[i] - h)
            num = (wp - wm) / (2.0 * h)
            assert np.max(np.abs(num - d)) <= 1e-6 * max(1.0, np.max(np.abs(d))), (e[i], E[i])


def test_ref_correction_sums_to_zero():
    rng = np.random.default_rng(450)
    e = rng.uniform(-1.0, 1.0, (300, 4))
    w0, _ = tr.simplex_weights(e, 0.1)
    w1, _ = tr.simplex_weights(e, 0.1, correction=True)
    assert np.max(np.abs(w0.sum(axis=1) - w1.sum(axis=1))) <= 1e-14
    assert np.max(np.abs(w0 - w1)) > 1e-4


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_ref_tie_rule(dim):
    nv = dim + 1
    for equal in range(2, nv + 1):
        for start in range(nv - equal + 1):
            e = np.arange(nv, dtype=float)
            e[start:start + equal] = e[start]
            for perm in (np.arange(nv), np.arange(nv)[::-1]):
                ep = e[perm][None, :]
                for E in np.concatenate([np.unique(e), np.unique(e) + 0.25, [e.min() - 1.0, e.max() + 1.0]]):
                    w, d = tr.simplex_weights(ep, E)
                    assert np.all(np.isfinite(w)) and np.all(np.isfinite(d))
                    assert np.all(w >= -1e-15) and w.sum() <= 1.0 + 1e-14 and np.all(d >= -1e-15)
                    if E >= e.max():
                        assert np.array_equal(w, np.full((1, nv), 1.0 / nv)) and not d.any()
                    elif E <= e.min():
                        assert not w.any() and not d.any()
                    # equal corners carry equal weights
                    for a in range(nv):
                        for b in range(a + 1, nv):
                            if ep[0, a] == ep[0, b]:
                                assert abs(w[0, a] - w[0, b]) <= 1e-14 and abs(d[0, a] - d[0, b]) <= 1e-13
    flat = np.full((1, nv), 0.5)
    for E, want in ((0.4999, 0.0), (0.5, 1.0), (0.6, 1.0)):
        w, d = tr.simplex_weights(flat, E)
        assert w.sum() == pytest.approx(want, abs=1e-15) and not d.any()


def test_ref_count_converges_like_one_over_n_squared():
    """N(E = -1) of E = 2 t (cos 2 pi k_x + cos 2 pi k_y), t = -1, evaluated directly: the error against the 512^2 value falls by a
    factor between 3 and 5 from 32^2 to 64^2."""
    def count(nmesh):
        k = np.arange(nmesh) / nmesh
        ev = -2.0 * (np.cos(2.0 * np.pi * k)[:, None] + np.cos(2.0 * np.pi * k)[None, :])
        return tr.count(ev.reshape(-1, 1), [nmesh, nmesh], -1.0)
    fine = count(512)
    e32, e64 = abs(count(32) - fine), abs(count(64) - fine)
    print("N(-1): 512^2 %.12f, error at 32^2 %.3e, at 64^2 %.3e, ratio %.3f" % (fine, e32, e64, e32 / e64))
    assert 3.0 <= e32 / e64 <= 5.0


# ---------------------------------------------------------------- GPU: against tetra_ref
@functools.lru_cache(maxsize=None)
def device_dos(name):
    m, mesh, _, _, en = case(name)
    return m.tetrahedron_dos_mesh(mesh, en, per_band=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", DOS_CASES)
def test_dos_and_idos_against_reference(name):
    m, mesh, ev, _, en = case(name)
    g_ref, n_ref = reference_dos(name)
    g, big = device_dos(name)
    assert g.shape == big.shape == (ev.shape[1], len(en))
    close(name + " idos", big, n_ref)
    close(name + " dos", g, g_ref)
    # the totals, and N above the spectrum
    gt, nt = m.tetrahedron_dos_mesh(mesh, en)
    assert gt.shape == nt.shape == (len(en),)
    scale = max(1.0, np.max(np.abs(g_ref.sum(axis=0))))
    assert np.max(np.abs(gt - g.sum(axis=0))) <= 1e-12 * scale and np.max(np.abs(nt - big.sum(axis=0))) <= 1e-12 * ev.shape[1]
    assert nt[np.argmax(en)] == ev.shape[1] and nt[np.argmin(en)] == 0.0 and gt[np.argmax(en)] == 0.0
    assert np.array_equal(g[:, 3], g[:, -1]) and np.array_equal(big[:, 3], big[:, -1])       # the repeated energy


@pytest.mark.gpu
@pytest.mark.parametrize("name", DOS_CASES)
def test_weights_against_reference_and_identities(name):
    m, mesh, ev, _, en = case(name)
    mu = inner_energy(name)
    j = int(np.flatnonzero(en == mu)[0])
    g, big = device_dos(name)
    nk = ev.shape[0]
    w = m.tetrahedron_weights_mesh(mesh, mu)
    d = m.tetrahedron_weights_mesh(mesh, mu, derivative=True)
    assert w.shape == d.shape == (ev.shape[1], nk)
    close(name + " weights", w, tr.weights(ev, mesh, mu))
    close(name + " derivative weights", d, tr.weights(ev, mesh, mu, derivative=True))
    # sum_k weights = per-band idos, sum_k derivative weights = per-band dos
    assert np.max(np.abs(w.sum(axis=1) - big[:, j])) <= 1e-12
    assert np.max(np.abs(d.sum(axis=1) - g[:, j])) <= 1e-12 * max(1.0, np.max(np.abs(g[:, j])))
    assert np.array_equal(w, m.tetrahedron_weights_mesh(mesh, mu))
    if len(mesh) == 3:
        wc = m.tetrahedron_weights_mesh(mesh, mu, correction=True)
        close(name + " corrected weights", wc, tr.weights(ev, mesh, mu, correction=True))
        assert np.max(np.abs(wc.sum(axis=1) - w.sum(axis=1))) <= 1e-12
        assert np.max(np.abs(wc - w)) > 1e-6 * np.max(np.abs(w))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PDOS_CASES))
def test_projected_dos_against_reference(name):
    m, mesh, ev, u, en = case(name)
    n = ev.shape[1]
    states = PDOS_CASES[name]
    sel = list(range(n)) if states is None else states
    ref = tr.pdos(ev, u, mesh, en, sel)
    g, big, p = m.tetrahedron_dos_mesh(mesh, en, per_band=True, states=sel)
    assert p.shape == (len(sel), n, len(en))
    close(name + " pdos", p, ref)
    gt, nt, pt = m.tetrahedron_dos_mesh(mesh, en, states=sel)
    assert pt.shape == (len(sel), len(en))
    scale = max(1.0, np.max(np.abs(gt)))
    assert np.max(np.abs(pt - p.sum(axis=1))) <= 1e-12 * scale       # per-band rows sum to the total
    assert np.max(np.abs(gt - g.sum(axis=0))) <= 1e-12 * scale
    if states is None:
        assert np.max(np.abs(pt.sum(axis=0) - gt)) <= 1e-12 * scale   # the sum over all states is the DOS
        assert np.max(np.abs(p.sum(axis=0) - g)) <= 1e-12 * scale
    if name != "big40":
        g2, big2 = device_dos(name)
        assert np.array_equal(g, g2) and np.array_equal(big, big2)   # the same bits with and without a selection
    # bits: the same call twice, a subset of the states, one energy alone
    again = m.tetrahedron_dos_mesh(mesh, en, per_band=True, states=sel)
    assert all(np.array_equal(a, b) for a, b in zip((g, big, p), again))
    sub = m.tetrahedron_dos_mesh(mesh, en, per_band=True, states=sel[1:2])[2]
    assert np.array_equal(sub[0], p[1])
    one = m.tetrahedron_dos_mesh(mesh, en[5:6], per_band=True, states=sel[1:2])[2]
    assert np.array_equal(one[0, :, 0], p[1, :, 5])


@pytest.mark.gpu
def test_exact_ties_of_a_flat_band():
    m = flat_band()
    mesh = [4, 3]
    g, big = m.tetrahedron_dos_mesh(mesh, [0.4999, 0.5, 0.6])
    assert np.max(np.abs(big - np.array([0.0, 1.0, 1.0]))) <= 1e-13 and not g.any()
    w = m.tetrahedron_weights_mesh(mesh, 0.5)
    assert w.shape == (1, 12) and np.max(np.abs(w - 1.0 / 12.0)) <= 1e-13
    assert not m.tetrahedron_weights_mesh(mesh, 0.5, derivative=True).any()
    assert not m.tetrahedron_weights_mesh(mesh, 0.4999).any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["chain41", "haldane", "cubic16", "random34"])
def test_same_bits_twice_and_alone(name):
    m, mesh, _, _, en = case(name)
    g, big = device_dos(name)
    g2, big2 = m.tetrahedron_dos_mesh(mesh, en, per_band=True)
    assert np.array_equal(g, g2) and np.array_equal(big, big2)
    for j in (0, 7, len(en) - 1):
        g1, big1 = m.tetrahedron_dos_mesh(mesh, en[j:j + 1], per_band=True)
        assert np.array_equal(g1[:, 0], g[:, j]) and np.array_equal(big1[:, 0], big[:, j])
    gt, nt = m.tetrahedron_dos_mesh(mesh, en)
    g1, n1 = m.tetrahedron_dos_mesh(mesh, en[7:8])
    assert g1[0] == gt[7] and n1[0] == nt[7]


@pytest.mark.gpu
def test_many_energies_cross_the_tiles():
    """More energies than one launch takes (1024), not a multiple of 256: every tile against the same energies alone."""
    m, mesh, ev, _, _ = case("haldane")
    en = np.linspace(ev.min() - 0.3, ev.max() + 0.3, 2300) + 1e-4 * np.sqrt(2.0)
    g, big = m.tetrahedron_dos_mesh(mesh, en, per_band=True)
    for sl in (slice(0, 3), slice(1020, 1030), slice(2290, 2300)):
        g1, n1 = m.tetrahedron_dos_mesh(mesh, en[sl], per_band=True)
        assert np.array_equal(g1, g[:, sl]) and np.array_equal(n1, big[:, sl])
    assert np.all(np.diff(big.sum(axis=0)) >= -1e-13) and big[:, -1].sum() == 2.0


@pytest.mark.gpu
def test_band_tiles_of_the_cell_form():
    """A per-band call whose group partials pass the cap of one launch (1024 k-groups x 16 bands x 1024 energies): the bands go in
    tiles of 4 per launch, the energies in two tiles.  The same bits as a call small enough for one launch."""
    m = hp.cubic16(tb.tb_model)
    mesh = [26, 26, 26]
    en = np.linspace(-6.0, 6.0, 1100) + 1e-4 * np.sqrt(3.0)
    g, big = m.tetrahedron_dos_mesh(mesh, en, per_band=True)
    assert g.shape == big.shape == (16, 1100)
    pick = [0, 517, 1023, 1024, 1099]
    g1, n1 = m.tetrahedron_dos_mesh(mesh, en[pick], per_band=True)
    assert np.array_equal(g1, g[:, pick]) and np.array_equal(n1, big[:, pick])
    gt, nt = m.tetrahedron_dos_mesh(mesh, en)
    assert np.max(np.abs(gt - g.sum(axis=0))) <= 1e-12 * np.max(gt) and np.max(np.abs(nt - big.sum(axis=0))) <= 1e-12 * 16
    assert np.array_equal(big[:, -1], np.ones(16)) and not big[:, 0].any() and np.all(np.diff(nt) >= -1e-12)


@pytest.mark.gpu
def test_band_tiles_of_the_projected_dos():
    """16 states x 40 bands x 1113 energies over two chunks: the bands go in tiles of 6 per launch.  The columns of the reference-checked
    energies and states have the bits of the small call."""
    m, mesh, _, _, en = case("big40")
    sel = PDOS_CASES["big40"]
    more = np.concatenate([en, np.linspace(en.min(), en.max(), 1100) + 1e-5 * np.sqrt(2.0)])
    states = sel + list(range(4, 28, 2))
    g, big, p = m.tetrahedron_dos_mesh(mesh, more, per_band=True, states=states)
    assert p.shape == (16, 40, len(more))
    g0, big0, p0 = m.tetrahedron_dos_mesh(mesh, en, per_band=True, states=sel)
    k = len(en)
    assert np.array_equal(p[:len(sel), :, :k], p0) and np.array_equal(g[:, :k], g0) and np.array_equal(big[:, :k], big0)
    tiny = 1e-12 * np.max(g)
    assert np.all(p >= -tiny) and np.all(p.sum(axis=0) <= g + tiny)             # 16 of the 40 states: a part of the DOS


@pytest.mark.gpu
def test_fermi_level():
    # an insulator: the middle of the gap
    m, mesh, ev, _, _ = case("haldane")
    width = float(ev.max() - ev.min())
    mu = m.tetrahedron_fermi_level_mesh(mesh, 1.0)
    assert abs(mu - 0.5 * (ev[:, 0].max() + ev[:, 1].min())) <= 1e-12 * width
    assert m.tetrahedron_fermi_level_mesh(mesh, 1.0) == mu
    # a metal: the root of N(mu) = n
    m, mesh, ev, _, _ = case("square")
    n = 0.25
    mu = m.tetrahedron_fermi_level_mesh(mesh, n)
    root = tr.fermi_level(ev, mesh, n)
    print("square n=0.25: mu %.17g, reference root %.17g, N_ref(mu) - n %.3e" % (mu, root, tr.count(ev, mesh, mu) - n))
    assert abs(mu - root) <= 1e-10 and abs(tr.count(ev, mesh, mu) - n) <= 1e-12 * n
    assert m.tetrahedron_fermi_level_mesh(mesh, n) == mu
    # touching bands: mu is only as determined as N is
    m, mesh, ev, _, _ = case("graphene")
    mu = m.tetrahedron_fermi_level_mesh(mesh, 1.0)
    print("graphene n=1: mu %.17g, N_ref(mu) - n %.3e" % (mu, tr.count(ev, mesh, mu) - 1.0))
    assert abs(tr.count(ev, mesh, mu) - 1.0) <= 1e-12
    # a filling inside a band of a 3-D model
    m, mesh, ev, _, _ = case("random3d")
    mu = m.tetrahedron_fermi_level_mesh(mesh, 1.37)
    assert abs(tr.count(ev, mesh, mu) - 1.37) <= 1e-12 * 1.37
