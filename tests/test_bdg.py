"""tb_model.nambu_model, density_matrix_pairs_mesh and bdg_mesh -- the Nambu model, selected entries of the density matrix and the
self-consistent Bogoliubov-de Gennes driver on k meshes -- against the oracle's ham_batch, closed forms, density_matrix_mesh and
the NumPy restatement in bdg_ref.py.

Bounds.  nambu_model against the blocks assembled from ham_batch: 1e-13.  Selected entries against density_matrix_mesh: 1e-12.
Fixed-count paths: 1e-10 A, with A the amplification of a 1e-9 change of one start occupation measured on two REFERENCE runs of
the same case (floored at 1, asserted <= 1e4), as test_mean_field.ref_amplification does.  Fixed points: tol + 1e-10 sum |V|.
Measured deviations: the table of section 36."""
import functools

import numpy as np
import pytest

import bdg_ref as bdr
import dm_ref as dmr
import helpers as hp
import mf_ref as mfr
from helpers import quiet
from oracle import tb_oracle as orc

import pythtb_amd as tb

KT = 0.05


# ---------------------------------------------------------------- models
def square_hubbard(t=-1.0):
    m = quiet(tb.tb_model, 2, 2, [[1.0, 0.0], [0.0, 1.0]], [[0.0, 0.0]], nspin=2)
    m.set_hop(t, 0, 0, [1, 0])
    m.set_hop(t, 0, 0, [0, 1])
    return m


def spinless_chain(t=-1.0, pos=0.0):
    m = quiet(tb.tb_model, 1, 1, [[1.0]], [[pos]])
    m.set_hop(t, 0, 0, [1])
    return m


def chain(norb, pot=0.6):
    """norb orbitals evenly spaced in a 1-D cell, off the origin, nearest-neighbour hops of alternating strength and an
    incommensurate on-site potential."""
    m = quiet(tb.tb_model, 1, 1, [[1.0]], [[(o + 0.25) / norb] for o in range(norb)])
    m.set_onsite([pot * np.cos(2.4 * o + 0.3) for o in range(norb)])
    for o in range(norb):
        t = -1.0 - 0.2 * (o % 2)
        if o + 1 < norb:
            m.set_hop(t, o, o + 1, [0])
        else:
            m.set_hop(t, o, 0, [1])
    return m


def chain_V(norb, V):
    return [(V, o, o + 1, [0]) if o + 1 < norb else (V, o, 0, [1]) for o in range(norb)]


def haldane_spinful():
    m = quiet(tb.tb_model, 2, 2, hp.LAT, hp.ORB, nspin=2)
    t2 = 0.15j
    m.set_onsite([-0.2, 0.2])
    for amp, i, j, R in ((-1.0, 0, 1, [0, 0]), (-1.0, 1, 0, [1, 0]), (-1.0, 1, 0, [0, 1]), (t2, 0, 0, [1, 0]), (t2, 1, 1, [1, -1]),
                         (t2, 1, 1, [0, 1]), (np.conj(t2), 1, 1, [1, 0]), (np.conj(t2), 0, 0, [1, -1]), (np.conj(t2), 0, 0, [0, 1])):
        m.set_hop(amp, i, j, R)
    return m


NN_HONEY = [(0, 1, [0, 0]), (1, 0, [1, 0]), (1, 0, [0, 1])]


def state_ham(m, k):
    """h(k), (nk, nsta, nsta)."""
    k = np.asarray(k, dtype=float).reshape(-1, m._dim_k)
    return np.asarray(orc.ham_batch(m, k)).reshape(len(k), m._nsta, m._nsta)


def pairing_matrix(m, pairing, k):
    """Delta(k): the entry (Delta, a, b, R) at [a, b] with e^{2 pi i k.(R + tau_b - tau_a)}, and its antisymmetric mirror."""
    n = m._nsta
    tau = dmr.state_positions(m)
    out = np.zeros((len(k), n, n), dtype=complex)
    for D, a, b, R in pairing:
        Rp = np.array(R, dtype=float)[m._per]
        out[:, a, b] += D * np.exp(2j * np.pi * (k @ (Rp + tau[b] - tau[a])))
        out[:, b, a] += -D * np.exp(2j * np.pi * (k @ (-Rp + tau[a] - tau[b])))
    return out


# ---------------------------------------------------------------- CPU: the Nambu model
@pytest.mark.parametrize("name", ["haldane", "kane_mele", "chain_off_origin"])
def test_nambu_matrix_without_gpu(name):
    """H_BdG(k) = [[h(k) - mu, Delta(k)], [Delta(k)+, -h(-k)^T + mu]] at random k; no inversion symmetry in the first two."""
    if name == "haldane":
        m = hp.haldane(tb.tb_model, delta=0.3)
        pairing = [(0.3 + 0.1j, 0, 1, [0, 0]), (-0.2j, 1, 0, [1, 0]), (0.25, 0, 0, [1, 0]), (0.15 - 0.05j, 1, 1, [-1, 1])]
    elif name == "kane_mele":
        m = hp.kane_mele(tb.tb_model)
        pairing = [(0.4, 0, 1, [0, 0]), (0.4j, 2, 3, [0, 0]), (0.1 + 0.2j, 0, 3, [0, -1]), (0.05, 1, 1, [1, 0]), (-0.3, 3, 0, [2, -1])]
    else:
        m = quiet(tb.tb_model, 1, 1, [[1.0]], [[0.2], [0.7]])
        m.set_onsite([0.1, -0.4])
        m.set_hop(-1.0 + 0.3j, 0, 1, [0])
        m.set_hop(0.5j, 1, 0, [1])
        m.set_hop(0.2, 0, 0, [2])
        pairing = [(0.3j, 0, 1, [0]), (0.2, 0, 0, [1]), (-0.1 + 0.4j, 1, 0, [3])]
    mu, n = 0.37, m._nsta
    nb = m.nambu_model(mu, pairing)
    assert nb._nspin == 1 and nb._norb == 2 * n and m._nsta == n
    k = np.random.default_rng(5).random((9, m._dim_k)) - 0.5
    H = state_ham(nb, k)
    hk, hmk, dk = state_ham(m, k), state_ham(m, -k), pairing_matrix(m, pairing, k)
    eye = np.eye(n)[None]
    want = np.zeros_like(H)
    want[:, :n, :n] = hk - mu * eye
    want[:, :n, n:] = dk
    want[:, n:, :n] = np.conj(np.transpose(dk, (0, 2, 1)))
    want[:, n:, n:] = -np.transpose(hmk, (0, 2, 1)) + mu * eye
    err = np.max(np.abs(H - want))
    print("%s: max |H_BdG - blocks| = %.3e" % (name, err))
    assert err <= 1e-13
    assert np.max(np.abs(dk + np.transpose(pairing_matrix(m, pairing, -k), (0, 2, 1)))) <= 1e-14      # Delta(k) = -Delta(-k)^T
    ev, evm = np.linalg.eigvalsh(H), np.linalg.eigvalsh(state_ham(nb, -k))
    assert np.max(np.abs(ev + evm[:, ::-1])) <= 1e-12                                                 # E_n(k) = -E_{2n-1-n}(-k)
    assert np.array_equal(nb._orb[:n], np.repeat(m._orb, m._nspin, axis=0)) and np.array_equal(nb._orb[n:], nb._orb[:n])


def test_kitaev_chain_without_gpu():
    """E(k) = +-sqrt((2 t cos 2 pi k + mu)^2 + 4 |Delta|^2 sin^2 2 pi k) for hop amplitude -t and p-wave Delta on the bond."""
    t, mu, D = 1.0, 0.7, 0.45 * np.exp(0.3j)
    m = spinless_chain(-t, pos=0.3)
    nb = m.nambu_model(mu, [(D, 0, 0, [1])])
    k = np.linspace(-0.5, 0.5, 41)
    ev = np.linalg.eigvalsh(state_ham(nb, k))
    want = np.sqrt((2.0 * t * np.cos(2 * np.pi * k) + mu) ** 2 + 4.0 * abs(D) ** 2 * np.sin(2 * np.pi * k) ** 2)
    assert np.max(np.abs(ev[:, 1] - want)) <= 1e-13 and np.max(np.abs(ev[:, 0] + want)) <= 1e-13


def test_argument_errors_without_gpu():
    m, s = spinless_chain(), square_hubbard()
    for bad in (np.inf, "x", None):
        with pytest.raises(Exception, match="fermi_level"):
            m.nambu_model(bad)
    for pairing, pat in (([(0.1, 0, 0, [0])], "antisymmetry"), ([(0.1, 0, 1, [0])], "out of scope"), ([(0.1, 0, 0, [1, 0])], "dim_r integers"),
                         ([(0.1, 0, 0, [1]), (0.2, 0, 0, [-1])], "given twice"), ([(np.nan, 0, 0, [1])], "finite"),
                         ([(0.1, 0, 0)], "list of"), ([(0.1, 0, 0, [2 ** 30])], "2\\*\\*30")):
        with pytest.raises(Exception, match=pat):
            m.nambu_model(0.0, pairing)
    with pytest.raises(Exception, match="given twice"):
        s.nambu_model(0.0, [(0.1, 0, 1, [0, 0]), (0.3, 1, 0, [0, 0])])
    big = quiet(tb.tb_model, 1, 1, [[1.0]], np.zeros((1025, 1)))
    with pytest.raises(Exception, match="1024"):
        big.nambu_model(0.0)
    with pytest.raises(Exception, match="1024"):
        big.bdg_mesh([4], [(1.0, 0, 1, [0])], n_electrons=1.0)
    # density_matrix_pairs_mesh
    for pairs, pat in ((None, "triples"), ([], "2\\*\\*20"), ([(0, 1, [0])], "out of scope"), ([(0, 0, [0, 0])], "dim_k integers"),
                       ([(0, 0, [0.5])], "dim_k integers"), ([(0, 0, [2 ** 30])], "2\\*\\*30"), ([(0, 0)], "triples")):
        with pytest.raises(Exception, match=pat):
            m.density_matrix_pairs_mesh([8], 0.0, pairs=pairs)
    with pytest.raises(Exception, match="kT"):
        m.density_matrix_pairs_mesh([8], 0.0, kT=-1.0, pairs=[(0, 0, [0])])
    with pytest.raises(Exception, match="fermi_level"):
        m.density_matrix_pairs_mesh([8], np.nan, pairs=[(0, 0, [0])])
    # bdg_mesh
    V = [(-3.0, 0, 0, [1])]
    flat = quiet(tb.tb_model, 0, 1, [[1.0]], [[0.0]])
    with pytest.raises(Exception, match="dim_k"):
        flat.bdg_mesh([4], V, n_electrons=0.4)
    with pytest.raises(Exception, match="exactly one"):
        m.bdg_mesh([8], V)
    with pytest.raises(Exception, match="exactly one"):
        m.bdg_mesh([8], V, n_electrons=0.4, fermi_level=0.0)
    for nel in (0.0, 1.0, -0.2, np.nan):
        with pytest.raises(Exception):
            m.bdg_mesh([8], V, n_electrons=nel)
    with pytest.raises(Exception, match="interaction list, U, or both"):
        m.bdg_mesh([8], n_electrons=0.4)
    with pytest.raises(Exception, match="self-interaction"):
        m.bdg_mesh([8], [(1.0, 0, 0, [0])], n_electrons=0.4)
    with pytest.raises(Exception, match="given twice"):
        m.bdg_mesh([8], [(1.0, 0, 0, [1]), (1.0, 0, 0, [-1])], n_electrons=0.4)
    with pytest.raises(Exception, match="nspin"):
        m.bdg_mesh([8], U=-1.0, n_electrons=0.4)
    with pytest.raises(Exception, match="switched off"):
        m.bdg_mesh([8], V, n_electrons=0.4, hartree=False, pairing=False)
    for kw, pat in ((dict(history=9), "history"), (dict(history=-1), "history"), (dict(max_iter=0), "max_iter"),
                    (dict(max_iter=65537), "max_iter"), (dict(check_every=0), "check_every"), (dict(mixing=0.0), "mixing"),
                    (dict(mixing=1.5), "mixing"), (dict(tol=-1.0), "tol"), (dict(tol=np.nan), "tol"), (dict(mu_step=0.0), "mu_step"),
                    (dict(mu_step=np.inf), "mu_step"), (dict(pairing_seed=np.nan), "pairing_seed"), (dict(kT=-1.0), "kT"),
                    (dict(start=np.zeros(3)), "start"), (dict(start=[np.nan]), "start"), (dict(mu_start=np.nan), "start")):
        with pytest.raises(Exception, match=pat):
            m.bdg_mesh([8], V, n_electrons=0.4, **kw)
    with pytest.raises(Exception, match="4096 distinct"):
        m.bdg_mesh([8], [(1.0, 0, 0, [r]) for r in range(1, 4098)], n_electrons=0.4)
    with pytest.raises(Exception, match="2\\*\\*22"):
        chain(800).bdg_mesh([4], chain_V(800, -1.0), n_electrons=400.0, return_density=True)   # 2 x 1600^2 > 2^22


# ---------------------------------------------------------------- the four fixed points of the reference
FIXED = {
    "hubbard_kT0": (square_hubbard, [8, 8], dict(U=-4.0, n_electrons=0.8, kT=0.0), 14),
    "hubbard_kT": (square_hubbard, [8, 8], dict(U=-4.0, n_electrons=0.8, kT=KT), 14),
    "chain": (spinless_chain, [16], dict(interaction=[(-3.0, 0, 0, [1])], n_electrons=0.4, kT=KT), 25),
    "chain_fock": (spinless_chain, [16], dict(interaction=[(-3.0, 0, 0, [1])], n_electrons=0.4, kT=KT, fock=True), 29),
}
FIXED_KW = dict(mixing=0.5, history=4, mu_step=1.0, pairing_seed=0.1, tol=1e-11, max_iter=100)


@functools.lru_cache(maxsize=None)
def fixed_ref(name):
    build, mesh, kw, _ = FIXED[name]
    return bdr.run(build(), mesh, **kw, **FIXED_KW)


def gap_equation(U, x, mu, nel, kT, mesh):
    """1 - (|U| / N_k) sum tanh(E / 2 kT) / 2 E with E^2 = (eps_k + U n / 2 - mu)^2 + (U |F|)^2 on the square lattice, t = 1."""
    k = np.stack(np.meshgrid(*[np.arange(N) / N for N in mesh], indexing="ij"), -1).reshape(-1, 2)
    xi = -2.0 * (np.cos(2 * np.pi * k[:, 0]) + np.cos(2 * np.pi * k[:, 1])) + U * nel / 2.0 - mu
    E = np.sqrt(xi ** 2 + (U * abs(x)) ** 2)
    th = np.tanh(E / (2.0 * kT)) if kT > 0.0 else np.ones_like(E)
    return 1.0 - abs(U) * np.mean(th / (2.0 * E))


@pytest.mark.parametrize("name", list(FIXED))
def test_reference_fixed_points_without_gpu(name):
    r = fixed_ref(name)
    lay = r["lay"]
    F, mu = abs(lay.F(r["x_out"], 0)), r["x_out"][lay.par_mu]
    print("%s: %d iterations, |F| = %.6f, mu = %.6f, gap = %.4f" % (name, r["iterations"], F, mu, r["gap"]))
    assert r["converged"] and r["iterations"] == FIXED[name][3]
    want = {"hubbard_kT0": (0.332437, -2.235258), "hubbard_kT": (0.332437, -2.235258), "chain": (0.215166, -3.116152),
            "chain_fock": (0.278769, -2.817957)}[name]
    assert abs(F - want[0]) < 1e-6 and abs(mu - want[1]) < 1e-6
    if name == "chain":
        assert abs(r["gap"] - 1.149) < 1e-3
    if name == "chain_fock":
        assert abs(abs(lay.D(r["x_out"], 0)) - 0.188697) < 1e-6
    if name.startswith("hubbard"):
        kT = FIXED[name][2]["kT"]
        assert abs(gap_equation(-4.0, lay.F(r["x_out"], 0), mu, 0.8, kT, [8, 8])) < 1e-9
        assert abs(r["n_electrons"] - 0.8) < 1e-10


# ---------------------------------------------------------------- GPU: selected entries of the density matrix
def pair_cases():
    hal = hp.haldane(tb.tb_model, delta=0.2)
    return {
        "n2": (hal, [5, 7], 0.1),
        "n4": (hp.kane_mele(tb.tb_model), [6, 6], 0.3),
        "n18": (quiet(hal.make_supercell, [[3, 0], [0, 3]]), [7, 1], 0.15),
        "n34": (chain(34), [7], 0.05),
        "n40": (quiet(hal.make_supercell, [[5, 0], [0, 4]]), [37, 37], 0.2),
    }


def triples_of(n, dk, rs):
    """i = j, i > j, i < j, R = 0 and R != 0, a repeated triple; 70 of them or more: a second tile of 64."""
    rng = np.random.default_rng(n)
    out = [(0, 0, 0), (n - 1, 0, 0), (0, n - 1, len(rs) - 1), (n - 1, 0, 0)]
    while len(out) < 70:
        out.append((int(rng.integers(n)), int(rng.integers(n)), int(rng.integers(len(rs)))))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n2", "n4", "n18", "n34", "n40"])
def test_pairs_against_density_matrix(name):
    m, mesh, mu0 = pair_cases()[name]
    n, dk = m._nsta, m._dim_k
    rs = np.array([[0] * dk, [1] + [0] * (dk - 1), [-1] + [2] * (dk - 1), [mesh[0] + 1] + [-2] * (dk - 1)])
    tri = triples_of(n, dk, rs)
    pairs = [(i, j, rs[r]) for i, j, r in tri]
    for kT, mu in ((0.0, dmr_safe_mu(m, mesh, mu0)), (KT, mu0 + 0.11)):
        whole = m.density_matrix_mesh(mesh, mu, kT, rs).reshape(len(rs), n, n)
        got = m.density_matrix_pairs_mesh(mesh, mu, kT, pairs)
        assert got.dtype == complex and got.shape == (len(pairs),)
        want = np.array([whole[r, i, j] for i, j, r in tri])
        err = np.max(np.abs(got - want))
        print("%s kT=%g: max |pairs - matrix entries| = %.3e" % (name, kT, err))
        assert err <= 1e-12
        assert got[1] == got[3]                                                        # a repeated triple
        np.testing.assert_array_equal(got, m.density_matrix_pairs_mesh(mesh, mu, kT, pairs))   # two calls
        for p in (2, 69):                                                              # alone, and elsewhere in another list
            assert m.density_matrix_pairs_mesh(mesh, mu, kT, [pairs[p]])[0] == got[p]
        assert m.density_matrix_pairs_mesh(mesh, mu, kT, pairs[60:] + pairs[:3])[9] == got[69]
        assert m.density_matrix_pairs_mesh(mesh, mu, kT, [(0, 0, None)])[0] == got[0]


def dmr_safe_mu(m, mesh, target):
    """The midpoint of the two reference levels around `target` (a gap of 2e-6 or more, asserted)."""
    s = np.unique(dmr.levels(m, mesh).ravel())
    j = int(np.searchsorted(s, target))
    assert 0 < j < len(s) and s[j] - s[j - 1] >= 2e-6
    return 0.5 * (s[j - 1] + s[j])


# ---------------------------------------------------------------- GPU: iteration paths
def path_cases():
    """name -> (model, mesh, keyword arguments without the filling, n_electrons, fermi_level)."""
    hs = haldane_spinful()
    sc20 = quiet(hp.haldane(tb.tb_model, delta=0.2).make_supercell, [[5, 0], [0, 2]])
    return {
        "hubbard_kT": (square_hubbard(), [8, 8], dict(U=-4.0, kT=KT), 0.8, -2.2),
        "hubbard_kT0": (square_hubbard(), [8, 8], dict(U=-4.0, kT=0.0), 0.8, -2.2),
        "chain": (spinless_chain(), [16], dict(interaction=[(-3.0, 0, 0, [1])], kT=KT), 0.4, -3.1),
        "chain_fock": (spinless_chain(), [16], dict(interaction=[(-3.0, 0, 0, [1])], kT=KT, fock=True), 0.4, -2.8),
        "haldane_all": (hs, [5, 7], dict(interaction=[(-1.5, i, j, R) for i, j, R in NN_HONEY], U=-2.0, kT=KT, fock=True), 1.6, -1.5),
        "n9": (chain(9), [7], dict(interaction=chain_V(9, -2.0), kT=KT, fock=True), 3.7, -2.5),
        "n17": (chain(17), [5], dict(interaction=chain_V(17, -2.0), kT=KT), 7.2, -2.5),
        "n20": (sc20, [37, 37], dict(interaction=[(-2.0, 0, 1, [0, 0]), (-1.5, 3, 2, [0, 0]), (-1.0, 4, 4, [1, 0])], kT=KT, fock=True),
                8.3, -1.0),
    }


def ref_amplification(m, mesh, kw, iters):
    """A of the module docstring, and the unperturbed reference run."""
    n = m._nsta
    start = 0.5 + 0.1 * np.cos(np.arange(float(n)))
    base = bdr.run(m, mesh, tol=0.0, max_iter=iters, start=start, **kw)
    st = start.copy()
    st[base["lay"].touched[0]] += 1e-9
    pert = bdr.run(m, mesh, tol=0.0, max_iter=iters, start=st, **kw)
    A = max(1.0, np.max(np.abs(pert["x_out"] - base["x_out"])) / 1e-9, np.max(np.abs(pert["history"][-1] - base["history"][-1])) / 1e-9)
    return A, base, start


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["n_electrons", "fermi_level"])
@pytest.mark.parametrize("name", ["hubbard_kT", "hubbard_kT0", "chain", "chain_fock", "haldane_all", "n9", "n17", "n20"])
def test_iteration_path(name, form):
    m, mesh, kw, nel, mu = path_cases()[name]
    kw = dict(kw, history=0, mixing=0.5, **({"n_electrons": nel} if form == "n_electrons" else {"fermi_level": mu}))
    A, ref, start = ref_amplification(m, mesh, kw, 6)
    assert A <= 1e4
    res = m.bdg_mesh(mesh, tol=0.0, max_iter=6, start=start.reshape(m._norb, 2) if m._nspin == 2 else start, **kw)
    n = m._nsta
    dev = max(np.max(np.abs(res.history.reshape(6, n) - ref["history"])), np.max(np.abs(res.field - ref["x_out"])),
              np.max(np.abs(res._x - ref["x_in"])))
    print("%s %s: A = %.3g, max deviation of the path = %.3e, residual %.3e" % (name, form, A, dev, res.residuals[-1]))
    assert res.iterations == 6 and not res.converged
    assert dev <= 1e-10 * A
    assert np.max(np.abs(res.residuals - ref["residuals"])) <= 1e-10 * A
    for key in ("energy", "entropy", "free_energy", "grand_potential", "gap", "n_electrons"):
        assert abs(getattr(res, key) - ref[key]) <= 1e-9 * A, key
    assert abs(res.fermi_level - ref["mu"]) <= 1e-10 * A


# ---------------------------------------------------------------- GPU: fixed points
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FIXED))
def test_fixed_points(name):
    build, mesh, kw, iters = FIXED[name]
    ref = fixed_ref(name)
    res = build().bdg_mesh(mesh, **kw, **FIXED_KW)
    lay = ref["lay"]
    sumV = sum(abs(V) for V, _, _, _ in lay.ent)
    dev = np.max(np.abs(res.field - ref["x_out"]))
    print("%s: %d iterations (reference %d), max |x - x_ref| = %.3e" % (name, res.iterations, ref["iterations"], dev))
    assert res.converged and res.iterations == ref["iterations"] == iters
    assert dev <= FIXED_KW["tol"] + 1e-10 * sumV
    assert abs(res.anomalous[0] - lay.F(ref["x_out"], 0)) <= FIXED_KW["tol"] + 1e-10 * sumV
    if name.startswith("hubbard"):
        assert abs(gap_equation(-4.0, res.anomalous[0], res.field[-1], 0.8, kw["kT"], mesh)) < 1e-9
        assert abs(res.gap - np.min(np.abs(dmr.levels(ref["model"], mesh)))) < 1e-9
    for key in ("energy", "free_energy", "grand_potential"):
        assert abs(getattr(res, key) - ref[key]) <= 1e-9, key


# ---------------------------------------------------------------- GPU: the normal limit
@pytest.mark.gpu
def test_normal_limit():
    """pairing=False, fock=True at a given Fermi level: the occupation path of mean_field_mesh."""
    hs = haldane_spinful()
    inter = [(1.2, i, j, R) for i, j, R in NN_HONEY]
    start = np.array([[0.7, 0.3], [0.4, 0.6]])
    kw = dict(interaction=inter, U=2.0, fermi_level=1.1, kT=KT, fock=True, mixing=0.5, history=0, tol=0.0, max_iter=6, start=start)
    a = mfr.run(hs, [5, 7], **kw)
    st2 = start.copy()
    st2[0, 0] += 1e-9
    b = mfr.run(hs, [5, 7], **dict(kw, start=st2))
    A = max(1.0, np.max(np.abs(a["history"][-1] - b["history"][-1])) / 1e-9)
    mf = hs.mean_field_mesh([5, 7], **kw)
    bd = hs.bdg_mesh([5, 7], pairing=False, **kw)
    dev = np.max(np.abs(bd.history - mf.history))
    print("normal limit: A = %.3g, max |bdg - mean field| = %.3e" % (A, dev))
    assert dev <= 1e-10 * A and bd.pairing == [] and bd.anomalous.size == 0
    assert np.max(np.abs(bd.field - mf.field)) <= 1e-10 * A


# ---------------------------------------------------------------- GPU: the returned model
@pytest.mark.gpu
def test_result_model_consistency():
    hs = haldane_spinful()
    inter = [(-1.5, i, j, R) for i, j, R in NN_HONEY]
    mesh, n = [5, 7], 4
    res = hs.bdg_mesh(mesh, inter, U=-2.0, n_electrons=1.6, kT=KT, fock=True, tol=0.0, max_iter=8, return_density=True)
    D = res.nambu_density
    assert D.shape == (len(res.R_list), 2 * n, 2 * n)
    again = res.model.density_matrix_mesh(mesh, 0.0, KT, res.R_list)
    assert np.max(np.abs(again - D)) <= 1e-10
    ref = dmr.density_matrix(res.model, mesh, 0.0, KT, res.R_list)
    print("nambu_density against the reference: %.3e" % np.max(np.abs(D - ref)))
    assert np.max(np.abs(D - ref)) <= 1e-10
    # the hole block is delta - conj(D)
    for r, R in enumerate(res.R_list):
        want = (np.eye(n) if not np.any(R) else 0.0) - np.conj(D[r][:n, :n])
        assert np.max(np.abs(D[r][n:, n:] - want)) <= 1e-10
    # x_out is made of the matching entries
    ent = mfr.entries(hs, inter, -2.0)
    lay = bdr.Layout(hs, ent, True, True, True, True)
    Rl = [tuple(int(x) for x in R) for R in res.R_list]
    x = res.field
    for a in lay.touched:
        assert abs(x[lay.par[a]] - D[0][a, a].real) <= 1e-12
    for e, (V, a, b, R) in enumerate(ent):
        r = Rl.index(R)
        assert abs(lay.D(x, e) - D[r][a, b]) <= 1e-12 and abs(lay.F(x, e) - D[r][a, n + b]) <= 1e-12
        assert abs(res.anomalous[e] - D[r][a, n + b]) <= 1e-12
    assert abs(res.n_electrons - np.trace(D[0][:n, :n]).real) <= 1e-12
    # Wick: <H - mu N> + mu N = <H_0> + sum_e V [n_a n_b - |D|^2 + |F|^2] in the state of the last iteration
    table = dmr.hopping_table(hs)
    normal = dmr.density_matrix(res.model, mesh, 0.0, KT, np.array([R for R, _ in table]))[:, :n, :n]
    e0 = dmr.energy_from_density_matrix(table, normal)
    wick = e0 + sum(V * (x[lay.par[a]] * x[lay.par[b]] - abs(lay.D(x, e)) ** 2 + abs(lay.F(x, e)) ** 2) for e, (V, a, b, _) in enumerate(ent))
    print("Wick identity: %.3e" % abs(res.energy - wick))
    assert abs(res.energy - wick) <= 1e-9
    # the free energy of the paired Hubbard solution and of the normal one, against the reference
    for pairing in (True, False):
        kw = dict(U=-4.0, n_electrons=0.8, kT=KT, pairing=pairing, tol=1e-11, max_iter=100)
        r = bdr.run(square_hubbard(), [8, 8], **kw)
        g = square_hubbard().bdg_mesh([8, 8], **kw)
        print("pairing=%s: F = %.10f (reference %.10f), %d iterations" % (pairing, g.free_energy, r["free_energy"], g.iterations))
        assert g.converged and r["converged"] and abs(g.free_energy - r["free_energy"]) <= 1e-9


# ---------------------------------------------------------------- GPU: restarts and bits
@pytest.mark.gpu
def test_restart_and_bits():
    m = spinless_chain()
    kw = dict(interaction=[(-3.0, 0, 0, [1])], n_electrons=0.4, kT=KT, fock=True)
    a = m.bdg_mesh([16], tol=0.0, max_iter=6, **kw)
    b = m.bdg_mesh([16], tol=0.0, max_iter=6, **kw)
    for key in ("field", "_x", "residuals", "history"):
        np.testing.assert_array_equal(getattr(a, key), getattr(b, key))
    assert a.energy == b.energy and a.gap == b.gap
    c = m.bdg_mesh([16], tol=0.0, max_iter=3, **kw)
    np.testing.assert_array_equal(c.history, a.history[:3])
    np.testing.assert_array_equal(c.residuals, a.residuals[:3])
    d = m.bdg_mesh([16], tol=0.0, max_iter=6, check_every=3, **kw)
    np.testing.assert_array_equal(d.field, a.field)
    np.testing.assert_array_equal(d.history, a.history)
    # a restart repeats the last iteration: the same residual
    r = m.bdg_mesh([16], tol=0.0, max_iter=1, start=a, **kw)
    assert r.iterations == 1 and r.residuals[0] == a.residuals[-1]
    np.testing.assert_array_equal(r.field, a.field)
    with pytest.raises(Exception, match="another model size"):
        m.bdg_mesh([16], tol=0.0, max_iter=1, start=a, **dict(kw, fock=False))
    # the Nambu model feeds the other calls: a fully gapped quasi-particle spectrum on a finer mesh
    full = m.bdg_mesh([16], tol=1e-11, max_iter=100, **kw)
    ev = full.model.solve_all(np.linspace(0.0, 1.0, 33))
    assert full.converged and np.min(np.abs(ev)) > 0.5 * full.gap
