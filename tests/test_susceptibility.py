"""The bare (Lindhard) susceptibility chi0(q, w) on k meshes (tb_model.susceptibility_mesh) against the NumPy restatement in
chi_ref.py, the closed forms of the one-band square lattice, and the properties of the formula."""
import numpy as np
import pytest

import chi_ref as chr_
import helpers as hp
from helpers import quiet
from oracle import tb_oracle as orc

import pythtb_amd as tb

OMEGA = np.array([-1.3, -0.2, 0.0, 0.35, 1.1, 2.7])
ETA = 0.05
KT = 0.07


def haldane(delta=0.2):
    return hp.haldane(tb.tb_model, delta=delta)


def square(t=-1.0):
    """One orbital on the square lattice, on a lattice point: E = 2 t (cos 2 pi k_x + cos 2 pi k_y)."""
    m = quiet(tb.tb_model, 2, 2, [[1.0, 0.0], [0.0, 1.0]], [[0.0, 0.0]])
    m.set_hop(t, 0, 0, [1, 0])
    m.set_hop(t, 0, 0, [0, 1])
    return m


def square_dispersion(mesh, t=-1.0):
    kx, ky = np.meshgrid(np.arange(mesh[0]) / mesh[0], np.arange(mesh[1]) / mesh[1], indexing="ij")
    return 2.0 * t * (np.cos(2.0 * np.pi * kx) + np.cos(2.0 * np.pi * ky))


def levels(m, kpts):
    return np.linalg.eigvalsh(orc.ham_batch(m, np.asarray(kpts, dtype=float).reshape(-1, m._dim_k)))


def safe_mu(m, mesh, qs, target):
    """The midpoint of the two levels around `target` among every level at k and at k + q: asserted to be at least 1e-6 from
    all of them, so that no kT = 0 occupation depends on the last bits of an eigenvalue."""
    kk = np.asarray(m.k_uniform_mesh(mesh), dtype=float).reshape(-1, m._dim_k)
    s = np.unique(np.concatenate([levels(m, kk).ravel()] + [levels(m, kk + np.asarray(q)[None, :]).ravel() for q in qs]))
    j = int(np.searchsorted(s, target))
    if j == 0:
        return s[0] - 1.0
    if j == len(s):
        return s[-1] + 1.0
    mu = 0.5 * (s[j - 1] + s[j])
    assert s[j] - s[j - 1] >= 2e-6
    assert np.min(np.abs(s - mu)) >= 1e-6
    return mu


def q_mix(mesh):
    """q = 0, a q commensurate with the mesh, an incommensurate one and one with a component beyond 1."""
    d = len(mesh)
    comm = [(1 + i) / mesh[i] * (-1.0) ** i for i in range(d)]
    return np.array([[0.0] * d, comm, [0.137, 0.291, -0.413][:d], [1.3, -0.45, 0.21][:d]])


def close(got, want, rel=1e-10):
    scale = np.max(np.abs(want))
    if scale == 0.0:                                         # (kT = 0, mu outside the spectrum)
        assert np.all(got == 0.0)
        return
    err = np.max(np.abs(got - want))
    print("max abs error / max |reference| = %.3e" % (err / scale))
    assert err <= rel * scale, err / scale


# ---------------------------------------------------------------- CPU: argument errors
def test_argument_errors_without_gpu():
    m = haldane()
    flat = quiet(tb.tb_model, 0, 2, hp.LAT, hp.ORB)
    with pytest.raises(Exception, match="dim_k"):
        flat.susceptibility_mesh([4], [[0.1]], [0.1], 0.1)
    q = [[0.25, 0.1]]
    for bad in ([8], [8, 0], [8, 8, 8]):
        with pytest.raises(Exception):
            m.susceptibility_mesh(bad, q, [0.1], 0.1)
    for bad in ([0.1], [[0.1]], [[0.1, 0.2, 0.3]], [[[0.1, 0.2]]], np.zeros((0, 2)), [], [[0.1, np.nan]], [np.inf, 0.0],
                np.zeros((65537, 2))):
        with pytest.raises(Exception, match="q_list"):
            m.susceptibility_mesh([8, 8], bad, [0.1], 0.1)
        with pytest.raises(Exception, match="q_list"):
            m.susceptibility_mesh([8, 8], bad)
    for w in ([], [[0.1, 0.2]], [0.1, np.nan], [np.inf], np.zeros(65537)):
        with pytest.raises(Exception, match="omega"):
            m.susceptibility_mesh([8, 8], q, w, 0.1)
    for eta in (0.0, -0.1, np.inf, np.nan):
        with pytest.raises(Exception, match="eta"):
            m.susceptibility_mesh([8, 8], q, [0.1], eta)
    with pytest.raises(Exception, match="eta"):              # static mode: eta has no meaning
        m.susceptibility_mesh([8, 8], q, eta=0.1)
    with pytest.raises(Exception, match="eta"):              # dynamic mode: eta is needed
        m.susceptibility_mesh([8, 8], q, [0.1])
    for kT in (-1e-3, np.inf):
        with pytest.raises(Exception, match="kT"):
            m.susceptibility_mesh([8, 8], q, [0.1], 0.1, kT=kT)
        with pytest.raises(Exception, match="kT"):
            m.susceptibility_mesh([8, 8], q, kT=kT)
    with pytest.raises(Exception, match="fermi_level"):
        m.susceptibility_mesh([8, 8], q, [0.1], 0.1, fermi_level=np.nan)
    with pytest.raises(Exception, match="fermi_level"):
        m.susceptibility_mesh([8, 8], q, fermi_level=np.inf)
    with pytest.raises(Exception, match="nq"):               # 65 x 65536 > 2**22
        m.susceptibility_mesh([8, 8], np.zeros((65, 2)), np.zeros(65536), 0.1)


# ---------------------------------------------------------------- CPU: the reference's own properties and closed forms
SQ_MESH = [16, 16]
SQ_STATIC_Q = 0.507732137760894          # mean_k tanh(E / 2kT) / (2 E), 1 / (4 kT) where E = 0
SQ_STATIC_0 = 0.236611421459283          # mean_k 1 / (4 kT cosh^2(E / 2kT))
SQ_DYNAMIC_Q = 0.361247208095623         # mean_k tanh(E / 2kT) 2 E / (4 E^2 + eta^2), eta = 1e-3


def square_closed_forms(kT=0.2, eta=1e-3):
    e = square_dispersion(SQ_MESH)
    zero = np.abs(e) < 1e-12                                 # (the dispersion's own rounding at the nested points)
    es = np.where(zero, 1.0, e)
    stat_q = np.mean(np.where(zero, 1.0 / (4.0 * kT), np.tanh(es / (2.0 * kT)) / (2.0 * es)))
    stat_0 = np.mean(1.0 / (4.0 * kT * np.cosh(e / (2.0 * kT)) ** 2))
    dyn_q = np.mean(np.where(zero, 0.0, np.tanh(es / (2.0 * kT)) * 2.0 * es / (4.0 * es * es + eta * eta)))
    return stat_q, stat_0, dyn_q


def test_numpy_square_lattice_closed_forms():
    stat_q, stat_0, dyn_q = square_closed_forms()
    assert abs(stat_q - SQ_STATIC_Q) <= 1e-14 and abs(stat_0 - SQ_STATIC_0) <= 1e-14 and abs(dyn_q - SQ_DYNAMIC_Q) <= 1e-14
    m = square()
    grid = np.array([[i / 16.0, j / 16.0] for i in range(16) for j in range(16)])
    chi = chr_.susceptibility(m, SQ_MESH, grid, mu=0.0, kT=0.2)
    assert abs(chi[8 * 16 + 8] - SQ_STATIC_Q) <= 1e-12
    assert abs(chi[0] - SQ_STATIC_0) <= 1e-12
    order = np.argsort(chi)
    assert order[-1] == 8 * 16 + 8 and abs(chi[order[-2]] - 0.4448) <= 1e-4     # the nesting vector is the maximum
    dyn = chr_.susceptibility(m, SQ_MESH, [[0.5, 0.5]], [0.0], 1e-3, mu=0.0, kT=0.2)[0, 0]
    assert abs(dyn.real - SQ_DYNAMIC_Q) <= 1e-12             # (the E = 0 points are gone: what the static mode is for)
    assert chr_.susceptibility(m, SQ_MESH, [[0.5, 0.5]], mu=0.0, kT=0.2, matrix_elements=False)[0] == chi[8 * 16 + 8]


def test_numpy_static_is_the_dynamic_limit():
    m = haldane()
    for q, mu, kT, eta, want in [([0.25, -0.3], 0.0, 0.0, 1e-7, 0.3068332106), ([0.137, 0.291], 0.3, 0.15, 1e-9, 0.1680335096)]:
        st = chr_.susceptibility(m, [12, 10], [q], mu=mu, kT=kT)[0]
        dy = chr_.susceptibility(m, [12, 10], [q], [0.0], eta, mu=mu, kT=kT)[0, 0]
        assert abs(st - want) <= 1e-9 and abs(dy.real - want) <= 1e-9 and abs(st - dy.real) <= 1e-9


def test_numpy_reference_properties():
    """Sign, charge conservation, and the two symmetries that hold only under a condition."""
    m = haldane()
    mesh = [12, 10]
    w = np.array([-1.1, -0.3, 0.0, 0.3, 1.1])
    comm, incomm = [3.0 / 12.0, -2.0 / 10.0], [0.137, 0.291]
    for kT, mu in ((0.0, 0.013), (0.15, 0.3)):
        chi = chr_.susceptibility(m, mesh, [[0.0, 0.0], comm, [-comm[0], -comm[1]], incomm, [-incomm[0], -incomm[1]]], w, ETA, mu=mu, kT=kT)
        scale = np.max(np.abs(chi))
        assert np.max(np.abs(chi[0])) <= 1e-28                                  # chi0(q = 0, w) = 0
        assert np.min(chi[1:, 2].real) >= 0.0 and np.min(chi[1:, 3:].imag) >= 0.0
        assert np.max(np.abs(chi[2, ::-1] - np.conj(chi[1]))) <= 1e-13 * scale   # commensurate q: chi0(-q, -w) = conj chi0(q, w)
        if kT > 0.0:
            assert np.max(np.abs(chi[4, ::-1] - np.conj(chi[3]))) >= 1e-3 * scale   # ... and not for an incommensurate one
    shifted = chr_.susceptibility(m, mesh, [incomm, [incomm[0] + 1.0, incomm[1]]], w, ETA, mu=0.3, kT=0.15)
    assert np.max(np.abs(shifted[0] - shifted[1])) >= 1e-2                       # orbitals off the lattice points: a form factor
    sq = square()
    shifted = chr_.susceptibility(sq, [8, 8], [incomm, [incomm[0] + 1.0, incomm[1] - 2.0]], w, ETA, mu=0.2, kT=0.15)
    assert np.max(np.abs(shifted[0] - shifted[1])) <= 1e-13 * np.max(np.abs(shifted))


# ---------------------------------------------------------------- GPU: against the NumPy form
def build(name):
    """(model, mesh, target of the Fermi level, insulator with the level in a gap)."""
    if name == "square_1":
        return square(), [16, 16], 0.3, False
    if name == "haldane_2":
        return haldane(), [12, 10], 0.0, True
    if name == "chain3_3":
        return hp.chain3(tb.tb_model, -1.3, 2.0, 0.3), [41], None, True
    if name == "kane_mele_4":
        return hp.kane_mele(tb.tb_model), [12, 10], None, True
    if name == "cubic16_16":
        return hp.cubic16(tb.tb_model), [4, 3, 5], 0.0, True
    if name == "haldane4x4_32":                               # the last size of the LDS pair kernel
        return quiet(haldane().make_supercell, [[4, 0], [0, 4]]), [3, 4], 0.0, True
    if name == "ribbon_34":                                   # the first wide size; 34 = 2 x 16 + 2: tile remainders
        return quiet(haldane().cut_piece, 17, 1), [7], 0.0, False
    raise KeyError(name)


def gap_target(m, mesh, qs):
    """The middle of the widest gap between consecutive bands over the mesh and its shifts."""
    kk = np.asarray(m.k_uniform_mesh(mesh), dtype=float).reshape(-1, m._dim_k)
    ev = np.concatenate([levels(m, kk)] + [levels(m, kk + q[None, :]) for q in qs])
    gaps = ev[:, 1:].min(axis=0) - ev[:, :-1].max(axis=0)
    b = int(np.argmax(gaps))
    assert gaps[b] > 0.05
    return 0.5 * (ev[:, b].max() + ev[:, b + 1].min())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["square_1", "haldane_2", "chain3_3", "kane_mele_4", "cubic16_16", "haldane4x4_32", "ribbon_34"])
def test_models(name):
    m, mesh, target, insulator = build(name)
    qs = q_mix(mesh)
    if target is None:
        target = gap_target(m, mesh, qs)
    mu0 = safe_mu(m, mesh, qs, target)
    for kT, mu in ((0.0, mu0), (KT, target + 0.11)):
        for me in (True, False):
            want = chr_.susceptibility(m, mesh, qs, OMEGA, ETA, mu=mu, kT=kT, matrix_elements=me)
            got = m.susceptibility_mesh(mesh, qs, OMEGA, ETA, fermi_level=mu, kT=kT, matrix_elements=me)
            assert got.shape == want.shape == (len(qs), len(OMEGA)) and got.dtype == complex
            close(got, want)
            if kT == 0.0 and not insulator:                   # a metal's static sum at kT = 0 has arbitrarily small denominators
                continue
            want = chr_.susceptibility(m, mesh, qs, mu=mu, kT=kT, matrix_elements=me)
            got = m.susceptibility_mesh(mesh, qs, fermi_level=mu, kT=kT, matrix_elements=me)
            assert got.shape == want.shape == (len(qs),) and got.dtype == float
            close(got, want)


@pytest.mark.gpu
def test_square_lattice_closed_forms_on_the_device():
    m = square()
    grid = np.array([[i / 16.0, j / 16.0] for i in range(16) for j in range(16)])
    chi = m.susceptibility_mesh(SQ_MESH, grid, fermi_level=0.0, kT=0.2)
    assert abs(chi[8 * 16 + 8] - SQ_STATIC_Q) <= 1e-10 * SQ_STATIC_Q
    assert abs(chi[0] - SQ_STATIC_0) <= 1e-10 * SQ_STATIC_Q
    order = np.argsort(chi)
    assert order[-1] == 8 * 16 + 8 and abs(chi[order[-2]] - 0.4448) <= 1e-4
    dyn = m.susceptibility_mesh(SQ_MESH, [0.5, 0.5], [0.0], 1e-3, fermi_level=0.0, kT=0.2)
    assert dyn.shape == (1,) and abs(dyn[0].real - SQ_DYNAMIC_Q) <= 1e-10 * SQ_DYNAMIC_Q
    # |M| = 1 for one state: with and without matrix elements
    qs = q_mix(SQ_MESH)
    for kw in ({}, {"omega": OMEGA, "eta": ETA}):
        a = m.susceptibility_mesh(SQ_MESH, qs, fermi_level=0.2, kT=KT, matrix_elements=True, **kw)
        b = m.susceptibility_mesh(SQ_MESH, qs, fermi_level=0.2, kT=KT, matrix_elements=False, **kw)
        assert np.max(np.abs(a - b)) <= 1e-14 * np.max(np.abs(b))


# ---------------------------------------------------------------- GPU: the boundaries of the pipeline
@pytest.mark.gpu
def test_chunk_edge_wide():
    """34 states on 1900 points: two chunks (32 MB / (34^2 16 B) = 1814 points, then 86 -- fewer than the 1024 k-groups, and 1814 is
    no multiple of them), static and two frequencies."""
    m = quiet(haldane().cut_piece, 17, 1)
    mesh = [1900]
    qs = np.array([[0.137]])
    w = np.array([-0.4, 0.9])
    stat, dyn = chr_.susceptibility_both(m, mesh, qs, w, ETA, mu=0.1, kT=KT)
    close(m.susceptibility_mesh(mesh, qs, fermi_level=0.1, kT=KT), stat)
    close(m.susceptibility_mesh(mesh, qs, w, ETA, fermi_level=0.1, kT=KT), dyn)


@pytest.mark.gpu
def test_frequency_tiles():
    """1030 frequencies: two full tiles of 512 and a third of six."""
    m = haldane()
    mesh = [12, 10]
    qs = q_mix(mesh)[1:3]
    w = np.linspace(-4.0, 4.0, 1030)
    mu = safe_mu(m, mesh, qs, 0.0)
    for kT in (0.0, KT):
        close(m.susceptibility_mesh(mesh, qs, w, ETA, fermi_level=mu, kT=kT), chr_.susceptibility(m, mesh, qs, w, ETA, mu=mu, kT=kT))


# ---------------------------------------------------------------- GPU: properties
@pytest.mark.gpu
def test_properties_on_the_device():
    m = hp.kane_mele(tb.tb_model)
    mesh = [12, 10]
    w = np.array([-1.1, -0.3, 0.0, 0.3, 1.1])
    comm = [3.0 / 12.0, -2.0 / 10.0]
    qs = np.array([[0.0, 0.0], comm, [-comm[0], -comm[1]], [0.137, 0.291]])
    for kT in (0.0, KT):
        mu = safe_mu(m, mesh, qs, 0.3) if kT == 0.0 else 0.3
        chi = m.susceptibility_mesh(mesh, qs, w, ETA, fermi_level=mu, kT=kT)
        assert np.max(np.abs(chi[0])) <= 1e-12                                   # charge conservation
        assert np.max(np.abs(chi[2, ::-1] - np.conj(chi[1]))) <= 1e-12           # commensurate q
        assert np.min(chi[1:, 3:].imag) >= 0.0 and np.min(chi[1:, 2].real) >= 0.0
        st = m.susceptibility_mesh(mesh, qs, fermi_level=mu, kT=kT)
        assert abs(st[0]) <= 1e-12 or kT > 0.0                                   # (kT > 0: -f' of a metal's Fermi surface stays)
        assert np.min(st) >= 0.0


@pytest.mark.gpu
def test_repeat_sublist_single_and_zeros():
    for m, mesh in ((haldane(), [12, 10]), (quiet(haldane().cut_piece, 17, 1), [7])):
        qs = q_mix(mesh)[1:]
        for kw in ({}, {"omega": OMEGA, "eta": ETA}):
            for me in (True, False):
                a = m.susceptibility_mesh(mesh, qs, fermi_level=0.1, kT=KT, matrix_elements=me, **kw)
                np.testing.assert_array_equal(a, m.susceptibility_mesh(mesh, qs, fermi_level=0.1, kT=KT, matrix_elements=me, **kw))
                one = m.susceptibility_mesh(mesh, qs[1:2], fermi_level=0.1, kT=KT, matrix_elements=me, **kw)
                np.testing.assert_array_equal(one[0], a[1])                      # alone and inside a three-q list
                single = m.susceptibility_mesh(mesh, qs[1], fermi_level=0.1, kT=KT, matrix_elements=me, **kw)
                assert single.shape == a.shape[1:]                               # a (dim_k,) q drops the leading axis
                np.testing.assert_array_equal(single, a[1])
            e = m.solve_all_mesh(mesh)
            for mu in (e.min() - 1.0, e.max() + 1.0):                            # (the bands of k + q span the same range)
                kk = np.asarray(m.k_uniform_mesh(mesh)).reshape(-1, m._dim_k)
                ev = np.concatenate([levels(m, kk + q[None, :]).ravel() for q in qs])
                assert mu < ev.min() - 0.5 or mu > ev.max() + 0.5
                z = m.susceptibility_mesh(mesh, qs, fermi_level=mu, **kw)
                assert np.all(z == 0.0)
