"""The orbital-resolved susceptibility matrix chi0_ab(q, w) and its RPA on k meshes (tb_model.susceptibility_matrix_mesh) against the
NumPy restatement in chim_ref.py, the scalar chi0 of susceptibility_mesh, the closed forms of the one-band square lattice, and the
properties of the formula."""
import numpy as np
import pytest

import chi_ref as chr_
import chim_ref as cmr
import helpers as hp
from helpers import quiet
from oracle import tb_oracle as orc

import pythtb_amd as tb

OMEGA = np.array([-1.3, -0.2, 0.0, 0.35, 1.1, 2.7])          # (the frequencies of the scalar tests)
ETA = 0.05
KT = 0.07
SQ_MESH = [16, 16]
SQ_STATIC_Q = 0.507732137760894                               # mean_k tanh(E / 2kT) / (2 E) at kT = 0.2 (test_susceptibility.py)
V2 = np.array([[2.5, 0.4 - 0.3j], [0.4 + 0.3j, 2.0]])
COND_BOUND = 10.0                                             # asserted from the reference before any RPA comparison


def haldane(delta=0.2):
    return hp.haldane(tb.tb_model, delta=delta)


def square(t=-1.0):
    m = quiet(tb.tb_model, 2, 2, [[1.0, 0.0], [0.0, 1.0]], [[0.0, 0.0]])
    m.set_hop(t, 0, 0, [1, 0])
    m.set_hop(t, 0, 0, [0, 1])
    return m


def chain1(t=-1.0):
    m = quiet(tb.tb_model, 1, 1, [[1.0]], [[0.0]])
    m.set_hop(t, 0, 0, [1])
    return m


def levels(m, kpts):
    return np.linalg.eigvalsh(orc.ham_batch(m, np.asarray(kpts, dtype=float).reshape(-1, m._dim_k)))


def all_levels(m, mesh, qs):
    kk = np.asarray(m.k_uniform_mesh(mesh), dtype=float).reshape(-1, m._dim_k)
    return np.unique(np.concatenate([levels(m, kk).ravel()] + [levels(m, kk + np.asarray(q)[None, :]).ravel() for q in qs]))


def safe_mu(m, mesh, qs, target):
    """The midpoint of the two levels around `target` among every level at k and at k + q: asserted to be at least 1e-6 from
    all of them, so that no kT = 0 occupation depends on the last bits of an eigenvalue (the rule of test_susceptibility.py)."""
    s = all_levels(m, mesh, qs)
    j = int(np.searchsorted(s, target))
    if j == 0:
        return s[0] - 1.0
    if j == len(s):
        return s[-1] + 1.0
    mu = 0.5 * (s[j - 1] + s[j])
    assert s[j] - s[j - 1] >= 2e-6
    assert np.min(np.abs(s - mu)) >= 1e-6
    return mu


def mid_target(m, mesh, qs):
    """A target for safe_mu inside the spectrum: the middle of the widest gap between consecutive levels of the central half."""
    s = all_levels(m, mesh, qs)
    lo, hi = len(s) // 4, max(len(s) // 4 + 2, 3 * len(s) // 4)
    c = s[lo:hi]
    j = int(np.argmax(np.diff(c)))
    return 0.5 * (c[j] + c[j + 1])


def q_mix(mesh):
    """q = 0, a q commensurate with the mesh, an incommensurate one and one with a component beyond 1."""
    d = len(mesh)
    comm = [(1 + i) / mesh[i] * (-1.0) ** i for i in range(d)]
    return np.array([[0.0] * d, comm, [0.137, 0.291, -0.413][:d], [1.3, -0.45, 0.21][:d]])


def close(got, want, rel=1e-10, what=""):
    scale = np.max(np.abs(want))
    if scale == 0.0:
        assert np.all(got == 0.0)
        return
    err = np.max(np.abs(got - want))
    print("%s max abs error / max |reference| = %.3e" % (what, err / scale))
    assert err <= rel * scale, err / scale


def cases(m, mesh, qs):
    """(kT, mu): kT = 0 with a safe level inside the spectrum, and kT = 0.07."""
    t = mid_target(m, mesh, qs)
    return ((0.0, safe_mu(m, mesh, qs, t)), (KT, t + 0.11))


_REF = {}


def haldane_ref(kT):
    """The reference of Haldane [6, 5] on the four-q mix, computed once: (model, mesh, qs, mu, static, dynamic)."""
    if kT not in _REF:
        m, mesh = haldane(), [6, 5]
        qs = q_mix(mesh)
        mu = 0.1 if kT > 0.0 else safe_mu(m, mesh, qs, 0.0)
        _REF[kT] = (m, mesh, qs, mu, cmr.chi0_matrix(m, mesh, qs, mu=mu, kT=kT), cmr.chi0_matrix(m, mesh, qs, OMEGA, ETA, mu=mu, kT=kT))
    return _REF[kT]


# ---------------------------------------------------------------- CPU: argument errors
def test_argument_errors_without_gpu():
    m = haldane()
    f = m.susceptibility_matrix_mesh
    flat = quiet(tb.tb_model, 0, 2, hp.LAT, hp.ORB)
    with pytest.raises(Exception, match="dim_k"):
        flat.susceptibility_matrix_mesh([4], [[0.1]], [0.1], 0.1)
    q = [[0.25, 0.1]]
    for bad in ([8], [8, 0], [8, 8, 8]):
        with pytest.raises(Exception):
            f(bad, q, [0.1], 0.1)
    for bad in ([0.1], [[0.1]], [[0.1, 0.2, 0.3]], [[[0.1, 0.2]]], np.zeros((0, 2)), [], [[0.1, np.nan]], [np.inf, 0.0],
                np.zeros((65537, 2))):
        with pytest.raises(Exception, match="q_list"):
            f([8, 8], bad, [0.1], 0.1)
        with pytest.raises(Exception, match="q_list"):
            f([8, 8], bad)
    for w in ([], [[0.1, 0.2]], [0.1, np.nan], [np.inf], np.zeros(65537)):
        with pytest.raises(Exception, match="omega"):
            f([8, 8], q, w, 0.1)
    for eta in (0.0, -0.1, np.inf, np.nan):
        with pytest.raises(Exception, match="eta"):
            f([8, 8], q, [0.1], eta)
    with pytest.raises(Exception, match="eta"):              # static mode: eta has no meaning
        f([8, 8], q, eta=0.1)
    with pytest.raises(Exception, match="eta"):              # dynamic mode: eta is needed
        f([8, 8], q, [0.1])
    for kT in (-1e-3, np.inf):
        with pytest.raises(Exception, match="kT"):
            f([8, 8], q, [0.1], 0.1, kT=kT)
        with pytest.raises(Exception, match="kT"):
            f([8, 8], q, kT=kT)
    with pytest.raises(Exception, match="fermi_level"):
        f([8, 8], q, [0.1], 0.1, fermi_level=np.nan)
    with pytest.raises(Exception, match="fermi_level"):
        f([8, 8], q, fermi_level=np.inf)
    with pytest.raises(Exception, match="nq"):               # 65 x 65536 x 1 > 2**22
        f([8, 8], np.zeros((65, 2)), np.zeros(65536), 0.1, states=[0])
    with pytest.raises(Exception, match="nq"):               # 1025 x 1024 x 4 > 2**22
        f([8, 8], np.zeros((1025, 2)), np.zeros(1024), 0.1)
    big = quiet(haldane().make_supercell, [[3, 0], [0, 3]])   # 18 states
    for st in ([], [0, 0], [1, 0, 1], [18], [-1], [0, 18], list(range(17)), [0.0, 1.0], [[0, 1]]):
        with pytest.raises(Exception, match="states"):
            big.susceptibility_matrix_mesh([8, 8], q, states=st)
    with pytest.raises(Exception, match="states"):           # all of more than 16 states
        big.susceptibility_matrix_mesh([8, 8], q)
    for v in (np.eye(3), np.zeros((2, 2, 2)), np.zeros(2), [[1.0, np.nan], [0.0, 1.0]], [[1.0, np.inf], [0.0, 1.0]], 1.5):
        with pytest.raises(Exception, match="interaction"):
            f([8, 8], q, interaction=v)
    with pytest.raises(Exception, match="interaction"):      # (nq, na, na) for another nq
        f([8, 8], [[0.1, 0.2]] * 3, interaction=np.zeros((2, 2, 2)))
    with pytest.raises(Exception, match="interaction"):      # (na, na) of the selection, not of the model
        f([8, 8], q, states=[1], interaction=np.eye(2))
    with pytest.raises(Exception, match="return_det"):
        f([8, 8], q, return_det=True)


# ---------------------------------------------------------------- CPU: the reference's own properties and closed forms
@pytest.mark.parametrize("kT", [KT, 0.0])
def test_numpy_reference_properties(kT):
    m, mesh, qs, mu, stat, dyn = haldane_ref(kT)
    assert stat.shape == (4, 2, 2) and dyn.shape == (4, 6, 2, 2)
    # the sum over all a, b is the scalar chi0
    es = np.max(np.abs(stat.sum(axis=(-2, -1)) - chr_.susceptibility(m, mesh, qs, mu=mu, kT=kT)))
    ed = np.max(np.abs(dyn.sum(axis=(-2, -1)) - chr_.susceptibility(m, mesh, qs, OMEGA, ETA, mu=mu, kT=kT)))
    print("sum over a, b against the scalar: static %.1e dynamic %.1e" % (es, ed))
    assert es <= 1e-13 and ed <= 1e-13
    # static: Hermitian, positive semidefinite, not real
    assert np.max(np.abs(stat - np.conj(np.transpose(stat, (0, 2, 1))))) <= 1e-15
    assert min(np.linalg.eigvalsh(0.5 * (s + s.conj().T)).min() for s in stat) >= -1e-15
    assert np.max(np.abs(stat.imag)) >= 1e-3
    # q = 0: charge conservation per orbital in the dynamic matrix; the static one keeps the intraband -f' term at kT > 0
    assert np.max(np.abs(dyn[0].sum(axis=-1))) <= 1e-14 and np.max(np.abs(dyn[0].sum(axis=-2))) <= 1e-14
    if kT > 0.0:
        assert np.min(np.abs(stat[0].sum(axis=-1))) > 1e-5 and np.min(np.abs(stat[0].sum(axis=-2))) > 1e-5


def test_numpy_square_lattice_rpa_closed_form():
    chi0 = cmr.chi0_matrix(square(), SQ_MESH, [[0.5, 0.5]], mu=0.0, kT=0.2)
    assert chi0.shape == (1, 1, 1) and abs(chi0[0, 0, 0] - SQ_STATIC_Q) <= 1e-12
    chi, det, cond = cmr.rpa(chi0, [[1.5]])
    assert abs(det[0] - (1.0 - 1.5 * SQ_STATIC_Q)) <= 1e-12
    assert abs(chi[0, 0, 0] - SQ_STATIC_Q / (1.0 - 1.5 * SQ_STATIC_Q)) <= 1e-11


# ---------------------------------------------------------------- GPU: against the NumPy form
def build(name):
    """(model, mesh, states)."""
    if name == "haldane_2":
        return haldane(), [6, 5], None
    if name == "chain_1":
        return chain1(), [7], None
    if name == "kane_mele_4_sub":                             # an unsorted subset; degeneracies at the TRIM
        return hp.kane_mele(tb.tb_model), [5, 4], [3, 0, 2]
    if name == "cubic16_all":
        return hp.cubic16(tb.tb_model), [3, 2, 2], None
    if name == "cubic16_sub":
        return hp.cubic16(tb.tb_model), [3, 2, 2], [15, 0, 7]
    if name == "random_32":                                   # the last size of the LDS kernel: one point per batch
        return hp.random_model(tb.tb_model, 32, 2, 1, seed=5), [3, 2], [31, 4, 0, 17, 9]
    if name == "haldane3x6_36":                               # the wide form
        return quiet(haldane().make_supercell, [[3, 0], [0, 6]]), [3, 2], [0, 5, 17, 35]
    raise KeyError(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["haldane_2", "chain_1", "kane_mele_4_sub", "cubic16_all", "cubic16_sub", "random_32", "haldane3x6_36"])
def test_models(name):
    m, mesh, states = build(name)
    qs = q_mix(mesh)
    na = m._nsta if states is None else len(states)
    for kT, mu in cases(m, mesh, qs):
        want = cmr.chi0_matrix(m, mesh, qs, mu=mu, kT=kT, states=states)
        got = m.susceptibility_matrix_mesh(mesh, qs, fermi_level=mu, kT=kT, states=states)
        assert got.shape == want.shape == (len(qs), na, na) and got.dtype == complex
        close(got, want, what="%s kT=%g static" % (name, kT))
        want = cmr.chi0_matrix(m, mesh, qs, OMEGA, ETA, mu=mu, kT=kT, states=states)
        got = m.susceptibility_matrix_mesh(mesh, qs, OMEGA, ETA, fermi_level=mu, kT=kT, states=states)
        assert got.shape == want.shape == (len(qs), len(OMEGA), na, na) and got.dtype == complex
        close(got, want, what="%s kT=%g dynamic" % (name, kT))


# ---------------------------------------------------------------- GPU: the boundaries of the pipeline
@pytest.mark.gpu
def test_chunk_edge_wide():
    """36 states, 4 selected, on 41 x 40 = 1640 points: two chunks (32 MB / (36^2 16 B) = 1618 points -- fewer than the 32 MB /
    (2 36 4^2 16 B) = 1820 that the tables allow -- then 22, fewer than the 1024 k-groups), static and two frequencies."""
    m = quiet(haldane().make_supercell, [[3, 0], [0, 6]])
    n, sel = m._nsta, [0, 5, 17, 35]
    chunk = min((32 << 20) // (n * n * 16), (32 << 20) // (2 * n * len(sel) ** 2 * 16))
    mesh = [41, 40]
    assert n == 36 and chunk == 1618 and chunk < mesh[0] * mesh[1] < 2 * chunk
    qs = np.array([[0.137, 0.291]])
    w = np.array([-0.4, 0.9])
    close(m.susceptibility_matrix_mesh(mesh, qs, fermi_level=0.1, kT=KT, states=sel),
          cmr.chi0_matrix(m, mesh, qs, mu=0.1, kT=KT, states=sel), what="static")
    close(m.susceptibility_matrix_mesh(mesh, qs, w, ETA, fermi_level=0.1, kT=KT, states=sel),
          cmr.chi0_matrix(m, mesh, qs, w, ETA, mu=0.1, kT=KT, states=sel), what="dynamic")


@pytest.mark.gpu
@pytest.mark.parametrize("nw", [257, 513])
def test_frequency_tiles(nw):
    """63 points (no multiple of a batch); 257 frequencies: a tile whose second half is empty; 513: a second tile of one."""
    m, mesh = haldane(), [9, 7]
    qs = q_mix(mesh)[2:3]
    w = np.linspace(-4.0, 4.0, nw)
    close(m.susceptibility_matrix_mesh(mesh, qs, w, ETA, fermi_level=0.1, kT=KT),
          cmr.chi0_matrix(m, mesh, qs, w, ETA, mu=0.1, kT=KT), what="nw=%d" % nw)
    close(m.susceptibility_matrix_mesh(mesh, qs, fermi_level=0.1, kT=KT), cmr.chi0_matrix(m, mesh, qs, mu=0.1, kT=KT), what="static")


@pytest.mark.gpu
def test_group_sum_by_lanes():
    """16 states and 32 frequencies: 2 x 16^2 x 32 = 16384 rows per q, the first size whose groups are added by one lane per row
    (31 frequencies: the last one with a workgroup per row)."""
    m, mesh = hp.cubic16(tb.tb_model), [3, 2, 2]
    qs = q_mix(mesh)[2:3]
    for nw in (31, 32):
        w = np.linspace(-3.0, 3.0, nw)
        close(m.susceptibility_matrix_mesh(mesh, qs, w, ETA, fermi_level=0.1, kT=KT),
              cmr.chi0_matrix(m, mesh, qs, w, ETA, mu=0.1, kT=KT), what="nw=%d" % nw)


# ---------------------------------------------------------------- GPU: properties
@pytest.mark.gpu
def test_properties_on_the_device():
    m, mesh = haldane(), [12, 10]
    qs = q_mix(mesh)
    for kT in (0.0, KT):
        mu = safe_mu(m, mesh, qs, 0.0) if kT == 0.0 else 0.1
        stat = m.susceptibility_matrix_mesh(mesh, qs, fermi_level=mu, kT=kT)
        dyn = m.susceptibility_matrix_mesh(mesh, qs, OMEGA, ETA, fermi_level=mu, kT=kT)
        close(stat.sum(axis=(-2, -1)), m.susceptibility_mesh(mesh, qs, fermi_level=mu, kT=kT), what="static sum")
        close(dyn.sum(axis=(-2, -1)), m.susceptibility_mesh(mesh, qs, OMEGA, ETA, fermi_level=mu, kT=kT), what="dynamic sum")
        assert np.max(np.abs(stat - np.conj(np.transpose(stat, (0, 2, 1))))) <= 1e-14 * np.max(np.abs(stat))
        # q = 0: <u_n|u_m> = delta_nm to the solver's rounding, divided by eta at worst: the bound of the scalar chi0(q = 0) test
        assert np.max(np.abs(dyn[0].sum(axis=-1))) <= 1e-12 and np.max(np.abs(dyn[0].sum(axis=-2))) <= 1e-12
        if kT > 0.0:
            assert np.min(np.abs(stat[0].sum(axis=-1))) > 1e-5
        for kw in ({}, {"omega": OMEGA, "eta": ETA}):
            a = m.susceptibility_matrix_mesh(mesh, qs, fermi_level=mu, kT=kT, states=[1, 0], **kw)
            b = stat if not kw else dyn
            assert np.max(np.abs(a - b[..., ::-1, ::-1])) <= 1e-13 * np.max(np.abs(b))
            one = m.susceptibility_matrix_mesh(mesh, qs, fermi_level=mu, kT=kT, states=[1], **kw)
            assert np.max(np.abs(one[..., 0, 0] - b[..., 1, 1])) <= 1e-13 * np.max(np.abs(b))


@pytest.mark.gpu
def test_repeat_sublist_single_and_zeros():
    for m, mesh, sel in ((haldane(), [12, 10], None), (quiet(haldane().make_supercell, [[3, 0], [0, 6]]), [3, 2], [0, 5, 17, 35])):
        qs = q_mix(mesh)[1:]
        v = V2 if sel is None else np.diag([1.0, 2.0, 0.5, 1.5]) + 0.1j
        for kw in ({}, {"omega": OMEGA, "eta": ETA}):
            a = m.susceptibility_matrix_mesh(mesh, qs, fermi_level=0.1, kT=KT, states=sel, **kw)
            np.testing.assert_array_equal(a, m.susceptibility_matrix_mesh(mesh, qs, fermi_level=0.1, kT=KT, states=sel, **kw))
            one = m.susceptibility_matrix_mesh(mesh, qs[2:3], fermi_level=0.1, kT=KT, states=sel, **kw)
            np.testing.assert_array_equal(one[0], a[2])                          # alone and inside a three-q list
            single = m.susceptibility_matrix_mesh(mesh, qs[2], fermi_level=0.1, kT=KT, states=sel, **kw)
            assert single.shape == a.shape[1:]                                   # a (dim_k,) q drops the leading axis
            np.testing.assert_array_equal(single, a[2])
            c0, chi, det = m.susceptibility_matrix_mesh(mesh, qs, fermi_level=0.1, kT=KT, states=sel, interaction=v, return_det=True, **kw)
            np.testing.assert_array_equal(c0, a)                                 # chi0 with an interaction: the same bits
            assert chi.shape == a.shape and det.shape == a.shape[:-2] and det.dtype == complex
            s0, schi, sdet = m.susceptibility_matrix_mesh(mesh, qs[2], fermi_level=0.1, kT=KT, states=sel, interaction=v, return_det=True,
                                                          **kw)
            np.testing.assert_array_equal(schi, chi[2])
            np.testing.assert_array_equal(sdet, det[2])
            for mu in (-50.0, 50.0):                                             # kT = 0, a level outside the spectrum: exact zeros
                z = m.susceptibility_matrix_mesh(mesh, qs, fermi_level=mu, states=sel, **kw)
                assert z.shape == a.shape and np.all(z == 0.0)


# ---------------------------------------------------------------- GPU: RPA
@pytest.mark.gpu
@pytest.mark.parametrize("kT", [KT, 0.0])
def test_rpa_parity(kT):
    m, mesh, qs, mu, stat, dyn = haldane_ref(kT)
    scale = np.array([1.0, 0.7, -0.4, 1.2])
    for v in (V2, scale[:, None, None] * V2[None]):
        for ref, kw in ((stat, {}), (dyn, {"omega": OMEGA, "eta": ETA})):
            want, wdet, cond = cmr.rpa(ref, v)
            print("max cond_2(1 - chi0 V) = %.2f, min |det| = %.3f" % (cond.max(), np.abs(wdet).min()))
            assert cond.max() <= COND_BOUND                                      # the inputs are well inside the bound of the tolerance
            c0, chi, det = m.susceptibility_matrix_mesh(mesh, qs, fermi_level=mu, kT=kT, interaction=v, return_det=True, **kw)
            close(c0, ref, what="chi0")
            close(chi, want, rel=1e-10 * COND_BOUND, what="chi_rpa")
            close(det, wdet, rel=1e-10 * COND_BOUND, what="det")
            two = m.susceptibility_matrix_mesh(mesh, qs, fermi_level=mu, kT=kT, interaction=v, **kw)
            assert len(two) == 2
            np.testing.assert_array_equal(two[1], chi)


@pytest.mark.gpu
def test_rpa_square_lattice_and_stoner_point():
    """The closed form chi = chi0 / (1 - V chi0) at the nesting vector, then the Stoner point V = 1 / chi0 of the device's own chi0.
    On an MI355X the fused 1 - chi0 V gave -2.7e-18, not 0.0: the second branch below ran, chi_rpa was finite."""
    m = square()
    d = 1.0 - 1.5 * SQ_STATIC_Q
    assert 1.0 / d <= COND_BOUND                                                  # d chi / chi = (d chi0 / chi0) / (1 - V chi0)
    c0, chi, det = m.susceptibility_matrix_mesh(SQ_MESH, [0.5, 0.5], fermi_level=0.0, kT=0.2, interaction=[[1.5]], return_det=True)
    assert c0.shape == chi.shape == (1, 1) and det.shape == ()
    close(np.array([c0[0, 0]]), np.array([SQ_STATIC_Q]), what="chi0(Q)")
    close(np.array([chi[0, 0]]), np.array([SQ_STATIC_Q / d]), rel=1e-10 * COND_BOUND, what="chi(Q)")
    close(np.array([det]), np.array([d]), rel=1e-10 * COND_BOUND, what="det(Q)")
    # the Stoner point itself, V = 1 / chi0 of the device's own value: no exception
    v = 1.0 / c0[0, 0]
    c1, chi, det = m.susceptibility_matrix_mesh(SQ_MESH, [0.5, 0.5], fermi_level=0.0, kT=0.2, interaction=[[v]], return_det=True)
    assert c1[0, 0] == c0[0, 0]
    if det == 0.0:
        print("1 - chi0 (1 / chi0) is exactly 0: det = 0, chi_rpa NaN")
        assert np.isnan(chi[0, 0])
    else:
        print("1 - chi0 (1 / chi0) = %r: no exact zero" % det)
        assert abs(det) <= 1e-15 and (np.isnan(chi[0, 0]) or np.isfinite(chi[0, 0]))
    # chi0 = 0 (kT = 0, the level below the spectrum): chi = 0 and det = 1 exactly
    z = haldane().susceptibility_matrix_mesh([6, 5], [[0.137, 0.291]], fermi_level=-50.0, interaction=np.eye(2), return_det=True)
    assert np.all(z[0] == 0.0) and np.all(z[1] == 0.0) and z[2][0] == 1.0
