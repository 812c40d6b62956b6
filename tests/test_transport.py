"""Fermi-surface transport (tb_model.band_velocity, anomalous_transport_mesh, drude_weight_mesh) against the NumPy restatement in
transport_ref.py, against finite differences of eigenvalues and curvatures (integration by parts, the Maxwell relation), and
against berry_curvature_mesh in the cold limit."""
import numpy as np
import pytest

import curv_ref as cr
import helpers as hp
import spin_curv_ref as sr
import transport_ref as tr
from helpers import quiet
from oracle import tb_oracle as orc
from test_berry_curvature import CURV_MODELS

import pythtb_amd as tb

GAP_MIN = 1e-3            # the threshold of test_spin_hall: a band is dropped where one of its own two neighbouring gaps is below it
LEVELS = np.linspace(-2.0, 1.5, 6)
KT = 0.1


def close(got, want, scale, rel=1e-9):
    err = np.max(np.abs(np.asarray(got) - np.asarray(want)))
    assert err <= rel * scale, (err, scale)


def strained(haldane=False, nspin=1):
    """Honeycomb with one nearest-neighbour bond stretched: time-reversal symmetric, no inversion (onsite -0.3, +0.3), no C3,
    gapped.  haldane=True adds Haldane's 0.15 i second-neighbour set; nspin=2 doubles it without any spin dependence."""
    m = quiet(tb.tb_model, 2, 2, hp.LAT, hp.ORB, nspin=nspin)
    m.set_onsite([-0.3, 0.3])
    m.set_hop(-1.0, 0, 1, [0, 0])
    m.set_hop(-1.4, 1, 0, [1, 0])
    m.set_hop(-1.0, 1, 0, [0, 1])
    if haldane:
        t2 = 0.15j
        for amp, i, R in [(t2, 0, [1, 0]), (t2, 1, [1, -1]), (t2, 1, [0, 1]), (-t2, 1, [1, 0]), (-t2, 0, [1, -1]), (-t2, 0, [0, 1])]:
            m.set_hop(amp, i, i, R)
    return m


def strained_kane_mele():
    """helpers.kane_mele ("odd") with the nearest-neighbour hop along [0, -1] changed from 1 to 1.4: still time-reversal
    symmetric (Kramers pairs at the four time-reversal-invariant k, which lie on every even mesh), no C3."""
    m = quiet(tb.tb_model, 2, 2, hp.LAT, hp.ORB, nspin=2)
    so, ra, r3h = 0.3, 0.25, np.sqrt(3.0) / 2.0
    sx, sy, sz = np.array([0.0, 1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0, 0.0]), np.array([0.0, 0.0, 0.0, 1.0])
    m.set_onsite([1.0, -1.0])
    m.set_hop(1.0, 0, 1, [0, 0])
    m.set_hop(1.4, 0, 1, [0, -1])
    m.set_hop(1.0, 0, 1, [-1, 0])
    for sign, i, R in [(-1, 0, [0, 1]), (1, 0, [1, 0]), (-1, 0, [1, -1]), (1, 1, [0, 1]), (-1, 1, [1, 0]), (1, 1, [1, -1])]:
        m.set_hop(sign * 1.0j * so * sz, i, i, R)
    m.set_hop(1.0j * ra * (0.5 * sx - r3h * sy), 0, 1, [0, 0], mode="add")
    m.set_hop(1.0j * ra * (-1.0 * sx), 0, 1, [0, -1], mode="add")
    m.set_hop(1.0j * ra * (0.5 * sx + r3h * sy), 0, 1, [-1, 0], mode="add")
    return m


def supercell(m, s):
    return quiet(m.make_supercell, [[s, 0], [0, s]])


def haldane():
    return hp.haldane(tb.tb_model, delta=0.2)


def fd4(fn, kk, c, h):
    """4th-order central difference of fn(k) along reduced axis c."""
    e = np.zeros(kk.shape[1])
    e[c] = h
    return (-fn(kk + 2 * e) + 8.0 * fn(kk + e) - 8.0 * fn(kk - e) + fn(kk - 2 * e)) / (12.0 * h)


def ibp_dipole_error(m, mesh=(128, 128), h=2e-3):
    """(largest |dipole[c] - mean sum_n f_n d_c Omega_n| over c and LEVELS, max |dipole|), restatement only."""
    kk = m.k_uniform_mesh(mesh)
    e = np.linalg.eigvalsh(orc.ham_batch(m, kk)).T
    _, _, dip, sc = tr.transport(m, mesh, LEVELS, KT)
    err = 0.0
    for c in range(2):
        dom = fd4(lambda q: cr.curvature(m, q), kk, c, h)
        want = np.array([(tr.weights(e, mu, KT)[0] * dom).sum(axis=0).mean() for mu in LEVELS])
        err = max(err, np.max(np.abs(dip[c] - want)))
    return err, np.max(np.abs(dip))


def ibp_drude_error(m, mesh=(128, 128), h=2e-3):
    """(largest |D_cd - mean sum_n f_n d_c v^d_n|, D's scale), restatement only; the bands must not be degenerate anywhere."""
    kk = m.k_uniform_mesh(mesh)
    e = np.linalg.eigvalsh(orc.ham_batch(m, kk)).T
    dd, sc = tr.drude(m, mesh, LEVELS, KT)
    err = 0.0
    for c in range(2):
        dv = fd4(lambda q: tr.band_terms(m, q)[1], kk, c, h)            # (d, n, nk)
        for d in range(2):
            want = np.array([(tr.weights(e, mu, KT)[0] * dv[d]).sum(axis=0).mean() for mu in LEVELS])
            err = max(err, np.max(np.abs(dd[:, c, d] - want)))
    return err, sc


def maxwell_error(m, mesh=(64, 64), h=1e-4):
    """largest |d nernst / d mu - d hall / d kT| over LEVELS by central differences, restatement only."""
    dn = (tr.transport(m, mesh, LEVELS + h, KT)[1] - tr.transport(m, mesh, LEVELS - h, KT)[1]) / (2.0 * h)
    dh = (tr.transport(m, mesh, LEVELS, KT + h)[0] - tr.transport(m, mesh, LEVELS, KT - h)[0]) / (2.0 * h)
    return np.max(np.abs(dn - dh)), np.max(np.abs(dh))


# ---------------------------------------------------------------- CPU: the restatement alone, and argument errors
def test_numpy_time_reversal_gives_a_dipole_and_no_hall():
    """Strained honeycomb, 128^2, kT = 0.1: hall and nernst vanish (2.2e-16 and 1.1e-16 when this was written) while
    max |dipole| = 2.64."""
    m = strained()
    assert hasattr(m, "anomalous_transport_mesh")          # (the restatement alone does not need the feature)
    hall, nernst, dip, _ = tr.transport(m, [128, 128], LEVELS, KT)
    print(np.max(np.abs(hall)), np.max(np.abs(nernst)), np.max(np.abs(dip)))
    assert np.max(np.abs(hall)) < 1e-15 and np.max(np.abs(nernst)) < 1e-15
    assert np.max(np.abs(dip)) > 2.5


def test_numpy_c3_gives_a_hall_integral_and_no_dipole():
    """Haldane (delta = 0.2), the same settings: max |dipole| = 4.4e-16 when this was written, max |hall| = 6.28."""
    m = haldane()
    assert hasattr(m, "anomalous_transport_mesh")
    hall, _, dip, _ = tr.transport(m, [128, 128], LEVELS, KT)
    print(np.max(np.abs(hall)), np.max(np.abs(dip)))
    assert np.max(np.abs(dip)) <= 1e-12
    assert abs(np.max(np.abs(hall)) - 6.28) < 0.01


def test_numpy_integration_by_parts():
    """dipole[c] = mean sum f d_c Omega and D_cd = mean sum f d_c v^d on 128^2 at kT = 0.1, the derivatives by 4th-order central
    differences (h = 2e-3) of the restatement's curvature and velocity.  The finite differences limit the agreement, so each
    tolerance is 10 x what the restatement gave when this was written: 3.16e-7 with max |dipole| = 2.64 (strained), 1.92e-7 with
    0.294 (strained + Haldane), and 4.67e-7 for D on a scale of 10.95 (strained + Haldane)."""
    assert hasattr(strained(), "drude_weight_mesh")
    for m, tol in ((strained(), 3.16e-6), (strained(True), 1.92e-6)):
        err, sc = ibp_dipole_error(m)
        print("dipole", err, sc)
        assert err <= tol
    err, sc = ibp_drude_error(strained(True))
    print("drude", err, sc)
    assert abs(sc - 10.95) < 0.01
    assert err <= 4.67e-6


def test_numpy_maxwell_relation():
    """d nernst / d mu = d hall / d kT (both are mean sum x f (1 - f) Omega / kT), central differences with h = 1e-4 on
    strained + Haldane, 64^2.  The restatement gave 7.47e-7 at most (derivatives up to 1.84) when this was written; the tolerance
    is 10 x that."""
    m = strained(True)
    assert hasattr(m, "anomalous_transport_mesh")
    err, sc = maxwell_error(m)
    print(err, sc)
    assert sc > 1.0
    assert err <= 7.47e-6


def test_numpy_group_rule():
    """Random unitaries inside every group of the restatement's eigenvectors leave the dipole and D unchanged, and the spin-doubled
    model gives twice the spinless one."""
    assert hasattr(strained(), "drude_weight_mesh")
    mesh = [24, 24]
    one = tr.transport(strained(), mesh, LEVELS, KT)
    one_d = tr.drude(strained(), mesh, LEVELS, KT)
    for m in (strained(nspin=2), strained_kane_mele()):
        gid = tr.group_ids(np.linalg.eigvalsh(orc.ham_batch(m, m.k_uniform_mesh(mesh))))
        assert np.any(gid[0] != np.arange(4))               # k = 0 holds Kramers (or spin) pairs
        lv = LEVELS
        plain, plain_d = tr.transport(m, mesh, lv, KT), tr.drude(m, mesh, lv, KT)
        assert np.max(np.abs(plain[2])) > 0.1 and np.max(np.abs(plain_d[0])) > 1.0
        for seed in (1, 2):
            rot = tr.transport(m, mesh, lv, KT, rng=np.random.default_rng(seed))
            rot_d = tr.drude(m, mesh, lv, KT, rng=np.random.default_rng(seed))
            close(rot[2], plain[2], plain[3][2], rel=1e-12)
            close(rot_d[0], plain_d[0], plain_d[1], rel=1e-12)
    dbl, dbl_d = tr.transport(strained(nspin=2), mesh, LEVELS, KT), tr.drude(strained(nspin=2), mesh, LEVELS, KT)
    close(dbl[2], 2.0 * one[2], one[3][2], rel=1e-12)
    close(dbl_d[0], 2.0 * one_d[0], one_d[1], rel=1e-12)


def test_argument_errors_without_gpu():
    m = haldane()
    chain = hp.chain3(tb.tb_model, -1.0, 0.5, 0.1)
    dot = quiet(tb.tb_model, 0, 1, [[1.0]], [[0.0], [0.5]])
    lv = [0.0, 0.1]
    # dim_k
    with pytest.raises(Exception, match="dim_k >= 1"):
        dot.band_velocity([])
    with pytest.raises(Exception, match="dim_k >= 2"):
        chain.anomalous_transport_mesh([8], lv, 0.1)
    with pytest.raises(Exception, match="dim_k"):
        dot.drude_weight_mesh([], lv, 0.1)
    # dirs
    for bad in (2, -1, 0.5, (0, 1), "x"):
        with pytest.raises(Exception, match="dirs"):
            m.band_velocity([[0.1, 0.2]], dirs=bad)
    with pytest.raises(Exception, match="wrong shape"):
        m.band_velocity([[0.1, 0.2, 0.3]])
    for bad in [(0, 0), (1, 1), (0, 2), (-1, 0), (0,)]:
        with pytest.raises(Exception):
            m.anomalous_transport_mesh([8, 8], lv, 0.1, dirs=bad)
    # kT
    for bad in (0.0, -0.1, np.inf, np.nan):
        with pytest.raises(Exception, match="kT"):
            m.anomalous_transport_mesh([8, 8], lv, bad)
        with pytest.raises(Exception, match="kT"):
            m.drude_weight_mesh([8, 8], lv, bad)
    # levels
    for bad, what in (([[0.0, 1.0]], "1-D"), (0.0, "1-D"), ([], "1-D"), (np.zeros(8193), "1-D"), ([0.0, np.nan], "finite"),
                      ([np.inf], "finite")):
        with pytest.raises(Exception, match=what):
            m.anomalous_transport_mesh([8, 8], bad, 0.1)
        with pytest.raises(Exception, match=what):
            m.drude_weight_mesh([8, 8], bad, 0.1)
    # meshes
    for bad in ([8, 0], [8, 8, 8], [8]):
        with pytest.raises(Exception):
            m.anomalous_transport_mesh(bad, lv, 0.1)
        with pytest.raises(Exception):
            m.drude_weight_mesh(bad, lv, 0.1)
    with pytest.raises(Exception):
        chain.drude_weight_mesh([8, 8], lv, 0.1)
    # cartesian
    for bad in (1, "yes", None, [True]):
        with pytest.raises(Exception, match="cartesian"):
            m.drude_weight_mesh([8, 8], lv, 0.1, cartesian=bad)


# ---------------------------------------------------------------- GPU
VEL_MODELS = dict(CURV_MODELS)
VEL_MODELS["strained_kane_mele_3x3"] = (lambda: supercell(strained_kane_mele(), 3), None)      # 36 states, Kramers pairs


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(VEL_MODELS))
def test_band_velocity_on_random_k(name):
    """64 seeded k against the restatement, to 1e-9 max|v|.  Entries next to a gap below GAP_MIN are dropped (inside a group, and
    next to one, the raw diagonal element depends on the solver's basis); at most 10 % may be.  By the restatement's eigenvalues alone
    this seed drops 1.0 % (haldane_3x3), 1.6 % (haldane_4x4), 3.8 % (haldane_6x6), 0.9 % (strained_kane_mele_3x3) and nothing for the
    other models."""
    m = VEL_MODELS[name][0]()
    dk = m._dim_k
    k = np.random.default_rng(1).random((64, dk))
    ok = sr.band_gaps(m, k) >= GAP_MIN
    print(name, "dropped", 1.0 - ok.mean())
    assert ok.sum() >= 0.9 * ok.size, (name, ok.sum())
    want = tr.band_terms(m, k)[1]
    got = m.band_velocity(k)
    assert got.shape == want.shape == (dk, m._nsta, 64)
    scale = np.max(np.abs(want))
    print(name, np.max(np.abs(got - want)[:, ok]) / scale)
    close(got[:, ok], want[:, ok], scale)
    for d in range(dk):
        one = m.band_velocity(k, dirs=d)
        assert one.shape == (m._nsta, 64)
        np.testing.assert_array_equal(one, got[d])
    assert m.band_velocity(np.zeros((0, dk))).shape == (dk, m._nsta, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["haldane", "cubic16"])
def test_band_velocity_against_eigenvalue_differences(name):
    """Hellmann-Feynman: central differences (h = 1e-5) of solve_all's eigenvalues, with the same filter.  The tolerance is 10 x the
    difference between the restatement's velocity and the same differences of numpy.linalg.eigvalsh."""
    m = VEL_MODELS[name][0]()
    dk, h = m._dim_k, 1e-5
    k = np.random.default_rng(1).random((64, dk))
    ok = sr.band_gaps(m, k) >= GAP_MIN
    assert ok.sum() >= 0.9 * ok.size
    ref = tr.band_terms(m, k)[1]
    got = m.band_velocity(k)
    for d in range(dk):
        e = np.zeros(dk)
        e[d] = h
        fd_ref = (np.linalg.eigvalsh(orc.ham_batch(m, k + e)) - np.linalg.eigvalsh(orc.ham_batch(m, k - e))).T / (2.0 * h)
        fd_dev = (m.solve_all(k + e) - m.solve_all(k - e)) / (2.0 * h)
        ref_err = np.max(np.abs(ref[d] - fd_ref)[ok])
        err = np.max(np.abs(got[d] - fd_dev)[ok])
        print(name, d, err, ref_err)
        assert err <= 10.0 * ref_err


def mesh_levels(m):
    e = np.linalg.eigvalsh(orc.ham_batch(m, m.k_uniform_mesh([4] * m._dim_k)))
    return np.linspace(e.min() - 0.2, e.max() + 0.2, 6)


MESH_MODELS = {
    "haldane": (haldane, [48, 40]),
    "strained_haldane": (lambda: strained(True), [48, 40]),
    "strained_kane_mele": (strained_kane_mele, [24, 24]),
    "strained_doubled": (lambda: strained(nspin=2), [24, 24]),
    "cubic16": (lambda: hp.cubic16(tb.tb_model), [8, 6, 5]),
    "strained_kane_mele_3x3": (lambda: supercell(strained_kane_mele(), 3), [6, 6]),
    "haldane_6x6": (CURV_MODELS["haldane_6x6"][0], [5, 4]),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MESH_MODELS))
def test_mesh_forms_against_numpy(name):
    make, mesh = MESH_MODELS[name]
    m = make()
    dk = m._dim_k
    lv = mesh_levels(m)
    for dirs in ([(0, 1), (2, 0)] if dk == 3 else [(0, 1)]):
        want = tr.transport(m, mesh, lv, KT, dirs)
        got = m.anomalous_transport_mesh(mesh, lv, KT, dirs=dirs)
        tail = () if dk == 2 else (mesh[3 - dirs[0] - dirs[1]],)
        assert [g.shape for g in got] == [(6,) + tail, (6,) + tail, (dk, 6) + tail]
        for g, w, s, what in zip(got, want[:3], want[3], ("hall", "nernst", "dipole")):
            print(name, dirs, what, np.max(np.abs(g - w)), s)
            close(g, w, s)
    want, s = tr.drude(m, mesh, lv, KT)
    got = m.drude_weight_mesh(mesh, lv, KT)
    assert got.shape == (6, dk, dk)
    print(name, "drude", np.max(np.abs(got - want)), s)
    close(got, want, s)
    np.testing.assert_array_equal(got, np.transpose(got, (0, 2, 1)))
    assert np.all(got[:, np.arange(dk), np.arange(dk)] >= 0.0)
    a = np.array(m._lat, dtype=float)[m._per]
    cart = m.drude_weight_mesh(mesh, lv, KT, cartesian=True)
    assert cart.shape == (6, m._dim_r, m._dim_r)
    close(cart, np.einsum("ia,wij,jb->wab", a, want, a) / ((2.0 * np.pi) ** 2 * np.sqrt(np.linalg.det(a @ a.T))),
          s * np.max(np.abs(a)) ** 2 / ((2.0 * np.pi) ** 2 * np.sqrt(np.linalg.det(a @ a.T))))


@pytest.mark.gpu
def test_drude_weight_of_a_chain():
    m = hp.chain3(tb.tb_model, -1.0, 0.5, 0.1)
    lv = mesh_levels(m)
    want, s = tr.drude(m, [64], lv, KT)
    got = m.drude_weight_mesh([64], lv, KT)
    assert got.shape == (6, 1, 1)
    close(got, want, s)
    one = quiet(tb.tb_model, 1, 1, [[1.0]], [[0.0]])          # one band: E = 2 t cos 2 pi k
    one.set_hop(-1.0, 0, 0, [1])
    want, s = tr.drude(one, [64], [0.0, 1.0], KT)
    close(one.drude_weight_mesh([64], [0.0, 1.0], KT), want, s)


@pytest.mark.gpu
def test_shapes_and_orders_of_the_levels():
    m = strained(True)
    mesh = [16, 16]
    many = np.linspace(-3.5, 3.5, 8192)
    base = m.anomalous_transport_mesh(mesh, many, KT)
    base_d = m.drude_weight_mesh(mesh, many, KT)
    assert [b.shape for b in base] == [(8192,), (8192,), (2, 8192)] and base_d.shape == (8192, 2, 2)
    want = tr.transport(m, mesh, many[::512], KT)
    for g, w, s in zip(base, want[:3], want[3]):
        close(g[..., ::512], w, s)
    wd, s = tr.drude(m, mesh, many[::512], KT)
    close(base_d[::512], wd, s)
    pick = np.concatenate([np.random.default_rng(3).permutation(8192)[:300], [17, 17, 4000]])     # unsorted, with repeats
    for idx in (pick, pick[:1]):
        got = m.anomalous_transport_mesh(mesh, many[idx], KT)
        assert [g.shape for g in got] == [(len(idx),), (len(idx),), (2, len(idx))]
        for g, b in zip(got, base):
            np.testing.assert_array_equal(g, b[..., idx])
        np.testing.assert_array_equal(m.drude_weight_mesh(mesh, many[idx], KT), base_d[idx])


@pytest.mark.gpu
def test_cold_limit_is_the_t0_hall_integral():
    m = haldane()
    mesh = [64, 64]
    e = m.solve_all_mesh(mesh)
    gap = e[1].min() - e[0].max()
    assert gap > 0.3
    mu = 0.5 * (e[1].min() + e[0].max())
    hall, nernst, dip = m.anomalous_transport_mesh(mesh, [mu], gap / 200.0)
    t0 = m.berry_curvature_mesh(mesh, fermi_levels=[mu])
    print(hall, t0, nernst, dip)
    assert abs(t0[0]) > 6.0
    assert abs(hall[0] - t0[0]) <= 1e-12 * abs(t0[0])
    assert abs(nernst[0]) <= 1e-12 * abs(t0[0]) and np.max(np.abs(dip)) <= 1e-12 * abs(t0[0])
    assert np.max(np.abs(m.drude_weight_mesh(mesh, [mu], gap / 200.0))) <= 1e-12 * abs(t0[0])


@pytest.mark.gpu
def test_chunks_of_a_32_state_mesh_and_repeats():
    """16 spinful orbitals on 48^2 = 2304 points: two chunks (32 MiB of 32 x 32 eigenvectors = 2048 points)."""
    m = hp.random_model(tb.tb_model, 16, 2, 2, 34)
    mesh = [48, 48]
    assert (32 << 20) // (32 * 32 * 16) == 2048 < mesh[0] * mesh[1]
    lv = mesh_levels(m)
    want = tr.transport(m, mesh, lv, KT)
    got = m.anomalous_transport_mesh(mesh, lv, KT)
    for g, w, s in zip(got, want[:3], want[3]):
        close(g, w, s)
    wd, s = tr.drude(m, mesh, lv, KT)
    gd = m.drude_weight_mesh(mesh, lv, KT)
    close(gd, wd, s)
    for g, a in zip(got, m.anomalous_transport_mesh(mesh, lv, KT)):
        np.testing.assert_array_equal(g.view(np.uint64), a.view(np.uint64))
    np.testing.assert_array_equal(gd.view(np.uint64), m.drude_weight_mesh(mesh, lv, KT).view(np.uint64))
    kk = m.k_uniform_mesh(mesh)
    v = m.band_velocity(kk)
    np.testing.assert_array_equal(v.view(np.uint64), m.band_velocity(kk).view(np.uint64))
    wide = supercell(strained_kane_mele(), 3)                 # 36 states: the wide form, with Kramers pairs at k = 0
    wl = mesh_levels(wide)
    for a, b in zip(wide.anomalous_transport_mesh([6, 6], wl, KT), wide.anomalous_transport_mesh([6, 6], wl, KT)):
        np.testing.assert_array_equal(a.view(np.uint64), b.view(np.uint64))
    np.testing.assert_array_equal(wide.drude_weight_mesh([6, 6], wl, KT).view(np.uint64),
                                  wide.drude_weight_mesh([6, 6], wl, KT).view(np.uint64))
