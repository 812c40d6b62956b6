"""Spin Berry curvature and spin Hall conductivity by the Kubo formula (tb_model._gen_jham, spin_berry_curvature,
spin_hall_conductivity_mesh) against the NumPy restatement in spin_curv_ref.py, against the charge curvature of the two spin
sectors of an S_z-conserving model, and against anchors computed with the restatement on 24^2, 48^2 and 96^2 meshes."""
import numpy as np
import pytest

import curv_ref as cr
import helpers as hp
import spin_curv_ref as sr
from helpers import quiet
from oracle import tb_oracle as orc
from test_berry_curvature import spin_doubled_haldane

import pythtb_amd as tb

TWO_PI = 2.0 * np.pi
GAP_MIN = 1e-3            # the threshold of test_berry_curvature.test_curvature_on_random_k
SPINS = [0, 1, 2, [0.6, 0.0, 0.8]]
# mean / 2 pi of the band set [0, 1] on k_uniform_mesh([48, 48]) (restatement; the last three agree on 48^2 and 96^2 to 1e-14)
ANCHORS = [("sz_odd", 2, -2.0, 1e-12), ("sz_even", 2, 0.0, 1e-12), ("odd", 2, -2.054316152716, 1e-10),
           ("odd", 0, -0.105159351316, 1e-10), ("even", 2, -0.00106443922711, 1e-10)]


def close(got, want, scale, rel=1e-9):
    err = np.max(np.abs(np.asarray(got) - np.asarray(want)))
    assert err <= rel * scale, (err, scale)


def safe_levels(e, targets):
    """For each target, the midpoint of the two mesh levels around it (or 1 below / above the spectrum)."""
    s = np.unique(e.ravel())
    out = []
    for t in targets:
        j = int(np.searchsorted(s, t))
        out.append(s[0] - 1.0 if j == 0 else (s[-1] + 1.0 if j == len(s) else 0.5 * (s[j - 1] + s[j])))
    return np.array(out)


def kane_mele_sz(topological="odd", sector=None):
    """helpers.kane_mele without its Rashba lines: amplitudes of 1 and sigma_z only, so S_z is conserved.  sector = +1 / -1:
    the nspin = 1 model of the spin-up / spin-down diagonal entries."""
    esite = 2.5 if topological == "even" else 1.0
    so = 0.6 * 0.5
    if sector is None:
        m = quiet(tb.tb_model, 2, 2, hp.LAT, hp.ORB, nspin=2)
        sz = np.array([0.0, 0.0, 0.0, 1.0])
    else:
        m = quiet(tb.tb_model, 2, 2, hp.LAT, hp.ORB)
        sz = float(sector)
    m.set_onsite([esite, -esite])
    for R in ([0, 0], [0, -1], [-1, 0]):
        m.set_hop(1.0, 0, 1, R)
    for sign, i, R in [(-1, 0, [0, 1]), (1, 0, [1, 0]), (-1, 0, [1, -1]), (1, 1, [0, 1]), (-1, 1, [1, 0]), (1, 1, [1, -1])]:
        m.set_hop(sign * 1.0j * so * sz, i, i, R)
    return m


def anchor_model(name):
    return kane_mele_sz(name[3:]) if name.startswith("sz_") else hp.kane_mele(tb.tb_model, name)


def one_orbital():
    """One spinful orbital: two states, served by k_kubo_lds with 64 points per workgroup (the n = 2 closed form of the charge
    curvature is for two velocities and must not be taken)."""
    m = quiet(tb.tb_model, 2, 2, hp.LAT, [[0.0, 0.0]], nspin=2)
    m.set_onsite([[0.1, 0.3, -0.2, 0.5]])
    m.set_hop([0.7, 0.2, 0.1j, -0.3], 0, 0, [1, 0])
    m.set_hop(np.array([[0.3, 0.5 - 0.2j], [0.1j, -0.4]]), 0, 0, [0, 1])
    m.set_hop([0.1j, -0.2, 0.3, 0.25j], 0, 0, [1, 1])
    return m


def supercell(m, s):
    return quiet(m.make_supercell, [[s, 0], [0, s]])


def stacked_kane_mele(tz=0.1):
    """Kane-Mele layers (helpers.kane_mele, "odd") along a third axis with a weak interlayer hop."""
    lat = [[1.0, 0.0, 0.0], [0.5, np.sqrt(3.0) / 2.0, 0.0], [0.0, 0.0, 1.0]]
    orb = [[1.0 / 3.0, 1.0 / 3.0, 0.0], [2.0 / 3.0, 2.0 / 3.0, 0.0]]
    m = quiet(tb.tb_model, 3, 3, lat, orb, nspin=2)
    so, ra, r3h = 0.3, 0.25, np.sqrt(3.0) / 2.0
    sx, sy, sz = np.array([0.0, 1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0, 0.0]), np.array([0.0, 0.0, 0.0, 1.0])
    m.set_onsite([1.0, -1.0])
    for R in ([0, 0, 0], [0, -1, 0], [-1, 0, 0]):
        m.set_hop(1.0, 0, 1, R)
    for sign, i, R in [(-1, 0, [0, 1, 0]), (1, 0, [1, 0, 0]), (-1, 0, [1, -1, 0]), (1, 1, [0, 1, 0]), (-1, 1, [1, 0, 0]),
                       (1, 1, [1, -1, 0])]:
        m.set_hop(sign * 1.0j * so * sz, i, i, R)
    m.set_hop(1.0j * ra * (0.5 * sx - r3h * sy), 0, 1, [0, 0, 0], mode="add")
    m.set_hop(1.0j * ra * (-1.0 * sx), 0, 1, [0, -1, 0], mode="add")
    m.set_hop(1.0j * ra * (0.5 * sx + r3h * sy), 0, 1, [-1, 0, 0], mode="add")
    m.set_hop(tz, 0, 0, [0, 0, 1])
    m.set_hop(0.5 * tz * np.array([1.0, 0.0, 0.0, 0.3]), 1, 1, [0, 0, 1])
    return m


# ---------------------------------------------------------------- CPU: argument errors, anchors and identities of the restatement
def test_argument_errors_without_gpu():
    m = hp.kane_mele(tb.tb_model)
    k = [[0.1, 0.2]]
    for plain in (hp.haldane(tb.tb_model, delta=0.2), hp.chain3(tb.tb_model, -1.0, 0.5, 0.1)):
        kp = [[0.1] * plain._dim_k]
        with pytest.raises(Exception, match="nspin = 2"):
            plain.spin_berry_curvature(kp)
        with pytest.raises(Exception, match="nspin = 2"):
            plain.spin_hall_conductivity_mesh([8] * plain._dim_k)
        with pytest.raises(Exception, match="nspin = 2"):
            plain._gen_jham(kp[0], 0, 2)
    for bad in (3, -1, [1, 0], [0, 0, np.nan], "z", [0.0, 1.0, np.inf], [[0, 0, 1]], 1.0, [1j, 0, 0]):
        with pytest.raises(Exception, match="spin"):
            m.spin_berry_curvature(k, bad)
        with pytest.raises(Exception, match="spin"):
            m.spin_hall_conductivity_mesh([8, 8], spin=bad)
        with pytest.raises(Exception, match="spin"):
            m._gen_jham(k[0], 0, bad)
    chain = quiet(tb.tb_model, 1, 1, [[1.0]], [[0.0]], nspin=2)
    chain.set_hop([0.5, 0.1, 0.0, 0.2], 0, 0, [1])
    with pytest.raises(Exception, match="dim_k >= 2"):
        chain.spin_berry_curvature([[0.1]])
    with pytest.raises(Exception, match="dim_k >= 2"):
        chain.spin_hall_conductivity_mesh([8])
    for bad in [(0, 0), (1, 1), (0, 2), (-1, 0), (0,)]:
        with pytest.raises(Exception):
            m.spin_berry_curvature(k, dirs=bad)
        with pytest.raises(Exception):
            m.spin_hall_conductivity_mesh([8, 8], dirs=bad)
    with pytest.raises(IndexError):
        m.spin_berry_curvature(k, occ=[4])
    with pytest.raises(IndexError):
        m.spin_hall_conductivity_mesh([8, 8], occ=[-5])
    with pytest.raises(Exception, match="twice"):
        m.spin_berry_curvature(k, occ=[0, -4])
    with pytest.raises(Exception, match="not both"):
        m.spin_hall_conductivity_mesh([8, 8], occ=[0], fermi_levels=[0.0])
    with pytest.raises(Exception, match="1-D"):
        m.spin_hall_conductivity_mesh([8, 8], fermi_levels=[[0.0, 1.0]])
    with pytest.raises(Exception, match="1-D"):
        m.spin_hall_conductivity_mesh([8, 8], fermi_levels=np.zeros(8193))
    with pytest.raises(Exception, match="finite"):
        m.spin_hall_conductivity_mesh([8, 8], fermi_levels=[0.0, np.nan])
    with pytest.raises(Exception):
        m.spin_hall_conductivity_mesh([8, 0])
    with pytest.raises(Exception):
        m.spin_hall_conductivity_mesh([8, 8, 8])
    with pytest.raises(Exception, match="wrong shape"):
        m.spin_berry_curvature([[0.1, 0.2, 0.3]])
    with pytest.raises(Exception):
        m._gen_jham([0.1, 0.2], 2)
    with pytest.raises(Exception, match="wrong shape"):
        m._gen_jham([0.1, 0.2, 0.3], 0)


@pytest.mark.parametrize("name,spin,want,tol", ANCHORS)
def test_reference_anchors(name, spin, want, tol):
    m = anchor_model(name)
    assert hasattr(m, "spin_berry_curvature")             # (the restatement alone does not need the feature)
    kk = m.k_uniform_mesh([48, 48])
    assert cr.smallest_gap(m, kk, occ=[0, 1]).min() >= 0.86
    got = sr.spin_curvature(m, kk, spin, occ=[0, 1]).mean() / TWO_PI
    assert abs(got - want) <= tol, got


def test_identities_of_the_restatement():
    m = hp.kane_mele(tb.tb_model)
    assert hasattr(m, "spin_hall_conductivity_mesh")
    k = np.random.default_rng(2).random((50, 2))
    for occ in (None, [0, 1]):
        np.testing.assert_array_equal(sr.spin_curvature(m, k, None, occ=occ), cr.curvature(m, k, occ=occ))
    x, z = sr.spin_curvature(m, k, 0), sr.spin_curvature(m, k, 2)
    mix = sr.spin_curvature(m, k, [0.6, 0.0, 0.8])
    scale = max(np.max(np.abs(x)), np.max(np.abs(z)))
    close(mix, 0.6 * x + 0.8 * z, scale, rel=1e-12)
    for spin in SPINS:
        per = sr.spin_curvature(m, k, spin)
        man = sr.spin_curvature(m, k, spin, occ=[0, 1])
        close(per[0] + per[1], man, np.max(np.abs(per)), rel=1e-12)
        close(sr.spin_curvature(m, -k, spin, occ=[0, 1]), man, np.max(np.abs(per)), rel=1e-12)
        close(sr.spin_curvature(m, -k, spin), per, np.max(np.abs(per)), rel=1e-12)


# ---------------------------------------------------------------- GPU
SPIN_MODELS = {
    "one_orbital": (one_orbital, [0]),
    "kane_mele": (lambda: hp.kane_mele(tb.tb_model), [0, 1]),
    "random_3": (lambda: hp.random_model(tb.tb_model, 3, 2, 2, 31), [0, 1, 2]),
    "random_4": (lambda: hp.random_model(tb.tb_model, 4, 2, 2, 32), [0, 1, 2, 3]),
    "random_8": (lambda: hp.random_model(tb.tb_model, 8, 2, 2, 33), list(range(8))),
    "random_16": (lambda: hp.random_model(tb.tb_model, 16, 2, 2, 34), list(range(16))),
    "kane_mele_3x3": (lambda: supercell(hp.kane_mele(tb.tb_model), 3), list(range(18))),
    "kane_mele_4x4": (lambda: supercell(hp.kane_mele(tb.tb_model), 4), list(range(32))),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SPIN_MODELS))
def test_spin_curvature_on_random_k(name):
    """Per band and band set at 64 seeded k.  A band set keeps the points whose gap across the set passes GAP_MIN.  Per band the
    same threshold acts on (k, band) entries -- a band is dropped where one of its own two neighbouring gaps is below it -- and
    not on whole points: the folded bands of the 36- and 64-state supercells come closer than 1e-3 somewhere at 11 and 33 of the
    64 points (by the restatement's eigenvalues alone), while only 1.1 % and 2.6 % of their entries sit next to such a gap.  At
    most 10 % of the entries (of the points, for a band set) may be dropped; for the models up to 32 states nothing is."""
    make, occ = SPIN_MODELS[name]
    m = make()
    k = np.random.default_rng(1).random((64, 2))
    assert np.array_equal(sr.band_gaps(m, k).min(axis=0), cr.smallest_gap(m, k))
    for o in (None, occ):
        ok = sr.band_gaps(m, k) >= GAP_MIN if o is None else cr.smallest_gap(m, k, occ=o) >= GAP_MIN
        assert ok.sum() >= 0.9 * ok.size, (name, o, ok.sum())
        for spin in SPINS:
            for dirs in [(0, 1), (1, 0)]:
                got = m.spin_berry_curvature(k, spin, occ=o, dirs=dirs)
                want = sr.spin_curvature(m, k, spin, dirs=dirs, occ=o)
                assert got.shape == want.shape == ok.shape
                g, w = got[ok], want[ok]
                print(name, o is not None, spin, dirs, np.max(np.abs(g - w)) / np.max(np.abs(w)))
                close(g, w, np.max(np.abs(w)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one_orbital", "kane_mele", "random_8", "kane_mele_3x3"])
def test_gen_jham(name):
    m = SPIN_MODELS[name][0]()
    rng = np.random.default_rng(1)
    n = m._nsta
    for _ in range(4):
        k = rng.random(2) * 2.0 - 0.5
        for d in range(2):
            for spin in SPINS:
                got = np.asarray(m._gen_jham(k, d, spin))
                assert got.shape == (m._norb, 2, m._norb, 2)
                want = sr.jham_batch(m, k[None, :], d, spin)[0]
                close(got.reshape(n, n), want, np.max(np.abs(cr.dham_batch(m, k[None, :], d))), rel=1e-13)


@pytest.mark.gpu
@pytest.mark.parametrize("topological", ["odd", "even"])
def test_sz_conserving_model_against_the_charge_curvature(topological):
    m, up, dn = kane_mele_sz(topological), kane_mele_sz(topological, +1), kane_mele_sz(topological, -1)
    k = np.random.default_rng(1).random((64, 2))
    cu, cd_ = up.berry_curvature(k, occ=[0]), dn.berry_curvature(k, occ=[0])
    got = m.spin_berry_curvature(k, 2, occ=[0, 1])
    close(got, cu - cd_, max(np.max(np.abs(cu)), np.max(np.abs(cd_))))
    close(m.berry_curvature(k, occ=[0, 1]), cu + cd_, max(np.max(np.abs(cu)), np.max(np.abs(cd_))))


@pytest.mark.gpu
def test_degenerate_pairs_spin_doubled():
    h, d = hp.haldane(tb.tb_model, delta=0.2), spin_doubled_haldane()
    mesh = [48, 48]
    charge = d.berry_curvature_mesh(mesh, occ=[0, 1])
    assert abs(charge - 2.0 * h.berry_curvature_mesh(mesh, occ=[0])) <= 1e-9 * abs(charge)
    assert abs(charge / TWO_PI + 2.0) < 1e-6
    assert abs(d.spin_hall_conductivity_mesh(mesh, 2, occ=[0, 1])) <= 1e-9 * abs(charge)
    k = np.random.default_rng(5).random((64, 2))
    scale = np.max(np.abs(h.berry_curvature(k)))
    for spin in SPINS:
        got = d.spin_berry_curvature(k, spin)
        want = sr.spin_curvature(d, k, spin)
        for pair in ([0, 1], [2, 3]):                      # (inside a degenerate pair the split is the solver's choice of basis)
            close(got[pair].sum(axis=0), want[pair].sum(axis=0), scale)
            close(got[pair].sum(axis=0), 0.0, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("mesh", [[48, 48], [512, 512]])
def test_mesh_anchors(mesh):
    for name, spin, want, tol in ANCHORS:
        got = anchor_model(name).spin_hall_conductivity_mesh(mesh, spin, occ=[0, 1]) / TWO_PI
        print(name, spin, mesh, got, got - want)
        assert isinstance(got, float)
        assert abs(got - want) <= tol, (name, spin, got)


@pytest.mark.gpu
def test_mesh_per_band_means():
    m = hp.random_model(tb.tb_model, 3, 2, 2, 31)
    mesh = [24, 20]
    kk = m.k_uniform_mesh(mesh)
    assert cr.smallest_gap(m, kk).min() >= GAP_MIN
    for spin in SPINS:
        for dirs in [(0, 1), (1, 0)]:
            want = sr.spin_curvature(m, kk, spin, dirs=dirs)
            got = m.spin_hall_conductivity_mesh(mesh, spin, dirs=dirs)
            assert got.shape == (6,)
            close(got, want.mean(axis=1), np.max(np.abs(want)))


@pytest.mark.gpu
def test_fermi_scan_kane_mele():
    m = hp.kane_mele(tb.tb_model)
    mesh = [64, 64]
    kk = m.k_uniform_mesh(mesh)
    e = m.solve_all_mesh(mesh)
    ref_e = np.linalg.eigvalsh(orc.ham_batch(m, kk))
    levels = safe_levels(np.concatenate([e.ravel(), ref_e.ravel()]), np.linspace(e.min() - 0.1, e.max() + 0.1, 64))
    for spin in (2, [0.6, 0.0, 0.8]):
        got = m.spin_hall_conductivity_mesh(mesh, spin, fermi_levels=levels)
        want = sr.fermi_scan(m, kk, levels, spin)
        assert got.shape == (64,)
        assert got[0] == 0.0
        close(got, want, np.max(np.abs(want)))
        gap = 0.5 * (e[1].max() + e[2].min())
        close(m.spin_hall_conductivity_mesh(mesh, spin, fermi_levels=[gap])[0],
              m.spin_hall_conductivity_mesh(mesh, spin, occ=[0, 1]), np.max(np.abs(want)))
        shuffled = np.concatenate([levels[np.random.default_rng(3).permutation(64)], levels[5:6]])
        again = m.spin_hall_conductivity_mesh(mesh, spin, fermi_levels=shuffled)
        np.testing.assert_array_equal(again, got[[int(np.flatnonzero(levels == x)[0]) for x in shuffled]])


@pytest.mark.gpu
def test_slices_of_a_3d_mesh():
    m = stacked_kane_mele()
    mesh = [12, 10, 6]
    kk = m.k_uniform_mesh(mesh)
    assert cr.smallest_gap(m, kk, occ=[0, 1]).min() >= GAP_MIN
    for dirs in [(0, 1), (2, 0), (1, 2)]:
        other = 3 - dirs[0] - dirs[1]
        axes = tuple(a for a in range(3) if a != other)
        for spin in (2, [0.6, 0.0, 0.8]):
            want = sr.spin_curvature(m, kk, spin, dirs=dirs, occ=[0, 1])
            got = m.spin_hall_conductivity_mesh(mesh, spin, occ=[0, 1], dirs=dirs)
            assert got.shape == (mesh[other],)
            close(got, want.reshape(mesh).mean(axis=axes), np.max(np.abs(want)))
    per = m.spin_hall_conductivity_mesh(mesh, 2, dirs=(2, 0))
    assert per.shape == (4, 10)
    scan = m.spin_hall_conductivity_mesh(mesh, 2, fermi_levels=[-10.0, 0.0, 10.0], dirs=(1, 2))
    assert scan.shape == (3, 12)
    assert np.all(scan[0] == 0.0)


@pytest.mark.gpu
def test_chunks_of_a_32_state_mesh_and_repeats():
    """16 spinful orbitals on 48^2 = 2304 points: two chunks of the LDS path (32 MiB of 32 x 32 eigenvectors = 2048 points)."""
    m = hp.random_model(tb.tb_model, 16, 2, 2, 34)
    mesh = [48, 48]
    assert (32 << 20) // (32 * 32 * 16) == 2048 < mesh[0] * mesh[1]
    kk = m.k_uniform_mesh(mesh)
    occ = list(range(16))
    lst = m.spin_berry_curvature(kk, 2)
    msh = m.spin_hall_conductivity_mesh(mesh, 2)
    scale = max(1.0, np.max(np.abs(lst)))
    close(msh, lst.mean(axis=1), scale, rel=1e-12)
    man = m.spin_berry_curvature(kk, 2, occ=occ)
    close(m.spin_hall_conductivity_mesh(mesh, 2, occ=occ), man.mean(), max(1.0, np.max(np.abs(man))), rel=1e-12)
    # points of the second chunk against the NumPy form: the chunk offset of the list form is right on its own
    pick = 2048 + np.random.default_rng(11).choice(len(kk) - 2048, 32, replace=False)
    ok = cr.smallest_gap(m, kk[pick]) >= GAP_MIN
    assert ok.sum() >= 0.9 * len(pick)
    ref = sr.spin_curvature(m, kk[pick], 2)
    close(lst[:, pick][:, ok], ref[:, ok], np.max(np.abs(ref[:, ok])))
    np.testing.assert_array_equal(lst.view(np.uint64), m.spin_berry_curvature(kk, 2).view(np.uint64))
    np.testing.assert_array_equal(msh.view(np.uint64), m.spin_hall_conductivity_mesh(mesh, 2).view(np.uint64))
    wide = supercell(hp.kane_mele(tb.tb_model), 3)                     # 36 states: the wide path
    wmesh, wocc = [8, 8], list(range(18))
    wk = wide.k_uniform_mesh(wmesh)
    spin = [0.6, 0.0, 0.8]
    for o in (None, wocc):
        a, b = wide.spin_berry_curvature(wk, spin, occ=o), wide.spin_berry_curvature(wk, spin, occ=o)
        np.testing.assert_array_equal(a.view(np.uint64), b.view(np.uint64))
        c = np.atleast_1d(wide.spin_hall_conductivity_mesh(wmesh, spin, occ=o))
        d = np.atleast_1d(wide.spin_hall_conductivity_mesh(wmesh, spin, occ=o))
        np.testing.assert_array_equal(c.view(np.uint64), d.view(np.uint64))
        close(c, a.reshape(-1, len(wk)).mean(axis=1), max(1.0, np.max(np.abs(a))), rel=1e-12)
