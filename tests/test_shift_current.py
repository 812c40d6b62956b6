"""Shift and injection photocurrents (tb_model._gen_ddham, shift_current, shift_current_mesh, injection_current_mesh) against the
NumPy restatement in shift_ref.py; the restatement itself against finite differences in a parallel-transport gauge, against random
rotations inside degenerate groups and against the symmetry rules of the two tensors."""
import numpy as np
import pytest

import curv_ref as cr
import helpers as hp
import shift_ref as sh
from helpers import quiet
from oracle import tb_oracle as orc
from test_transport import strained, strained_kane_mele

import pythtb_amd as tb

GAP_MIN = 1e-3            # the smallest gap between levels of different groups that a device comparison accepts
REL = 1e-9                # of the scale: the tolerance of every Kubo test here
OMEGA = np.array([0.0, 0.7, 1.9, 2.6, -1.9, 4.2])
ETA = 0.08


def close(got, want, scale, rel=REL, what=""):
    err = np.max(np.abs(np.asarray(got) - np.asarray(want)))
    print("%s err %.3e scale %.3e ratio %.3e" % (what, err, scale, err / scale if scale else 0.0))
    assert err <= rel * scale, (what, err, scale)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---------------------------------------------------------------- CPU: the restatement alone, and argument errors
def fd_models():
    for n in range(2, 9):
        yield hp.random_model(tb.tb_model, n, 1 + n % 3, 1, 100 + n)
    yield hp.random_model(tb.tb_model, 3, 2, 2, 77)            # spinful, six states


def test_numpy_ddham_matches_central_differences_of_dham():
    """d_d d_e H of shift_ref.ddham_batch against central differences of curv_ref.dham_batch along e; the tolerance is 10 x the
    finite-difference error the test measures itself by halving h."""
    rng = np.random.default_rng(5)
    for m in fd_models():
        dk = m._dim_k
        kk = rng.random((5, dk))
        for d in range(dk):
            for e in range(dk):
                def fd(h):
                    s = np.zeros(dk)
                    s[e] = h
                    return (cr.dham_batch(m, kk + s, d) - cr.dham_batch(m, kk - s, d)) / (2.0 * h)
                f1, f2 = fd(1e-4), fd(5e-5)
                est = np.max(np.abs(f1 - f2))
                want = sh.ddham_batch(m, kk, d, e)
                err = np.max(np.abs(want - f1))
                print(m._nsta, d, e, err, est, np.max(np.abs(want)))
                assert est <= 1e-4 * np.max(np.abs(want)) and err <= 10.0 * est     # (the estimate itself is small: h is in range)


def aligned_r(m, u0, kq, b):
    """r^b(kq) = -i V^b / E in the eigenvectors of kq with the phase of each fixed by <u_n(k0)|u_n(kq)> > 0 (parallel transport)."""
    e, u = np.linalg.eigh(orc.ham_batch(m, kq[None])[0])
    ph = np.sum(np.conj(u0) * u, axis=0)
    u = u * np.conj(ph / np.abs(ph))[None, :]
    v = np.conj(u.T) @ cr.dham_batch(m, kq[None], b)[0] @ u
    de = e[:, None] - e[None, :]
    np.fill_diagonal(de, 1.0)
    r = -1j * v / de
    np.fill_diagonal(r, 0.0)
    return r


def test_numpy_sum_rule_matches_finite_differences():
    """The generalized derivative by the sum rule against central differences of r in a parallel-transport gauge (in which the
    diagonal Berry connection vanishes at the centre, so r_;a = d_a r there), 2..8 states in 1 to 3 dimensions, random k.  The
    tolerance is 10 x the finite-difference error the test measures itself by halving h."""
    rng = np.random.default_rng(6)
    for m in fd_models():
        dk = m._dim_k
        for k0 in rng.random((3, dk)):
            pt = sh.Point(m, k0[None])
            assert np.all(pt.gid[0] == np.arange(m._nsta)) and pt.min_gap()[0] > 1e-2
            _, u0 = np.linalg.eigh(orc.ham_batch(m, k0[None])[0])
            for a in range(dk):
                for b in range(dk):
                    def fd(h):
                        s = np.zeros(dk)
                        s[a] = h
                        return (aligned_r(m, u0, k0 + s, b) - aligned_r(m, u0, k0 - s, b)) / (2.0 * h)
                    f1, f2 = fd(1e-5), fd(5e-6)
                    want = pt.r_deriv(b, a)[0]
                    est = np.max(np.abs(f1 - f2))
                    err = np.max(np.abs(want - f1))
                    print(m._nsta, dk, a, b, err, est, np.max(np.abs(want)))
                    assert est <= 1e-3 * np.max(np.abs(want)) and err <= 10.0 * est       # (the estimate itself is small: h is in range)


def test_numpy_group_rule_is_basis_independent():
    """A spin-doubled model is degenerate at every k.  Random unitaries inside every group leave K and N unchanged to 1e-12 of the
    scale, and both are twice the spinless model's.  With Kramers pairs (strained Kane-Mele) the group form is as steady, while T^{ba} in the
    diagonal-element form moves with the rotation."""
    mesh = [12, 12]
    one, dbl = strained(True), strained(True, nspin=2)
    for kind in (0, 1):
        base, sc, _ = sh.mesh_response(one, mesh, OMEGA, ETA, kind=kind)
        plain, sc2, _ = sh.mesh_response(dbl, mesh, OMEGA, ETA, kind=kind)
        turned, _, _ = sh.mesh_response(dbl, mesh, OMEGA, ETA, kind=kind, rng=np.random.default_rng(3))
        assert sc > 0.1
        close(plain, 2.0 * base, sc, rel=1e-12, what="doubled kind %d" % kind)
        close(turned, plain, sc2, rel=1e-12, what="rotated kind %d" % kind)
    # Kramers pairs at the four time-reversal-invariant points of the mesh: their velocity blocks are not multiples of the identity
    km, comps = strained_kane_mele(), [(0, 0, 0), (1, 0, 1)]
    for kind in (0, 1):
        plain, sc, _ = sh.mesh_response(km, [6, 6], OMEGA, ETA, kind=kind)
        turned, _, _ = sh.mesh_response(km, [6, 6], OMEGA, ETA, kind=kind, rng=np.random.default_rng(4))
        close(turned, plain, sc, rel=1e-12, what="Kramers kind %d" % kind)
    a, sc, _ = sh.mesh_response(km, [6, 6], OMEGA, ETA, comps=comps, grouped=False)
    b, _, _ = sh.mesh_response(km, [6, 6], OMEGA, ETA, comps=comps, grouped=False, rng=np.random.default_rng(4))
    print("diagonal form moves by", np.max(np.abs(a - b)), "of", sc)
    assert np.max(np.abs(a - b)) > 1e-3 * sc


def test_numpy_symmetries():
    """Inversion (Haldane, delta = 0) gives no K and no N; gapped graphene (C3v) obeys sigma^{yyy} = -sigma^{yxx} = -sigma^{xxy},
    sigma^{xxx} = 0 through the Cartesian transform; K_abc = K_acb, K(-w) = K(w), N_acb = conj N_abc; Re N = 0 with time reversal and
    not without it; Im N = 0 for the C3 models and not for the strained honeycomb."""
    mesh = [24, 24]
    w = np.array([0.9, 1.6, 2.3, -1.6])
    gg, hi, h3, st = hp.graphene(tb.tb_model, 0.5), hp.haldane(tb.tb_model, 0.0), hp.haldane(tb.tb_model, 0.3), strained()
    k_gg, sc, _ = sh.mesh_response(gg, mesh, w, ETA)
    n_gg, scn, _ = sh.mesh_response(gg, mesh, w, ETA, kind=1)
    k_hi, _, _ = sh.mesh_response(hi, mesh, w, ETA)
    n_hi, _, _ = sh.mesh_response(hi, mesh, w, ETA, kind=1)
    n_h3, sc3, _ = sh.mesh_response(h3, mesh, w, ETA, kind=1)
    n_st, scs, _ = sh.mesh_response(st, mesh, w, ETA, kind=1)
    print(np.max(np.abs(k_gg)), sc, np.max(np.abs(k_hi)), np.max(np.abs(n_hi)), np.max(np.abs(n_h3.real)), np.max(np.abs(n_st.imag)))
    assert np.max(np.abs(k_gg)) > 0.1
    assert np.max(np.abs(k_hi)) <= 1e-12 * sc and np.max(np.abs(n_hi)) <= 1e-12 * scn
    s = sh.cartesian(gg, k_gg)
    top = np.max(np.abs(s))
    assert np.max(np.abs(s[:, 0, 0, 0])) <= 1e-12 * top
    assert np.max(np.abs(s[:, 1, 1, 1] + s[:, 1, 0, 0])) <= 1e-12 * top
    assert np.max(np.abs(s[:, 1, 1, 1] + s[:, 0, 0, 1])) <= 1e-12 * top
    assert np.max(np.abs(s[:, 1, 1, 1])) > 0.1 * top
    for m in (gg, h3, st):
        k, sk, _ = sh.mesh_response(m, mesh, w, ETA)
        n, sn, _ = sh.mesh_response(m, mesh, w, ETA, kind=1)
        assert np.max(np.abs(k - np.transpose(k, (0, 1, 3, 2)))) <= 1e-12 * sk
        assert np.max(np.abs(k[1] - k[3])) <= 1e-12 * sk                       # w = 1.6 and -1.6
        assert np.max(np.abs(n - np.conj(np.transpose(n, (0, 1, 3, 2))))) <= 1e-12 * sn
        assert np.max(np.abs(n[1] - n[3])) <= 1e-12 * sn
    assert np.max(np.abs(n_gg.real)) <= 1e-12 * scn and np.max(np.abs(n_st.real)) <= 1e-12 * scs      # time reversal
    assert np.max(np.abs(n_h3.real)) > 1e-3 * sc3                                                        # broken
    assert np.max(np.abs(n_gg.imag)) <= 1e-12 * scn and np.max(np.abs(n_h3.imag)) <= 1e-12 * sc3       # C3
    assert np.max(np.abs(n_st.imag)) > 1e-3 * scs                                                        # low symmetry


def test_argument_errors():
    m = hp.haldane(tb.tb_model, 0.2)
    for call in (m.shift_current_mesh, m.injection_current_mesh):
        for args, kw in ((([8, 8], [1.0], 0.0), {}), (([8, 8], [1.0], -0.1), {}), (([8, 8], [1.0], np.nan), {}),
                         (([8, 8], [], 0.1), {}), (([8, 8], [[1.0]], 0.1), {}), (([8, 8], [np.inf], 0.1), {}),
                         (([8, 8], np.zeros(65537), 0.1), {}), (([8, 8], [1.0], 0.1), dict(kT=-1.0)),
                         (([8, 8], [1.0], 0.1), dict(kT=np.nan)), (([8, 8], [1.0], 0.1), dict(fermi_level=np.inf)),
                         (([8, 8], [1.0], 0.1), dict(dirs=(0, 1))), (([8, 8], [1.0], 0.1), dict(dirs=(0, 1, 2))),
                         (([8, 8], [1.0], 0.1), dict(dirs=(0, -1, 0))), (([8, 8], [1.0], 0.1), dict(dirs=(0, 0.5, 0))),
                         (([8, 8], [1.0], 0.1), dict(dirs=(0, 0, 0), cartesian=True)), (([8], [1.0], 0.1), {}),
                         (([8, 0], [1.0], 0.1), {})):
            with pytest.raises(Exception):
                call(*args, **kw)
    k = np.zeros((3, 2))
    for args in ((k, [0], (0, 1)), (k, [0], (0, 1, 2)), (k, [0], (0, 0, -1)), (k, [0], (0, 0, 1.5)), (k, [], (0, 0, 0)),
                 (k, [0, 0], (0, 0, 0)), (k, [2], (0, 0, 0)), (np.zeros((3, 3)), [0], (0, 0, 0))):
        with pytest.raises(Exception):
            m.shift_current(*args)
    for args in (([0.0, 0.0], 2, 0), ([0.0, 0.0], 0, -1), ([0.0, 0.0], 0.5, 0), ([0.0], 0, 0), ([0.0, 0.0, 0.0], 0, 1)):
        with pytest.raises(Exception):
            m._gen_ddham(*args)
    z = quiet(tb.tb_model, 0, 2, hp.LAT, hp.ORB)
    for call, args in ((z._gen_ddham, ([], 0, 0)), (z.shift_current, ([], [0], (0, 0, 0))),
                       (z.shift_current_mesh, ([], [1.0], 0.1)), (z.injection_current_mesh, ([], [1.0], 0.1))):
        with pytest.raises(Exception):
            call(*args)


# ---------------------------------------------------------------- GPU: against the restatement
def random_states(n, dk, seed):
    return hp.random_model(tb.tb_model, n, dk, 1, seed)


@pytest.mark.gpu
def test_gen_ddham_matches_the_restatement():
    rng = np.random.default_rng(21)
    models = [hp.haldane(tb.tb_model, 0.2), hp.kane_mele(tb.tb_model), hp.chain3(tb.tb_model, -1.3, 0.8, 0.15),
              hp.cubic16(tb.tb_model), random_states(36, 2, 12), hp.random_model(tb.tb_model, 5, 3, 2, 4)]
    for m in models:
        dk = m._dim_k
        for k in rng.random((3, dk)):
            for d in range(dk):
                for e in range(dk):
                    want = sh.ddham_batch(m, k[None], d, e)[0]
                    got = np.asarray(m._gen_ddham(k, d, e)).reshape(m._nsta, m._nsta)
                    assert np.max(np.abs(got - want)) <= 1e-12 * max(np.linalg.norm(want), 1e-300)
        assert m._gen_ddham(np.zeros(dk), 0, 0).shape == ((m._norb, 2, m._norb, 2) if m._nspin == 2 else (m._nsta, m._nsta))


LIST_SEEDS = {2: 31, 3: 32, 4: 33, 8: 34, 16: 35, 32: 36, 36: 37, 72: 38}


@pytest.mark.gpu
@pytest.mark.parametrize("dk", [1, 2, 3])
@pytest.mark.parametrize("n", sorted(LIST_SEEDS))
def test_shift_current_list_matches_the_restatement(n, dk):
    """64 random k, the lower half of the bands and a non-contiguous set; 2..32 states take the LDS kernel, 36 and 72 the wide
    kernels.  Points whose smallest gap (restatement) is below GAP_MIN are dropped, at most 10 % of them."""
    m = random_states(n, dk, LIST_SEEDS[n] + 100 * dk)
    k = np.random.default_rng(n + dk).random((64, dk))
    dirs = [(0, 0, 0), (dk - 1, 0, dk - 1), (0, dk - 1, (dk - 1) // 2)]
    for occ in (list(range(max(1, n // 2))), sorted({0, n // 3, n - 1})[: max(1, n - 1)]):
        for d in dirs:
            want, mag, gap = sh.shift_list(m, k, occ, d)
            keep = gap >= GAP_MIN
            assert keep.sum() >= 0.9 * len(k), (n, dk, gap.min())
            got = m.shift_current(k, occ, d)
            assert got.shape == (64,)
            close(got[keep], want[keep], mag[keep].mean(), what="list n=%d dk=%d occ=%s dirs=%s gap %.2e" % (n, dk, occ[:3], d, gap.min()))


MESH_MODELS = {
    "haldane": (lambda: hp.haldane(tb.tb_model, 0.3), [24, 20]),
    "graphene": (lambda: hp.graphene(tb.tb_model, 0.5), [24, 24]),
    "strained": (lambda: strained(True), [20, 24]),
    "kane_mele": (lambda: hp.kane_mele(tb.tb_model), [12, 12]),
    "strained_kane_mele": (strained_kane_mele, [12, 12]),
    "strained_doubled": (lambda: strained(True, nspin=2), [12, 12]),
    "cubic16": (lambda: hp.cubic16(tb.tb_model), [6, 5, 4]),
    "random36": (lambda: random_states(36, 2, 41), [12, 12]),
    "random72": (lambda: random_states(72, 3, 42), [6, 6, 6]),
    "chain3": (lambda: hp.chain3(tb.tb_model, -1.3, 0.8, 0.15), [96]),
}


def fermi_cases(m):
    """(mu, kT): a level in the widest gap at kT = 0, and a level inside a band at kT > 0."""
    e = np.sort(np.linalg.eigvalsh(orc.ham_batch(m, m.k_uniform_mesh([6] * m._dim_k))), axis=1)
    lo, hi = e.max(axis=0)[:-1], e.min(axis=0)[1:]
    j = int(np.argmax(hi - lo))
    mid = 0.5 * (lo[j] + hi[j]) if hi[j] > lo[j] else float(np.median(e))
    return (float(mid), 0.0), (float(np.median(e[:, e.shape[1] // 2])), 0.07)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("name", sorted(MESH_MODELS))
def test_mesh_calls_match_the_restatement(name, kind):
    """Both mesh calls, the full tensor and single components, a Fermi level in a gap at kT = 0 and one inside a band at kT > 0."""
    make, mesh = MESH_MODELS[name]
    m = make()
    dk = m._dim_k
    e = np.linalg.eigvalsh(orc.ham_batch(m, m.k_uniform_mesh([4] * dk)))
    omega = np.array([0.0, 0.31, 0.55, 0.83, -0.55, 1.2]) * (e.max() - e.min())
    call = m.shift_current_mesh if kind == 0 else m.injection_current_mesh
    for mu, kT in fermi_cases(m):
        want, scale, gap = sh.mesh_response(m, mesh, omega, ETA, mu, kT, kind)
        assert gap >= GAP_MIN, (name, gap)
        assert scale > 0.0
        got = call(mesh, omega, ETA, fermi_level=mu, kT=kT)
        assert got.shape == (len(omega), dk, dk, dk) and got.dtype == (complex if kind else float)
        close(got, want, scale, what="%s kind %d mu %.3f kT %g gap %.2e full" % (name, kind, mu, kT, gap))
        for d in [(0, 0, 0), (dk - 1, 0, dk - 1), (0, dk - 1, 0), (dk - 1, dk - 1, (dk - 1) // 2)]:
            one = call(mesh, omega, ETA, fermi_level=mu, kT=kT, dirs=d)
            assert one.shape == (len(omega),)
            close(one, want[(slice(None),) + d], scale, what="%s kind %d dirs %s" % (name, kind, d))


@pytest.mark.gpu
def test_spin_doubled_model_gives_twice_the_spinless_response():
    mesh = [12, 12]
    one, dbl = strained(True), strained(True, nspin=2)
    for kind, name in ((0, "shift_current_mesh"), (1, "injection_current_mesh")):
        _, scale, _ = sh.mesh_response(one, mesh, OMEGA, ETA, 0.0, 0.0, kind)
        a = getattr(one, name)(mesh, OMEGA, ETA)
        b = getattr(dbl, name)(mesh, OMEGA, ETA)
        close(b, 2.0 * a, 2.0 * scale, what="doubled " + name)


@pytest.mark.gpu
def test_inversion_null_and_c3v_relations_on_the_device():
    mesh = [48, 48]
    w = np.linspace(0.2, 4.0, 9)
    gg, hi = hp.graphene(tb.tb_model, 0.5), hp.haldane(tb.tb_model, 0.0)
    _, scale, _ = sh.mesh_response(gg, mesh, w[:1], ETA, comps=[(0, 0, 0)])
    assert np.max(np.abs(hi.shift_current_mesh(mesh, w, ETA))) <= REL * scale
    assert np.max(np.abs(hi.injection_current_mesh(mesh, w, ETA))) <= REL * scale
    s = gg.shift_current_mesh(mesh, w, ETA, cartesian=True)
    assert s.shape == (9, 2, 2, 2)
    top = np.max(np.abs(s))
    print("graphene: max |K|", np.max(np.abs(gg.shift_current_mesh(mesh, w, ETA))), "max |sigma|", top)
    assert np.max(np.abs(s[:, 1, 1, 1])) > 0.1 * top
    assert np.max(np.abs(s[:, 0, 0, 0])) <= REL * top
    assert np.max(np.abs(s[:, 1, 1, 1] + s[:, 1, 0, 0])) <= REL * top
    assert np.max(np.abs(s[:, 1, 1, 1] + s[:, 0, 0, 1])) <= REL * top
    n = gg.injection_current_mesh(mesh, w, ETA, cartesian=True)
    want = sh.cartesian(gg, gg.injection_current_mesh(mesh, w, ETA), kind=1)
    assert n.shape == (9, 2, 2, 2) and np.max(np.abs(n - want)) <= 1e-14 * max(np.max(np.abs(want)), 1e-300)
    assert np.max(np.abs(s - sh.cartesian(gg, gg.shift_current_mesh(mesh, w, ETA)))) <= 1e-14 * top


@pytest.mark.gpu
def test_exact_zeros():
    one = quiet(tb.tb_model, 1, 1, [[1.0]], [[0.0]])
    one.set_hop(-1.0, 0, 0, [1])
    m = hp.kane_mele(tb.tb_model)
    for call_one, call in ((one.shift_current_mesh, m.shift_current_mesh), (one.injection_current_mesh, m.injection_current_mesh)):
        assert not np.any(call_one([16], OMEGA, ETA))
        assert not np.any(call_one([16], OMEGA, ETA, dirs=(0, 0, 0)))
        for mu in (-50.0, 50.0):
            assert not np.any(call([8, 8], OMEGA, ETA, fermi_level=mu))
    assert not np.any(one.shift_current(np.zeros((4, 1)), [0], (0, 0, 0)))
    assert not np.any(m.shift_current(np.random.default_rng(0).random((4, 2)), [0, 1, 2, 3], (0, 1, 1)))


@pytest.mark.gpu
def test_frequency_edge_cases():
    """1 and 65 536 frequencies (a subset compared with the restatement); unsorted and repeated frequencies give equal bits per
    frequency."""
    m = strained(True)
    mesh = [12, 10]
    many = np.linspace(-1.0, 6.0, 65536)
    pick = np.array([0, 1, 255, 256, 511, 512, 4097, 30000, 65535])
    for kind, call in ((0, m.shift_current_mesh), (1, m.injection_current_mesh)):
        want, scale, _ = sh.mesh_response(m, mesh, many[pick], ETA, 0.1, 0.05, kind)
        big = call(mesh, many, ETA, fermi_level=0.1, kT=0.05)
        assert big.shape == (65536, 2, 2, 2)
        close(big[pick], want, scale, what="65536 kind %d" % kind)
        single = call(mesh, many[30000:30001], ETA, fermi_level=0.1, kT=0.05)
        assert single.shape == (1, 2, 2, 2)
        close(single[0], want[7], scale, what="1 frequency kind %d" % kind)
        # the same number of frequencies (the k-groups depend on it), in another order and with repeats
        perm = np.random.default_rng(1).permutation(1300)
        base = call(mesh, np.concatenate([many[:1300], many[:7]]), ETA, fermi_level=0.1, kT=0.05)
        mixed = call(mesh, np.concatenate([many[:1300][perm], many[:7]]), ETA, fermi_level=0.1, kT=0.05)
        np.testing.assert_array_equal(bits(base[1300:]), bits(base[:7]))
        np.testing.assert_array_equal(bits(mixed[:1300]), bits(base[:1300][perm]))
        np.testing.assert_array_equal(bits(mixed[1300:]), bits(base[:7]))
        one = call(mesh, np.concatenate([many[:1300][perm], many[:7]]), ETA, fermi_level=0.1, kT=0.05, dirs=(1, 0, 1))
        np.testing.assert_array_equal(bits(one[1300:]), bits(one[np.argsort(perm)[:7]]))


@pytest.mark.gpu
def test_a_32_state_mesh_that_spans_two_chunks():
    """2304 points of 32 states: the chunk holds 2048, so the second chunk adds to the first one's partial sums."""
    m = random_states(32, 2, 43)
    mesh = [48, 48]
    w = np.array([0.5, 2.0, 3.5])
    for kind, call in ((0, m.shift_current_mesh), (1, m.injection_current_mesh)):
        want, scale, gap = sh.mesh_response(m, mesh, w, ETA, 0.0, 0.05, kind, comps=[(0, 0, 0), (1, 0, 1), (0, 1, 0)])
        assert gap >= GAP_MIN, gap
        got = call(mesh, w, ETA, kT=0.05)
        for d in [(0, 0, 0), (1, 0, 1), (0, 1, 0)]:
            close(got[(slice(None),) + d], want[(slice(None),) + d], scale, what="two chunks kind %d %s gap %.2e" % (kind, d, gap))


@pytest.mark.gpu
def test_repeated_calls_give_equal_bits():
    k = np.random.default_rng(8).random((64, 2))
    for m, mesh in ((hp.kane_mele(tb.tb_model), [24, 24]), (random_states(16, 3, 44), [6, 6, 6]), (random_states(36, 2, 41), [8, 8])):
        kk = k if m._dim_k == 2 else np.random.default_rng(8).random((64, 3))
        for call in (m.shift_current_mesh, m.injection_current_mesh):
            np.testing.assert_array_equal(bits(call(mesh, OMEGA, ETA, kT=0.05)), bits(call(mesh, OMEGA, ETA, kT=0.05)))
            np.testing.assert_array_equal(bits(call(mesh, OMEGA, ETA, dirs=(1, 0, 1))), bits(call(mesh, OMEGA, ETA, dirs=(1, 0, 1))))
        np.testing.assert_array_equal(bits(m.shift_current(kk, [0, 1], (0, 1, 1))), bits(m.shift_current(kk, [0, 1], (0, 1, 1))))
