"""Surface Green's functions by iterative decimation (tb_model.principal_layer, _gen_layer_blocks, surface_green, surface_spectral,
surface_dos_mesh).  The CPU tests check the NumPy restatement sgf_ref.py against exact facts (slab resolvents,
the closed form of the chain, the k-perpendicular mean of the bulk resolvent) and the argument errors; the GPU tests check the
device against the direct slab inverse and the restatement, to 1e-9 of max|G| (max|A|), and that a point's bits do not depend on
the rest of the call."""
import functools

import numpy as np
import pytest

import helpers as hp
import sgf_ref as sr
from helpers import quiet
from oracle import tb_oracle as orc

import pythtb_amd as tb

TOL = 1e-9          # of max|G| or max|A|: the tolerance of the Kubo features
OMEGA13 = np.array([-2.9, -1.7, -1.05, -0.6, -0.15, 0.0, 0.15, 0.33, 0.8, 1.3, 2.1, 2.75, 3.6])
K7 = np.array([0.03, 0.17, 0.31, 0.465, 0.58, 0.74, 0.92])


def chain1(e=0.3, t=-0.8):
    m = quiet(tb.tb_model, 1, 1, [[1.0]], [[0.0]])
    m.set_onsite([e])
    m.set_hop(t, 0, 0, [1])
    return m


def no_coupling():
    """Two orbitals, hoppings along direction 1 only: cut along direction 0 the layers do not couple (H01 = 0)."""
    m = quiet(tb.tb_model, 2, 2, hp.LAT, hp.ORB)
    m.set_onsite([-0.3, 0.4])
    m.set_hop(-1.0, 0, 1, [0, 0])
    m.set_hop(0.7 + 0.2j, 1, 0, [0, 1])
    m.set_hop(0.15j, 0, 0, [0, 1])
    return m


@functools.lru_cache(maxsize=None)
def model(name):
    """(model, fin_dir) of the test cases, by name."""
    T = tb.tb_model
    return {
        "haldane0": lambda: (hp.haldane(T, delta=0.2), 0),                       # N = 2
        "haldane1": lambda: (hp.haldane(T, delta=0.2), 1),
        "kane_mele": lambda: (hp.kane_mele(T), 0),                               # N = 4
        "chain3": lambda: (hp.chain3(T, -1.0, 0.4, 0.3), 0),                     # N = 3, no k
        "chain1": lambda: (chain1(), 0),                                         # N = 1
        "rand2d": lambda: (hp.random_model(T, 3, 2, 1, seed=7, rmax=2), 0),      # L = 2, N = 6
        "rand2d_spin": lambda: (hp.random_model(T, 2, 2, 2, seed=7, rmax=2), 0),  # L = 2, N = 8
        "rand3d": lambda: (hp.random_model(T, 2, 3, 1, seed=7, rmax=2), 0),      # L = 2, N = 4, surface zone 2-D
        "rand3d_spin": lambda: (hp.random_model(T, 2, 3, 2, seed=7, rmax=2), 0),  # L = 2, N = 8
        "cubic16": lambda: (hp.cubic16(T), 2),                                   # N = 16, surface zone 2-D
        "n32": lambda: (hp.random_model(T, 16, 2, 2, seed=3, rmax=1), 1),        # the top of the LDS regime
        "n36": lambda: (hp.random_model(T, 18, 2, 2, seed=4, rmax=1), 0),        # the first workspace size
        "n128": lambda: (hp.random_model(T, 64, 2, 2, seed=5, rmax=1), 0),
        "n132": lambda: (hp.random_model(T, 66, 2, 2, seed=6, rmax=1), 0),
    }[name]()


def kpts(name, nk=7):
    m, _ = model(name)
    dk = m._dim_k - 1
    if dk == 0:
        return None
    if dk == 1:
        return K7[:nk].reshape(-1, 1)
    return np.column_stack([K7[:nk], K7[::-1][:nk] * 0.77])


def relerr(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max()


# ================================================================ CPU: the restatement against exact facts
CPU_MODELS = ["haldane0", "haldane1", "kane_mele", "chain3", "rand2d", "rand2d_spin", "rand3d", "rand3d_spin"]


def test_layer_sizes():
    for name, L, N in (("haldane0", 1, 2), ("kane_mele", 1, 4), ("chain3", 1, 3), ("rand2d", 2, 6), ("rand2d_spin", 2, 8),
                       ("rand3d", 2, 4), ("rand3d_spin", 2, 8), ("cubic16", 1, 16), ("n32", 1, 32), ("n36", 1, 36), ("n128", 1, 128)):
        m, fd = model(name)
        assert m.principal_layer(fd) == L == sr.principal_layer(m, fd)
        assert L * m._nsta == N


@pytest.mark.parametrize("name", CPU_MODELS)
@pytest.mark.parametrize("steps", [0, 1, 3, 5])
def test_fact1_slab_blocks(name, steps):
    """After i steps G_0 / G_1 are the first / last diagonal block of the resolvent of the slab of L 2^i cells, G_b the middle block of
    the slab of L (2^(i+1) - 1) cells."""
    m, fd = model(name)
    k = kpts(name, 2)
    om = [-1.3, -0.15, 0.4]
    eta = 0.004 if name.startswith("haldane") else 0.01
    g, took = sr.green(m, k, om, eta, fd, tol=0.0, max_iter=steps)
    assert np.all(took == steps)
    assert relerr(g, sr.slab_blocks(m, k, om, eta, fd, steps)) < 1e-11


def test_fact2_chain_closed_form():
    e, t = 0.3, -0.8
    m, fd = model("chain1")
    om = np.array([-2.5, -1.2, 0.3, 0.31, 1.85, 1.95, 3.0])
    for eta in (0.05, 1e-3):
        g, _ = sr.green(m, None, om, eta, fd, tol=1e-14, max_iter=60)
        x = om + 1j * eta - e
        r = np.sqrt(x * x - 4 * t * t + 0j)
        g0 = (x - r) / (2 * t * t)
        g0 = np.where(g0.imag < 0, g0, (x + r) / (2 * t * t))
        # every step inverts z - e, whose condition number inside the band reaches bandwidth / eta = 3.2 / eta, and about
        # log2(bandwidth / eta) + 4 <= 16 steps add up: 16 x 3.2 x 2.2e-16 / eta = 1.1e-14 / eta; ten times that is the bound
        bound = 1e-13 / eta
        assert relerr(g[0, 0, :, 0, 0], g0) < bound
        assert relerr(g[1, 0, :, 0, 0], g0) < bound
        assert relerr(g[2, 0, :, 0, 0], 1.0 / (x - 2 * t * t * g0)) < bound


@pytest.mark.parametrize("name", CPU_MODELS)
def test_fact3_bulk_is_kperp_mean(name):
    """tr G_b(k_par, z) = L mean over k_perp of tr (z - H(k_par, k_perp))^-1 (the trace does not see the orbital phases)."""
    m, fd = model(name)
    L = m.principal_layer(fd)
    k = kpts(name, 2)
    om, eta, nperp = np.array([-0.9, 0.2]), 0.05, 4000
    g, _ = sr.green(m, k, om, eta, fd, tol=1e-14, max_iter=60)
    kk = sr.kpar(m, k)
    pos = list(m._per).index(fd)
    for ik in range(kk.shape[0]):
        full = np.zeros((nperp, m._dim_k))
        rest = [d for d in range(m._dim_k) if d != pos]
        full[:, rest] = kk[ik][:len(rest)]
        full[:, pos] = np.arange(nperp) / nperp
        ev = np.linalg.eigvalsh(orc.ham_batch(m, full))
        for iw, w in enumerate(om):
            want = L * np.mean(np.sum(1.0 / (w + 1j * eta - ev), axis=1))
            assert abs(np.trace(g[2, ik, iw]) - want) < 1e-10 * abs(want)


def edge_peaks(spectral, delta, fin_dir=0, t2abs=0.15):
    """k of the in-gap peaks of A(k) at w = -0.15, 0, 0.15 on side 0 and side 1, eta = 0.01: two lists of three arrays."""
    m = hp.haldane(tb.tb_model, delta=delta, t2abs=t2abs)
    ks = np.arange(400) / 400.0
    a = spectral(m, ks.reshape(-1, 1), [-0.15, 0.0, 0.15], 0.01, fin_dir)
    return [[ks[sr.peaks(a[s, :, w], 5.0)] for w in range(3)] for s in range(2)], a


def check_chiral_pair(pk):
    for s in range(2):
        assert [p.size for p in pk[s]] == [1, 1, 1]                  # exactly one in-gap mode per edge: |C| = 1
    k0 = [float(p[0]) for p in pk[0]]
    k1 = [float(p[0]) for p in pk[1]]
    s0, s1 = np.sign(np.diff(k0)), np.sign(np.diff(k1))
    assert abs(s0.sum()) == 2 and abs(s1.sum()) == 2 and s0[0] == -s1[0]   # monotonic, opposite directions
    return s0[0]


def test_haldane_edge_modes_restatement():
    pk, _ = edge_peaks(lambda *a: sr.spectral(*a)[0], 0.2)
    check_chiral_pair(pk)
    assert np.allclose([p[0] for p in pk[0]], [p[0] for p in pk[1]][::-1], atol=1e-9)
    pk, a = edge_peaks(lambda *a: sr.spectral(*a)[0], 1.5)           # trivial: 3 sqrt(3) t2 < delta
    assert all(p.size == 0 for s in range(2) for p in pk[s]) and a[:2].max() < 0.1


def test_kane_mele_time_reversal_restatement():
    m, fd = model("kane_mele")
    k = K7.reshape(-1, 1)
    a, _ = sr.spectral(m, k, OMEGA13[3:9], 0.02, fd)
    b, _ = sr.spectral(m, -k, OMEGA13[3:9], 0.02, fd)
    assert relerr(a, b) < 1e-10


class DeviceTouched(BaseException):
    """Raised by the stand-in below: not an Exception, so no `pytest.raises(Exception)` can take it for an argument error."""


@pytest.fixture
def no_device(monkeypatch):
    """Any use of the device handle of a model ends the test: the argument errors must come first."""
    def touched(self):
        raise DeviceTouched()
    monkeypatch.setattr(tb.tb_model, "_device_model", touched)


def test_argument_errors(no_device):
    m, _ = model("haldane0")
    om = [0.0, 0.1]
    k = [[0.1], [0.2]]
    calls = {
        "green": lambda **kw: m.surface_green(kw.get("k", k), kw.get("omega", om), kw.get("eta", 0.05), kw.get("fin_dir", 0),
                                              kw.get("side", 0), tol=kw.get("tol", 1e-12), max_iter=kw.get("max_iter", 50)),
        "spectral": lambda **kw: m.surface_spectral(kw.get("k", k), kw.get("omega", om), kw.get("eta", 0.05), kw.get("fin_dir", 0),
                                                    tol=kw.get("tol", 1e-12), max_iter=kw.get("max_iter", 50)),
        "dos": lambda **kw: m.surface_dos_mesh(kw.get("mesh", [4]), kw.get("omega", om), kw.get("eta", 0.05), kw.get("fin_dir", 0),
                                               tol=kw.get("tol", 1e-12), max_iter=kw.get("max_iter", 50)),
    }
    # the control: with valid arguments every call passes its checks and reaches the device
    for call in calls.values():
        with pytest.raises(DeviceTouched):
            call()
    with pytest.raises(DeviceTouched):
        m._gen_layer_blocks([0.1], 0)
    assert m.principal_layer(0) == 1 and m.principal_layer(1) == 1
    direction = "fin_dir must be a lattice direction"
    omega = "omega must be a 1-D array of 1..65536 frequencies"
    common = [(dict(fin_dir=2), direction), (dict(fin_dir=-1), direction), (dict(fin_dir=0.5), direction),
              (dict(omega=[]), omega), (dict(omega=[[0.0]]), omega), (dict(omega=np.zeros(65537)), omega),
              (dict(omega=[0.0, np.nan]), "omega must be finite"), (dict(omega=[np.inf]), "omega must be finite"),
              (dict(eta=0.0), "eta must be finite and > 0"), (dict(eta=-0.1), "eta must be finite and > 0"),
              (dict(eta=np.inf), "eta must be finite and > 0"), (dict(eta=np.nan), "eta must be finite and > 0"),
              (dict(tol=-1.0), "tol must be finite and >= 0"), (dict(tol=np.nan), "tol must be finite and >= 0"),
              (dict(max_iter=-1), "max_iter must be an integer in 0..64"), (dict(max_iter=65), "max_iter must be an integer in 0..64"),
              (dict(max_iter=2.5), "max_iter must be an integer in 0..64")]
    for name, call in calls.items():
        for kw, msg in common:
            with pytest.raises(Exception, match=msg):
                call(**kw)
    shape = "k-vector of wrong shape"
    for name in ("green", "spectral"):
        for bad, msg in (([[0.1, 0.2]], shape), ([[[0.1]]], shape), (np.zeros((0, 1)), shape), ([[np.nan]], "k must be finite"),
                         ([[0.1], [np.inf]], "k must be finite"), (None, "Have to provide a k-vector")):
            with pytest.raises(Exception, match=msg):
                calls[name](k=bad)
    for side in (3, -1, 0.5, None):
        with pytest.raises(Exception, match="side must be 0, 1 or 2"):
            calls["green"](side=side)
    for mesh, msg in (([4, 4], "Incorrect size of the specified k-mesh"), ([], "Incorrect size of the specified k-mesh"),
                      ([0], "Mesh must have positive non-zero number of elements")):
        with pytest.raises(Exception, match=msg):
            calls["dos"](mesh=mesh)
    with pytest.raises(Exception, match=direction):
        m.principal_layer(5)
    with pytest.raises(Exception, match=shape):
        m._gen_layer_blocks([0.1, 0.2], 0)
    with pytest.raises(Exception, match=shape):
        m._gen_layer_blocks([[0.1]], 0)
    with pytest.raises(Exception, match="k must be finite"):
        m._gen_layer_blocks([np.nan], 0)
    with pytest.raises(Exception, match=direction):
        m._gen_layer_blocks([0.1], 3)
    # a direction that is not periodic; a model without k; a 1-D model has neither a k list nor a surface mesh
    ribbon = quiet(m.cut_piece, 3, 0)
    finite = "Can not make model finite along this direction"
    for call in (lambda: ribbon.surface_spectral(None, om, 0.05, 0), lambda: ribbon.surface_green(None, om, 0.05, 0, 0),
                 lambda: ribbon.surface_dos_mesh([4], om, 0.05, 0), lambda: ribbon.principal_layer(0),
                 lambda: ribbon._gen_layer_blocks(None, 0)):
        with pytest.raises(Exception, match=finite):
            call()
    dot = quiet(ribbon.cut_piece, 3, 1)
    for call in (lambda: dot.principal_layer(0), lambda: dot.surface_spectral(None, om, 0.05, 0),
                 lambda: dot.surface_green(None, om, 0.05, 0, 0), lambda: dot.surface_dos_mesh([4], om, 0.05, 0),
                 lambda: dot._gen_layer_blocks(None, 0)):
        with pytest.raises(Exception, match="need a model with dim_k >= 1"):
            call()
    with pytest.raises(Exception, match="surface_dos_mesh needs a model with dim_k >= 2"):
        ribbon.surface_dos_mesh([4], om, 0.05, 1)
    for call in (lambda: ribbon.surface_green([[0.1]], om, 0.05, 1, 0), lambda: ribbon.surface_spectral([0.1], om, 0.05, 1),
                 lambda: ribbon._gen_layer_blocks([0.1], 1)):
        with pytest.raises(Exception, match=shape):                       # dim_k == 1: no k
            call()
    with pytest.raises(DeviceTouched):                                     # ... and one point without it
        ribbon.surface_spectral(None, om, 0.05, 1)


def test_layer_beyond_128_states_is_unsupported(no_device):
    m, fd = model("n132")
    with pytest.raises(tb._lib.TbkError, match="132 states"):
        m.surface_spectral([[0.1]], [0.0], 0.05, fd)
    with pytest.raises(tb._lib.TbkError, match="at most 128"):
        m.surface_green([[0.1]], [0.0], 0.05, fd, 2)


# ================================================================ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["haldane0", "haldane1", "kane_mele", "chain3", "rand2d", "rand2d_spin", "rand3d", "cubic16", "n36"])
def test_layer_blocks(gpu_ctx, name):
    m, fd = model(name)
    k = kpts(name, 3)
    h00, h01 = sr.layer_blocks(m, fd, k)
    for ik in range(h00.shape[0]):
        g00, g01 = m._gen_layer_blocks(None if k is None else k[ik], fd)
        assert g00.shape == g01.shape == h00.shape[1:]
        scale = max(np.abs(h00[ik]).max(), np.abs(h01[ik]).max())
        assert np.abs(g00 - h00[ik]).max() < 1e-12 * scale and np.abs(g01 - h01[ik]).max() < 1e-12 * scale
        assert np.array_equal(g00, g00.conj().T)


def band_edge(m, kpar, pos, nperp=600):
    """The bottom of the second-lowest bulk band over k_perp at one k_par of a 2-D model: an edge of the projected bulk spectrum."""
    full = np.zeros((nperp, 2))
    full[:, 1 - pos] = kpar
    full[:, pos] = np.arange(nperp) / nperp
    return np.linalg.eigvalsh(orc.ham_batch(m, full))[:, 2].min()


SLAB_CASES = [("haldane0", 5, 7, 0.01), ("chain3", 5, 1, 0.01), ("kane_mele", 5, 7, 0.01), ("rand2d", 4, 7, 0.02),
              ("rand2d_spin", 4, 7, 0.02), ("cubic16", 3, 3, 0.02), ("n32", 3, 2, 0.05), ("n36", 2, 2, 0.05), ("n128", 2, 2, 0.05)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,steps,nk,eta", SLAB_CASES)
def test_green_is_slab_block(gpu_ctx, name, steps, nk, eta):
    """tol=0, max_iter=i against the direct NumPy inverse of the slab (independent of the restatement's loop)."""
    m, fd = model(name)
    k = kpts(name, nk)
    om = OMEGA13.copy() if nk > 3 or k is None else OMEGA13[[1, 5, 9]] if name != "cubic16" else OMEGA13[[1, 4, 5, 8, 11]]
    if name == "kane_mele":
        om[6] = band_edge(m, k[3, 0], 0) + 0.5 * eta       # within eta of a band edge at k[3]
    want = sr.slab_blocks(m, k, om, eta, fd, steps)
    for side in range(3):
        g = m.surface_green(k, om, eta, fd, side, tol=0.0, max_iter=steps)
        assert g.shape == want[side].shape
        err = relerr(g, want[side])
        print("%s side %d: |G - slab| / max|G| = %.3g" % (name, side, err))
        assert err < TOL


@functools.lru_cache(maxsize=None)
def reference(name, eta):
    """The restatement at the default tol on the 7 x 13 points (3 x 5 for the larger layers): (k, omega, G, steps)."""
    m, fd = model(name)
    big = m.principal_layer(fd) * m._nsta >= 16
    k = kpts(name, 3 if big else 7)
    om = OMEGA13[[1, 4, 5, 8, 11]] if big else OMEGA13
    g, steps = sr.green(m, k, om, eta, fd)
    for x in (g, steps, om):
        x.setflags(write=False)
    return k, om, g, steps


REF_CASES = [("haldane0", 0.01), ("haldane1", 0.01), ("chain3", 0.01), ("kane_mele", 0.01), ("rand2d", 0.02), ("rand2d_spin", 0.02),
             ("rand3d", 0.02), ("cubic16", 0.02), ("n32", 0.05), ("n36", 0.05), ("n128", 0.05)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,eta", REF_CASES)
def test_spectral_against_restatement(gpu_ctx, name, eta):
    m, fd = model(name)
    k, om, g, steps = reference(name, eta)
    a, info = m.surface_spectral(k, om, eta, fd, return_info=True)
    ap = m.surface_spectral(k, om, eta, fd, per_state=True)
    want, wantp = sr.spectral_of(g, m._nsta), sr.spectral_of(g, m._nsta, per_state=True)
    assert a.shape == want.shape and ap.shape == wantp.shape and info.shape == steps.shape and info.dtype == np.int32
    print("%s: |A - ref| / max|A| = %.3g, per state %.3g, steps %d..%d (ref %d..%d)" %
          (name, relerr(a, want), relerr(ap, wantp), info.min(), info.max(), steps.min(), steps.max()))
    assert relerr(a, want) < TOL and relerr(ap, wantp) < TOL
    assert np.abs(info.astype(int) - steps).max() <= 1
    for side in range(3):
        assert relerr(m.surface_green(k, om, eta, fd, side), g[side]) < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("name,eta,mesh", [("haldane0", 0.01, [7]), ("kane_mele", 0.01, [5]), ("rand2d_spin", 0.02, [5]),
                                            ("rand3d", 0.02, [3, 4]), ("cubic16", 0.02, [2, 3]), ("n32", 0.05, [3]),
                                            ("n36", 0.05, [3]), ("n128", 0.05, [2])])
def test_dos_mesh_against_restatement(gpu_ctx, name, eta, mesh):
    m, fd = model(name)
    om = OMEGA13[[1, 4, 5, 8, 11]]
    for per_state in (False, True):
        d = m.surface_dos_mesh(mesh, om, eta, fd, per_state=per_state)
        want = sr.dos_mesh(m, mesh, om, eta, fd, per_state=per_state)
        assert d.shape == want.shape
        assert relerr(d, want) < TOL
        assert np.array_equal(d, m.surface_dos_mesh(mesh, om, eta, fd, per_state=per_state))
        a = m.surface_spectral(sr.surface_mesh(m, mesh, fd), om, eta, fd, per_state=per_state)
        assert relerr(d, a.mean(axis=1)) < 1e-13


@pytest.mark.gpu
@pytest.mark.parametrize("name,eta", [("rand2d", 0.02), ("rand2d_spin", 0.02), ("rand3d", 0.02)])
def test_bulk_is_the_same_in_every_cell_of_the_layer(gpu_ctx, name, eta):
    m, fd = model(name)
    k, om, _, _ = reference(name, eta)
    g = m.surface_green(k, om, eta, fd, 2)
    ns = m._nsta
    assert g.shape[-1] == 2 * ns
    assert relerr(g[..., ns:, ns:], g[..., :ns, :ns]) < TOL


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("name,eta", [("haldane0", 0.01), ("kane_mele", 0.01), ("rand2d_spin", 0.02), ("cubic16", 0.02), ("n36", 0.05)])
def test_a_point_does_not_depend_on_its_batch(gpu_ctx, name, eta):
    m, fd = model(name)
    k, om = kpts(name, 7), OMEGA13
    ik, iw = 3, 5
    a = m.surface_spectral(k, om, eta, fd, per_state=True)
    assert np.array_equal(bits(a), bits(m.surface_spectral(k, om, eta, fd, per_state=True)))           # repeated calls
    alone = m.surface_spectral(k[ik:ik + 1], om[iw:iw + 1], eta, fd, per_state=True)
    assert np.array_equal(bits(alone[:, 0, 0]), bits(a[:, ik, iw]))                                     # alone
    pk, pw = np.random.default_rng(0).permutation(7), np.random.default_rng(1).permutation(13)
    b = m.surface_spectral(k[pk], om[pw], eta, fd, per_state=True)                                      # other positions, unsorted
    assert np.array_equal(bits(b), bits(a[:, pk][:, :, pw]))
    rep = m.surface_spectral(k[[ik, 0, ik]], om[[iw, iw, 2, iw]], eta, fd, per_state=True)              # repeated k and omega
    for i in (0, 2):
        for j in (0, 1, 3):
            assert np.array_equal(bits(rep[:, i, j]), bits(a[:, ik, iw]))
    for side in range(3):
        g = m.surface_green(k, om, eta, fd, side)
        g1 = m.surface_green(k[ik:ik + 1], om[iw:iw + 1], eta, fd, side)
        assert np.array_equal(bits(g1[0, 0]), bits(g[ik, iw]))
    assert np.array_equal(bits(m.surface_spectral(k, om, eta, fd)[:, ik, iw]),
                          bits(m.surface_spectral(k[ik:ik + 1], om[iw:iw + 1], eta, fd)[:, 0, 0]))


@pytest.mark.gpu
def test_a_point_across_the_chunk_boundary_and_many_frequencies(gpu_ctx):
    """A chunk holds at most 2^20 (k, omega) problems: 17 k x 65 536 omega of the Haldane model are two chunks (16 k + 1 k)."""
    m, fd = model("haldane0")
    rng = np.random.default_rng(5)
    om = rng.uniform(-3.5, 3.5, 65536)                     # unsorted
    k = rng.random((17, 1))
    a = m.surface_spectral(k, om, 0.01, fd)
    assert a.shape == (3, 17, 65536) and np.all(np.isfinite(a)) and a.min() > 0.0
    for ik, iw in ((16, 777), (15, 65535), (0, 0)):
        alone = m.surface_spectral(k[ik:ik + 1], om[iw:iw + 1], 0.01, fd)                               # n_omega = 1
        assert alone.shape == (3, 1, 1)
        assert np.array_equal(bits(alone[:, 0, 0]), bits(a[:, ik, iw]))
    one_k = m.surface_spectral(k[16:17], om, 0.01, fd)                                                  # nk = 1, n_omega = 65 536
    assert np.array_equal(bits(one_k[:, 0]), bits(a[:, 16]))
    want, _ = sr.spectral(m, k[16:17], om[:40], 0.01, fd)
    assert relerr(a[:, 16:17, :40], want) < TOL


@pytest.mark.gpu
def test_mesh_mean_over_two_chunks(gpu_ctx):
    """A mesh of 17 k x 65 536 omega is two chunks (16 k + 1 k): the chunk sums and the sum over the chunks."""
    m, fd = model("haldane0")
    om = np.random.default_rng(6).uniform(-3.5, 3.5, 65536)
    for per_state in (False, True):
        d = m.surface_dos_mesh([17], om, 0.01, fd, per_state=per_state)
        assert d.shape == ((3, 65536, 2) if per_state else (3, 65536))
        assert np.array_equal(bits(d), bits(m.surface_dos_mesh([17], om, 0.01, fd, per_state=per_state)))
        a = m.surface_spectral(sr.surface_mesh(m, [17], fd), om, 0.01, fd, per_state=per_state)
        assert relerr(d, a.mean(axis=1)) < 1e-13
        assert relerr(d[:, :40], sr.dos_mesh(m, [17], om[:40], 0.01, fd, per_state=per_state)) < TOL


@pytest.mark.gpu
def test_uncoupled_layers_and_zero_steps(gpu_ctx):
    m = no_coupling()
    k, om, eta = K7[:3].reshape(-1, 1), OMEGA13[[2, 5, 7]], 0.02
    h00, h01 = sr.layer_blocks(m, 0, k)
    assert np.abs(h01).max() == 0.0
    a, info = m.surface_spectral(k, om, eta, 0, per_state=True, return_info=True)
    assert np.all(info == 0)
    for ik in range(3):
        for iw, w in enumerate(om):
            g = np.linalg.inv((w + 1j * eta) * np.identity(2) - h00[ik])
            for side in range(3):
                assert relerr(m.surface_green(k[ik:ik + 1], [w], eta, 0, side)[0, 0], g) < TOL
                assert np.abs(a[side, ik, iw] + np.diag(g).imag / np.pi).max() < TOL * np.abs(g).max()
    # max_iter = 0 without a test: the isolated layer of a model whose layers do couple
    hm, fd = model("haldane0")
    h00, _ = sr.layer_blocks(hm, fd, k)
    g = hm.surface_green(k, om, eta, fd, 2, tol=0.0, max_iter=0)
    for ik in range(3):
        for iw, w in enumerate(om):
            assert relerr(g[ik, iw], np.linalg.inv((w + 1j * eta) * np.identity(2) - h00[ik])) < TOL
    _, info = hm.surface_spectral(k, om, eta, fd, tol=0.0, max_iter=7, return_info=True)
    assert np.all(info == 7)


@pytest.mark.gpu
def test_non_convergence_is_reported(gpu_ctx):
    m, fd = model("haldane0")
    k, om = K7.reshape(-1, 1), OMEGA13
    _, steps = m.surface_spectral(k, om, 0.01, fd, return_info=True)   # the device's own step counts
    limit = 6
    nfail = int((steps > limit).sum())
    assert 0 < nfail < 91
    with pytest.raises(Exception, match="%d of 91 .* did not reach tol" % nfail):
        m.surface_spectral(k, om, 0.01, fd, tol=1e-12, max_iter=limit)
    with pytest.raises(Exception, match="91 of 91"):
        m.surface_spectral(k, om, 0.01, fd, tol=1e-12, max_iter=2)
    cm, cfd = model("rand2d_spin")                                     # the workgroup kernel reports the same way
    with pytest.raises(Exception, match="did not reach tol"):
        cm.surface_green(kpts("rand2d_spin", 2), om[:3], 0.02, cfd, 0, max_iter=1)


@pytest.mark.gpu
def test_haldane_edge_modes_and_chern_sign(gpu_ctx):
    """One chiral mode per edge, opposite directions on the two edges, reversed with the sign of the Chern number; none when trivial."""
    rel = []
    for t2abs in (0.15, -0.15):
        pk, _ = edge_peaks(lambda m, *a: m.surface_spectral(*a), 0.2, t2abs=t2abs)
        slope = check_chiral_pair(pk)
        m = hp.haldane(tb.tb_model, delta=0.2, t2abs=t2abs)
        c = m.berry_curvature_mesh([64, 64], occ=[0]) / (2.0 * np.pi)
        assert abs(abs(c) - 1.0) < 1e-2
        rel.append(slope * np.sign(c))
    assert rel[0] == rel[1]
    pk, a = edge_peaks(lambda m, *a: m.surface_spectral(*a), 1.5)
    assert all(p.size == 0 for s in range(2) for p in pk[s]) and a[:2].max() < 0.1
    c = hp.haldane(tb.tb_model, delta=1.5).berry_curvature_mesh([64, 64], occ=[0]) / (2.0 * np.pi)
    assert abs(c) < 1e-2
