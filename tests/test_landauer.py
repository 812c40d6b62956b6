"""Landauer transmission through a scattering region between two leads of the crystal (tb_model.lead_self_energy, _gen_device_blocks,
transmission, conductance_mesh).  The CPU tests check the NumPy restatement landauer_ref.py against exact facts
(the dense inverse, the channel count of a clean wire, the closed form of one impurity in a chain, the quantised edge channel of a
disordered Chern ribbon) and the argument errors; the GPU tests check the device against the restatement to 1e-9 of max(1, max|T|)
(max|Sigma|), and that a point's bits do not depend on the rest of the call."""
import functools

import numpy as np
import pytest

import helpers as hp
import landauer_ref as lr
import sgf_ref as sr
from helpers import quiet
from oracle import tb_oracle as orc

import pythtb_amd as tb

TOL = 1e-9          # of max(1, max|T|) or max|Sigma|: the tolerance of the surface Green's functions
OMEGA13 = np.array([-2.9, -1.7, -1.05, -0.6, -0.15, 0.0, 0.15, 0.33, 0.8, 1.3, 2.1, 2.75, 3.6])
K7 = np.array([0.03, 0.17, 0.31, 0.465, 0.58, 0.74, 0.92])


def chain1(e=0.3, t=-0.8):
    m = quiet(tb.tb_model, 1, 1, [[1.0]], [[0.0]])
    m.set_onsite([e])
    m.set_hop(t, 0, 0, [1])
    return m


@functools.lru_cache(maxsize=None)
def model(name):
    """(model, fin_dir) of the test cases, by name: the table of tests/test_surface_green.py."""
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


def eta_of(name):
    return 0.004 if name.startswith("haldane") else 0.01


def relerr(a, b, floor=0.0):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(floor, np.abs(b).max())


@functools.lru_cache(maxsize=None)
def device(name, nlayers, hop=True):
    """The disordered device of a case: on-site shifts in +-0.5 and, with `hop`, one hopping scaled by 1.3."""
    m, fd = model(name)
    return lr.disordered(m, fd, nlayers, seed=11 + nlayers, hop=(3, 1.3) if hop else None)


# ================================================================ CPU: the restatement against exact facts
@pytest.mark.parametrize("name", ["haldane0", "kane_mele", "chain3", "rand2d", "rand2d_spin"])
@pytest.mark.parametrize("nlayers", [1, 2, 5])
def test_sweep_is_the_dense_inverse(name, nlayers):
    m, fd = model(name)
    dev = device(name, nlayers, hop=False)
    k, om, eta = kpts(name, 2), [-1.3, -0.15, 0.4, 1.1], eta_of(name)
    t, _ = lr.transmission(m, k, om, eta, fd, dev)
    want, _ = lr.transmission(m, k, om, eta, fd, dev, route=lr.dense)
    assert t.max() > 1e-3
    assert relerr(t, want) < 1e-11


CHANNEL_CASES = [("haldane0", 0.31, (-1.4, 1.35)), ("kane_mele", 0.17, (-1.55, 1.55)), ("chain3", None, (-1.62, 0.0, 1.6)),
                 ("chain1", None, (-0.9, 0.7, 1.5)), ("rand2d", 0.31, (-1.7,))]


@pytest.mark.parametrize("name,k,omegas", CHANNEL_CASES)
def test_channel_count_of_a_clean_wire(name, k, omegas):
    """A pristine region transmits every open channel: T = the number of bands that cross omega with positive velocity, up to the
    loss 2 M eta / |v| of the broadening."""
    m, fd = model(name)
    kk = None if k is None else [[k]]
    dev = quiet(m.cut_piece, 3 * m.principal_layer(fd), fd)
    t, _ = lr.transmission(m, kk, omegas, 1e-6, fd, dev)
    open_channels = 0
    for iw, w in enumerate(omegas):
        n, margin = lr.channels(m, fd, k, w)
        assert margin >= 0.05, (name, w, margin)               # omega well inside its bands: the velocities are not small
        assert abs(t[0, iw] - n) < 1e-3, (name, w, t[0, iw], n)
        open_channels += n
    assert open_channels > 0


def impurity_closed_form(omega, e=0.3, t=-0.8, eps=0.7):
    c = (np.asarray(omega) - e) / (2 * t)
    return 1.0 / (1.0 + (eps / (2 * abs(t))) ** 2 / (1.0 - c * c))


def impurity_device():
    m, fd = model("chain1")
    dev = quiet(m.cut_piece, 5, fd)
    dev.set_onsite(0.7, 2, mode="add")                         # site 3 of 5
    return m, fd, dev


def test_one_impurity_in_the_chain_restatement():
    m, fd, dev = impurity_device()
    t, _ = lr.transmission(m, None, [-0.9, 1.2, 2.5], 1e-6, fd, dev)
    assert np.abs(t[0, :2] - impurity_closed_form([-0.9, 1.2])).max() < 1e-4
    assert abs(t[0, 2]) < 1e-12                                # outside the band


RIBBON_OMEGA = [-0.3, 0.2, 1.5]


@functools.lru_cache(maxsize=None)
def ribbon(delta):
    """The Haldane ribbon of 8 cells (N = 16), a region of M = 6 layers with on-site disorder in +-0.5."""
    m = quiet(hp.haldane(tb.tb_model, delta).cut_piece, 8, 1)
    dev = quiet(m.cut_piece, 6, 0)
    for i, x in enumerate(np.random.default_rng(5).uniform(-0.5, 0.5, dev._norb)):
        dev.set_onsite(float(x), i, mode="add")
    return m, dev


def check_ribbon(t_chern, t_trivial):
    assert abs(t_chern[0] - 1.0) < 1e-3 and abs(t_chern[1] - 1.0) < 1e-3      # the edge channel does not scatter
    assert t_chern[2] < 5.0                                                     # bulk channels do
    assert np.all(np.abs(t_trivial) < 1e-12)


def test_chern_ribbon_restatement():
    m, dev = ribbon(0.2)
    assert m.principal_layer(0) == 1 and m._nsta == 16 and dev._norb == 96
    t, _ = lr.transmission(m, None, RIBBON_OMEGA, 1e-6, 0, dev)
    m0, dev0 = ribbon(2.5)
    t0, _ = lr.transmission(m0, None, RIBBON_OMEGA, 1e-6, 0, dev0)
    check_ribbon(t[0], t0[0])


class DeviceTouched(BaseException):
    """Raised by the stand-in below: not an Exception, so no `pytest.raises(Exception)` can take it for an argument error."""


@pytest.fixture
def no_device(monkeypatch):
    """Any use of the device handle of a model ends the test: the argument errors must come first."""
    def touched(self):
        raise DeviceTouched()
    monkeypatch.setattr(tb.tb_model, "_device_model", touched)


def test_valid_calls_reach_the_device(no_device):
    m, fd = model("haldane0")
    dev = device("haldane0", 3)
    om, k = [0.0, 0.1], [[0.1], [0.2]]
    for call in (lambda: m.transmission(k, om, 0.05, fd), lambda: m.transmission(k, om, 0.05, fd, device=dev),
                 lambda: m.lead_self_energy(k, om, 0.05, fd, 0), lambda: m.lead_self_energy(k, om, 0.05, fd, 1),
                 lambda: m.conductance_mesh([4], om, 0.05, fd), lambda: m.conductance_mesh([4], om, 0.05, fd, device=dev),
                 lambda: m._gen_device_blocks([0.1], fd, dev)):
        with pytest.raises(DeviceTouched):
            call()
    c, cfd = model("chain1")
    with pytest.raises(DeviceTouched):                                         # dim_k == 1: no k, one point
        c.transmission(None, om, 0.05, cfd, device=quiet(c.cut_piece, 4, cfd))


def test_device_errors(no_device):
    m, fd = model("haldane0")
    om, k = [0.0, 0.1], [[0.1], [0.2]]
    good = quiet(m.cut_piece, 3, fd)

    def calls(dev):
        return (lambda: m.transmission(k, om, 0.05, fd, device=dev), lambda: m.conductance_mesh([4], om, 0.05, fd, device=dev),
                lambda: m._gen_device_blocks([0.1], fd, dev))

    def raises(dev, msg):
        for call in calls(dev):
            with pytest.raises(Exception, match=msg) as info:
                call()
            assert str(info.value).startswith("\n\n")

    raises("ribbon", "device must be a tb_model\\.")
    raises(orc, "device must be a tb_model\\.")
    lattice = "device must share the lattice and nspin of the model\\."
    other = quiet(tb.tb_model, 1, 2, [[1.0, 0.0], [0.0, 1.0]], good._orb, per=[1])
    raises(other, lattice)
    raises(quiet(hp.kane_mele(tb.tb_model).cut_piece, 3, fd), lattice)                       # nspin
    raises(quiet(tb.tb_model, 1, 3, np.identity(3), np.zeros((6, 3)), per=[1]), lattice)     # dim_r
    period = "device must be finite along fin_dir and periodic along the other periodic directions\\."
    raises(quiet(m.cut_piece, 3, 1), period)                                   # cut along the other direction
    raises(m, period)                                                          # not cut at all
    raises(quiet(good.cut_piece, 2, 1), period)                                # cut twice
    count = "device must hold 1\\.\\.1024 principal layers of 2 orbitals\\."
    raises(quiet(tb.tb_model, 1, 2, hp.LAT, good._orb[:5], per=[1]), count)
    raises(quiet(tb.tb_model, 1, 2, hp.LAT, np.zeros((2050, 2)), per=[1]), count)
    moved = quiet(m.cut_piece, 3, fd)
    moved._orb[4, 1] += 1e-9
    raises(moved, "device orbitals must be those of cut_piece\\(3, fin_dir\\)\\.")
    far = quiet(m.cut_piece, 4, fd)
    far.set_hop(0.1, 6, 1, [0, 0])
    raises(far, "device couples layers 1 and 4: only neighbouring principal layers may couple\\.")
    r, rfd = model("rand2d")                                                   # L = 2: layers of two cells
    assert r.principal_layer(rfd) == 2
    with pytest.raises(Exception, match="device must hold 1\\.\\.1024 principal layers of 6 orbitals"):
        r.transmission(k, om, 0.05, rfd, device=quiet(r.cut_piece, 3, rfd))
    with pytest.raises(Exception, match="device orbitals must be those of cut_piece\\(4, fin_dir\\)"):
        shifted = quiet(r.cut_piece, 4, rfd)
        shifted._orb[:, rfd] += 1.0
        r.transmission(k, om, 0.05, rfd, device=shifted)
    far = quiet(r.cut_piece, 6, rfd)
    far.set_hop(0.1, 1, 13, [0, 0])
    with pytest.raises(Exception, match="device couples layers 1 and 3"):
        r.transmission(k, om, 0.05, rfd, device=far)
    near = quiet(r.cut_piece, 6, rfd)
    near.set_hop(0.1, 1, 11, [0, 0], mode="add")                               # layers 1 and 2: fine
    with pytest.raises(DeviceTouched):
        r.transmission(k, om, 0.05, rfd, device=near)


def test_shared_argument_errors(no_device):
    m, fd = model("haldane0")
    dev = device("haldane0", 2)
    om = [0.0, 0.1]
    k = [[0.1], [0.2]]
    calls = {
        "sigma": lambda **kw: m.lead_self_energy(kw.get("k", k), kw.get("omega", om), kw.get("eta", 0.05), kw.get("fin_dir", 0),
                                                 kw.get("side", 0), tol=kw.get("tol", 1e-12), max_iter=kw.get("max_iter", 50)),
        "t": lambda **kw: m.transmission(kw.get("k", k), kw.get("omega", om), kw.get("eta", 0.05), kw.get("fin_dir", 0),
                                         device=dev, tol=kw.get("tol", 1e-12), max_iter=kw.get("max_iter", 50)),
        "t0": lambda **kw: m.transmission(kw.get("k", k), kw.get("omega", om), kw.get("eta", 0.05), kw.get("fin_dir", 0),
                                          tol=kw.get("tol", 1e-12), max_iter=kw.get("max_iter", 50)),
        "mesh": lambda **kw: m.conductance_mesh(kw.get("mesh", [4]), kw.get("omega", om), kw.get("eta", 0.05), kw.get("fin_dir", 0),
                                                device=dev, tol=kw.get("tol", 1e-12), max_iter=kw.get("max_iter", 50)),
    }
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
    for name in ("sigma", "t", "t0"):
        for bad, msg in (([[0.1, 0.2]], shape), ([[[0.1]]], shape), (np.zeros((0, 1)), shape), ([[np.nan]], "k must be finite"),
                         ([[0.1], [np.inf]], "k must be finite"), (None, "Have to provide a k-vector")):
            with pytest.raises(Exception, match=msg):
                calls[name](k=bad)
    for side in (2, 3, -1, 0.5, None):
        with pytest.raises(Exception, match="side must be 0 or 1\\."):
            calls["sigma"](side=side)
    for mesh, msg in (([4, 4], "Incorrect size of the specified k-mesh"), ([], "Incorrect size of the specified k-mesh"),
                      ([0], "Mesh must have positive non-zero number of elements")):
        with pytest.raises(Exception, match=msg):
            calls["mesh"](mesh=mesh)
    with pytest.raises(Exception, match=shape):
        m._gen_device_blocks([0.1, 0.2], 0, dev)
    with pytest.raises(Exception, match=direction):
        m._gen_device_blocks([0.1], 3, dev)
    # a 1-D model has neither a k list nor a surface mesh; a direction that is not periodic; a model without k
    rib = quiet(m.cut_piece, 3, 0)
    with pytest.raises(Exception, match="conductance_mesh needs a model with dim_k >= 2"):
        rib.conductance_mesh([4], om, 0.05, 1)
    for call in (lambda: rib.transmission([[0.1]], om, 0.05, 1), lambda: rib.lead_self_energy([0.1], om, 0.05, 1, 0)):
        with pytest.raises(Exception, match=shape):
            call()
    finite = "Can not make model finite along this direction"
    for call in (lambda: rib.transmission(None, om, 0.05, 0), lambda: rib.lead_self_energy(None, om, 0.05, 0, 1),
                 lambda: rib.conductance_mesh([4], om, 0.05, 0)):
        with pytest.raises(Exception, match=finite):
            call()
    dot = quiet(rib.cut_piece, 3, 1)
    for call in (lambda: dot.transmission(None, om, 0.05, 0), lambda: dot.lead_self_energy(None, om, 0.05, 0, 0),
                 lambda: dot.conductance_mesh([4], om, 0.05, 0)):
        with pytest.raises(Exception, match="need a model with dim_k >= 1"):
            call()


def test_layer_beyond_128_states_is_unsupported(no_device):
    m, fd = model("n132")
    with pytest.raises(tb._lib.TbkError, match="132 states"):
        m.transmission([[0.1]], [0.0], 0.05, fd)
    with pytest.raises(tb._lib.TbkError, match="at most 128"):
        m.lead_self_energy([[0.1]], [0.0], 0.05, fd, 1)
    with pytest.raises(tb._lib.TbkError, match="at most 128"):
        m.conductance_mesh([3], [0.0], 0.05, fd)
    with pytest.raises(tb._lib.TbkError, match="at most 128"):
        m._gen_device_blocks([0.1], fd, quiet(m.cut_piece, 2, fd))


# ================================================================ GPU
def grid(name):
    """(k, omega) of a case: 7 x 13 points, 3 x 5 from 16 states, 1 x 2 for the three largest layers."""
    m, fd = model(name)
    n = m.principal_layer(fd) * m._nsta
    if n >= 32:
        return kpts(name, 1), OMEGA13[[4, 9]]
    if n >= 16:
        return kpts(name, 3), OMEGA13[[1, 4, 5, 8, 11]]
    return kpts(name, 7), OMEGA13


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["haldane0", "rand2d_spin", "n36"])
def test_device_blocks(gpu_ctx, name):
    m, fd = model(name)
    dev = device(name, 3)
    k = kpts(name, 2)
    d, u, far = lr.device_blocks(m, fd, k, dev)
    assert far == 0.0 and np.abs(u).max() > 0.0
    for ik in range(d.shape[0]):
        gd, gu = m._gen_device_blocks(k[ik], fd, dev)
        assert gd.shape == d[ik].shape and gu.shape == u[ik].shape
        bound = 1e-13 * min(1.0, max(np.abs(d[ik]).max(), np.abs(u[ik]).max()))
        assert np.abs(gd - d[ik]).max() < bound and np.abs(gu - u[ik]).max() < bound
        assert np.array_equal(gd, gd.conj().transpose(0, 2, 1))
    one, none = m._gen_device_blocks(k[0], fd, device(name, 1))
    assert one.shape == d[0, :1].shape and none.shape == (0,) + d.shape[2:]


@functools.lru_cache(maxsize=None)
def sigma_reference(name):
    m, fd = model(name)
    k, om = grid(name)
    ref = lr.self_energies(m, k, om, eta_of(name), fd)
    for x in ref:
        x.setflags(write=False)
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["haldane0", "chain1", "kane_mele", "rand2d", "n32", "n36", "n128"])
def test_self_energies_against_restatement(gpu_ctx, name):
    m, fd = model(name)
    k, om = grid(name)
    sl, sg, _ = sigma_reference(name)
    for side, want in ((0, sg), (1, sl)):
        s = m.lead_self_energy(k, om, eta_of(name), fd, side)
        assert s.shape == want.shape and s.dtype == complex
        print("%s side %d: |Sigma - ref| / max|Sigma| = %.3g" % (name, side, relerr(s, want)))
        assert relerr(s, want) < TOL


T_CASES = [("chain1", 5), ("chain3", 3), ("haldane0", 1), ("haldane0", 4), ("haldane1", 1), ("haldane1", 4), ("kane_mele", 3),
           ("rand2d", 2), ("rand2d_spin", 2), ("rand3d_spin", 2), ("cubic16", 2), ("n32", 2), ("n36", 2), ("n128", 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,nlayers", T_CASES)
def test_transmission_against_restatement(gpu_ctx, name, nlayers):
    m, fd = model(name)
    dev = device(name, nlayers)
    k, om = grid(name)
    eta = eta_of(name)
    want, steps = lr.transmission(m, k, om, eta, fd, dev)
    t, info = m.transmission(k, om, eta, fd, device=dev, return_info=True)
    assert t.shape == want.shape and t.dtype == float and info.shape == steps.shape and info.dtype == np.int32
    err = np.abs(t - want).max()
    print("%s M=%d: max T = %.4g, |T - ref| = %.3g (%.3g of 1e-9 max(1, max|T|)), steps %d..%d (ref %d..%d)" %
          (name, nlayers, want.max(), err, err / (TOL * max(1.0, want.max())), info.min(), info.max(), steps.min(), steps.max()))
    assert want.max() > 1e-3                                                   # the case transmits
    assert err < TOL * max(1.0, want.max())
    assert np.abs(info.astype(int) - steps).max() <= 1
    assert np.array_equal(t, m.transmission(k, om, eta, fd, device=dev))


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["haldane0", "chain1", "kane_mele", "rand2d", "cubic16", "n36"])
def test_no_device_is_the_pristine_layer(gpu_ctx, name):
    m, fd = model(name)
    k, om = grid(name)
    t = m.transmission(k, om, eta_of(name), fd)
    same = m.transmission(k, om, eta_of(name), fd, device=quiet(m.cut_piece, m.principal_layer(fd), fd))
    assert np.array_equal(bits(t), bits(same))
    want, _ = lr.transmission(m, k, om, eta_of(name), fd)
    assert relerr(t, want, 1.0) < TOL


@pytest.mark.gpu
def test_one_impurity_in_the_chain(gpu_ctx):
    m, fd, dev = impurity_device()
    t = m.transmission(None, [-0.9, 1.2, 2.5], 1e-6, fd, device=dev)
    assert t.shape == (1, 3)
    assert np.abs(t[0, :2] - impurity_closed_form([-0.9, 1.2])).max() < 1e-4
    assert abs(t[0, 2]) < 1e-12


@pytest.mark.gpu
def test_chern_ribbon(gpu_ctx):
    m, dev = ribbon(0.2)
    m0, dev0 = ribbon(2.5)
    t = m.transmission(None, RIBBON_OMEGA, 1e-6, 0, device=dev)
    t0 = m0.transmission(None, RIBBON_OMEGA, 1e-6, 0, device=dev0)
    print("Chern ribbon: T = %s, trivial %s" % (t[0], t0[0]))
    check_ribbon(t[0], t0[0])
    for mm, dd in ((m, dev), (m0, dev0)):
        want, _ = lr.transmission(mm, None, RIBBON_OMEGA, 0.004, 0, dd)
        got = mm.transmission(None, RIBBON_OMEGA, 0.004, 0, device=dd)
        assert relerr(got, want, 1.0) < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["haldane0", "kane_mele", "rand2d_spin", "cubic16", "n36"])
def test_a_point_does_not_depend_on_its_batch(gpu_ctx, name):
    m, fd = model(name)
    dev = device(name, 3)
    eta = eta_of(name)
    k, om = kpts(name, 7), OMEGA13
    ik, iw = 3, 5
    a = m.transmission(k, om, eta, fd, device=dev)                                                      # 91 points
    assert np.array_equal(bits(a), bits(m.transmission(k, om, eta, fd, device=dev)))                    # repeated calls
    alone = m.transmission(k[ik:ik + 1], om[iw:iw + 1], eta, fd, device=dev)
    assert np.array_equal(bits(alone[0, 0]), bits(a[ik, iw]))                                           # alone
    pk, pw = np.random.default_rng(0).permutation(7), np.random.default_rng(1).permutation(13)
    b = m.transmission(k[pk], om[pw], eta, fd, device=dev)                                              # other positions, unsorted
    assert np.array_equal(bits(b), bits(a[pk][:, pw]))
    rep = m.transmission(k[[ik, 0, ik]], om[[iw, iw, 2, iw]], eta, fd, device=dev)                      # repeated k and omega
    for i in (0, 2):
        for j in (0, 1, 3):
            assert np.array_equal(bits(rep[i, j]), bits(a[ik, iw]))
    for side in range(2):
        s = m.lead_self_energy(k, om, eta, fd, side)
        s1 = m.lead_self_energy(k[ik:ik + 1], om[iw:iw + 1], eta, fd, side)
        assert np.array_equal(bits(s1[0, 0]), bits(s[ik, iw]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["haldane0", "kane_mele", "rand2d_spin", "cubic16", "n36"])
@pytest.mark.parametrize("stop", [{}, dict(tol=0.0, max_iter=3)])
def test_leads_and_surface_run_one_decimation(gpu_ctx, name, stop):
    """The surface unit and this one must decimate alike (the surface unit's workgroup kernel holds a copy of the shared loop): the
    step counts of the two are the same integers at every point, in every storage regime (a lane per problem, P = 16, P = 4, 256
    threads per problem, the workspace).  It guards against the two drifting apart later; it holds before the code was shared too."""
    m, fd = model(name)
    k, om, eta = kpts(name, 7), OMEGA13, eta_of(name)
    _, surface = m.surface_spectral(k, om, eta, fd, return_info=True, **stop)
    _, leads = m.transmission(k, om, eta, fd, return_info=True, **stop)
    assert surface.shape == leads.shape == (7, 13) and surface.dtype == leads.dtype == np.int32
    assert np.array_equal(surface, leads)
    if stop:
        assert np.all(leads == 3)
    else:
        assert leads.min() >= 1 and leads.max() < 50


@pytest.mark.gpu
def test_a_point_across_the_chunk_boundary(gpu_ctx):
    """A chunk holds at most 2^20 (k, omega) problems: 17 k x 65 536 omega of the Haldane model are two chunks (16 k + 1 k)."""
    m, fd = model("haldane0")
    dev = device("haldane0", 1)
    rng = np.random.default_rng(5)
    om = rng.uniform(-3.5, 3.5, 65536)                     # unsorted
    k = rng.random((17, 1))
    a = m.transmission(k, om, 0.004, fd, device=dev)
    assert a.shape == (17, 65536) and np.all(np.isfinite(a)) and a.min() > -1e-12
    for ik, iw in ((16, 777), (15, 65535), (0, 0)):
        alone = m.transmission(k[ik:ik + 1], om[iw:iw + 1], 0.004, fd, device=dev)
        assert np.array_equal(bits(alone[0, 0]), bits(a[ik, iw]))
    one_k = m.transmission(k[16:17], om, 0.004, fd, device=dev)
    assert np.array_equal(bits(one_k[0]), bits(a[16]))
    want, _ = lr.transmission(m, k[16:17], om[:40], 0.004, fd, dev)
    assert relerr(a[16:17, :40], want, 1.0) < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("name,mesh", [("kane_mele", [9]), ("rand3d", [4, 5]), ("n36", [3])])
def test_conductance_mesh_is_the_mean_of_the_list(gpu_ctx, name, mesh):
    m, fd = model(name)
    dev = device(name, 2)
    om, eta = OMEGA13[[1, 4, 5, 8, 11]], eta_of(name)
    g = m.conductance_mesh(mesh, om, eta, fd, device=dev)
    assert g.shape == (5,) and g.dtype == float
    assert np.array_equal(bits(g), bits(m.conductance_mesh(mesh, om, eta, fd, device=dev)))
    t = m.transmission(sr.surface_mesh(m, mesh, fd), om, eta, fd, device=dev)
    assert relerr(g, t.mean(axis=0)) < 1e-12
    g0 = m.conductance_mesh(mesh, om, eta, fd)
    assert relerr(g0, m.transmission(sr.surface_mesh(m, mesh, fd), om, eta, fd).mean(axis=0)) < 1e-12


@pytest.mark.gpu
def test_conductance_mesh_over_two_chunks(gpu_ctx):
    m, fd = model("haldane0")
    dev = device("haldane0", 1)
    om = np.random.default_rng(6).uniform(-3.5, 3.5, 65536)
    g = m.conductance_mesh([17], om, 0.004, fd, device=dev)
    assert g.shape == (65536,)
    assert np.array_equal(bits(g), bits(m.conductance_mesh([17], om, 0.004, fd, device=dev)))
    t = m.transmission(sr.surface_mesh(m, [17], fd), om, 0.004, fd, device=dev)
    assert relerr(g, t.mean(axis=0)) < 1e-12


@pytest.mark.gpu
def test_non_convergence_is_reported(gpu_ctx):
    m, fd = model("haldane0")
    k, om = K7.reshape(-1, 1), OMEGA13
    with pytest.raises(Exception, match="91 of 91 .* did not reach tol"):
        m.transmission(k, om, 0.004, fd, device=device("haldane0", 2), max_iter=1)
    with pytest.raises(Exception, match="91 of 91 .* did not reach tol"):
        m.lead_self_energy(k, om, 0.004, fd, 0, max_iter=1)
    cm, cfd = model("rand2d_spin")                                     # the workgroup kernel reports the same way
    with pytest.raises(Exception, match="6 of 6 .* did not reach tol"):
        cm.transmission(kpts("rand2d_spin", 2), om[:3], 0.01, cfd, device=device("rand2d_spin", 2), max_iter=1)
    with pytest.raises(Exception, match="did not reach tol"):
        cm.conductance_mesh([3], om[:3], 0.01, cfd, max_iter=1)
