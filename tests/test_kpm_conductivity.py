"""Kernel polynomial Kubo-Bastin conductivity on the sparse operator (tb_model.kpm_double_moments, kpm_conductivity,
kpm_conductivity_reconstruct).  The CPU tests check the NumPy restatement kpm_cond_ref.py -- the dense
recursion against the eigendecomposition, the Hall plateau of a Haldane supercell, its sign against the Chern number, the trace
symmetries; the GPU tests check the device moments against the restatement with the same vectors, scaled by ||V^a||_2 ||V^b||_2
(the size the moments can reach), against the eigen form, the plateau from device moments and the stochastic trace."""
import functools

import numpy as np
import pytest

import helpers as hp
import kpm_cond_ref as kc
import test_kpm as tk
from helpers import quiet

import pythtb_amd as tb

TOL = 1e-12          # the project's parity bound, times ||V^a||_2 ||V^b||_2
TM = 16              # moments per tile of the device contraction (KPMC_TM)
NVECS = (1, 3, 8, 9)
NMOMS = (1, 2, 3, TM - 1, TM, TM + 1, 65)
T = tb.tb_model
GAP_ENERGIES = (-0.2, 0.0, 0.2, 0.4)       # inside the gap (-0.667, 0.667) of the Haldane model below
SIGN = -1.0                                # sigma_01(gap) = SIGN * C, the docstring of kpm_conductivity


def chain_ring(nsites):
    """the chain of test_kpm.chain_cut as a periodic supercell of nsites orbitals (dim_k = 1: the velocity needs a periodic axis)"""
    m = quiet(T, 1, 1, [[1.0]], [[0.0]])
    m.set_onsite([0.3])
    m.set_hop(-0.8, 0, 0, [1])
    return quiet(m.make_supercell, [[nsites]])


@functools.lru_cache(maxsize=None)
def model(name):
    if name in ("chain63", "chain64", "chain65"):
        return chain_ring(int(name[5:]))
    return tk.model(name)


@functools.lru_cache(maxsize=None)
def hall_model(sign=1, W=0.0):
    """the Haldane model of the README example (t = -1, t2 = 0.15 e^{+-i pi/2}, on-site -+0.2) and its 10 x 10 supercell (200
    states), with box disorder of width W on the on-site energies"""
    prim = hp.haldane(T, delta=0.2)
    if sign < 0:
        for hop in prim._hoppings:
            hop[0] = np.conj(hop[0])
        prim.invalidate_device_cache()
    sc = quiet(prim.make_supercell, [[10, 0], [0, 10]])
    if W > 0.0:
        eps = np.random.default_rng(41).uniform(-0.5 * W, 0.5 * W, sc._nsta)
        sc.set_onsite(list(eps), mode="add")
    return prim, sc


@functools.lru_cache(maxsize=None)
def hall_reference(sign=1, W=0.0, M=256):
    """(bounds = spectrum +- 0.3, exact trace moments (M, M) at Gamma, ||V^0||_2 ||V^1||_2) of the supercell"""
    _, sc = hall_model(sign, W)
    H, Va, Vb = kc.operators(sc, [0.0, 0.0], (0, 1))
    w = np.linalg.eigvalsh(H)
    bnd = (w[0] - 0.3, w[-1] + 0.3)
    return bnd, kc.double_moments_eigen(H, Va, Vb, M, bnd), np.linalg.norm(Va, 2) * np.linalg.norm(Vb, 2)


@functools.lru_cache(maxsize=None)
def hall_weights(bnd, M=256):
    return kc.conductivity_weights(M, GAP_ENERGIES, bnd)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_ref_recursion_matches_eigen_form():
    """(i) against (ii) on the 6 x 6 Haldane supercell (72 states) at a generic k, unit vectors at every state and three random
    vectors, M = 65 (the largest of the device test) and 256.  The worst difference over ||V^a||_2 ||V^b||_2 is the floor the
    device tolerance of 1e-12 is judged against: measured 1.8e-15 at M = 65 and 6.4e-15 at M = 256 (printed)."""
    m = model("haldane6x6")
    H, Va, Vb = kc.operators(m, [0.137, 0.731], (0, 1))
    bnd = tk.default_bounds(m)
    scale = np.linalg.norm(Va, 2) * np.linalg.norm(Vb, 2)
    rng = np.random.default_rng(3)
    rand = rng.standard_normal((3, m._nsta)) + 1j * rng.standard_normal((3, m._nsta))
    for M in (65, 256):
        V = np.concatenate([np.identity(m._nsta), rand])
        got = kc.double_moments_recursion(H, Va, Vb, V, M, bnd)
        ref = kc.double_moments_eigen(H, Va, Vb, M, bnd, vectors=V)
        floor = np.abs(got - ref).max() / scale
        print("haldane6x6: M = %d, worst |recursion - eigen| / (|Va| |Vb|) = %.2e" % (M, floor))
        assert floor < TOL
        # the trace form of (ii) is the mean of the unit-vector moments
        assert np.abs(got[:m._nsta].mean(axis=0) - kc.double_moments_eigen(H, Va, Vb, M, bnd)).max() < TOL * scale
        assert np.abs(got).max() <= scale * (1.0 + 1e-9)


@pytest.mark.parametrize("W", [0.0, 1.0])
def test_hall_plateau_from_exact_moments(W):
    """kpm_conductivity_reconstruct on the exact trace moments of the 10 x 10 Haldane supercell at Gamma, M = 256, Jackson kernel:
    |sigma_01| within 5e-3 of 1 at four Fermi levels in the gap (measured 1.1e-3 clean, 1.4e-3 with W = 1), |Im G| < 1e-6; and the
    same numbers from the explicit weights of the restatement."""
    bnd, mu, _ = hall_reference(1, W)
    G = tb.kpm_conductivity_reconstruct(mu, GAP_ENERGIES, bnd)
    sigma = 200 * G.real
    print("W = %g: sigma_01 =" % W, sigma, " max |Im G| = %.1e" % np.abs(G.imag).max())
    assert np.abs(np.abs(sigma) - 1.0).max() < 5e-3
    assert np.abs(G.imag).max() < 1e-6
    assert np.abs(G - np.einsum("emn,mn->e", hall_weights(bnd), mu)).max() < 1e-10
    # a stack of moment sets, and the thermal occupation tending to the step
    both = tb.kpm_conductivity_reconstruct(np.stack([mu, 0.5 * mu]), GAP_ENERGIES, bnd)
    assert both.shape == (2, 4) and np.abs(both[1] - 0.5 * both[0]).max() < 1e-14
    assert np.abs(200 * tb.kpm_conductivity_reconstruct(mu, GAP_ENERGIES, bnd, kT=0.01).real - sigma).max() < 5e-3
    for bad in ([bnd[0]], [bnd[1]], [bnd[1] + 1.0], [0.0, bnd[0] - 1e-9]):
        with pytest.raises(Exception, match="open interval"):
            tb.kpm_conductivity_reconstruct(mu, bad, bnd)
    with pytest.raises(Exception, match="kernel"):
        tb.kpm_conductivity_reconstruct(mu, [0.0], bnd, "fejer")
    with pytest.raises(Exception, match=r"\(\.\.\., M, M\)"):
        tb.kpm_conductivity_reconstruct(mu[:, :5], [0.0], bnd)


def test_hall_sign():
    """sigma_01 in the gap flips with t2 -> conj(t2) and equals SIGN * C, C the Chern number of the lower band in the convention
    of tb_model.berry_curvature (restated on the host, 24 x 24 mesh)."""
    for sign in (1, -1):
        prim, _ = hall_model(sign)
        bnd, mu, _ = hall_reference(sign)
        C = kc.chern_number(prim, [0], 24)
        sigma = 200 * tb.kpm_conductivity_reconstruct(mu, [0.0], bnd).real[0]
        print("t2 phase %+d pi/2: C = %.6f, sigma_01(0) = %.6f" % (sign, C, sigma))
        assert abs(C + sign) < 1e-6            # C = -1 for t2 = 0.15 e^{+i pi/2}
        assert abs(sigma - SIGN * C) < 5e-3


def test_trace_symmetries():
    """exact trace: mu^{ab}_mn = conj(mu^{ab}_nm) (cyclicity and Hermiticity of the four operators); mu^{aa} real and symmetric"""
    m = model("haldane6x6")
    bnd = tk.default_bounds(m)
    eye = np.identity(m._nsta)
    for dirs in ((0, 1), (1, 0), (1, 1)):
        H, Va, Vb = kc.operators(m, [0.21, 0.4], dirs)
        scale = np.linalg.norm(Va, 2) * np.linalg.norm(Vb, 2)
        mu = kc.double_moments_recursion(H, Va, Vb, eye, 40, bnd).mean(axis=0)
        assert np.abs(mu - mu.conj().T).max() < TOL * scale
        if dirs[0] == dirs[1]:
            assert np.abs(mu.imag).max() < TOL * scale and np.abs(mu - mu.T).max() < TOL * scale


def test_host_generator_is_unimodular():
    v = kc.random_phase_vectors(7, 2, 3, 50)
    assert v.shape == (3, 50) and np.abs(np.abs(v) - 1.0).max() < 1e-15
    assert len(set(v.reshape(-1).tolist())) == 150


# ---------------------------------------------------------------------------------------------------------------- GPU
GPU_CASES = [("chain63", 1, (0, 0)), ("chain64", 1, (0, 0)), ("chain65", 1, (0, 0)), ("haldane", 5, (0, 1)), ("haldane", 5, (1, 0)),
             ("haldane", 5, (1, 1)), ("kane_mele", 3, (0, 1)), ("haldane6x6", 3, (0, 1)), ("cubic16x2", 2, (0, 2)),
             ("isolated", 2, (0, 0))]


@functools.lru_cache(maxsize=None)
def case_operators(name, nk, dirs):
    """(k list, bounds, [(H, V^a, V^b)] per k, [||V^a||_2 ||V^b||_2] per k)"""
    m = model(name)
    k = tk.kpoints(m, nk)
    ops = [kc.operators(m, k[q], dirs) for q in range(nk)]
    return k, tk.default_bounds(m), ops, [np.linalg.norm(o[1], 2) * np.linalg.norm(o[2], 2) for o in ops]


@functools.lru_cache(maxsize=None)
def case_reference(name, nk, dirs):
    """supplied vectors (9, n) and their reference moments (nk, 9, 65, 65), computed once per case"""
    m = model(name)
    _, bnd, ops, _ = case_operators(name, nk, dirs)
    rng = np.random.default_rng(17)
    V = rng.standard_normal((max(NVECS), m._nsta)) + 1j * rng.standard_normal((max(NVECS), m._nsta))
    return V, np.stack([kc.double_moments_recursion(H, Va, Vb, V, max(NMOMS), bnd) for H, Va, Vb in ops])


@pytest.mark.gpu
@pytest.mark.parametrize("name,nk,dirs", GPU_CASES)
def test_double_moments_supplied_vectors(name, nk, dirs, gpu_ctx):
    m = model(name)
    k, bnd, _, scale = case_operators(name, nk, dirs)
    V, ref = case_reference(name, nk, dirs)
    worst = 0.0
    for nvec in NVECS:
        for M in NMOMS:
            mu, got_bnd = m.kpm_double_moments(M, dirs, k, vectors=V[:nvec])
            assert got_bnd == pytest.approx(bnd, rel=1e-14)
            assert mu.shape == (nk, nvec, M, M) and mu.dtype == np.complex128
            for q in range(nk):
                worst = max(worst, np.abs(mu[q] - ref[q, :nvec, :M, :M]).max() / scale[q])
    print("%s %s: worst |device - reference| / (|Va| |Vb|) = %.2e" % (name, dirs, worst))
    assert worst <= TOL


@pytest.mark.gpu
@pytest.mark.parametrize("name,nk,dirs", GPU_CASES)
def test_double_moments_device_vectors(name, nk, dirs, gpu_ctx):
    """the random-phase vectors of the device, read back by kpm_vectors: the k-point with index q uses numbers q nvec + v"""
    m = model(name)
    k, bnd, ops, scale = case_operators(name, nk, dirs)
    seed = 20240229
    pool = m.kpm_vectors(max(NVECS) * nk, seed=seed)
    assert np.abs(pool - kc.random_phase_vectors(seed, 0, len(pool), m._nsta)).max() < 1e-14      # the host restatement
    ref = np.stack([kc.double_moments_recursion(H, Va, Vb, pool, max(NMOMS), bnd) for H, Va, Vb in ops])
    worst = 0.0
    for nvec in NVECS:
        for M in NMOMS:
            mu, _ = m.kpm_double_moments(M, dirs, k, n_vectors=nvec, seed=seed)
            for q in range(nk):
                worst = max(worst, np.abs(mu[q] - ref[q, q * nvec:(q + 1) * nvec, :M, :M]).max() / scale[q])
    print("%s %s: worst |device - reference| / (|Va| |Vb|) = %.2e" % (name, dirs, worst))
    assert worst <= TOL


@pytest.mark.gpu
def test_unit_vectors_against_eigen_form(gpu_ctx):
    """states= on the 6 x 6 Haldane supercell (72 states) against the eigendecomposition: independent of the reference recursion;
    and the velocity operator of the restatement against _gen_dham"""
    m = model("haldane6x6")
    k = tk.kpoints(m, 2)
    bnd = tk.default_bounds(m)
    states = [0, 1, 17, 35, 36, 37, 70, 71, 5]
    mu, _ = m.kpm_double_moments(65, (0, 1), k, states=states)
    assert mu.shape == (2, len(states), 65, 65)
    for q in range(2):
        H, Va, Vb = kc.operators(m, k[q], (0, 1))
        assert np.abs(Va - m._gen_dham(k[q], 0)).max() < 1e-12 and np.abs(Vb - m._gen_dham(k[q], 1)).max() < 1e-12
        scale = np.linalg.norm(Va, 2) * np.linalg.norm(Vb, 2)
        ref = kc.double_moments_eigen(H, Va, Vb, 65, bnd, vectors=np.identity(m._nsta)[states])
        err = np.abs(mu[q] - ref).max() / scale
        print("unit vectors, k %d: worst |device - eigen| / (|Va| |Vb|) = %.2e" % (q, err))
        assert err <= TOL


@pytest.mark.gpu
def test_two_calls_same_bits(gpu_ctx):
    m = model("haldane6x6")
    k = tk.kpoints(m, 2)
    a, _ = m.kpm_double_moments(33, (0, 1), k, n_vectors=9, seed=5)
    b, _ = m.kpm_double_moments(33, (0, 1), k, n_vectors=9, seed=5)
    assert np.array_equal(a, b)
    big = model("chain65")                                      # more rows than one row tile of the contraction
    a, _ = big.kpm_double_moments(17, (0, 0), [[0.3]], n_vectors=3, seed=5)
    assert np.array_equal(a, big.kpm_double_moments(17, (0, 0), [[0.3]], n_vectors=3, seed=5)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("sign", [1, -1])
def test_hall_plateau_exact_trace_on_device(sign, gpu_ctx):
    """the 10 x 10 Haldane supercell at Gamma, states=range(200), M = 256: sigma from the device moments against sigma from the
    reference moments within 200 sum_mn |W_mn(E)| 1e-12 ||V^a|| ||V^b|| (W the reconstruction's linear weights: the bound of the
    moment test carried through), and sigma_01(gap) = SIGN * C with C from berry_curvature_mesh of the primitive model"""
    prim, sc = hall_model(sign)
    bnd, mu_ref, scale = hall_reference(sign)
    E = np.array(GAP_ENERGIES)
    mu, got_bnd = sc.kpm_double_moments(256, (0, 1), [[0.0, 0.0]], states=range(200), bounds=bnd)
    assert got_bnd == bnd
    sig_dev = 200 * tb.kpm_conductivity_reconstruct(mu[0].mean(axis=0), E, bnd).real
    sig_ref = 200 * tb.kpm_conductivity_reconstruct(mu_ref, E, bnd).real
    bound = 200 * np.abs(hall_weights(bnd)).sum(axis=(1, 2)) * TOL * scale
    print("sigma_01 device", sig_dev, "reference", sig_ref, "|difference|", np.abs(sig_dev - sig_ref), "bound", bound)
    assert np.all(np.abs(sig_dev - sig_ref) <= bound)
    assert np.array_equal(sig_dev, sc.kpm_conductivity(E, 256, (0, 1), [[0.0, 0.0]], states=range(200), bounds=bnd))
    C = prim.berry_curvature_mesh([64, 64], occ=[0], dirs=(0, 1)) / (2.0 * np.pi)
    print("C = %.9f" % C)
    assert abs(C + sign) < 1e-6
    assert np.abs(sig_dev - SIGN * C).max() < 5e-3


STOCH_SEED = 3


@pytest.mark.gpu
def test_stochastic_trace(gpu_ctx):
    """the supercell with box disorder W = 1, 16 random-phase vectors of a fixed seed, M = 128: sigma_01(0) within 4 reported
    standard errors of the exact trace of the same model (the seed was chosen so that the dense restatement on the same vectors,
    kc.random_phase_vectors, satisfies this on the host: 1.0270 +- 0.0209 against the exact 1.0105, 0.8 standard errors)"""
    _, sc = hall_model(1, 1.0)
    bnd, mu_exact, scale = hall_reference(1, 1.0, 128)
    exact = 200 * tb.kpm_conductivity_reconstruct(mu_exact, [0.0], bnd).real[0]
    sigma, err = sc.kpm_conductivity([0.0], 128, (0, 1), [[0.0, 0.0]], n_vectors=16, seed=STOCH_SEED, bounds=bnd, return_error=True)
    H, Va, Vb = kc.operators(sc, [0.0, 0.0], (0, 1))
    each = 200 * tb.kpm_conductivity_reconstruct(kc.double_moments_recursion(H, Va, Vb, sc.kpm_vectors(16, seed=STOCH_SEED), 128, bnd),
                                                 [0.0], bnd).real[:, 0]
    print("sigma_01(0): exact %.6f, device %.6f +- %.6f, restatement %.6f +- %.6f" %
          (exact, sigma[0], err[0], each.mean(), each.std(ddof=1) / 4.0))
    assert err[0] > 0.0 and abs(sigma[0] - exact) <= 4.0 * err[0]
    assert abs(sigma[0] - each.mean()) < 1e-9 and abs(err[0] - each.std(ddof=1) / 4.0) < 1e-9


@pytest.mark.gpu
def test_errors(gpu_ctx):
    m = model("haldane")
    k = np.array([[0.0, 0.0], [0.1, 0.05]])
    V = np.ones((2, 2), dtype=complex)
    with pytest.raises(tb._lib.TbkError, match=r"bounds \(-1, 1\) do not contain the spectrum \(Gershgorin interval"):
        m.kpm_double_moments(64, (0, 1), k, vectors=V, bounds=(-1, 1))
    mu, bnd = m.kpm_double_moments(8, (0, 1), k, vectors=V)    # the context is as good as new
    H, Va, Vb = kc.operators(m, k[1], (0, 1))
    assert np.abs(mu[1] - kc.double_moments_recursion(H, Va, Vb, V, 8, bnd)).max() <= TOL * np.linalg.norm(Va, 2) * np.linalg.norm(Vb, 2)
    bad = [
        (dict(dirs=(0, 2)), "dirs"),
        (dict(dirs=(-1, 0)), "dirs"),
        (dict(dirs=(0,)), "dirs"),
        (dict(dirs=(0, 1), vectors=V, states=[0]), "not both"),
        (dict(dirs=(0, 1), states=[2]), "out of range"),
        (dict(dirs=(0, 1), n_vectors=0), "n_vectors"),
        (dict(dirs=(0, 1), bounds=(1.0, 1.0)), "bounds"),
    ]
    for kw, text in bad:
        with pytest.raises(Exception, match=text):
            m.kpm_double_moments(8, k_list=k, **kw)
    with pytest.raises(Exception, match="n_moments"):
        m.kpm_double_moments(0, (0, 1), k)
    with pytest.raises(Exception, match="dim_k >= 1"):
        tk.model("flake0").kpm_double_moments(8, (0, 0), None)
    with pytest.raises(Exception, match="dim_k >= 1"):
        tk.model("flake0").kpm_conductivity([0.0], 8, (0, 0), None)
    with pytest.raises(Exception, match="open interval"):
        m.kpm_conductivity([9.0], 8, (0, 1), k, n_vectors=2)
    with pytest.raises(Exception, match="dirs"):
        m.kpm_conductivity([0.0], 8, (0, 3), k)
