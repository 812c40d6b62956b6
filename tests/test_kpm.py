"""Kernel polynomial DOS / LDOS on the sparse operator (tb_model.kpm_moments, kpm_vectors, kpm_dos, kpm_ldos, kpm_reconstruct;
DESIGN.md section 21).  The CPU tests check the NumPy restatement kpm_ref.py against exact eigen-moments, the host assembly of the
CSR operator against the dense H(k) of the oracle, and the reconstruction against Chebyshev-Gauss quadrature; the GPU tests check
the device moments against the restatement with the same vectors (moments satisfy |mu| <= 1: absolute bounds), against the exact
eigen-moments, past the dense limit of 2048 states, and the generator's and the error paths' contracts."""
import ctypes as C
import functools
import time

import numpy as np
import pytest

import helpers as hp
import kpm_ref as kr
from helpers import quiet
from oracle import tb_oracle as orc

import pythtb_amd as tb

TOL = 1e-12          # the project's eigenvalue parity bound
NVECS = (1, 3, 8, 9)
NMOMS = (1, 2, 3, 64, 257)
T = tb.tb_model


def dense_ham(m, k=None):
    return np.asarray(orc.gen_ham(m, k)).reshape(m._nsta, m._nsta)


def flake(m, nx, ny):
    return quiet(lambda: m.cut_piece(nx, 0, glue_edgs=False).cut_piece(ny, 1, glue_edgs=False))


def chain_cut(nsites):
    m = quiet(T, 1, 1, [[1.0]], [[0.0]])
    m.set_onsite([0.3])
    m.set_hop(-0.8, 0, 0, [1])
    return quiet(m.cut_piece, nsites, 0)


def isolated_model():
    """three orbitals per cell, the last one with zero on-site energy and no hopping: an empty CSR row"""
    m = quiet(T, 1, 1, [[1.0]], [[0.0], [0.4], [0.7]])
    m.set_onsite([0.3, -0.2, 0.0])
    m.set_hop(-1.0, 0, 1, [0])
    m.set_hop(0.5 + 0.2j, 1, 0, [1])
    return m


def random_repeats(nspin, seed):
    """hp.random_model with repeated (i, j, R) hops and R = 0 self-pairs appended to the table"""
    m = hp.random_model(T, 4, 2, nspin, seed=seed, rmax=2)
    rng = np.random.default_rng(seed + 100)
    for h in (0, 3, 3, 5):
        m._hoppings.append(list(m._hoppings[h]))
    for i in (0, 2):
        amp = complex(rng.standard_normal(), rng.standard_normal()) if nspin == 1 else \
            rng.standard_normal((2, 2)) + 1j * rng.standard_normal((2, 2))
        m._hoppings.append([amp, i, i, np.array([0, 0])])
    m.invalidate_device_cache()
    return m


@functools.lru_cache(maxsize=None)
def model(name):
    return {
        "haldane": lambda: hp.haldane(T, delta=0.2),
        "kane_mele": lambda: hp.kane_mele(T),
        "cubic16": lambda: hp.cubic16(T),
        "chain3": lambda: hp.chain3(T, -1.0, 0.4, 0.3),
        "random": lambda: random_repeats(1, 11),
        "random_spin": lambda: random_repeats(2, 12),
        "flake0": lambda: flake(hp.haldane(T, delta=0.2), 3, 4),          # dim_k = 0
        "isolated": isolated_model,
        "chain63": lambda: chain_cut(63),
        "chain64": lambda: chain_cut(64),
        "chain65": lambda: chain_cut(65),
        "haldane6x6": lambda: quiet(hp.haldane(T, delta=0.2).make_supercell, [[6, 0], [0, 6]]),      # 72 states, dim_k = 2
        "cubic16x2": lambda: quiet(hp.cubic16(T).make_supercell, [[2, 0, 0], [0, 1, 0], [0, 0, 1]]),   # 32 states, long rows
        "flake7x9": lambda: flake(hp.haldane(T, delta=0.2), 7, 9),        # 126 states
        "flake10x12": lambda: flake(hp.haldane(T, delta=0.2), 10, 12),    # 240 states
    }[name]()


def kpoints(m, nk, seed=5):
    if m._dim_k == 0:
        return None
    return np.random.default_rng(seed).random((nk, m._dim_k))


def default_bounds(m):
    lo, hi = kr.gershgorin(kr.flatten_host(m))
    pad = 0.01 * (hi - lo)
    return lo - pad, hi + pad


# ---------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("name,M", [("flake7x9", 257), ("flake10x12", 1024)])
def test_ref_recursion_matches_exact_eigen_moments(name, M):
    """The restatement's recursion (with the doubling identities) against mu^(i)_m = sum_j |U_ij|^2 T_m(x_j), per site, on open
    Haldane flakes, bound 1e-12.  Measured with NumPy alone: worst error 1.4e-14 for the 7 x 9-cell flake (126 states) at M = 257
    and 4.4e-14 for the 10 x 12-cell flake (240 states) at M = 1024; this test prints the figure it finds (the same order)."""
    m = model(name)
    H = dense_ham(m)
    bnd = default_bounds(m)
    got = kr.moments_recursion(H, np.identity(m._nsta), M, bnd)
    ref = kr.moments_exact(H, M, bnd)
    err = np.abs(got - ref).max()
    print("%s: n = %d, M = %d, worst |recursion - exact| = %.2e" % (name, m._nsta, M, err))
    assert err < TOL
    # the trace form
    assert abs(got.mean(axis=0) - ref.mean(axis=0)).max() < TOL
    # arbitrary vectors
    V = np.random.default_rng(1).standard_normal((3, m._nsta)) + 1j * np.random.default_rng(2).standard_normal((3, m._nsta))
    assert np.abs(kr.moments_recursion(H, V, 64, bnd) - kr.moments_exact_vectors(H, V, 64, bnd)).max() < TOL


@pytest.mark.parametrize("name", ["haldane", "kane_mele", "cubic16", "chain3", "random", "random_spin", "flake0", "isolated"])
def test_flatten_host_matches_gen_ham(name):
    m = model(name)
    op = kr.flatten_host(m)
    n = m._nsta
    rp, col, R = op["row_ptr"], op["col"], op["R"]
    assert rp[0] == 0 and rp[-1] == len(col) and np.all(np.diff(rp) >= 0)
    assert np.all((col >= 0) & (col < n)) and np.all(R[:, m._dim_k:] == 0)
    assert not np.any((op["amp"].real == 0) & (op["amp"].imag == 0))
    entries = {}
    for a in range(n):
        keys = [(int(col[e]),) + tuple(int(x) for x in R[e]) for e in range(rp[a], rp[a + 1])]
        assert keys == sorted(keys), "row %d: (col, R) not ascending" % a
        assert len(set(keys)) == len(keys), "row %d: repeated (col, R)" % a
        for e, key in zip(range(rp[a], rp[a + 1]), keys):
            entries[(a,) + key] = op["amp"][e]
        if m._dim_k == 0:
            assert len(set(k_[0] for k_ in keys)) == len(keys)
    for (a, b, r0, r1, r2, r3), amp in entries.items():            # every entry has its conjugate partner
        assert abs(entries[(b, a, -r0, -r1, -r2, -r3)] - np.conj(amp)) <= 1e-15 * np.abs(op["amp"]).max()
    if name == "isolated":
        assert rp[3] == rp[2]                                       # the empty row
    lo, hi = op["gersh"]
    assert (lo, hi) == pytest.approx(kr.gershgorin(op), rel=1e-15, abs=1e-15)
    ks = [None] if m._dim_k == 0 else list(kpoints(m, 3))
    for k in ks:
        H = dense_ham(m, k)
        assert np.abs(kr.csr_to_dense(op, k) - H).max() <= 1e-14 * np.abs(H).max()
        w = np.linalg.eigvalsh(H)
        assert lo <= w[0] and w[-1] <= hi


@pytest.mark.parametrize("kernel", ["jackson", "lorentz", None])
def test_reconstruct_quadrature(kernel):
    """On the Chebyshev-Gauss nodes (N > M) the quadrature of rho T_n is exact for n < 2 N - M: the integral is g_0 mu_0 and the
    first energy moment a g_1 mu_1 + b, both to 1e-12 (M = 48, N = 64: the rounding of cos(m arccos x) stays below 1e-13)."""
    M, N = 48, 64
    rng = np.random.default_rng(3)
    w = np.sort(rng.uniform(-2.0, 3.0, 40))                     # a spectrum inside the bounds
    bnd = (-2.6, 3.3)
    a, b = 0.5 * (bnd[1] - bnd[0]), 0.5 * (bnd[1] + bnd[0])
    mu = kr.chebyshev_T((w - b) / a, M).mean(axis=1)
    x, E = kr.gauss_nodes(N, bnd)
    g = kr.kernel_coefficients(M, kernel)
    for rec in (tb.kpm_reconstruct, kr.reconstruct):
        rho = rec(mu, E, bnd, kernel)
        wq = (np.pi / N) * np.sqrt(1.0 - x * x) * a
        assert abs(np.sum(wq * rho) - g[0] * mu[0]) < 1e-12
        assert abs(np.sum(wq * rho * E) - (a * g[1] * mu[1] + b)) < 1e-12
        if kernel == "jackson":
            assert rho.min() >= 0.0
    assert np.abs(tb.kpm_reconstruct(mu, E, bnd, kernel) - kr.reconstruct(mu, E, bnd, kernel)).max() < 1e-12
    # a stack of moment sets
    both = tb.kpm_reconstruct(np.stack([mu, 0.5 * mu]), E, bnd, kernel)
    assert both.shape == (2, N) and np.abs(both[1] - 0.5 * both[0]).max() < 1e-14
    for bad in ([bnd[0]], [bnd[1]], [bnd[1] + 1.0], [0.0, bnd[0] - 1e-9]):
        with pytest.raises(Exception, match="open interval"):
            tb.kpm_reconstruct(mu, bad, bnd, kernel)
    with pytest.raises(Exception, match="kernel"):
        tb.kpm_reconstruct(mu, E, bnd, "fejer")


def test_jackson_nonnegative_on_fine_grid():
    M = 64
    bnd = (-1.5, 2.5)
    a, b = 2.0, 0.5
    w = np.array([-1.2, -1.2, 0.0, 0.7, 2.3])
    mu = kr.chebyshev_T((w - b) / a, M).mean(axis=1)
    E = np.linspace(bnd[0], bnd[1], 2003)[1:-1]
    assert tb.kpm_reconstruct(mu, E, bnd, "jackson").min() >= 0.0
    assert tb.kpm_reconstruct(mu, E, bnd, None).min() < 0.0     # the bare series is not


# ---------------------------------------------------------------------------------------------------------------- GPU
GPU_CASES = [("chain63", 1), ("chain64", 1), ("chain65", 1), ("haldane", 5), ("chain3", 2), ("kane_mele", 3), ("haldane6x6", 3),
             ("cubic16x2", 2), ("isolated", 2), ("flake0", 1)]


@functools.lru_cache(maxsize=None)
def case_reference(name, nk):
    """(k list, bounds, supplied vectors (9, n), their reference moments (nk, 9, 257)), computed once per case"""
    m = model(name)
    k = kpoints(m, nk)
    bnd = default_bounds(m)
    rng = np.random.default_rng(17)
    V = rng.standard_normal((max(NVECS), m._nsta)) + 1j * rng.standard_normal((max(NVECS), m._nsta))
    hams = [dense_ham(m, None if k is None else k[q]) for q in range(nk)]
    ref = np.stack([kr.moments_recursion(H, V, max(NMOMS), bnd) for H in hams])
    return k, bnd, V, ref, hams


@pytest.mark.gpu
@pytest.mark.parametrize("name,nk", GPU_CASES)
def test_moments_supplied_vectors(name, nk, gpu_ctx):
    m = model(name)
    k, bnd, V, ref, _ = case_reference(name, nk)
    worst = 0.0
    for nvec in NVECS:
        for M in NMOMS:
            mu, got_bnd = m.kpm_moments(M, k, vectors=V[:nvec])
            assert got_bnd == pytest.approx(bnd, rel=1e-14)
            mu = mu.reshape(nk, nvec, M)
            assert mu.shape == (nk, nvec, M)
            worst = max(worst, np.abs(mu - ref[:, :nvec, :M]).max())
    print("%s: worst |device - reference| = %.2e" % (name, worst))
    assert worst < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("name,nk", GPU_CASES)
def test_moments_device_vectors(name, nk, gpu_ctx):
    """the random-phase vectors of the device, read back by kpm_vectors: the k-point with index q uses numbers q nvec + v"""
    m = model(name)
    k, bnd, _, _, hams = case_reference(name, nk)
    seed = 20240229
    pool = m.kpm_vectors(max(NVECS) * nk, seed=seed)           # numbers 0 .. 9 nk - 1
    ref = np.stack([kr.moments_recursion(H, pool, max(NMOMS), bnd) for H in hams])     # (nk, 9 nk, 257)
    worst = 0.0
    for nvec in NVECS:
        for M in NMOMS:
            mu, _ = m.kpm_moments(M, k, n_vectors=nvec, seed=seed)
            mu = mu.reshape(nk, nvec, M)
            for q in range(nk):
                worst = max(worst, np.abs(mu[q] - ref[q, q * nvec:(q + 1) * nvec, :M]).max())
    print("%s: worst |device - reference| = %.2e" % (name, worst))
    assert worst < TOL


@pytest.mark.gpu
def test_empty_row_negates_previous_vector(gpu_ctx):
    """symmetric bounds (b = 0): the isolated zero-energy orbital has alpha_m+1 = -alpha_m-1, i.e. T_m(0): 1, 0, -1, 0, ..."""
    m = model("isolated")
    mu, _ = m.kpm_moments(9, [[0.3]], states=[2], bounds=(-3.0, 3.0))
    assert np.array_equal(mu[0, 0], np.array([1.0, 0.0, -1.0, 0.0, 1.0, 0.0, -1.0, 0.0, 1.0]))


@pytest.mark.gpu
def test_ldos_moments_against_exact_eigen_moments(gpu_ctx):
    """unit start vectors on the 7 x 9 flake (126 states) against the eigendecomposition: independent of the reference recursion"""
    m = model("flake7x9")
    states = [0, 1, 17, 62, 63, 64, 100, 124, 125]
    mu, bnd = m.kpm_moments(257, states=states)
    assert mu.shape == (len(states), 257)
    ref = kr.moments_exact(dense_ham(m), 257, bnd, states)
    err = np.abs(mu - ref).max()
    print("LDOS moments: worst |device - exact| = %.2e" % err)
    assert err < TOL


@pytest.mark.gpu
def test_generator_contract(gpu_ctx):
    m = model("flake7x9")
    n = m._nsta
    v = m.kpm_vectors(5, seed=7)
    assert v.shape == (5, n) and v.dtype == np.complex128
    assert np.abs(np.abs(v) - 1.0).max() <= 1e-15
    assert len(set(v.reshape(-1).tolist())) == 5 * n                       # all entries differ across index and vector
    assert not np.any(v == m.kpm_vectors(5, seed=8))                       # and across seed
    assert np.array_equal(v[2:], m.kpm_vectors(3, seed=7, first=2))        # a pure function of (seed, number, index)
    mu5, bnd = m.kpm_moments(64, n_vectors=5, seed=7)
    assert np.abs(mu5[:, 0] - 1.0).max() <= 1e-14
    assert np.array_equal(mu5, m.kpm_moments(64, vectors=v)[0])            # same bits from the read-back vectors
    assert np.array_equal(mu5[:3], m.kpm_moments(64, n_vectors=3, seed=7)[0])
    assert np.array_equal(mu5, m.kpm_moments(64, n_vectors=5, seed=7)[0])  # and from run to run
    # with a k list: the second k-point continues the numbering
    h = model("haldane6x6")
    k = kpoints(h, 2)
    mk, _ = h.kpm_moments(33, k, n_vectors=3, seed=7)
    assert np.array_equal(mk[1], h.kpm_moments(33, k[1:], vectors=h.kpm_vectors(3, seed=7, first=3))[0][0])
    assert np.array_equal(mk, h.kpm_moments(33, k, n_vectors=3, seed=7)[0])


@pytest.mark.gpu
def test_two_calls_same_bits(gpu_ctx):
    """the partial sums of a step are added in a fixed order: nine vectors (a full and a short block) at two k-points"""
    m = model("haldane6x6")
    k = kpoints(m, 2)
    a, _ = m.kpm_moments(64, k, n_vectors=9, seed=5)
    b, _ = m.kpm_moments(64, k, n_vectors=9, seed=5)
    assert a.shape == (2, 9, 64) and np.array_equal(a, b)


@functools.lru_cache(maxsize=None)
def ring_reference(ctype=complex):
    """The long ring of kpm_ref.ring_tables at one k with nine supplied vectors, in NumPy: H v = eps v + h roll(v, -1) +
    conj(h) roll(v, 1) with h = hop e^{2 pi i k / n}, and V = dH/dk the hopping part times +- 2 pi i / n.  Returns the arguments
    (tables, k, bounds, vectors, coefficients (2, 4)) and the references: moments (9, 5), series (2, 9, n), double moments (9, 3, 3).
    ctype=np.clongdouble runs the same recursions in extended precision (the check of this float64 reference)."""
    tab = kr.ring_tables()
    n = kr.RING_N
    ftype = np.longdouble if ctype is np.clongdouble else float
    k = 0.3125
    eps = tab["onsite"].real.astype(ftype)
    hop0 = complex(tab["hop_amp"][0])
    lo, hi = eps.min() - 2 * abs(hop0), eps.max() + 2 * abs(hop0)          # the Gershgorin interval, 1 % wider on each side
    bnd = (float(lo - 0.01 * (hi - lo)), float(hi + 0.01 * (hi - lo)))
    a, b = ftype(0.5) * (ftype(bnd[1]) - ftype(bnd[0])), ftype(0.5) * (ftype(bnd[1]) + ftype(bnd[0]))
    two_pi = 8 * np.arctan(ftype(1))
    h = ctype(hop0) * np.exp(ctype(1j) * (two_pi * ftype(k) / n))
    rng = np.random.default_rng(17)
    vec = rng.standard_normal((9, n)) + 1j * rng.standard_normal((9, n))
    coef = rng.standard_normal((2, 4)) + 1j * rng.standard_normal((2, 4))

    def Ht(v):
        return (eps * v + h * np.roll(v, -1, axis=-1) + np.conj(h) * np.roll(v, 1, axis=-1) - b * v) / a

    def Vel(v):
        return ctype(1j) * (two_pi / n) * (h * np.roll(v, -1, axis=-1) - np.conj(h) * np.roll(v, 1, axis=-1))

    def cheb(v, M):
        T = [v, Ht(v)]
        while len(T) < M:
            T.append(2 * Ht(T[-1]) - T[-2])
        return T[:M]

    def dot(x, y):       # pairwise sums over the ring
        return np.sum(np.conj(x) * y, axis=-1)

    v = vec.astype(ctype)
    norm = dot(v, v).real
    T = cheb(v, 5)
    mu = np.stack([dot(v, t).real / norm for t in T], axis=1)
    series = np.stack([sum(ctype(c) * t for c, t in zip(cs, T)) for cs in coef])
    dbl = np.stack([np.stack([dot(v, Vel(tm)) / norm for tm in cheb(Vel(tn), 3)], axis=1) for tn in T[:3]], axis=2)
    return (tab, k, bnd, vec, coef), (mu, series, dbl)


def ring_velocity_bound(tab):
    n, vb = len(tab["orb"]), np.zeros(4)
    tb._lib.check(tb._lib.lib.tbk_sparse_velocity_bounds_host(
        1, n, 1, tb._lib.dptr(tab["orb"]), tb._lib.dptr(tab["onsite"].view(float)), n, tb._lib.iptr(tab["hop_i"]),
        tb._lib.iptr(tab["hop_j"]), tb._lib.iptr(tab["hop_R"].reshape(-1)), tb._lib.dptr(tab["hop_amp"].view(float)), tb._lib.dptr(vb)))
    return vb[0]


def test_ring_reference_against_extended_precision():
    """the float64 reference of test_rows_past_the_grid stays within a tenth of each of its bounds of the same recursions in
    numpy.longdouble (measured: moments 2.3e-16, series 4.7e-16 of max|result|, double moments 2.6e-16 of ||V||^2, each against
    a bound of 1e-12; printed)"""
    (tab, _, _, _, _), (mu, series, dbl) = ring_reference()
    _, (mu_x, series_x, dbl_x) = ring_reference(np.clongdouble)
    e_mu = np.abs(mu - mu_x).max()
    e_series = np.abs(series - series_x).max() / np.abs(series).max()
    e_dbl = np.abs(dbl - dbl_x).max() / ring_velocity_bound(tab) ** 2
    print("ring reference against longdouble: moments %.2e, series %.2e, double moments %.2e" % (e_mu, e_series, e_dbl))
    assert max(e_mu, e_series, e_dbl) <= 0.1 * TOL


@pytest.mark.gpu
def test_rows_past_the_grid(gpu_ctx):
    """A ring of 2048 * 32 + 33 orbitals: more row tiles than the 2048 workgroups of a step, so workgroup 0 strides to a second
    full tile and workgroup 1 to a tail tile of one row -- in every kernel on the row mapping (start vectors, the steps with each
    epilogue).  Moments, a series and double moments of nine supplied vectors against the NumPy ring."""
    (tab, k, bnd, vec, coef), (mu_ref, series_ref, dbl_ref) = ring_reference()
    L, n, nvec = tb._lib, kr.RING_N, len(vec)
    sp = C.c_void_p()
    L.check(L.lib.tbk_sparse_upload(gpu_ctx.handle, 1, n, 1, L.dptr(tab["orb"]), L.dptr(tab["onsite"].view(float)), n,
                                    L.iptr(tab["hop_i"]), L.iptr(tab["hop_j"]), L.iptr(tab["hop_R"].reshape(-1)),
                                    L.dptr(tab["hop_amp"].view(float)), C.byref(sp)))
    try:
        kk, V = np.array([[k]]), L.dptr(vec.view(float))
        mu = np.empty((nvec, 5))
        L.check(L.lib.tbk_kpm_moments(sp, L.dptr(kk), 1, 5, bnd[0], bnd[1], nvec, V, None, 0, L.dptr(mu)))
        out = np.empty((2, nvec, n), dtype=complex)
        L.check(L.lib.tbk_kpm_apply_series(sp, L.dptr(kk), 1, 4, 2, L.dptr(coef.view(float)), bnd[0], bnd[1], nvec, V, None, 0,
                                           L.dptr(out.view(float))))
        dbl = np.empty((nvec, 3, 3), dtype=complex)
        L.check(L.lib.tbk_kpm_double_moments(sp, L.dptr(kk), 1, 3, bnd[0], bnd[1], 0, 0, nvec, V, None, 0, L.dptr(dbl.view(float))))
    finally:
        L.check(L.lib.tbk_sparse_free(sp))
    e_mu = np.abs(mu - mu_ref).max()
    e_series = np.abs(out - series_ref).max() / np.abs(series_ref).max()
    e_dbl = np.abs(dbl - dbl_ref).max() / ring_velocity_bound(tab) ** 2
    print("ring of %d: moments %.2e, series %.2e of max|result|, double moments %.2e of |V|^2" % (n, e_mu, e_series, e_dbl))
    assert e_mu < TOL
    assert e_series <= TOL
    assert e_dbl <= TOL


@pytest.fixture(scope="module")
def big_flake():
    """a spinful Kane-Mele flake of 24 x 22 cells, 2112 states: past TBK_MAX_NSTA = 2048 (the two cut_piece calls were measured at
    0.23 s; the time is printed)"""
    t0 = time.perf_counter()
    m = flake(hp.kane_mele(T), 24, 22)
    dt = time.perf_counter() - t0
    print("24 x 22 Kane-Mele flake: %d states built in %.2f s" % (m._nsta, dt))
    return m


@pytest.mark.gpu
def test_past_the_dense_limit(big_flake, gpu_ctx):
    m = big_flake
    n = m._nsta
    assert n == 2112 and n > tb._lib.MAX_NSTA
    rng = np.random.default_rng(23)
    V = rng.standard_normal((4, n)) + 1j * rng.standard_normal((4, n))
    mu, bnd = m.kpm_moments(64, vectors=V)
    ref = kr.moments_recursion(dense_ham(m), V, 64, bnd)
    err = np.abs(mu - ref).max()
    print("n = %d: worst |device - reference| = %.2e" % (n, err))
    assert err < TOL
    assert m._tbk_cache is None                                 # the dense upload was never made
    with pytest.raises(Exception, match="exceeds this build's limit"):
        m._device_model()                                       # and still refuses, as before


@pytest.mark.gpu
def test_dos_exact_trace(gpu_ctx):
    m = model("flake7x9")
    n, M = m._nsta, 96
    bnd = default_bounds(m)
    x, E = kr.gauss_nodes(160, bnd)
    exact = kr.moments_exact(dense_ham(m), M, bnd)
    for kernel in ("jackson", "lorentz"):
        ref = kr.reconstruct(exact.mean(axis=0), E, bnd, kernel)
        rho = m.kpm_dos(E, M, kernel=kernel, states=range(n))
        assert np.abs(rho - ref).max() < 1e-10 * ref.max()
        ld = m.kpm_ldos(E, [0, 5, n - 1], M, kernel=kernel)
        assert ld.shape == (3, len(E))
        assert np.abs(ld - kr.reconstruct(exact[[0, 5, n - 1]], E, bnd, kernel)).max() < 1e-10 * ref.max()
    a = 0.5 * (bnd[1] - bnd[0])
    rho = m.kpm_dos(E, M, states=range(n))
    assert abs(np.sum((np.pi / len(E)) * np.sqrt(1.0 - x * x) * a * rho) - 1.0) < 1e-12
    # the stochastic trace: the estimate and its standard error over the samples
    rs, err = m.kpm_dos(E, M, n_vectors=16, seed=1, return_error=True)
    assert rs.shape == err.shape == E.shape and np.all(err >= 0.0)
    assert abs(np.sum((np.pi / len(E)) * np.sqrt(1.0 - x * x) * a * rs) - 1.0) < 1e-12
    # k-averaged, periodic model
    h = model("haldane6x6")
    k = kpoints(h, 2)
    hb = default_bounds(h)
    xh, Eh = kr.gauss_nodes(64, hb)
    ex = np.mean([kr.moments_exact(dense_ham(h, kq), 32, hb).mean(axis=0) for kq in k], axis=0)
    ref = kr.reconstruct(ex, Eh, hb)
    assert np.abs(h.kpm_dos(Eh, 32, k, states=range(h._nsta)) - ref).max() < 1e-10 * ref.max()


def launches(ctx):
    return sum(v["launches"] for v in ctx.prof_report().values())


@pytest.mark.gpu
def test_errors(gpu_ctx):
    m = model("haldane")
    k = np.array([[0.0, 0.0], [0.1, 0.05]])                     # levels near +-3 at both points
    V = np.ones((2, 2), dtype=complex)
    ref = np.stack([kr.moments_recursion(dense_ham(m, kq), V, 64, default_bounds(m)) for kq in k])
    with pytest.raises(tb._lib.TbkError, match=r"bounds \(-1, 1\) do not contain the spectrum"):
        m.kpm_moments(64, k, vectors=V, bounds=(-1, 1))
    mu, _ = m.kpm_moments(64, k, vectors=V)                     # the context is as good as new
    assert np.abs(mu - ref).max() < TOL
    # argument errors: raised in Python, before any launch or transfer
    m._sparse_model()
    gpu_ctx.prof_enable(1)
    try:
        gpu_ctx.prof_reset()
        xfer = gpu_ctx.transfer_stats()
        bad = [
            (dict(n_moments=0), "n_moments"),
            (dict(n_moments=2.0), "n_moments"),
            (dict(n_moments=8, states=[2]), "out of range"),
            (dict(n_moments=8, states=[-1]), "out of range"),
            (dict(n_moments=8, states=[]), "states"),
            (dict(n_moments=8, vectors=np.ones((2, 3), dtype=complex)), "vectors"),
            (dict(n_moments=8, vectors=np.ones(2, dtype=complex)), "vectors"),
            (dict(n_moments=8, vectors=np.ones((2, 2))), "vectors"),
            (dict(n_moments=8, vectors=V, states=[0]), "not both"),
            (dict(n_moments=8, n_vectors=0), "n_vectors"),
            (dict(n_moments=8, bounds=(1.0, 1.0)), "bounds"),
        ]
        for kw, text in bad:
            with pytest.raises(Exception, match=text):
                m.kpm_moments(k_list=k, **kw)
        with pytest.raises(Exception, match="Have to provide a k-vector!"):
            m.kpm_moments(8)
        with pytest.raises(Exception, match="out of range"):
            m.kpm_ldos([0.0], [5], 8, k)
        with pytest.raises(Exception, match="n_vectors"):
            m.kpm_vectors(0)
        assert launches(gpu_ctx) == 0
        assert gpu_ctx.transfer_stats() == xfer
        m.kpm_moments(8, k, vectors=V)
        assert launches(gpu_ctx) > 0                            # the counter does see this call's kernels
    finally:
        gpu_ctx.prof_enable(0)
        gpu_ctx.prof_reset()
