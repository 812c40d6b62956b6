"""Eigenpairs in an energy window on the sparse operator (tb_model.kpm_eigs, kpm_window_coefficients).
The CPU tests run the NumPy restatement kpm_eigs_ref.py of the algorithm on the dense H of the oracle: it finds exactly the
states numpy.linalg.eigvalsh finds wherever the subspace is large enough and says "raise n_search" where it is not, and without
the filter-norm test it does not.  The GPU tests hold the device to the dense eigendecomposition: the count, the eigenvalues, the
residuals, orthonormality, the spectral projector, bit-reproducibility, the layouts and the error paths."""
import ctypes as C
import functools

import numpy as np
import pytest

import helpers as hp
import kpm_eigs_ref as er
import kpm_ref as kr
import test_kpm as tk
from helpers import quiet
from oracle import tb_oracle as orc  # noqa: F401  (dense_ham goes through it)

import pythtb_amd as tb

T = tb.tb_model
TOL = 1e-12          # the project's eigenvalue parity bound, here times the half-width a
BIG = "km24x22"

# name -> (k-point, window, exact number of states in it).  "isolated5" is five cells of test_kpm's `isolated` model at k = 0.3:
# the model itself has 3 states, fewer than the smallest n_search; the supercell has 15, five of them the empty CSR rows, whose
# eigenvalue is exactly 0 and whose eigenvectors are unit vectors.  The window of chain64 ends at 1.95, above the default bounds of
# that chain (its Gershgorin interval [-1.3, 1.9] widened by 1 %: 1.932), and a window has to lie inside the bounds: that case
# passes BOUNDS explicitly; every other case takes the default.
BOUNDS = {"chain64": (-1.4, 2.0)}
CASES = {
    "flake10x12-gap": ("flake10x12", None, (-0.35, 0.35), 6),
    "flake10x12-bulk": ("flake10x12", None, (0.9, 1.3), 35),
    "flake7x9": ("flake7x9", None, (-0.5, 0.5), 6),
    "chain63": ("chain63", None, (-1.3, -1.0), 12),
    "chain64": ("chain64", None, (1.85, 1.95), 5),
    "chain65": ("chain65", None, (-0.2, 0.5), 9),
    "haldane6x6": ("haldane6x6", (0.137, 0.731), (-1.6, -1.2), 8),
    "isolated5": ("isolated5", (0.3,), (-0.05, 0.05), 5),
    "km6x6": ("km6x6", None, (-0.6, 0.6), 8),
    BIG: (BIG, None, (-0.3, 0.3), 18),
}


@functools.lru_cache(maxsize=None)
def model(name):
    if name == "isolated5":
        return quiet(tk.model("isolated").make_supercell, [[5]])
    if name == "km6x6":
        return tk.flake(hp.kane_mele(T), 6, 6)
    if name == BIG:
        return tk.flake(hp.kane_mele(T), 24, 22)       # the flake of test_kpm.test_past_the_dense_limit, 2112 states
    return tk.model(name)


@functools.lru_cache(maxsize=None)
def dense(case):
    """(model, k, window, H, bounds, w, U, mask of the states in the window), computed once per case and left unchanged"""
    name, k, win, count = CASES[case]
    m = model(name)
    H = tk.dense_ham(m, k)
    w, U = np.linalg.eigh(H)
    inside = (w >= win[0]) & (w <= win[1])
    assert inside.sum() == count and m._nsta == NSTA[case]
    return m, k, win, H, BOUNDS.get(case, tk.default_bounds(m)), w, U, inside


def strong_count(case, degree):
    """the number of eigenvalues at which the filter of this degree is >= 1/2: the Ritz pairs that will count"""
    _, _, win, _, bnd, w, _, _ = dense(case)
    c = er.window_coefficients(er.widened(win, degree, bnd), degree + 1, bnd)
    a, b = 0.5 * (bnd[1] - bnd[0]), 0.5 * (bnd[1] + bnd[0])
    return int((er.filter_value(c, (w - b) / a) >= 0.5).sum())


NSTA = {"flake10x12-gap": 240, "flake10x12-bulk": 240, "flake7x9": 126, "chain63": 63, "chain64": 64, "chain65": 65, "haldane6x6": 72,
        "isolated5": 15, "km6x6": 144, BIG: 2112}


def combos(pairs):
    """(case, n_search, degree) as far as the model allows: n_search <= nsta rounded down to 8"""
    return [(c, ns, d) for c in CASES for ns, d in pairs if ns <= NSTA[c] - NSTA[c] % 8]


def check_pairs(case, th, X, resid_bound):
    """th (m,), X (n, m) against the dense eigendecomposition; returns the figures"""
    _, _, _, H, bnd, w, U, inside = dense(case)
    a = 0.5 * (bnd[1] - bnd[0])
    assert len(th) == inside.sum()
    if len(th) == 0:
        return 0.0, 0.0, 0.0, 0.0
    assert np.all(np.diff(th) >= 0.0)
    e_val = np.abs(th - w[inside]).max() / a
    e_res = np.linalg.norm(H @ X - X * th, axis=0).max() / a
    e_orth = np.abs(X.conj().T @ X - np.identity(len(th))).max()
    e_proj = np.abs(X @ X.conj().T - U[:, inside] @ U[:, inside].conj().T).max()
    print("%s: |theta - w| %.1e a, residual %.1e a, orthonormality %.1e, projector %.1e" % (case, e_val, e_res, e_orth, e_proj))
    assert e_val <= TOL
    assert e_res <= resid_bound
    assert e_orth <= 1e-12
    assert e_proj <= 1e-9
    return e_val, e_res, e_orth, e_proj


# ---------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("case,n_search,degree", combos([(16, 64), (32, 128), (64, 256)]))
def test_ref_finds_the_exact_count(case, n_search, degree):
    """The restatement on every model: exactly the states of eigvalsh where n_search exceeds the number of eigenvalues with a
    filter value >= 1/2, "raise n_search" where it does not.  Figures of the converged cases as measured with NumPy alone:
    3 to 12 filter applications, |theta - w| <= 2.4e-15 a, residuals <= 1.0e-10 a, orthonormality <= 4.7e-15, projector <= 4.3e-11.
    The 2112-state flake applies the filter through the eigendecomposition it needs anyway (the same polynomial of H)."""
    _, _, win, H, bnd, w, U, _ = dense(case)
    spectral = (w, U) if case == BIG else None
    if n_search > strong_count(case, degree):
        th, X, info = er.eigs(H, win, bnd, n_search, degree, spectral=spectral)
        assert info["strong"] == strong_count(case, degree) and info["applications"] >= 2
        check_pairs(case, th, X, 1e-10)
    else:
        with pytest.raises(er.Saturated, match="raise n_search"):
            er.eigs(H, win, bnd, n_search, degree, max_iter=6, spectral=spectral)


def test_ref_saturated_subspace():
    """35 states in the window, 32 vectors: every Ritz pair passes the filter, and the call must not return 32 of the 35"""
    _, _, win, H, bnd, _, _, _ = dense("flake10x12-bulk")
    with pytest.raises(er.Saturated, match="raise n_search: 32 pairs"):
        er.eigs(H, win, bnd, 32, 128, max_iter=8)


def test_ref_without_filter_norm_reports_spurious_states():
    """Why the filter-norm test is there.  The plain algorithm (every Ritz value inside the window counts) on the 10 x 12 flake,
    gap window, n_search = 64, degree = 128: the subspace holds mixtures of states below and above the window whose Rayleigh
    quotient falls inside it; they are no eigenvectors, their residuals never fall, and the count is above the six states
    that are there.  With the test the same call returns the six."""
    _, _, win, H, bnd, _, _, _ = dense("flake10x12-gap")
    with pytest.raises(er.NotConverged) as e:
        er.eigs(H, win, bnd, 64, 128, use_tau=False, max_iter=12)
    print("without the filter norm:", e.value)
    assert e.value.count > 6
    th, X, _ = er.eigs(H, win, bnd, 64, 128)
    check_pairs("flake10x12-gap", th, X, 1e-10)


def test_window_coefficients_against_quadrature():
    """kpm_window_coefficients(kernel=None) against kpm_coefficients of the indicator, with the bound of
    test_kpm_series.test_fermi_coefficients_against_quadrature for each of the two jumps: with both edges on cell edges of the
    midpoint rule the two agree to rounding after the factor (m h / 2) / sin(m h / 2); for a generic window they differ by the
    two cells that hold the jumps, at most 2 / K each, plus the midpoint error (m h)^2 / 24 of |c_m| <= 4 / (m pi)."""
    bnd = (-3.1, 3.4)
    a, b = 0.5 * (bnd[1] - bnd[0]), 0.5 * (bnd[1] + bnd[0])
    M, K = 64, 4096
    h = np.pi / K
    m = np.arange(M)
    win = (a * np.cos(h * 2500) + b, a * np.cos(h * 1500) + b)
    ind = lambda e: ((e > win[0]) & (e < win[1])).astype(float)
    exact = tb.kpm_window_coefficients(win, M, bnd, kernel=None)
    quad = tb.kpm_coefficients(ind, M, bnd, n_quad=K)
    factor = np.where(m == 0, 1.0, (0.5 * m * h) / np.sin(0.5 * np.maximum(m, 1) * h))
    assert exact.dtype == float and np.abs(quad - exact * factor).max() < 1e-12
    win = (-0.7123, 0.3217)
    exact = tb.kpm_window_coefficients(win, M, bnd, kernel=None)
    quad = tb.kpm_coefficients(ind, M, bnd, n_quad=K)
    err = np.abs(quad - exact)
    print("generic window: worst |quadrature - analytic| = %.2e (4 / K = %.2e)" % (err.max(), 4.0 / K))
    assert np.all(err <= 4.0 / K + m * h * h / (3.0 * np.pi) + 1e-14)
    # the difference of two Fermi steps, the kernel factors term by term, and the restatement
    step = tb.kpm_fermi_coefficients(win[1], M, bnd, kernel=None) - tb.kpm_fermi_coefficients(win[0], M, bnd, kernel=None)
    assert np.abs(exact - step).max() < 1e-15
    for kernel in ("jackson", "lorentz"):
        assert np.array_equal(tb.kpm_window_coefficients(win, M, bnd, kernel), exact * kr.kernel_coefficients(M, kernel))
    assert np.abs(tb.kpm_window_coefficients(win, M, bnd) - er.window_coefficients(win, M, bnd)).max() < 1e-15
    # the Jackson-damped filter is 1/2 at the edges, 1 well inside and 0 well outside, up to the kernel's tails (measured: 4e-6 at
    # the edges, 6e-5 inside)
    c = tb.kpm_window_coefficients(win, 257, bnd)
    p = er.filter_value(c, (np.array([win[0], win[1], -0.2, -2.5, 2.5]) - b) / a)
    assert np.abs(p[:2] - 0.5).max() < 1e-3 and abs(p[2] - 1.0) < 1e-3 and np.abs(p[3:]).max() < 1e-3
    for bad in ((0.5, 0.2), (-3.1, 0.0), (0.0, 3.4), (0.0, np.inf)):
        with pytest.raises(Exception, match="window"):
            tb.kpm_window_coefficients(bad, M, bnd)
    with pytest.raises(Exception, match="n_terms"):
        tb.kpm_window_coefficients(win, 0, bnd)
    with pytest.raises(Exception, match="kernel"):
        tb.kpm_window_coefficients(win, M, bnd, kernel="fejer")


def test_ref_generator_is_the_device_generator_formula():
    """unit modulus, distinct entries, a pure function of (seed, number, index)"""
    v = er.random_phases(126, 5, seed=7)
    assert v.shape == (126, 5) and np.abs(np.abs(v) - 1.0).max() <= 1e-15
    assert len(set(v.reshape(-1).tolist())) == v.size
    assert np.array_equal(v[:, 2:], er.random_phases(126, 3, seed=7, first=2))
    assert not np.any(v == er.random_phases(126, 5, seed=8))


# ---------------------------------------------------------------------------------------------------------------- GPU
def device_eigs(case, n_search, degree, **kw):
    m, k, win, _, _, _, _, _ = dense(case)
    th, vec, info = m.kpm_eigs(win, n_search=n_search, k_point=k, degree=degree, return_info=True, bounds=BOUNDS.get(case), **kw)
    return th, vec, info


@pytest.mark.gpu
@pytest.mark.parametrize("case,n_search,degree", combos([(ns, d) for ns in (8, 16, 64, 72) for d in (64, 257)]))
def test_eigs_against_dense(case, n_search, degree, gpu_ctx):
    """Where n_search exceeds the number of eigenvalues that pass the filter: the count of eigvalsh, |theta - w| <= 1e-12 a,
    residuals recomputed in NumPy <= 2 tol a, |X^H X - 1| <= 1e-12, |X X^H - P_dense| <= 1e-9, and a second call with the same
    bits.  Where it does not: the saturated-subspace error, never a partial answer."""
    m, k, win, _, bnd, _, _, _ = dense(case)
    strong = strong_count(case, degree)
    if n_search <= strong:
        with pytest.raises(tb._lib.TbkError, match="raise n_search"):
            device_eigs(case, n_search, degree)
        return
    th, vec, info = device_eigs(case, n_search, degree)
    n = m._nsta
    assert info["bounds"] == pytest.approx(bnd, rel=1e-14)
    assert th.dtype == float and vec.dtype == np.complex128
    X = vec.reshape(len(th), n).T
    tol = 1e-10
    a = 0.5 * (bnd[1] - bnd[0])
    print("%s n_search %d degree %d: %d applications, rank %d, %d pairs pass the filter" % (
        case, n_search, degree, info["applications"], info["rank"], info["strong"]))
    check_pairs(case, th, X, 2.0 * tol)
    assert info["strong"] == strong and info["returned"] == len(th) and 2 <= info["applications"] <= 40
    assert info["strong"] < info["rank"] <= n_search
    assert np.all(info["residuals"] <= tol * a)
    th2, vec2, info2 = device_eigs(case, n_search, degree)
    assert np.array_equal(th, th2) and np.array_equal(vec, vec2) and np.array_equal(info["residuals"], info2["residuals"])


@pytest.mark.gpu
def test_layouts_and_defaults(gpu_ctx):
    """nspin = 2: the shape of solve_one; the default degree; another seed finds the same subspace; no info unless asked"""
    m, _, win, _, bnd, w, U, inside = dense("km6x6")
    ev, vec = m.kpm_eigs(win, n_search=32)
    ref_ev, ref_vec = m.solve_one(eig_vectors=True)
    assert vec.shape == (8,) + ref_vec.shape[1:] == (8, m._norb, 2) and ev.shape == (8,)
    check_pairs("km6x6", ev, vec.reshape(8, -1).T, 2e-10)
    assert np.abs(ev - ref_ev[inside]).max() <= TOL * 0.5 * (bnd[1] - bnd[0])
    _, _, info = m.kpm_eigs(win, n_search=32, return_info=True)
    a = 0.5 * (bnd[1] - bnd[0])
    assert info["degree"] == min(4096, max(64, int(np.ceil(8.0 * a / (win[1] - win[0])))))
    ev7, vec7 = m.kpm_eigs(win, n_search=32, seed=7)
    check_pairs("km6x6", ev7, vec7.reshape(8, -1).T, 2e-10)
    assert not np.array_equal(vec7, vec)
    # nspin = 1 with a k-point
    h, k, hwin, _, _, _, _, _ = dense("haldane6x6")
    ev, vec = h.kpm_eigs(hwin, n_search=32, k_point=k, degree=128)
    assert vec.shape == (8, h._norb) == (8,) + h.solve_one(k, eig_vectors=True)[1].shape[1:]
    check_pairs("haldane6x6", ev, vec.T, 2e-10)


@pytest.mark.gpu
def test_window_without_states(gpu_ctx):
    """the middle third of the widest gap of the 7 x 9 flake's spectrum inside its bulk gap: m = 0 is an answer, not an error"""
    m, _, _, _, _, w, _, _ = dense("flake7x9")
    near = w[(w > -1.0) & (w < 1.0)]
    i = np.argmax(np.diff(near))
    lo, hi = near[i], near[i + 1]
    win = (lo + (hi - lo) / 3.0, hi - (hi - lo) / 3.0)
    ev, vec, info = m.kpm_eigs(win, n_search=32, degree=128, return_info=True)
    assert ev.shape == (0,) and vec.shape == (0, m._nsta) and info["returned"] == 0 and info["residuals"].shape == (0,)
    assert info["strong"] == int((er.filter_value(er.window_coefficients(er.widened(win, 128, info["bounds"]), 129, info["bounds"]),
                                                  (w - 0.5 * sum(info["bounds"])) / (0.5 * (info["bounds"][1] - info["bounds"][0])))
                                  >= 0.5).sum())


@pytest.mark.gpu
def test_past_the_dense_limit_without_a_dense_model(gpu_ctx):
    """2112 states, all levels doubly degenerate, the nearest level outside the window 0.0076 away: the 18 states, and the dense
    upload was never made"""
    m, _, win, _, _, _, _, _ = dense(BIG)
    assert m._nsta == 2112 > tb._lib.MAX_NSTA
    fresh = tk.flake(hp.kane_mele(T), 24, 22)
    ev, vec, info = fresh.kpm_eigs(win, n_search=64, degree=512, return_info=True)
    print("2112 states: %d applications, rank %d, %d pairs pass the filter" % (info["applications"], info["rank"], info["strong"]))
    assert vec.shape == (18, fresh._norb, 2)
    check_pairs(BIG, ev, vec.reshape(18, -1).T, 2e-10)
    assert fresh._tbk_cache is None
    with pytest.raises(Exception, match="exceeds this build's limit"):
        fresh._device_model()


@pytest.mark.gpu
def test_errors(gpu_ctx):
    m, _, win, _, bnd, _, _, _ = dense("flake10x12-gap")
    ref = m.kpm_eigs(win, n_search=32, degree=128)
    with pytest.raises(Exception, match="inside the open interval"):
        m.kpm_eigs((-0.35, bnd[1] + 0.1), n_search=32)
    with pytest.raises(Exception, match="inside the open interval"):
        m.kpm_eigs((-0.35, 0.35), n_search=32, bounds=(-0.3, 5.0))
    with pytest.raises(Exception, match="window"):
        m.kpm_eigs((0.35, -0.35), n_search=32)
    with pytest.raises(tb._lib.TbkError, match=r"bounds \(-1, 1\) do not contain the spectrum"):
        m.kpm_eigs(win, n_search=32, degree=128, bounds=(-1, 1))
    for bad in (12, 0, 4, 248, 16.0):
        with pytest.raises(Exception, match="n_search"):
            m.kpm_eigs(win, n_search=bad)
    with pytest.raises(Exception, match="n_search"):
        tk.model("isolated").kpm_eigs((-0.05, 0.05), n_search=8, k_point=[0.3])      # 3 states
    with pytest.raises(Exception, match="Have to provide a k-vector"):
        tk.model("haldane6x6").kpm_eigs((-1.6, -1.2), n_search=32)
    for kw in (dict(degree=1), dict(degree=2.5), dict(tol=0.0), dict(max_iter=1), dict(seed=-1)):
        with pytest.raises(Exception, match=list(kw)[0]):
            m.kpm_eigs(win, n_search=32, **kw)
    # the library's own checks, past the Python ones
    L = tb._lib
    sp = m._sparse_model()
    out = (C.c_int(0), np.zeros(32), np.zeros((32, m._nsta), dtype=complex), np.zeros(4, dtype=np.int32))

    def raw(e_lo, e_hi, ns, degree, max_iter=40):
        return L.lib.tbk_kpm_eigs(sp, None, e_lo, e_hi, bnd[0], bnd[1], ns, degree, 1e-10, max_iter, 0, C.byref(out[0]), L.dptr(out[1]),
                                  L.dptr(out[2].view(float)), None, L.iptr(out[3]))
    assert raw(0.35, -0.35, 32, 128) == 1 and raw(-0.35, bnd[1], 32, 128) == 1 and raw(-0.35, 0.35, 12, 128) == 1
    assert raw(-0.35, 0.35, 248, 128) == 1 and raw(-0.35, 0.35, 32, 1) == 1 and raw(-0.35, 0.35, 32, 128, 1) == 1
    # a saturated subspace: 35 states, 32 vectors
    _, _, bulk, _, _, _, _, _ = dense("flake10x12-bulk")
    with pytest.raises(tb._lib.TbkError, match=r"error 6: .*32 Ritz pairs .* raise n_search"):
        m.kpm_eigs(bulk, n_search=32, degree=128)
    # needs five filter applications
    with pytest.raises(tb._lib.TbkError, match=r"error 6: .*not converged after 2 filter applications.*worst residual"):
        m.kpm_eigs(win, n_search=32, degree=128, max_iter=2)
    again = m.kpm_eigs(win, n_search=32, degree=128)                                 # the context is as good as new
    assert np.array_equal(ref[0], again[0]) and np.array_equal(ref[1], again[1])


RING_EPS, RING_U, RING_SITE = 0.1, 2.0, 7


@functools.lru_cache(maxsize=None)
def impurity_ring():
    """The tables of kpm_ref.ring_tables (the long ring of test_kpm.ring_reference: 2048 * 32 + 33 orbitals, dim_k = 1) with the
    on-site energies replaced: the ring's own are random, so none of its levels is known in closed form.  Here every site has
    RING_EPS and site RING_SITE has RING_EPS + RING_U: one bound state above the band at eps + sqrt(U^2 + 4 |hop|^2) (the
    single-impurity level of the infinite chain; on this ring the correction is exp(-n kappa), kappa ~ 1, and the flux through
    the ring enters the same way).  The band ends at eps + 2 |hop|, 0.9 below."""
    tab = dict(kr.ring_tables())
    on = np.full(kr.RING_N, RING_EPS, dtype=complex)
    on[RING_SITE] += RING_U
    tab["onsite"] = on
    t = abs(complex(tab["hop_amp"][0]))
    lo, hi = RING_EPS - 2 * t, RING_EPS + RING_U + 2 * t
    bnd = (lo - 0.01 * (hi - lo), hi + 0.01 * (hi - lo))
    return tab, bnd, RING_EPS + np.sqrt(RING_U ** 2 + 4 * t * t)


@pytest.mark.gpu
def test_rows_past_the_grid(gpu_ctx):
    """More row tiles than workgroups in every new kernel (the Gram kernel: 1025 tiles of 64 rows on 256 workgroups; the
    rotation, the residual and the load: 2050 tiles of 32 rows on 2048): n_search = 8 on the ring of 65569 orbitals through the
    C ABI, a window of +-0.01 around the analytic impurity level.  No dense matrix: the level against its closed form to
    1e-12 a, the residual recomputed with numpy.roll to 2 tol a, the norm to 1e-12, and the state sits on the impurity."""
    tab, bnd, level = impurity_ring()
    L, n, k = tb._lib, kr.RING_N, 0.3125
    a = 0.5 * (bnd[1] - bnd[0])
    sp = C.c_void_p()
    L.check(L.lib.tbk_sparse_upload(gpu_ctx.handle, 1, n, 1, L.dptr(tab["orb"]), L.dptr(tab["onsite"].view(float)), n,
                                    L.iptr(tab["hop_i"]), L.iptr(tab["hop_j"]), L.iptr(tab["hop_R"].reshape(-1)),
                                    L.dptr(tab["hop_amp"].view(float)), C.byref(sp)))
    try:
        nf, ev, vec, res, info = C.c_int(0), np.zeros(8), np.zeros((8, n), dtype=complex), np.zeros(8), np.zeros(4, dtype=np.int32)
        L.check(L.lib.tbk_kpm_eigs(sp, L.dptr(np.array([k])), level - 0.01, level + 0.01, bnd[0], bnd[1], 8, 64, 1e-10, 40, 0,
                                   C.byref(nf), L.dptr(ev), L.dptr(vec.view(float)), L.dptr(res), L.iptr(info)))
    finally:
        L.check(L.lib.tbk_sparse_free(sp))
    assert nf.value == 1 and info[3] == 1 and info[2] == 1 and 1 < info[1] <= 8
    x = vec[0]
    h = complex(tab["hop_amp"][0]) * np.exp(2j * np.pi * k / n)
    Hx = tab["onsite"].real * x + h * np.roll(x, -1) + np.conj(h) * np.roll(x, 1)
    r = np.linalg.norm(Hx - ev[0] * x)
    print("ring of %d: |theta - level| = %.2e a, residual %.2e a (device %.2e a), %d applications" % (
        n, abs(ev[0] - level) / a, r / a, res[0] / a, info[0]))
    assert abs(ev[0] - level) <= TOL * a
    assert r <= 2e-10 * a and res[0] <= 1e-10 * a
    assert abs(np.vdot(x, x).real - 1.0) <= 1e-12
    assert np.argmax(np.abs(x)) == RING_SITE
