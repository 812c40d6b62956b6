"""NumPy restatement of the Chebyshev-filtered subspace iteration of tb_model.kpm_eigs on a dense H.
TEST INFRASTRUCTURE ONLY.

Steps 1 to 8 of the device driver in the same order: the Jackson-damped coefficients of the widened window, the random-phase
start vectors of the device generator, the filter by the Chebyshev recursion, the filter norms tau, the orthonormalisation
through the Gram matrix, Rayleigh-Ritz, the residuals and the stop test made at the start of the next iteration."""
import numpy as np

import kpm_ref as kr


class Saturated(Exception):
    pass


class NotConverged(Exception):
    pass


def widened(window, degree, bounds):
    """[e_lo - delta, e_hi + delta], delta = 2 pi a / degree, clipped to the open interval of the bounds"""
    a = 0.5 * (bounds[1] - bounds[0])
    d = 2.0 * np.pi * a / degree
    eps = 1e-9 * a
    return max(window[0] - d, bounds[0] + eps), min(window[1] + d, bounds[1] - eps)


def window_coefficients(window, n_terms, bounds):
    """c_0 = (th_lo - th_hi) / pi, c_m = 2 (sin m th_lo - sin m th_hi) / (m pi), th = arccos((e - b) / a), times the Jackson
    factors: the indicator of `window` itself (no widening here); a plain loop over m"""
    a, b = 0.5 * (bounds[1] - bounds[0]), 0.5 * (bounds[1] + bounds[0])
    tl, th = np.arccos((window[0] - b) / a), np.arccos((window[1] - b) / a)
    g = kr.kernel_coefficients(n_terms, "jackson")
    c = np.empty(n_terms)
    for m in range(n_terms):
        c[m] = (tl - th) / np.pi if m == 0 else 2.0 * (np.sin(m * tl) - np.sin(m * th)) / (m * np.pi)
    return c * g


def filter_value(c, x):
    """p(x) = sum_m c_m T_m(x) for scalars |x| <= 1"""
    return c @ kr.chebyshev_T(np.atleast_1d(x), len(c))


def _mix(z):
    z = (z + np.uint64(0x9E3779B97F4A7C15))
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def random_phases(n, count, seed=0, first=0):
    """the generator of tb_model.kpm_vectors on the host: (n, count), column g = vector number first + g"""
    with np.errstate(over="ignore"):
        s = _mix(np.array([seed], dtype=np.uint64))
        g = _mix(s ^ np.arange(first, first + count, dtype=np.uint64))
        h = _mix(g[None, :] ^ np.arange(n, dtype=np.uint64)[:, None])
    u = (h >> np.uint64(11)).astype(float) * 2.0 ** -53
    return np.exp(2.0j * np.pi * u)


def apply_filter(Ht, c, X):
    """sum_m c_m T_m(Ht) X by the recursion; also the largest column norm of a T_m X against that of X (the divergence guard)"""
    prev, cur = X, Ht @ X
    Y = c[0] * prev + c[1] * cur
    n0 = np.sum(np.abs(X) ** 2, axis=0)
    for m in range(2, len(c)):
        prev, cur = cur, 2.0 * (Ht @ cur) - prev
        Y = Y + c[m] * cur
        if not np.all(np.sum(np.abs(cur) ** 2, axis=0) <= (1.0 + 1e-6) * n0):
            raise ValueError("the bounds do not contain the spectrum")
    return Y


def eigs(H, window, bounds, n_search, degree, tol=1e-10, max_iter=40, seed=0, use_tau=True, spectral=None):
    """All eigenpairs of H in `window`: (theta (m,), X (n, m), info dict).  Raises Saturated ("raise n_search") or NotConverged.
    use_tau=False drops the filter-norm test (the plain algorithm): every Ritz value inside the window counts.
    spectral=(w, U): the eigendecomposition of H; the filter is then applied as U p(w) U^H X, which is the same polynomial of H
    to rounding and spares the recursion on a large dense matrix."""
    H = np.asarray(H, dtype=complex)
    n = len(H)
    a, b = 0.5 * (bounds[1] - bounds[0]), 0.5 * (bounds[1] + bounds[0])
    assert n_search % 8 == 0 and 8 <= n_search <= min(n - n % 8, 2048)
    c = window_coefficients(widened(window, degree, bounds), degree + 1, bounds)
    if spectral is None:
        Ht = (H - b * np.identity(n)) / a
        filt = lambda X: apply_filter(Ht, c, X)
    else:
        w, U = spectral
        pw = filter_value(c, (w - b) / a)
        filt = lambda X: U @ (pw[:, None] * (U.conj().T @ X))
    X = random_phases(n, n_search, seed) / np.sqrt(n)
    theta = resid = None
    rank = nstrong = 0
    assert max_iter >= 2
    for it in range(1, max_iter + 1):
        Y = filt(X)
        G = Y.conj().T @ Y
        tau = np.sqrt(np.diag(G).real)
        if theta is not None:
            live = np.arange(n_search) < rank
            strong = live & (tau >= 0.5) if use_tau else live
            sel = strong & (theta >= window[0]) & (theta <= window[1])
            nstrong = int(strong.sum())
            if np.all(resid[sel] <= tol * a):
                if use_tau and nstrong >= rank:
                    raise Saturated("raise n_search: %d pairs with tau >= 1/2 fill the subspace of rank %d" % (nstrong, rank))
                info = dict(applications=it, rank=rank, strong=nstrong, returned=int(sel.sum()), resid=resid[sel], tau=tau[sel])
                return theta[sel], X[:, sel], info
            if it == max_iter:
                if use_tau and nstrong >= rank:
                    raise Saturated("raise n_search: %d pairs with tau >= 1/2 fill the subspace of rank %d" % (nstrong, rank))
                e = NotConverged("not converged after %d filter applications: worst residual %.3e of %d pairs in the window"
                                 % (max_iter, resid[sel].max(), int(sel.sum())))
                e.count = int(sel.sum())
                raise e
        lam, U_ = np.linalg.eigh(G)
        keep = lam > 1e-12 * lam.max()
        rank = int(keep.sum())
        Wh = U_[:, keep] / np.sqrt(lam[keep])
        A = Y.conj().T @ (H @ Y)
        B = Wh.conj().T @ A @ Wh
        th, W = np.linalg.eigh(0.5 * (B + B.conj().T))
        X = np.zeros((n, n_search), dtype=complex)
        X[:, :rank] = Y @ (Wh @ W)
        theta = np.full(n_search, np.inf)
        theta[:rank] = th
        resid = np.full(n_search, np.inf)
        resid[:rank] = np.linalg.norm(H @ X[:, :rank] - X[:, :rank] * th, axis=0)
