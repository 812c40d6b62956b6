"""NumPy restatement of the kernel polynomial method.  TEST INFRASTRUCTURE ONLY.

Dense-matrix Chebyshev recursion with the doubling identities (what the device does on the sparse operator), the exact moments
from an eigendecomposition (an independent route to the same numbers), the CSR -> dense expansion and the Gershgorin interval of
the table `tbk_sparse_flatten_host` returns, and the reconstruction of a density from moments."""
import ctypes as C

import numpy as np


def flatten_host(m):
    """The CSR operator of a pythtb_amd model through the host-only entry point: dict(row_ptr, col, R, amp, gersh, orb, nsta, dim_k)."""
    from pythtb_amd import _lib
    orb_per, onsite, hop_i, hop_j, hop_R, hop_amp = m._flat_tables()
    n = m._nsta
    nnz = C.c_int64(0)
    gersh = np.zeros(2)

    def call(cap, row_ptr, col, R, amp):
        _lib.check(_lib.lib.tbk_sparse_flatten_host(
            m._dim_k, m._norb, m._nspin, _lib.dptr(orb_per), _lib.dptr(onsite.view(float)), len(hop_i), _lib.iptr(hop_i),
            _lib.iptr(hop_j), _lib.iptr(hop_R.reshape(-1)) if hop_R.size else None,
            _lib.dptr(hop_amp.view(float)) if hop_amp.size else None, cap, C.byref(nnz),
            None if row_ptr is None else row_ptr.ctypes.data_as(C.POINTER(C.c_int64)), _lib.iptr(col), _lib.iptr(R),
            None if amp is None else _lib.dptr(amp.view(float)), _lib.dptr(gersh)))

    call(0, None, None, None, None)              # capacity 0: sizes the arrays
    nz = nnz.value
    row_ptr = np.full(n + 1, -1, dtype=np.int64)
    col = np.full(nz, -1, dtype=np.int32)
    R = np.full((nz, 4), 99, dtype=np.int32)
    amp = np.full(nz, np.nan, dtype=complex)
    call(nz, row_ptr, col, R.reshape(-1), amp)
    assert nnz.value == nz
    orb = np.repeat(orb_per, m._nspin, axis=0)   # the orbital of every state
    return dict(row_ptr=row_ptr, col=col, R=R, amp=amp, gersh=(gersh[0], gersh[1]), orb=orb, nsta=n, dim_k=m._dim_k)


def csr_to_dense(op, k=None):
    """H(k) of the CSR table: entry (row, col) += amp exp(2 pi i k.(R + orb_col - orb_row))."""
    n, dk = op["nsta"], op["dim_k"]
    rows = np.repeat(np.arange(n), np.diff(op["row_ptr"]))
    val = op["amp"].copy()
    if dk > 0:
        rv = op["R"][:, :dk] + op["orb"][op["col"]] - op["orb"][rows]
        val = val * np.exp(2.0j * np.pi * (rv @ np.asarray(k, dtype=float)))
    H = np.zeros((n, n), dtype=complex)
    np.add.at(H, (rows, op["col"]), val)
    return H


def gershgorin(op):
    """[min_i (d_i - r_i), max_i (d_i + r_i)]: d_i the real R = 0 diagonal entry, r_i the sum of the moduli of the rest of row i."""
    n = op["nsta"]
    rows = np.repeat(np.arange(n), np.diff(op["row_ptr"]))
    on = (rows == op["col"]) & np.all(op["R"] == 0, axis=1)
    d = np.zeros(n)
    r = np.zeros(n)
    np.add.at(d, rows[on], op["amp"][on].real)
    np.add.at(r, rows[on], np.abs(op["amp"][on].imag))
    np.add.at(r, rows[~on], np.abs(op["amp"][~on]))
    return (d - r).min(), (d + r).max()


def moments_recursion(H, vectors, n_moments, bounds):
    """mu[v][m] = <v|T_m(H~)|v> / <v|v> by alpha_m+1 = 2 H~ alpha_m - alpha_m-1 and mu_2m = 2 <alpha_m|alpha_m> - mu_0,
    mu_2m+1 = 2 <alpha_m+1|alpha_m> - mu_1: n_moments // 2 products.  vectors (nvec, n) complex."""
    a, b = 0.5 * (bounds[1] - bounds[0]), 0.5 * (bounds[1] + bounds[0])
    Ht = (np.asarray(H, dtype=complex) - b * np.identity(len(H))) / a
    V = np.asarray(vectors, dtype=complex).T            # columns
    mu = np.zeros((V.shape[1], n_moments))
    a0 = np.sum(np.abs(V) ** 2, axis=0)
    mu[:, 0] = 1.0
    prev, cur = V, None
    b1 = None
    for j in range(1, n_moments // 2 + 1):
        nw = Ht @ prev if j == 1 else 2.0 * (Ht @ cur) - prev
        if j > 1:
            prev = cur
        cur = nw
        A = np.sum(np.abs(cur) ** 2, axis=0)
        B = np.sum((cur.conj() * prev).real, axis=0)
        if j == 1:
            b1 = B
            mu[:, 1] = B / a0
        else:
            mu[:, 2 * j - 1] = (2.0 * B - b1) / a0
        if 2 * j < n_moments:
            mu[:, 2 * j] = (2.0 * A - a0) / a0
    return mu


def chebyshev_T(x, n_moments):
    """T_m(x), m < n_moments, shape (n_moments, len(x)), |x| <= 1."""
    return np.cos(np.arange(n_moments)[:, None] * np.arccos(np.clip(x, -1.0, 1.0))[None, :])


def moments_exact(H, n_moments, bounds, states=None):
    """mu^(i)_m = sum_j |U_ij|^2 T_m(x_j) from the eigendecomposition, for the unit vectors at `states` (default: all),
    shape (len(states), n_moments); their mean over all states is the trace form Tr T_m(H~) / n."""
    a, b = 0.5 * (bounds[1] - bounds[0]), 0.5 * (bounds[1] + bounds[0])
    w, U = np.linalg.eigh(np.asarray(H, dtype=complex))
    T = chebyshev_T((w - b) / a, n_moments)              # (M, n)
    P = np.abs(U) ** 2                                    # P[i, j] = |<i|j>|^2
    if states is not None:
        P = P[np.asarray(states)]
    return P @ T.T


def moments_exact_vectors(H, vectors, n_moments, bounds):
    """<v|T_m(H~)|v> / <v|v> from the eigendecomposition for arbitrary vectors (nvec, n)."""
    a, b = 0.5 * (bounds[1] - bounds[0]), 0.5 * (bounds[1] + bounds[0])
    w, U = np.linalg.eigh(np.asarray(H, dtype=complex))
    T = chebyshev_T((w - b) / a, n_moments)
    V = np.asarray(vectors, dtype=complex)
    P = np.abs(V.conj() @ U) ** 2
    return (P @ T.T) / np.sum(np.abs(V) ** 2, axis=1)[:, None]


def kernel_coefficients(n_moments, kernel, lam=4.0):
    M = n_moments
    m = np.arange(M, dtype=float)
    if kernel == "jackson":
        q = np.pi / (M + 1.0)
        return ((M - m + 1.0) * np.cos(q * m) + np.sin(q * m) / np.tan(q)) / (M + 1.0)
    if kernel == "lorentz":
        return np.sinh(lam * (1.0 - m / M)) / np.sinh(lam)
    assert kernel is None
    return np.ones(M)


def reconstruct(mu, energies, bounds, kernel="jackson", lam=4.0):
    """rho(E) = [g_0 mu_0 + 2 sum_{m >= 1} g_m mu_m T_m(x)] / (pi a sqrt(1 - x^2)), x = (E - b) / a; a plain loop over m."""
    mu = np.asarray(mu, dtype=float)
    e = np.asarray(energies, dtype=float)
    a, b = 0.5 * (bounds[1] - bounds[0]), 0.5 * (bounds[1] + bounds[0])
    x = (e - b) / a
    if np.any(x <= -1.0) or np.any(x >= 1.0):
        raise ValueError("energies outside the open interval of the bounds")
    g = kernel_coefficients(mu.shape[-1], kernel, lam)
    th = np.arccos(x)
    s = np.zeros(mu.shape[:-1] + e.shape)
    for m in range(mu.shape[-1]):
        s = s + (1.0 if m == 0 else 2.0) * g[m] * mu[..., m, None] * np.cos(m * th)
    return s / (np.pi * a * np.sqrt(1.0 - x * x))


def gauss_nodes(n, bounds):
    """Chebyshev-Gauss nodes x_j = cos(pi (j + 1/2) / n) and the energies E_j = a x_j + b."""
    a, b = 0.5 * (bounds[1] - bounds[0]), 0.5 * (bounds[1] + bounds[0])
    x = np.cos(np.pi * (np.arange(n) + 0.5) / n)
    return x, a * x + b


RING_N = 2048 * 32 + 33      # one more full row tile for workgroup 0 and a tail tile of one row for workgroup 1, past 2048 workgroups


def ring_tables(n=RING_N, hop=-0.8 + 0.3j, seed=41):
    """The tables tbk_sparse_upload takes for a ring of n orbitals in one cell (dim_k = 1): orbital i at i / n, random real on-site
    energies in [-0.5, 0.5], the hop `hop` from every orbital to the next, the closing bond to the next cell (R = 1).  Built as
    arrays: a model of this size does not go through set_hop."""
    i = np.arange(n, dtype=np.int32)
    R = np.zeros((n, 1), dtype=np.int32)
    R[-1] = 1
    return dict(orb=np.ascontiguousarray((np.arange(n) / n).reshape(n, 1)),
                onsite=np.random.default_rng(seed).uniform(-0.5, 0.5, n).astype(complex), hop_i=i,
                hop_j=np.ascontiguousarray((i + 1) % n, dtype=np.int32), hop_R=R, hop_amp=np.full(n, hop, dtype=complex))
