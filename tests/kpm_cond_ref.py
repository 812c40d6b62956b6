"""NumPy restatement of the Kubo-Bastin kernel polynomial conductivity.  TEST INFRASTRUCTURE ONLY.

Dense H(k) and V^a = dH/dk_a from the model's hopping table (the convention of `_gen_ham` / `_gen_dham`), the double moments
mu_mn = <v| V^a T_m(H~) V^b T_n(H~) |v> / <v|v> by the dense recursion and, independently, from the eigendecomposition, the linear
weights W_mn(E) of the reconstruction written as a plain loop over the quadrature nodes, and the Chern number of a band set from
the Kubo curvature on a uniform mesh."""
import numpy as np

import kpm_ref as kr


def dense_ham_dham(m, k, dirs=()):
    """H(k) and the matrices dH/dk_a, a in dirs, (nsta, nsta) each: every hop t e^{2 pi i k.rv} of H, rv = (R + tau_j - tau_i) on the
    periodic axes, enters dH/dk_a as 2 pi i rv_a t e^{2 pi i k.rv}; the on-site terms do not depend on k."""
    no, ns = m._norb, m._nspin
    n = no * ns
    k = np.asarray(k, dtype=float).reshape(m._dim_k)
    H = np.zeros((no, ns, no, ns), dtype=complex)
    V = [np.zeros((no, ns, no, ns), dtype=complex) for _ in dirs]
    for a in range(no):
        H[a, :, a, :] = np.array(m._site_energies[a], dtype=complex).reshape(ns, ns) if ns == 2 else m._site_energies[a]
    for hop in m._hoppings:
        amp = np.array(hop[0], dtype=complex).reshape(ns, ns)
        a, b = hop[1], hop[2]
        rv = (-m._orb[a] + m._orb[b] + np.array(hop[3], dtype=float))[m._per]
        amp = amp * np.exp(2.0j * np.pi * np.dot(k, rv))
        H[a, :, b, :] += amp
        H[b, :, a, :] += amp.conj().T
        for V_d, d in zip(V, dirs):
            V_d[a, :, b, :] += 2.0j * np.pi * rv[d] * amp
            V_d[b, :, a, :] += (2.0j * np.pi * rv[d] * amp).conj().T
    return H.reshape(n, n), [V_d.reshape(n, n) for V_d in V]


def operators(m, k, dirs):
    """(H, V^a, V^b) for dirs = (a, b)."""
    H, V = dense_ham_dham(m, k, tuple(dirs))
    return H, V[0], V[1]


def rescaled(H, bounds):
    a, b = 0.5 * (bounds[1] - bounds[0]), 0.5 * (bounds[1] + bounds[0])
    return (np.asarray(H, dtype=complex) - b * np.identity(len(H))) / a


def chebyshev_stack(Ht, X, n_moments):
    """T_n(H~) X for n < n_moments by the three-term recursion, shape (n_moments,) + X.shape."""
    out = np.empty((n_moments,) + X.shape, dtype=complex)
    out[0] = X
    if n_moments > 1:
        out[1] = Ht @ X
    for j in range(2, n_moments):
        out[j] = 2.0 * (Ht @ out[j - 1]) - out[j - 2]
    return out


def double_moments_recursion(H, Va, Vb, vectors, n_moments, bounds):
    """(i) mu[v][m][n] = <psi_m|Phi_n> / <v|v>, Phi_n = T_n(H~) v, psi_m = V^b T_m(H~) V^a v; vectors (nvec, nsta) complex."""
    Ht = rescaled(H, bounds)
    R = np.asarray(vectors, dtype=complex).T                    # columns
    phi = chebyshev_stack(Ht, R, n_moments)                     # (M, n, nvec)
    psi = np.einsum("ij,mjv->miv", Vb, chebyshev_stack(Ht, Va @ R, n_moments))
    mu = np.matmul(psi.conj().transpose(2, 0, 1), phi.transpose(2, 1, 0))      # (nvec, M, n) @ (nvec, n, M)
    return mu / np.sum(np.abs(R) ** 2, axis=0)[:, None, None]


def double_moments_eigen(H, Va, Vb, n_moments, bounds, vectors=None):
    """(ii) from the eigendecomposition H = U w U^+, x = (w - b) / a.  vectors=None: the trace per state,
    Tr[V^a T_m V^b T_n] / nsta = sum_ij (V^a)_ij T_m(x_j) (V^b)_ji T_n(x_i) / nsta, shape (M, M); else per vector, (nvec, M, M):
    <v|V^a T_m V^b T_n|v> / <v|v> = sum_ij <v|V^a|j> T_m(x_j) <j|V^b|i> T_n(x_i) <i|v> / <v|v>."""
    a, b = 0.5 * (bounds[1] - bounds[0]), 0.5 * (bounds[1] + bounds[0])
    w, U = np.linalg.eigh(np.asarray(H, dtype=complex))
    T = kr.chebyshev_T((w - b) / a, n_moments)                  # (M, n)
    A = U.conj().T @ Va @ U
    B = U.conj().T @ Vb @ U
    if vectors is None:
        return T @ (A * B.T).T @ T.T / len(w)
    R = np.asarray(vectors, dtype=complex).T
    left = (U.conj().T @ (Va @ R)).conj()                       # <v|V^a|j>
    right = U.conj().T @ R                                      # <i|v>
    mu = np.stack([(T * left[:, v]) @ B @ (T * right[:, v]).T for v in range(R.shape[1])])
    return mu / np.sum(np.abs(R) ** 2, axis=0)[:, None, None]


def conductivity_weights(n_moments, energies, bounds, kernel="jackson", n_quad=None, lam=4.0):
    """W[e][m][n] with G(E_e) = sum_mn W[e][m][n] mu_mn: the formula of `kpm_conductivity_reconstruct` at kT = 0, a plain loop over
    the Chebyshev-Gauss nodes x_j = cos(pi (j + 1/2) / K), weights pi sqrt(1 - x_j^2) / K, restricted to x_j <= x_F."""
    M = n_moments
    K = 8 * M if n_quad is None else n_quad
    a, b = 0.5 * (bounds[1] - bounds[0]), 0.5 * (bounds[1] + bounds[0])
    xf = (np.asarray(energies, dtype=float) - b) / a
    if np.any(xf <= -1.0) or np.any(xf >= 1.0):
        raise ValueError("energies outside the open interval of the bounds")
    g = kr.kernel_coefficients(M, kernel, lam)
    h = g / np.where(np.arange(M) == 0, 2.0, 1.0)
    idx = np.arange(M)
    W = np.zeros((len(xf), M, M), dtype=complex)
    for j in range(K):
        th = np.pi * (j + 0.5) / K
        x, s = np.cos(th), np.sin(th)
        hit = x <= xf
        if not hit.any():
            continue
        Tx = np.cos(idx * th)
        gam = (x - 1j * idx * s)[None, :] * np.exp(1j * idx * th)[None, :] * Tx[:, None] \
            + (x + 1j * idx * s)[:, None] * np.exp(-1j * idx * th)[:, None] * Tx[None, :]
        W[hit] += (np.pi * s / K) / (1.0 - x * x) ** 2 * gam
    return (2.0 / (np.pi * a) ** 2) * W * (h[:, None] * h[None, :])


def conductivity(mu, energies, bounds, kernel="jackson", n_quad=None):
    """G(E) (..., nE) of moments (..., M, M) through the explicit weights."""
    W = conductivity_weights(mu.shape[-1], energies, bounds, kernel, n_quad)
    return np.einsum("emn,...mn->...e", W, mu)


def chern_number(m, occ, nmesh=64):
    """The Chern number of the band set occ of a 2-D model from Omega = -2 Im sum_{n in occ, m not in occ} <n|dH_0|m><m|dH_1|n> /
    (E_n - E_m)^2 (the convention of `tb_model.berry_curvature`): its mean over a uniform nmesh x nmesh mesh divided by 2 pi."""
    occ = np.asarray(occ)
    total = 0.0
    for i in range(nmesh):
        for j in range(nmesh):
            H, V0, V1 = operators(m, [i / nmesh, j / nmesh], (0, 1))
            w, U = np.linalg.eigh(H)
            rest = np.setdiff1d(np.arange(len(w)), occ)
            A = (U.conj().T @ V0 @ U)[np.ix_(occ, rest)]
            B = (U.conj().T @ V1 @ U)[np.ix_(rest, occ)]
            total += -2.0 * np.imag(np.sum(A * B.T / (w[occ][:, None] - w[rest][None, :]) ** 2))
    return total / nmesh ** 2 / (2.0 * np.pi)


def random_phase_vectors(seed, first, count, nsta):
    """The random-phase start vectors number first .. first + count - 1 of `seed`, (count, nsta): the counter-based generator of
    `tb_model.kpm_vectors` restated on the host (splitmix64 finaliser of (seed, vector number, element), 53 bits -> a phase)."""
    mask = (1 << 64) - 1

    def mix(z):
        z = (z + 0x9E3779B97F4A7C15) & mask
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & mask
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & mask
        return z ^ (z >> 31)

    out = np.empty((count, nsta), dtype=complex)
    for g in range(count):
        hg = mix(mix(seed) ^ (first + g))
        u = np.array([(mix(hg ^ i) >> 11) * 2.0 ** -53 for i in range(nsta)])
        out[g] = np.exp(2.0j * np.pi * u)
    return out
