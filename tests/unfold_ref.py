"""NumPy restatement of the unfolding calls of pythtb_amd.tb_model (unfolded_bands, unfolded_spectral), built on the oracle's ham_batch
and numpy.linalg.eigh: the checker of tests/test_unfolding.py.  All functions take the SUPERCELL model m.

    K = S_per k                                  the supercell's reduced k of the same Cartesian vector, not reduced modulo 1
    delta_j = orb[j] S - prim_orb[prim_index[j]],  delta_j -= round(delta_j)      (periodic directions; 0 without prim_orb)
    W_n,g(k) = (1 / N_c) | sum_{j in g} e^{2 pi i k.delta_j} u_n[j] |^2
    A_g(k, w) = sum_n W_n,g(k) (eta / pi) / ((w - E_n)^2 + eta^2) = -(1 / pi) Im <k,g| (w + i eta - H_sc(K))^-1 |k,g>

with (E_n, u_n) the eigenpairs of H_sc(K) and state (j, s) of a spinful model in group prim_index[j] * nspin + s."""
import numpy as np

from oracle import tb_oracle as orc


def setting(m, S, prim_index=None, prim_orb=None):
    """(group (nsta,) with -1 for no group, ng, delta (nsta, dim_k) per STATE, N_c, S_per)."""
    S = np.asarray(S, dtype=int)
    nc = int(round(abs(np.linalg.det(S))))
    norb, ns, per = m._norb, m._nspin, list(m._per)
    if prim_index is None:
        assert norb % nc == 0
        pi = np.arange(norb) % (norb // nc)
    else:
        pi = np.asarray(prim_index, dtype=int)
    n_prim = pi.max() + 1
    group = np.array([pi[j] * ns + s if pi[j] >= 0 else -1 for j in range(norb) for s in range(ns)])
    delta = np.zeros((norb, len(per)))
    if prim_orb is not None:
        po = np.asarray(prim_orb, dtype=float)
        for j in range(norb):
            if pi[j] >= 0:
                d = (np.asarray(m._orb[j]) @ S - po[pi[j]])[per]
                delta[j] = d - np.round(d)
    return group, n_prim * ns, np.repeat(delta, ns, axis=0), nc, S[np.ix_(per, per)]


def bloch_vectors(m, k, S, prim_index=None, prim_orb=None):
    """|k,g> in the solver's gauge, (ng, nsta): e^{-2 pi i k.delta_j} / sqrt(N_c) on the members of g."""
    group, ng, delta, nc, _ = setting(m, S, prim_index, prim_orb)
    v = np.zeros((ng, len(group)), dtype=complex)
    for j, g in enumerate(group):
        if g >= 0:
            v[g, j] = np.exp(-2.0j * np.pi * (delta[j] @ k)) / np.sqrt(nc)
    return v


def eigenpairs(m, k, S):
    """(E (nk, n), u[k][component][band]) of H_sc(S_per k)."""
    per = list(m._per)
    Sp = np.asarray(S, dtype=int)[np.ix_(per, per)]
    K = np.asarray(k, dtype=float).reshape(-1, m._dim_k) @ Sp.T
    return np.linalg.eigh(orc.ham_batch(m, K))


def weights(m, k, S, prim_index=None, prim_orb=None, pairs=None):
    """(E (nk, n), W (nk, n, ng))."""
    k = np.asarray(k, dtype=float).reshape(-1, m._dim_k)
    e, u = eigenpairs(m, k, S) if pairs is None else pairs
    ng = setting(m, S, prim_index, prim_orb)[1]
    w = np.zeros((len(k), e.shape[1], ng))
    for q in range(len(k)):
        v = bloch_vectors(m, k[q], S, prim_index, prim_orb)
        w[q] = (np.abs(np.conj(v) @ u[q]) ** 2).T
    return e, w


def lorentz(x, eta):
    return eta / np.pi / (x * x + eta * eta)


def spectral(e, w, omega, eta):
    """A (nk, nw, ng) from the levels e (nk, n) and weights w (nk, n, ng)."""
    om = np.atleast_1d(np.asarray(omega, dtype=float))
    return np.einsum("kwn,kng->kwg", lorentz(om[None, :, None] - e[:, None, :], eta), w)


def resolvent(m, k, S, omega, eta, prim_index=None, prim_orb=None):
    """A (nk, nw, ng) = -(1 / pi) Im <k,g| (w + i eta - H_sc(K))^-1 |k,g>, by a dense inverse: no eigenvectors."""
    k = np.asarray(k, dtype=float).reshape(-1, m._dim_k)
    om = np.atleast_1d(np.asarray(omega, dtype=float))
    per = list(m._per)
    Sp = np.asarray(S, dtype=int)[np.ix_(per, per)]
    h = orc.ham_batch(m, k @ Sp.T)
    n = h.shape[1]
    ng = setting(m, S, prim_index, prim_orb)[1]
    out = np.zeros((len(k), len(om), ng))
    for q in range(len(k)):
        v = bloch_vectors(m, k[q], S, prim_index, prim_orb)
        for j, x in enumerate(om):
            g = np.linalg.inv((x + 1j * eta) * np.identity(n) - h[q])
            out[q, j] = -np.imag(np.einsum("gi,ij,gj->g", np.conj(v), g, v)) / np.pi
    return out


def primitive_spectral(prim, k, omega, eta, pairs=None):
    """A_g (nk, nw, nsta_prim) of the primitive model itself: sum_m |u_m[g](k)|^2 L_eta(w - E_m(k)).  pairs: (E (nk, n),
    u[k][component][band]) from another solver."""
    k = np.asarray(k, dtype=float).reshape(-1, prim._dim_k)
    e, u = np.linalg.eigh(orc.ham_batch(prim, k)) if pairs is None else pairs
    return spectral(e, np.transpose(np.abs(u) ** 2, (0, 2, 1)), omega, eta)


def min_gap(e):
    """The smallest spacing of consecutive levels at any of the k-points, e (nk, n)."""
    return np.min(np.diff(np.sort(e, axis=1), axis=1)) if e.shape[1] > 1 else np.inf
