"""NumPy restatement of the Chebyshev operator functions and the local Chern marker.  TEST INFRASTRUCTURE ONLY.

f(H) v = sum_m c_m T_m(H~) v by the dense three-term recursion (what the device does on the sparse operator), the same operator
function from the eigendecomposition U f(w) U^+ (an independent route to the same numbers), the exact Fermi projector and time
evolution, and the marker c(s) = 4 pi Im (F A F B F)_ss from a dense F."""
import numpy as np

import kpm_cond_ref as kc
import kpm_ref as kr


def series_recursion(H, vectors, coeffs, bounds):
    """out[s][v] = sum_m coeffs[s][m] T_m(H~) vectors[v]: vectors (nvec, n), coeffs (nset, ncoef) -> (nset, nvec, n)."""
    c = np.atleast_2d(np.asarray(coeffs, dtype=complex))
    stack = kc.chebyshev_stack(kc.rescaled(H, bounds), np.asarray(vectors, dtype=complex).T, c.shape[1])      # (ncoef, n, nvec)
    return np.einsum("sm,miv->svi", c, stack)


def series_values(coeffs, x):
    """sum_m coeffs[s][m] T_m(x) at the points x in [-1, 1], T_m = cos(m arccos x): (nset, len(x))."""
    c = np.atleast_2d(np.asarray(coeffs, dtype=complex))
    return c @ kr.chebyshev_T(np.asarray(x, dtype=float), c.shape[1])


def series_eigen(H, vectors, coeffs, bounds):
    """The same from H = U w U^+: U f_s(x) U^+ v with f_s(x) = sum_m coeffs[s][m] T_m(x), x = (w - b) / a; (nset, nvec, n)."""
    a, b = 0.5 * (bounds[1] - bounds[0]), 0.5 * (bounds[1] + bounds[0])
    w, U = np.linalg.eigh(np.asarray(H, dtype=complex))
    f = series_values(coeffs, (w - b) / a)                                  # (nset, n)
    proj = U.conj().T @ np.asarray(vectors, dtype=complex).T                # (n, nvec)
    return np.einsum("ij,sj,jv->svi", U, f, proj)


def series_matrix(H, coeffs, bounds):
    """The dense F = sum_m coeffs[m] T_m(H~) of one coefficient set, by the recursion on the identity."""
    return series_recursion(H, np.identity(len(H)), coeffs, bounds)[0].T


def projector_exact(H, fermi_level):
    """P = sum over the levels below fermi_level of |n><n|."""
    w, U = np.linalg.eigh(np.asarray(H, dtype=complex))
    occ = U[:, w < fermi_level]
    return occ @ occ.conj().T


def evolve_exact(H, vectors, t):
    """U e^{-i w t} U^+ v: (nvec, n)."""
    w, U = np.linalg.eigh(np.asarray(H, dtype=complex))
    return ((U * np.exp(-1j * w * t)[None, :]) @ (U.conj().T @ np.asarray(vectors, dtype=complex).T)).T


def marker_dense(F, ra, rb, states=None):
    """c(s) = 4 pi Im (F A F B F)_ss, A = diag(ra), B = diag(rb), for the states `states` (default: all)."""
    c = 4.0 * np.pi * np.imag(np.einsum("si,i,ij,j,js->s", F, ra, F, rb, F))
    return c if states is None else c[np.asarray(states)]


def marker_scale(coeffs, ra, rb):
    """The size the marker can reach: 4 pi (sum_m |c_m|)^3 max|r_a| max|r_b| (||F|| <= sum |c_m| inside the bounds)."""
    return 4.0 * np.pi * np.abs(coeffs).sum() ** 3 * np.abs(ra).max() * np.abs(rb).max()


def state_coordinates(m, d):
    """The reduced coordinate along axis d of the orbital of every state (spin fastest)."""
    return np.repeat(np.asarray(m._orb)[:, d], m._nspin)


def cell_states(m, cell):
    """The states whose orbital lies in the cell with the integer corner `cell` (reduced coordinates)."""
    orb = np.repeat(np.asarray(m._orb), m._nspin, axis=0)
    hit = np.all(np.floor(orb[:, :len(cell)] + 1e-9) == np.asarray(cell)[None, :], axis=1)
    return np.nonzero(hit)[0]
