"""NumPy restatement of the Kubo-formula spin Berry curvature (pythtb_amd.tb_model.spin_berry_curvature): curv_ref's formulas
with the first velocity replaced by the spin current J^{s,a} = (S dH_a + dH_a S) / 2, S = 1_orb (x) s.sigma.  The checker of
tests/test_spin_hall.py.  k in reduced coordinates, H in the convention-II form of _gen_ham, spin index innermost."""
import numpy as np

import curv_ref as cr
from oracle import tb_oracle as orc

PAULI = np.array([[[0, 1], [1, 0]], [[0, -1j], [1j, 0]], [[1, 0], [0, -1]]], dtype=complex)


def spin_vector(spin):
    """0, 1, 2 (sigma_x, sigma_y, sigma_z) or a real 3-vector, as a float 3-vector."""
    if np.ndim(spin) == 0:
        v = np.zeros(3)
        v[int(spin)] = 1.0
        return v
    return np.asarray(spin, dtype=float).reshape(3)


def spin_op(m, spin):
    """S = 1_orb (x) s.sigma, (nsta, nsta).  spin=None: the identity (the charge current)."""
    if spin is None:
        return np.identity(m._norb * m._nspin, dtype=complex)
    assert m._nspin == 2
    return np.kron(np.identity(m._norb), np.tensordot(spin_vector(spin), PAULI, axes=1))


def jham_batch(m, kpts, d, spin):
    """J^{s,d} = (S dH/dk_d + dH/dk_d S) / 2 for many k: (nk, nsta, nsta)."""
    s = spin_op(m, spin)
    dh = cr.dham_batch(m, kpts, d)
    return 0.5 * (s @ dh + dh @ s)


def spin_curvature(m, kpts, spin=2, dirs=(0, 1), occ=None):
    """Formula (1) per band, (nsta, nk), or formula (2) for the band set occ, (nk,), with J^{s,a} for V^a."""
    e, u = np.linalg.eigh(orc.ham_batch(m, kpts))
    ja = np.einsum("kin,kij,kjm->knm", u.conj(), jham_batch(m, kpts, dirs[0], spin), u)
    vb = np.einsum("kin,kij,kjm->knm", u.conj(), cr.dham_batch(m, kpts, dirs[1]), u)
    n = e.shape[1]
    de = e[:, :, None] - e[:, None, :]
    prod = np.imag(ja * np.transpose(vb, (0, 2, 1)))       # Im J^a_nm V^b_mn
    if occ is None:
        scale = np.maximum(1.0, np.maximum(np.abs(e)[:, :, None], np.abs(e)[:, None, :]))
        keep = np.abs(de) > 1e-9 * scale
        with np.errstate(divide="ignore", invalid="ignore"):
            term = np.where(keep, prod / np.where(keep, de, 1.0) ** 2, 0.0)
        return (-2.0 * term.sum(axis=2)).T
    occ = np.arange(n)[occ]
    rest = np.setdiff1d(np.arange(n), occ)
    sub = prod[:, occ][:, :, rest] / de[:, occ][:, :, rest] ** 2
    return -2.0 * sub.sum(axis=(1, 2))


def fermi_scan(m, kpts, levels, spin=2, dirs=(0, 1)):
    """T = 0 scan I^s(mu) = mean_k sum_{n: E_n(k) <= mu} Omega^s_n(k) for every level, (nmu,)."""
    om = spin_curvature(m, kpts, spin, dirs)
    ev = np.linalg.eigvalsh(orc.ham_batch(m, kpts)).T
    return np.array([np.sum(np.where(ev <= mu, om, 0.0)) / ev.shape[1] for mu in levels])


def band_gaps(m, kpts):
    """Per (band, k): the smaller of the band's two neighbouring gaps, (nsta, nk), with curv_ref.smallest_gap's treatment of
    degenerate neighbours (they fall under the rule of (1) and do not count).  Its minimum over the bands is smallest_gap."""
    e = np.linalg.eigvalsh(orc.ham_batch(m, kpts))
    g = np.diff(e, axis=1)
    g = np.where(g > 1e-9 * np.maximum(1.0, np.abs(e[:, 1:])), g, np.inf)
    pad = np.full((len(e), 1), np.inf)
    return np.minimum(np.hstack([pad, g]), np.hstack([g, pad])).T
