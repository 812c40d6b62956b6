"""NumPy restatement of the Kubo-formula orbital moments and orbital magnetization (pythtb_amd.tb_model.orbital_moment,
orbital_magnetization_mesh) on top of curv_ref.velocities: the checker of tests/test_orbital_magnetization.py.  k reduced,
H in the convention-II form of _gen_ham, (a, b) = dirs, P_nm = Im V^a_nm V^b_mn, Delta_nm = E_n - E_m."""
import numpy as np

import curv_ref as cr


def pair_terms(m, kpts, dirs=(0, 1)):
    """(E[nk][n], P[nk][n][n], Delta[nk][n][n], keep[nk][n][n]); keep: the pairs outside the degeneracy rule."""
    e, va, vb = cr.velocities(m, kpts, dirs)
    p = np.imag(va * np.transpose(vb, (0, 2, 1)))
    de = e[:, :, None] - e[:, None, :]
    scale = np.maximum(1.0, np.maximum(np.abs(e)[:, :, None], np.abs(e)[:, None, :]))
    return e, p, de, np.abs(de) > 1e-9 * scale


def moments(m, kpts, dirs=(0, 1)):
    """(E, m_n, Omega_n), each (nsta, nk): formula (1), and the per-band curvature of curv_ref beside it."""
    e, p, de, keep = pair_terms(m, kpts, dirs)
    safe = np.where(keep, de, 1.0)
    mom = np.where(keep, -p / safe, 0.0).sum(axis=2)                 # P_nm / (E_m - E_n)
    om = -2.0 * np.where(keep, p / safe ** 2, 0.0).sum(axis=2)
    return e.T, mom.T, om.T


def band_set(m, kpts, occ, dirs=(0, 1)):
    """(LC, IC, Omega_occ), each (nk,): formula (2), no degeneracy rule."""
    e, p, de, _ = pair_terms(m, kpts, dirs)
    n = e.shape[1]
    occ = np.arange(n)[occ]
    rest = np.setdiff1d(np.arange(n), occ)
    w = p[:, occ][:, :, rest] / de[:, occ][:, :, rest] ** 2
    lc = (w * e[:, None, rest]).sum(axis=(1, 2))
    ic = (w * e[:, occ, None]).sum(axis=(1, 2))
    return lc, ic, -2.0 * w.sum(axis=(1, 2))


def scan_t0(e, mom, om, levels):
    """Formula (3) per point, the all-pairs prefix form: sum_{E_n <= mu} [m_n + (mu - E_n) Omega_n], (nmu, nk)."""
    return np.array([np.where(e <= mu, mom + (mu - e) * om, 0.0).sum(axis=0) for mu in levels])


def scan_t0_crossing(m, kpts, levels, dirs=(0, 1)):
    """Formula (3) per point from the pairs that cross mu only: sum_{E_n <= mu < E_m} P_nm (E_n + E_m - 2 mu) / Delta^2."""
    e, p, de, keep = pair_terms(m, kpts, dirs)
    safe = np.where(keep, de, 1.0)
    out = []
    for mu in levels:
        cross = (e[:, :, None] <= mu) & (e[:, None, :] > mu) & keep
        w = np.where(cross, p * (e[:, :, None] + e[:, None, :] - 2.0 * mu) / safe ** 2, 0.0)
        out.append(w.sum(axis=(1, 2)))
    return np.array(out)


def fermi_fg(e, mu, kT):
    """(f, g) of formula (4): f = 1 / (1 + e^x), g = kT ln(1 + e^-x), x = (E - mu) / kT, both without overflow."""
    x = (e - mu) / kT
    t = np.exp(-np.abs(x))
    f = np.where(x >= 0.0, t / (1.0 + t), 1.0 / (1.0 + t))
    g = kT * np.log1p(t) + np.where(x >= 0.0, 0.0, mu - e)
    return f, g


def scan_kt(e, mom, om, levels, kT):
    """Formula (4) per point: sum_n [f_n m_n + g_n Omega_n], (nmu, nk)."""
    out = []
    for mu in levels:
        f, g = fermi_fg(e, mu, kT)
        out.append((f * mom + g * om).sum(axis=0))
    return np.array(out)


def plane_means(x, mesh, dirs=(0, 1)):
    """Means of x[..., nk] (nk = prod(mesh), k_uniform_mesh order) over the dirs planes: (...,) for a 2-D mesh, (..., N_rest)
    for a 3-D one."""
    x = np.asarray(x)
    lead = x.ndim - 1
    return x.reshape(x.shape[:-1] + tuple(mesh)).mean(axis=tuple(lead + d for d in dirs))


def flake_magnetization(flake, mu, area):
    """(1 / 2A) sum_{E <= mu} <psi| x v_y - y v_x |psi> of a finite (dim_k = 0) model for charge +1, v = i [H, r] (hbar = 1),
    with H assembled in NumPy from its onsite energies and hoppings and r from its orbitals and lattice vectors."""
    h = np.diag(np.array(flake._site_energies, dtype=float)).astype(complex)
    for hop in flake._hoppings:
        amp, i, j = complex(np.asarray(hop[0]).reshape(())), hop[1], hop[2]
        h[i, j] += amp
        h[j, i] += np.conj(amp)
    r = np.asarray(flake._orb, dtype=float) @ np.asarray(flake._lat, dtype=float)
    x, y = r[:, 0], r[:, 1]
    vx = 1j * h * (x[None, :] - x[:, None])
    vy = 1j * h * (y[None, :] - y[:, None])
    lz = x[:, None] * vy - y[:, None] * vx
    e, u = np.linalg.eigh(h)
    occ = u[:, e <= mu]
    return np.real(np.einsum("in,ij,jn->", occ.conj(), lz, occ)) / (2.0 * area)
