"""NumPy restatement of the exciton calls of pythtb_amd.tb_model (exciton_apply_mesh, exciton_states_mesh, exciton_spectrum_mesh):
the checker of tests/test_excitons.py.  H_ex is built by the O(N_t^2) definition from numpy.linalg.eigh of H(k) -- deliberately not
by the real-space route the device takes:

    H_ex = Delta + K^x - K^d,   t = (k, v, c),   E = both directions (a, b, R), (b, a, -R) of every bond,  d_e = R + tau_b - tau_a
    K^d_tt' = (1/N) sum_e V_e e^{2 pi i (k-k').d_e} conj(u_ck[a]) u_c'k'[a] u_vk[b] conj(u_v'k'[b])
    K^x_tt' = (1/N) sum_e V_e conj(u_ck[a]) u_vk[a] conj(u_v'k'[b]) u_c'k'[b]
    D^a_t   = <u_ck| dH/dk_a |u_vk> / Delta_t
    chi_ab(w) = (1/N) <D^a| (H_ex - w - i eta)^-1 |D^b>

and the Lanczos recurrence with its continued fraction."""
import numpy as np

import dm_ref as dmr
import mf_ref as mfr


def ham_and_dham(m, kk, pert=None):
    """H[k] and dH/dk_a[a][k] from the hopping table; pert: a Hermitian matrix added to every H(k)."""
    tau = dmr.state_positions(m)
    n, dk = tau.shape[0], m._dim_k
    H = np.zeros((len(kk), n, n), dtype=complex)
    dH = np.zeros((dk, len(kk), n, n), dtype=complex)
    dt = tau[None, :, :] - tau[:, None, :]                               # (tau_b - tau_a)[a][b]
    for R, t in dmr.hopping_table(m):
        d = np.asarray(R, dtype=float)[None, None, :] + dt               # [a][b][dim]
        ph = np.exp(2.0j * np.pi * np.einsum("kd,abd->kab", kk, d)) * t[None]
        H += ph
        for a in range(dk):
            dH[a] += 2.0j * np.pi * d[None, :, :, a] * ph
    if pert is not None:
        H = H + pert[None]
    return H, dH


def hermitian_noise(n, seed, norm):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    a = a + a.conj().T
    return a * (norm / np.linalg.norm(a, 2))


def select(n, nocc, valence, conduction):
    v = list(range(nocc)) if valence is None else (list(range(nocc - valence, nocc)) if np.ndim(valence) == 0 else sorted(valence))
    c = list(range(nocc, n)) if conduction is None else (list(range(nocc, nocc + conduction)) if np.ndim(conduction) == 0
                                                          else sorted(conduction))
    return v, c


class Problem(object):
    """kk, E[k][n], u[k][orbital][band] (the reference's own eigenvectors, or `evec` in the layout of solve_all: [band][k][orbital]),
    v / c band lists, gaps[k][v][c], D[a][t], H (N_t, N_t)."""

    def __init__(self, m, mesh, interaction=None, U=None, fermi_level=0.0, valence=None, conduction=None, direct=True, exchange=True,
                 pert=None, evec=None, min_separation=0.05):
        kk = dmr.mesh_points(m, mesh)
        N = len(kk)
        Hk, dH = ham_and_dham(m, kk, pert)
        E, u = np.linalg.eigh(Hk)
        if evec is not None:
            u = np.transpose(np.asarray(evec).reshape(E.shape[1], N, E.shape[1]), (1, 2, 0))
        n = E.shape[1]
        cnt = (E <= fermi_level).sum(axis=1)
        assert np.all(cnt == cnt[0]), "not an insulator"
        self.nocc = int(cnt[0])
        v, c = select(n, self.nocc, valence, conduction)
        sel = v + c
        rest = [b for b in range(n) if b not in sel]
        if rest and min_separation:
            sep = np.min(np.abs(E[:, sel][:, :, None] - E[:, rest][:, None, :]))
            assert sep >= min_separation, "the selected bands come within %g of the others" % sep
        nv, nc = len(v), len(c)
        self.kk, self.E, self.u, self.v, self.c, self.N, self.mesh = kk, E, u, v, c, N, list(mesh)
        uv, uc = u[:, :, v], u[:, :, c]                                  # [k][orbital][band]
        self.gaps = E[:, None, c] - E[:, v, None]                        # [k][v][c]
        nt = N * nv * nc
        self.nt, self.nv, self.nc = nt, nv, nc
        self.D = np.stack([np.einsum("kac,kab,kbv->kvc", uc.conj(), dH[a], uv) / self.gaps for a in range(m._dim_k)]).reshape(m._dim_k, nt)
        tau = dmr.state_positions(m)
        Kd = np.zeros((N, nv, nc, N, nv, nc), dtype=complex)
        Kx = np.zeros_like(Kd)
        for V, a0, b0, R in mfr.entries(m, interaction, U):
            for a, b, Rr in ((a0, b0, np.asarray(R, dtype=float)), (b0, a0, -np.asarray(R, dtype=float))):
                d = Rr + tau[b] - tau[a]
                ph = np.exp(2.0j * np.pi * (kk @ d))
                left = ph[:, None, None] * uc[:, a, None, :].conj() * uv[:, b, :, None]              # [k][v][c]
                right = ph.conj()[:, None, None] * uc[:, a, None, :] * uv[:, b, :, None].conj()
                Kd += V * left[:, :, :, None, None, None] * right[None, None, None]
                lx = uc[:, a, None, :].conj() * uv[:, a, :, None]
                rx = uv[:, b, :, None].conj() * uc[:, b, None, :]
                Kx += V * lx[:, :, :, None, None, None] * rx[None, None, None]
        self.Kd, self.Kx = Kd.reshape(nt, nt) / N, Kx.reshape(nt, nt) / N
        self.H = np.diag(self.gaps.reshape(nt)).astype(complex)
        if exchange:
            self.H = self.H + self.Kx
        if direct:
            self.H = self.H - self.Kd
        self.gap = float(self.gaps.min())

    def states(self):
        w, A = np.linalg.eigh(self.H)
        return w, A, np.einsum("tl,at->la", A.conj(), self.D)            # energies, vectors A[t][lambda], d[lambda][a]

    def chi(self, omega, eta):
        """chi[w][a][b] by the dense resolvent."""
        w, A, d = self.states()
        res = 1.0 / (w[None, :] - np.asarray(omega)[:, None] - 1j * eta)
        return np.einsum("la,lb,wl->wab", d.conj(), d, res) / self.N

    def dipole_norm(self):
        return self.D.conj() @ self.D.T / self.N

    def to_orbital(self, X):
        """The gauge-invariant form of X[..., k, v, c]: sum_vc X_vc u_c[a] conj(u_v[b]) -> [..., k, a, b]."""
        X = np.asarray(X).reshape(X.shape[:X.ndim - len(self.mesh) - 2] + (self.N, self.nv, self.nc))
        return np.einsum("...kvc,kac,kbv->...kab", X, self.u[:, :, self.c], self.u[:, :, self.v].conj())


def lanczos(H, start, n_steps, floor=0.0):
    """alpha, beta, |start|^2, n_used of the recurrence the device runs: beta_j = |H q_j - alpha_j q_j - beta_{j-1} q_{j-1}|; a run whose
    beta falls below 1e-10 max(largest |alpha| so far, floor) ends."""
    alpha, beta = np.zeros(n_steps), np.zeros(n_steps)
    nrm = np.linalg.norm(start)
    q, qp, bp, amax, used = start / nrm, np.zeros_like(start), 0.0, floor, n_steps
    for j in range(n_steps):
        y = H @ q
        alpha[j] = np.vdot(q, y).real
        w = y - alpha[j] * q - bp * qp
        beta[j] = np.linalg.norm(w)
        amax = max(amax, abs(alpha[j]))
        if beta[j] < 1e-10 * amax:
            used = j + 1
            break
        qp, q, bp = q, w / beta[j], beta[j]
    return alpha, beta, nrm ** 2, used


def cfrac(alpha, beta, norm2, used, z):
    z = np.asarray(z, dtype=complex)
    d = alpha[used - 1] - z
    for j in range(used - 2, -1, -1):
        d = alpha[j] - z - beta[j] ** 2 / d
    return norm2 / d


def chi_lanczos(P, omega, eta, n_steps):
    """chi[w][a][b] by the recurrence: the runs and the polarisation algebra of the device."""
    dk = P.D.shape[0]
    z = np.asarray(omega) + 1j * eta
    floor = float(P.gaps.max())
    g = lambda s: cfrac(*lanczos(P.H, s, n_steps, floor), z)
    out = np.zeros((len(z), dk, dk), dtype=complex)
    ga = [g(P.D[a]) for a in range(dk)]
    for a in range(dk):
        out[:, a, a] = ga[a]
        for b in range(a + 1, dk):
            S = g(P.D[a] + P.D[b]) - ga[a] - ga[b]
            T = g(P.D[a] + 1j * P.D[b]) - ga[a] - ga[b]
            out[:, a, b], out[:, b, a] = 0.5 * (S - 1j * T), 0.5 * (S + 1j * T)
    return out / P.N
