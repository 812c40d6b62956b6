"""NumPy restatement of tb_model.bdg_mesh on top of dm_ref (density_matrix, levels, fermi, entropy) and mf_ref (entries, field_model,
anderson): the same map x_in -> x_out, the same mixing and the same energies.  The Nambu model of an x is
built by tb_model.nambu_model (held by test_bdg.py against the oracle's ham_batch), solved by numpy.linalg.eigh inside
dm_ref.density_matrix at the Fermi level 0, and the loop runs line by line.

    Psi = (c, c+): particle a, hole n + a.  D = the density matrix of the Nambu model at 0:
    n_a = D_aa(0)      <c+_{b,R} c_{a,0}> = D_ab(R)      F_ab(R) = <c_{b,R} c_{a,0}> = D_{a,n+b}(R)
    Hartree: eps_a += sum V n_b      Fock: t_ab(R) += -V D_ab(R)      pairing: Delta_ab(R) = V F_ab(R)

x = (n_a of the touched states, ascending; Re, Im of D_ab(R) per entry with fock; Re, Im of F_ab(R) per entry with pairing; mu last
with n_electrons)."""
import numpy as np

import dm_ref as dmr
import mf_ref as mfr


class Layout(object):
    def __init__(self, m, ent, hartree, fock, pairing, have_nel):
        self.n, self.ent, self.hartree, self.fock, self.pairing, self.have_nel = m._nsta, ent, hartree, fock, pairing, have_nel
        self.touched = sorted({a for _, a, _, _ in ent} | {b for _, _, b, _ in ent})
        self.par = {a: p for p, a in enumerate(self.touched)}
        self.nocc = len(self.touched)
        ne = len(ent)
        self.par_d = self.nocc if fock else -1
        self.par_f = self.nocc + (2 * ne if fock else 0) if pairing else -1
        self.np = self.nocc + 2 * ne * (int(fock) + int(pairing)) + int(have_nel)
        self.par_mu = self.np - 1 if have_nel else -1
        self.R = [(0,) * m._dim_k]
        for _, _, _, R in ent:
            if R not in self.R:
                self.R.append(R)
        # mf_ref's layout of the normal-state field (occupations, then D): the leading part of x
        self.mf = mfr.Layout(m, ent, fock)

    def D(self, x, e):
        return x[self.par_d + 2 * e] + 1j * x[self.par_d + 2 * e + 1]

    def F(self, x, e):
        return x[self.par_f + 2 * e] + 1j * x[self.par_f + 2 * e + 1]


def models(m, lay, x, fermi_level):
    """(normal model with the Hartree / Fock field of x, its Nambu model at mu with the pairing field of x, the pairing list)."""
    y = np.array(x[:lay.mf.np], dtype=float)
    if not lay.hartree:
        y[:lay.nocc] = 0.0
    normal = mfr.field_model(m, lay.mf, y)
    mu = x[lay.par_mu] if lay.have_nel else fermi_level
    pair = []
    if lay.pairing:
        for e, (V, a, b, R) in enumerate(lay.ent):
            Rf = np.zeros(m._dim_r, dtype=int)
            Rf[m._per] = R
            pair.append((V * lay.F(x, e), a, b, Rf))
    return normal, normal.nambu_model(mu, pair), pair


def step(m, mesh, lay, x, kT, n_electrons, fermi_level, mu_step):
    """One application of the map: (x_out, the Nambu density matrix at lay.R)."""
    n = lay.n
    nambu = models(m, lay, x, fermi_level)[1]
    D = dmr.density_matrix(nambu, mesh, 0.0, kT, np.array(lay.R))
    out = np.zeros(lay.np)
    for a in lay.touched:
        out[lay.par[a]] = D[0][a, a].real
    for e, (_, a, b, R) in enumerate(lay.ent):
        r = lay.R.index(R)
        if lay.fock:
            out[lay.par_d + 2 * e], out[lay.par_d + 2 * e + 1] = D[r][a, b].real, D[r][a, b].imag
        if lay.pairing:
            out[lay.par_f + 2 * e], out[lay.par_f + 2 * e + 1] = D[r][a, n + b].real, D[r][a, n + b].imag
    occ = np.real(np.diagonal(D[0]))[:n].copy()
    if lay.have_nel:
        out[lay.par_mu] = x[lay.par_mu] + mu_step * (n_electrons - occ.sum())
    return out, D, occ, nambu


def start_vector(m, lay, n_electrons, start=None, pairing_seed=0.1, mu_start=None):
    n, ns = lay.n, m._nspin
    occ = np.full(n, n_electrons / n if lay.have_nel else 0.5) if start is None else np.asarray(start, dtype=float).reshape(n)
    x = np.zeros(lay.np)
    for a in lay.touched:
        x[lay.par[a]] = occ[a]
    if lay.pairing:
        x[lay.par_f:lay.par_f + 2 * len(lay.ent):2] = pairing_seed
    if lay.have_nel:
        if mu_start is None:
            eps = np.array([np.real(np.array(m._site_energies[a // ns]).reshape(ns, ns)[a % ns, a % ns]) for a in range(n)])
            shift = np.zeros(n)
            if lay.hartree:
                for V, a, b, _ in lay.ent:
                    shift[a] += V * occ[b]
                    shift[b] += V * occ[a]
            x[lay.par_mu] = np.mean(eps) + np.mean(shift)
        else:
            x[lay.par_mu] = mu_start
    return x


def run(m, mesh, interaction=None, U=None, n_electrons=None, fermi_level=None, kT=0.0, hartree=True, fock=False, pairing=True, start=None,
        pairing_seed=0.1, mu_start=None, mu_step=1.0, mixing=0.5, history=4, tol=1e-10, max_iter=200):
    """The loop of bdg_mesh.  Returns a dict: x_in (the field the last iteration solved in), x_out, lay, D (the Nambu density matrix of
    the last iteration at lay.R), history (iterations, nsta), residuals, mu (of x_in), n_electrons (N_out), gap, energy, entropy,
    free_energy, grand_potential, converged, iterations, model (the Nambu model of x_in), normal_model."""
    have_nel = n_electrons is not None
    lay = Layout(m, mfr.entries(m, interaction, U), hartree, fock, pairing, have_nel)
    x = np.array(start["x"], dtype=float) if isinstance(start, dict) else start_vector(m, lay, n_electrons, start, pairing_seed, mu_start)
    mh = history
    ringx, ringr = np.zeros((max(mh, 1), lay.np)), np.zeros((max(mh, 1), lay.np))
    gram = np.zeros((mfr.HIST_MAX, mfr.HIST_MAX))
    occ_hist, res_hist = [], []
    converged = False
    for it in range(max_iter):
        x_in = x.copy()
        x_out, D, occ, nambu = step(m, mesh, lay, x_in, kT, n_electrons, fermi_level, mu_step)
        r = x_out - x_in
        res_hist.append(np.max(np.abs(r)))
        occ_hist.append(occ)
        c = None
        if mh > 0:
            slot, cnt = it % mh, min(it + 1, mh)
            ringx[slot], ringr[slot] = x_in, r
            for j in range(cnt):
                gram[slot, j] = gram[j, slot] = np.dot(r, ringr[j])
            if it >= mh:
                c = mfr.anderson(gram, cnt)
        if c is None:
            x = x_in + mixing * r
        else:
            x = sum(c[j] * (ringx[j] + mixing * ringr[j]) for j in range(cnt))
        if tol > 0.0 and res_hist[-1] <= tol:
            converged = True
            break
    # <H - mu N> = 1/2 (1/N_k) sum f E + 1/2 sum_a (eps_a + d eps_a^in - mu_in) - sum_e V [...]
    n, ns = lay.n, m._nspin
    ev = dmr.levels(nambu, mesh)
    mu_in = x_in[lay.par_mu] if have_nel else fermi_level
    eps = np.array([np.real(np.array(m._site_energies[a // ns]).reshape(ns, ns)[a % ns, a % ns]) for a in range(n)])
    tr = eps.sum() - n * mu_in
    edc = 0.0
    for e, (V, a, b, _) in enumerate(lay.ent):
        pa, pb = lay.par[a], lay.par[b]
        t = 0.0
        if hartree:
            tr += V * (x_in[pa] + x_in[pb])
            t += x_in[pa] * x_out[pb] + x_in[pb] * x_out[pa] - x_out[pa] * x_out[pb]
        if fock:
            t += -2.0 * np.real(np.conj(lay.D(x_in, e)) * lay.D(x_out, e)) + abs(lay.D(x_out, e)) ** 2
        if pairing:
            t += 2.0 * np.real(np.conj(lay.F(x_in, e)) * lay.F(x_out, e)) - abs(lay.F(x_out, e)) ** 2
        edc += V * t
    nk = ev.shape[0]
    omega = 0.5 * (dmr.fermi(ev, 0.0, kT) * ev).sum() / nk + 0.5 * tr - edc
    ent = 0.5 * dmr.entropy(ev, 0.0, kT).sum() / nk
    nout = occ.sum()
    energy = omega + mu_in * nout
    normal = models(m, lay, x_in, fermi_level)[0]
    return dict(x_in=x_in, x_out=x_out, lay=lay, D=D, history=np.array(occ_hist), residuals=np.array(res_hist), mu=mu_in, n_electrons=nout,
                gap=np.min(np.abs(ev)), energy=energy, entropy=ent, free_energy=energy - kT * ent,
                grand_potential=energy - kT * ent - mu_in * nout, converged=converged, iterations=len(res_hist), model=nambu,
                normal_model=normal)
