"""NumPy restatement of tb_model.mean_field_mesh on top of dm_ref (levels, fermi_level, density_matrix, hopping_table,
energy_from_density_matrix): the same map x_in -> x_out, the same mixing and the same energies.

    H_int = 1/2 sum_{a,b,R} V_ab(R) n_{a,0} n_{b,R}            D_ij(R) = <c+_{j,R} c_{i,0}>
    Hartree: eps_a += sum_{b,R} V_ab(R) n_b        Fock: t_ab(R) += -V_ab(R) D_ab(R), the mirror its conjugate

x = (n_a of the states some V touches, ascending; then Re, Im of D_ab(R) of every entry, in list order)."""
import copy

import numpy as np

import dm_ref as dmr

HIST_MAX = 8
REG = 1e-12
COEF_MAX = 1e6


def entries(m, interaction=None, U=None):
    """[(V, a, b, R)] over states, R a tuple over the periodic directions: an orbital entry couples total densities (all four spin
    pairs), U couples (o up, o down, 0)."""
    ns = m._nspin
    out = []
    for V, i, j, R in (interaction or []):
        Rp = tuple(int(x) for x in np.array(R, dtype=int)[m._per])
        for s in range(ns):
            for t in range(ns):
                out.append((float(V), i * ns + s, j * ns + t, Rp))
    if U is not None:
        Uv = np.full(m._norb, float(U)) if np.ndim(U) == 0 else np.asarray(U, dtype=float)
        for o in range(m._norb):
            out.append((float(Uv[o]), 2 * o, 2 * o + 1, (0,) * m._dim_k))
    return out


class Layout(object):
    def __init__(self, m, ent, fock):
        self.n, self.ent, self.fock = m._nsta, ent, fock
        self.touched = sorted({a for _, a, _, _ in ent} | {b for _, _, b, _ in ent})
        self.par = {a: p for p, a in enumerate(self.touched)}
        self.nocc = len(self.touched)
        self.np = self.nocc + (2 * len(ent) if fock else 0)
        self.R = [(0,) * m._dim_k]
        for _, _, _, R in ent:
            if R not in self.R:
                self.R.append(R)

    def gather(self, D):
        """x_out from D (nR, n, n) at self.R."""
        x = np.zeros(self.np)
        for a in self.touched:
            x[self.par[a]] = D[0][a, a].real
        if self.fock:
            for e, (_, a, b, R) in enumerate(self.ent):
                d = D[self.R.index(R)][a, b]
                x[self.nocc + 2 * e], x[self.nocc + 2 * e + 1] = d.real, d.imag
        return x

    def start(self, occ):
        x = np.zeros(self.np)
        occ = np.asarray(occ, dtype=float).reshape(self.n)
        for a in self.touched:
            x[self.par[a]] = occ[a]
        return x

    def row_sum(self):
        s = np.zeros(self.n)
        for V, a, b, _ in self.ent:
            s[a] += abs(V)
            s[b] += abs(V)
        return s.max()


def field_model(m, lay, x):
    """A copy of m with the field of x added."""
    ns, no = m._nspin, m._norb
    mm = copy.deepcopy(m)
    site = np.zeros((no, ns, ns), dtype=complex)
    hops = {}
    for e, (V, a, b, R) in enumerate(lay.ent):
        site[a // ns, a % ns, a % ns] += V * x[lay.par[b]]
        site[b // ns, b % ns, b % ns] += V * x[lay.par[a]]
        if not lay.fock:
            continue
        amp = -V * (x[lay.nocc + 2 * e] + 1j * x[lay.nocc + 2 * e + 1])
        if a // ns == b // ns and not any(R):
            site[a // ns, a % ns, b % ns] += amp
            site[a // ns, b % ns, a % ns] += np.conj(amp)
        else:
            hops.setdefault((a // ns, b // ns, R), np.zeros((ns, ns), dtype=complex))[a % ns, b % ns] += amp
    for o in range(no):
        mm.set_onsite(site[o] if ns == 2 else float(site[o, 0, 0].real), o, mode="add")
    for (i, j, R), blk in hops.items():
        Rf = np.zeros(m._dim_r, dtype=int)
        Rf[m._per] = R
        mm.set_hop(blk if ns == 2 else complex(blk[0, 0]), i, j, Rf, mode="add", allow_conjugate_pair=True)
    return mm


def step(m, mesh, lay, x, kT, n_electrons=None, fermi_level=None):
    """One application of the map: (x_out, mu, D, levels) of H[x]."""
    mm = field_model(m, lay, x)
    ev = dmr.levels(mm, mesh)
    mu = dmr.fermi_level(mm, mesh, n_electrons, kT, ev)[0] if n_electrons is not None else fermi_level
    D = dmr.density_matrix(mm, mesh, mu, kT, np.array(lay.R))
    return lay.gather(D), mu, D, ev


def anderson(B, cnt):
    """mf_anderson of tbk_mf.h, line by line: None where it reports failure (the linear step)."""
    d = np.zeros(cnt)
    for j in range(cnt):
        d[j] = np.sqrt(B[j, j])
        if not d[j] > 0.0 or not d[j] < 1.7e308:
            return None
    A = np.zeros((cnt, cnt + 1))
    for j in range(cnt):
        for k in range(cnt):
            A[j, k] = B[j, k] / (d[j] * d[k]) + (REG if j == k else 0.0)
        A[j, cnt] = 1.0 / d[j]
    for p in range(cnt):
        best = p
        for j in range(p + 1, cnt):
            if abs(A[j, p]) > abs(A[best, p]):
                best = j
        if not abs(A[best, p]) > 1e-14:
            return None
        if best != p:
            A[[p, best], p:] = A[[best, p], p:]
        for j in range(p + 1, cnt):
            f = A[j, p] / A[p, p]
            A[j, p:] -= f * A[p, p:]
    c = np.zeros(cnt)
    for p in range(cnt - 1, -1, -1):
        c[p] = (A[p, cnt] - np.dot(A[p, p + 1:cnt], c[p + 1:])) / A[p, p]
    c /= d
    s = c.sum()
    if not abs(s) > 0.0 or not abs(s) < 1.7e308:
        return None
    c /= s
    if not np.all(np.abs(c) <= COEF_MAX):
        return None
    return c


def run(m, mesh, interaction=None, U=None, n_electrons=None, fermi_level=None, kT=0.0, start=None, fock=True, mixing=0.5, history=4,
        tol=1e-10, max_iter=200):
    """The loop of mean_field_mesh.  Returns a dict: x_in (the field the last iteration solved in), x_out, mu, D, lay, occ history
    (iterations, nsta), residuals, energy, entropy, free_energy, converged, model."""
    lay = Layout(m, entries(m, interaction, U), fock)
    fill = dict(n_electrons=n_electrons, fermi_level=fermi_level)
    if start is None:
        x = step(m, mesh, lay, np.zeros(lay.np), kT, **fill)[0]
    elif isinstance(start, dict):                                  # a restart: the parameter vector itself
        x = np.array(start["x"], dtype=float)
    else:
        st = np.array(start, dtype=complex)
        if m._nspin == 2 and st.shape == (m._norb, 2, 2):
            x = lay.start(np.real(np.einsum("oss->os", st)))
            if fock:
                for e, (_, a, b, R) in enumerate(lay.ent):
                    if a // 2 == b // 2 and not any(R):
                        x[lay.nocc + 2 * e] = st[a // 2, a % 2, b % 2].real
                        x[lay.nocc + 2 * e + 1] = st[a // 2, a % 2, b % 2].imag
        else:
            x = lay.start(np.real(st))
    mh = history
    ringx, ringr = np.zeros((max(mh, 1), lay.np)), np.zeros((max(mh, 1), lay.np))
    gram = np.zeros((HIST_MAX, HIST_MAX))
    occ_hist, res_hist = [], []
    converged = False
    for it in range(max_iter):
        x_in = x.copy()
        x_out, mu, D, ev = step(m, mesh, lay, x_in, kT, **fill)
        r = x_out - x_in
        res_hist.append(np.max(np.abs(r)))
        occ_hist.append(np.real(np.diagonal(D[0])).copy())
        c = None
        if mh > 0:
            slot, cnt = it % mh, min(it + 1, mh)
            ringx[slot], ringr[slot] = x_in, r
            for j in range(cnt):
                gram[slot, j] = gram[j, slot] = np.dot(r, ringr[j])
            if it >= mh:
                c = anderson(gram, cnt)
        if c is None:
            x = x_in + mixing * r
        else:
            x = sum(c[j] * (ringx[j] + mixing * ringr[j]) for j in range(cnt))
        if tol > 0.0 and res_hist[-1] <= tol:
            converged = True
            break
    th = dmr.thermodynamics(field_model(m, lay, x_in), mesh, [mu], kT, ev)[:, 0]
    edc = 0.0
    for e, (V, a, b, _) in enumerate(lay.ent):
        pa, pb = lay.par[a], lay.par[b]
        t = x_in[pa] * x_out[pb] + x_in[pb] * x_out[pa] - x_out[pa] * x_out[pb]
        if fock:
            pr, pi = lay.nocc + 2 * e, lay.nocc + 2 * e + 1
            t += -2.0 * (x_in[pr] * x_out[pr] + x_in[pi] * x_out[pi]) + x_out[pr] ** 2 + x_out[pi] ** 2
        edc += V * t
    energy = th[1] - edc
    return dict(x_in=x_in, x_out=x_out, mu=mu, D=D, lay=lay, history=np.array(occ_hist), residuals=np.array(res_hist), energy=energy,
                entropy=th[2], free_energy=energy - kT * th[2], converged=converged, iterations=len(res_hist),
                model=field_model(m, lay, x_in))


def interaction_energy(lay, x):
    """sum over listed bonds of V [n_a n_b - |D_ab(R)|^2] = 1/2 sum_{a,b,R} V_ab(R) [...] (the second term with Fock only)."""
    e = 0.0
    for i, (V, a, b, _) in enumerate(lay.ent):
        t = x[lay.par[a]] * x[lay.par[b]]
        if lay.fock:
            t -= x[lay.nocc + 2 * i] ** 2 + x[lay.nocc + 2 * i + 1] ** 2
        e += V * t
    return e
