"""NumPy restatement of the shift- and injection-current calls (pythtb_amd.tb_model.shift_current, shift_current_mesh,
injection_current_mesh, _gen_ddham) on top of curv_ref.dham_batch, ddham_batch below, transport_ref.eigen (with its random
in-group rotations) and numpy.linalg.eigh: the checker of tests/test_shift_current.py.  k reduced, H in the convention-II form
of _gen_ham, V^a = dH/dk_a, W^{ab} = d^2H/dk_a dk_b, E_nm = E_n - E_m, G(n) the group of band n (transport_ref.group_ids).

With `same` the mask G(n) == G(m), P^a = V^a on the mask and O^a = V^a off it, R^a = O^a / E (entry by entry):
    r^b       = -i R^b
    T^{ba}    = P^a V^b + P^b V^a - V^b P^a - V^a P^b
    r^b_;a    = (i / E) (T^{ba} / E - W^{ba} + O^b R^a - R^a O^b)        off the mask, 0 on it
    X^{abc}   = (r^b)^T r^c_;a + (r^c)^T r^b_;a                          (entry by entry products with the transposes)
    Y^{abc}   = (P^a r^c)^T r^b - (r^c)^T (P^a r^b)
which are the matrix forms of the sums in the docstring of shift_current_mesh."""
import numpy as np

import curv_ref as cr
import transport_ref as tr


def ddham_batch(m, kpts, d, e):
    """d^2H/dk_d dk_e for many k: (nk, nsta, nsta), spin interleaved like curv_ref.dham_batch."""
    kpts = np.asarray(kpts, dtype=float).reshape(-1, max(m._dim_k, 1))
    nk = kpts.shape[0]
    no, ns = m._norb, m._nspin
    n = no * ns
    out = np.zeros((nk, n, n), dtype=complex)
    for hop in m._hoppings:
        amp = np.array(hop[0], dtype=complex).reshape(ns, ns)
        a, b = hop[1], hop[2]
        rv = (-np.asarray(m._orb[a], dtype=float) + np.asarray(m._orb[b], dtype=float)
              + np.array(hop[3], dtype=float))[m._per]
        ph = (2j * np.pi) ** 2 * rv[d] * rv[e] * np.exp(2j * np.pi * (kpts @ rv))
        out[:, a * ns:(a + 1) * ns, b * ns:(b + 1) * ns] += ph[:, None, None] * amp
        out[:, b * ns:(b + 1) * ns, a * ns:(a + 1) * ns] += np.conj(ph)[:, None, None] * amp.conj().T
    return out


class Point(object):
    """Eigenpairs, groups and the operators in the eigenbasis at many k; `rng` rotates every group's eigenvectors."""

    def __init__(self, m, kpts, rng=None):
        kpts = np.asarray(kpts, dtype=float).reshape(-1, m._dim_k)
        self.dk = m._dim_k
        self.e, u, self.gid = tr.eigen(m, kpts, rng)
        ut = np.conj(np.transpose(u, (0, 2, 1)))
        self.V = [ut @ cr.dham_batch(m, kpts, c) @ u for c in range(self.dk)]
        self.W = {}
        for c in range(self.dk):
            for d in range(c, self.dk):
                self.W[(c, d)] = self.W[(d, c)] = ut @ ddham_batch(m, kpts, c, d) @ u
        self.same = self.gid[:, :, None] == self.gid[:, None, :]
        de = self.e[:, :, None] - self.e[:, None, :]
        self.inv = np.where(self.same, 0.0, 1.0 / np.where(self.same, 1.0, de))

    def min_gap(self):
        """The smallest gap between neighbouring levels of different groups, per k."""
        g = np.where(np.diff(self.gid, axis=1) > 0, np.diff(self.e, axis=1), np.inf)
        return g.min(axis=1) if g.shape[1] else np.full(len(self.e), np.inf)

    def r(self, b):
        return -1j * self.V[b] * self.inv

    def r_deriv(self, b, a, grouped=True):
        """r^b_nm;a by the sum rule; grouped=False: T^{ba} in the diagonal-element (textbook) form, which depends on the
        basis inside a group."""
        V, inv = self.V, self.inv
        if grouped:
            pa, pb = V[a] * self.same, V[b] * self.same
            t = pa @ V[b] + pb @ V[a] - V[b] @ pa - V[a] @ pb
        else:
            da = np.real(np.diagonal(V[a], axis1=1, axis2=2))
            db = np.real(np.diagonal(V[b], axis1=1, axis2=2))
            t = V[b] * (da[:, :, None] - da[:, None, :]) + V[a] * (db[:, :, None] - db[:, None, :])
        ob, ra = V[b] * ~self.same, V[a] * inv
        ps = ob @ ra - ra @ ob
        return 1j * inv * (t * inv - self.W[(b, a)] + ps)

    def X(self, a, b, c, grouped=True):
        rb, rc = self.r(b), self.r(c)
        return (np.transpose(rb, (0, 2, 1)) * self.r_deriv(c, a, grouped)
                + np.transpose(rc, (0, 2, 1)) * self.r_deriv(b, a, grouped))

    def Y(self, a, b, c):
        rb, rc = self.r(b), self.r(c)
        pa = self.V[a] * self.same
        return np.transpose(pa @ rc, (0, 2, 1)) * rb - np.transpose(rc, (0, 2, 1)) * (pa @ rb)


def shift_list(m, kpts, occ, dirs, rng=None):
    """(values (nk,), sum of the terms' absolute values (nk,), smallest gap per k)."""
    pt = Point(m, kpts, rng)
    n = pt.e.shape[1]
    occ = np.atleast_1d(np.arange(n)[occ])
    rest = np.setdiff1d(np.arange(n), occ)
    x = np.imag(pt.X(*dirs))[:, occ][:, :, rest]
    return x.sum(axis=(1, 2)), np.abs(x).sum(axis=(1, 2)), pt.min_gap()


def occupations(e, mu, kT):
    return (e <= mu).astype(float) if kT == 0.0 else tr.weights(e, mu, kT)[0]


def broadening(eps, w, eta):
    return (eta / np.pi) * (1.0 / ((eps - w) ** 2 + eta ** 2) + 1.0 / ((eps + w) ** 2 + eta ** 2))


def mesh_response(m, mesh, omega, eta, mu=0.0, kT=0.0, kind=0, rng=None, comps=None, grouped=True):
    """(tensor (nw, dk, dk, dk), scale, smallest gap): K (kind 0, real) or N (kind 1, complex) over k_uniform_mesh(mesh), and the
    largest mean over the mesh of the summed terms' absolute values.  comps: the (a, b, c) to fill (default: all)."""
    pt = Point(m, m.k_uniform_mesh(mesh), rng)
    dk, e = pt.dk, pt.e
    n = e.shape[1]
    f = occupations(e, mu, kT)
    upper = np.triu(np.ones((n, n), dtype=bool), 1)[None] & ~pt.same
    fd = np.where(upper, f[:, :, None] - f[:, None, :], 0.0)           # f_n - f_m for E_m > E_n
    eps = e[:, None, :] - e[:, :, None]                                 # E_m - E_n
    omega = np.asarray(omega, dtype=float)
    out = np.zeros((len(omega), dk, dk, dk), dtype=complex if kind else float)
    scale = 0.0
    comps = comps if comps is not None else [(a, b, c) for a in range(dk) for b in range(dk) for c in range(dk)]
    for a, b, c in comps:
        t = fd * (np.imag(pt.X(a, b, c, grouped)) if kind == 0 else pt.Y(a, b, c))
        for i, w in enumerate(omega):
            d = broadening(eps, w, eta)
            out[i, a, b, c] = (t * d).sum(axis=(1, 2)).mean()
            scale = max(scale, (np.abs(t) * d).sum(axis=(1, 2)).mean())
    return out, scale, float(pt.min_gap().min())


def cartesian(m, tensor, kind=0):
    """The rank-3 transform of shift_current_mesh (with pi / 2) or injection_current_mesh (without)."""
    lat = np.array(m._lat, dtype=float)[m._per]
    vc = np.sqrt(np.linalg.det(lat @ lat.T))
    pref = (0.5 * np.pi if kind == 0 else 1.0) / ((2.0 * np.pi) ** 3 * vc)
    return pref * np.einsum("ax,by,cz,wabc->wxyz", lat, lat, lat, tensor)
