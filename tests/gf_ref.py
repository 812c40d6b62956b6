"""NumPy restatement of the Green's-function calls of pythtb_amd.tb_model (green_function_mesh, impurity_t_matrix_mesh,
impurity_ldos_mesh), built on the oracle's ham_batch and numpy.linalg.eigh: the checker of tests/test_green_function.py.

    G_ij(R, z) = (1 / N_k) sum_k sum_n u_n,i(k) conj(u_n,j(k)) / (z - E_n(k)) e^{-2 pi i k.(R + tau_j - tau_i)} = <i,0| (z - H)^-1 |j,R>
    g_ab = G_{i_a i_b}(R_b - R_a)        T = V (1 - g V)^-1
    ldos0[a]    = -(1 / pi) Im G_{s_a s_a}(0)
    dldos[r, a] = -(1 / pi) Im sum_{bc} G_{s_a i_b}(R_b - R_r) T_bc G_{i_c s_a}(R_r - R_c)

z is complex (z = omega + i eta for the retarded function; any z off the spectrum works).  G is the resolvent of the torus of the mesh,
whose Hamiltonian torus_hamiltonian builds from the hopping table."""
import numpy as np

import dm_ref as dmr
from oracle import tb_oracle as orc


def eigenpairs(m, mesh):
    """(k points (nk, dim_k), E (nk, n), u[k][i][n])."""
    kk = dmr.mesh_points(m, mesh)
    e, u = np.linalg.eigh(orc.ham_batch(m, kk))
    return kk, e, u


def green(m, mesh, z, R_list=None, states=None, pairs=None):
    """G (nw, nR, na, na) at the complex energies z and the lattice vectors of R_list (None: R = 0 alone)."""
    kk, e, u = eigenpairs(m, mesh) if pairs is None else pairs
    zs = np.atleast_1d(np.asarray(z, dtype=complex))
    Rs = np.zeros((1, m._dim_k)) if R_list is None else np.asarray(R_list, dtype=float).reshape(-1, m._dim_k)
    n = e.shape[1]
    sel = np.arange(n) if states is None else np.asarray(states) % n
    tau = dmr.state_positions(m)[sel]
    dt = tau[None, :, :] - tau[:, None, :]                       # (tau_j - tau_i)[i][j]
    us = u[:, sel, :]
    out = np.zeros((len(zs), len(Rs), len(sel), len(sel)), dtype=complex)
    for r, R in enumerate(Rs):
        ph = np.exp(-2.0j * np.pi * np.einsum("kd,ijd->kij", kk, R[None, None, :] + dt))
        for w, zz in enumerate(zs):
            p = (us / (zz - e)[:, None, :]) @ np.conj(np.transpose(us, (0, 2, 1)))
            out[w, r] = (p * ph).sum(axis=0) / len(kk)
    return out


def _site_arrays(m, sites):
    n = m._nsta
    st = np.array([s % n for s, _ in sites], dtype=int)
    Rs = np.array([R for _, R in sites], dtype=int).reshape(len(sites), m._dim_k)
    return st, Rs


def _potential(V, ns):
    v = np.array(V, dtype=complex)
    return np.diag(v) if v.ndim == 1 else v.reshape(ns, ns)


def t_matrix(m, mesh, z, sites, V, pairs=None):
    """(T (nw, ns, ns), det (nw,), cond (nw,)): cond is the 2-norm condition number of 1 - g V."""
    pairs = eigenpairs(m, mesh) if pairs is None else pairs
    zs = np.atleast_1d(np.asarray(z, dtype=complex))
    st, Rs = _site_arrays(m, sites)
    ns = len(st)
    v = _potential(V, ns)
    diffs = np.array([Rs[b] - Rs[a] for a in range(ns) for b in range(ns)])
    gall = green(m, mesh, zs, diffs, None, pairs)
    T = np.zeros((len(zs), ns, ns), dtype=complex)
    det = np.zeros(len(zs), dtype=complex)
    cond = np.zeros(len(zs))
    for w in range(len(zs)):
        g = np.array([[gall[w, a * ns + b, st[a], st[b]] for b in range(ns)] for a in range(ns)])
        a1 = np.identity(ns) - g @ v
        T[w] = v @ np.linalg.inv(a1)
        det[w] = np.linalg.det(a1)
        cond[w] = np.linalg.cond(a1)
    return T, det, cond


def impurity_ldos(m, mesh, z, sites, V, R_list=None, states=None, pairs=None):
    """(ldos0 (nw, na), dldos (nw, nR, na))."""
    pairs = eigenpairs(m, mesh) if pairs is None else pairs
    zs = np.atleast_1d(np.asarray(z, dtype=complex))
    n = m._nsta
    st, Rs = _site_arrays(m, sites)
    ns = len(st)
    Rp = np.zeros((1, m._dim_k), dtype=int) if R_list is None else np.asarray(R_list, dtype=int).reshape(-1, m._dim_k)
    sel = np.arange(n) if states is None else np.asarray(states) % n
    T = t_matrix(m, mesh, zs, sites, V, pairs)[0]
    g0 = green(m, mesh, zs, None, None, pairs)[:, 0]
    ldos0 = -np.imag(g0[:, sel, sel]) / np.pi
    dldos = np.zeros((len(zs), len(Rp), len(sel)))
    for r, R in enumerate(Rp):
        gout = green(m, mesh, zs, Rs - R, None, pairs)             # [w][b]: G(R_b - R_r)
        gin = green(m, mesh, zs, R - Rs, None, pairs)              # [w][c]: G(R_r - R_c)
        for w in range(len(zs)):
            for a, s in enumerate(sel):
                left = np.array([gout[w, b, s, st[b]] for b in range(ns)])
                right = np.array([gin[w, c, st[c], s] for c in range(ns)])
                dldos[w, r, a] = -np.imag(left @ T[w] @ right) / np.pi
    return ldos0, dldos


def cells(mesh):
    """The cells of the torus in C order, (ncell, dim_k)."""
    return np.array(np.meshgrid(*[np.arange(x) for x in mesh], indexing="ij")).reshape(len(mesh), -1).T


def torus_hamiltonian(m, mesh):
    """H_T ((ncell n, ncell n), cell-major in the order of `cells`): the block from cell c to cell c + R mod mesh is t(R)."""
    mesh = np.asarray(mesh, dtype=int)
    cs = cells(mesh)
    n = m._nsta
    index = {tuple(c): i for i, c in enumerate(cs)}
    h = np.zeros((len(cs) * n, len(cs) * n), dtype=complex)
    for R, t in dmr.hopping_table(m):
        for i, c in enumerate(cs):
            j = index[tuple((c + np.array(R)) % mesh)]
            h[i * n:(i + 1) * n, j * n:(j + 1) * n] += t
    assert np.max(np.abs(h - h.conj().T)) <= 1e-14
    return h


def torus_with_impurity(m, mesh, sites, V):
    """H_T + V, the impurity's sites at (R_a mod mesh, state i_a)."""
    mesh = np.asarray(mesh, dtype=int)
    cs = cells(mesh)
    n = m._nsta
    index = {tuple(c): i for i, c in enumerate(cs)}
    st, Rs = _site_arrays(m, sites)
    at = [index[tuple(Rs[a] % mesh)] * n + st[a] for a in range(len(st))]
    h = torus_hamiltonian(m, mesh)
    h[np.ix_(at, at)] += _potential(V, len(st))
    return h
