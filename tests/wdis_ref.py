"""NumPy restatement of tb_model.wannier_disentangle_mesh on the pieces of tests/wan_ref.py
(numpy.linalg.eigh, SVD, M over the star and its mirror formed explicitly) and of the b-vector shell search: the checker of
tests/test_wannier_dis.py.

    masks       win_n(k): lo <= E_n(k) <= hi;  frz_n(k): win and inside the frozen interval;  free = win and not frz
    M0(k, b) = V_bands(k)+ D_G V_bands(k + b) over the nb candidate bands,  M0(k, -b) = M0(k - b, b)+
    start       A = V_bands+ g~ with the rows outside the window zero,  U = A (A+ A)^-1/2,  P = U U+
    select(X)   the frozen unit vectors in band order, then the nw - n_frozen leading eigenvectors of X on the free indices
    iteration   Z = sum_{+-b} w_b T T+, T = M0(k, b) U_dis(k + b) of the previous iteration,  Z_in = alpha Z + (1 - alpha) Z_in
    Omega_I = (1 / N_k) sum_k sum_{+-b} w_b (nw - |U_dis(k)+ M0(k, b) U_dis(k + b)|_F^2)
    gauge       A' = U_dis+ A,  U0 = U_dis A' (A'+ A')^-1/2, then wan_ref's spread, descent, Hamiltonian and Fourier sums on
                M(k, b) = U0(k)+ M0(k, b) U0(k + b)

The basis inside the selected subspace is arbitrary (eigh's here, a Jacobi solver's on the device): only the projector
U_dis U_dis+, Omega_I and what follows the gauge step compare."""
import numpy as np

from oracle import tb_oracle as orc

import wan_ref as wr


def shells(lat, mesh):
    """(steps, weights, b Cartesian) by the shell search; lat: the periodic lattice vectors as rows.  ValueError when no star of
    positive weights is found within 6 vectors."""
    A = np.asarray(lat, dtype=float)
    dk = A.shape[0]
    N = np.asarray(mesh, dtype=float)
    rec = 2.0 * np.pi * np.linalg.inv(A @ A.T) @ A
    cand = []
    for idx in np.ndindex(*([3] * dk)):
        s = tuple(1 - i for i in idx)
        first = next((x for x in s if x != 0), 0)
        if first == 1:
            cand.append(s)
    cand = np.array(cand, dtype=int)
    b = (cand / N[None, :]) @ rec
    ln = np.linalg.norm(b, axis=1)
    groups = []
    for i in np.argsort(ln, kind="stable"):
        if groups and abs(ln[i] - ln[groups[-1][0]]) <= 1e-9 * ln[groups[-1][0]]:
            groups[-1].append(i)
        else:
            groups.append([i])
    groups = [sorted(g) for g in groups]
    iu = np.triu_indices(A.shape[1])
    rhs = np.eye(A.shape[1])[iu]
    cols, kept = [], []
    for g in groups:
        col = 2.0 * sum(np.outer(b[i], b[i]) for i in g)[iu]
        mat = np.array(cols + [col]).T
        if np.linalg.matrix_rank(mat / np.linalg.norm(mat, axis=0), tol=1e-9) <= len(cols):
            continue
        if sum(len(x) for x in kept) + len(g) > 6:
            break
        cols.append(col)
        kept.append(g)
        w = np.linalg.lstsq(mat, rhs, rcond=None)[0]
        if np.max(np.abs(mat @ w - rhs)) < 1e-12 and np.all(w > 0.0):
            pick = [i for x in kept for i in x]
            return cand[pick], np.concatenate([[w[j]] * len(x) for j, x in enumerate(kept)]), b[pick]
    raise ValueError("too skewed: no star within 6 vectors")


def star(lat, mesh, b_vectors="star"):
    return wr.bvectors(lat, mesh) if b_vectors == "star" else shells(lat, mesh)


def select(X, win, frz, nw):
    """(U_dis (nb, nw), gap) of one point from the Hermitian X (nb, nb) and its masks."""
    nb = X.shape[0]
    free = np.nonzero(win & ~frz)[0]
    fz = np.nonzero(frz)[0]
    nsel = nw - fz.size
    U = np.zeros((nb, nw), dtype=complex)
    U[fz, np.arange(fz.size)] = 1.0
    gap = np.inf
    if nsel > 0:
        lam, Q = np.linalg.eigh(X[np.ix_(free, free)])
        U[free, fz.size:] = Q[:, ::-1][:, :nsel]
        if free.size > nsel:
            gap = lam[free.size - nsel] - lam[free.size - nsel - 1]
    return U, gap


def run(m, mesh, trial, bands, window=None, frozen=None, dis_iter=200, dis_mixing=1.0, max_iter=0, check_every=10, R=None,
        functions=False, b_vectors="star"):
    dk, n = m._dim_k, m._nsta
    mesh = [int(x) for x in mesh]
    k = wr.mesh_points(m, mesh)
    nk = k.shape[0]
    ev, V = np.linalg.eigh(orc.ham_batch(m, k))
    bands = list(bands)
    nb = len(bands)
    Vb, Eb = V[:, :, bands], ev[:, bands]
    tau = wr.state_tau(m)
    terms = wr.trial_terms(m, trial)
    nw = len(terms)
    win = np.ones((nk, nb), dtype=bool) if window is None else (Eb >= window[0]) & (Eb <= window[1])
    frz = np.zeros((nk, nb), dtype=bool) if frozen is None else win & (Eb >= frozen[0]) & (Eb <= frozen[1])
    assert np.all(win.sum(axis=1) >= nw) and np.all(frz.sum(axis=1) <= nw)
    g = np.zeros((nk, n, nw), dtype=complex)
    for w, fn in enumerate(terms):
        for amp, s, Rv in fn:
            g[:, s, w] += amp * np.exp(-2j * np.pi * (k @ (Rv + tau[s])))
    A = np.einsum("kjb,kjw->kbw", Vb.conj(), g) * win[:, :, None]
    W, sv0, Zh = np.linalg.svd(A, full_matrices=False)
    U = W @ Zh
    steps, wb, bc = star(np.asarray(m._lat, dtype=float)[m._per], mesh, b_vectors)
    nbv = len(wb)
    wall, ball = np.concatenate([wb, wb]), np.concatenate([bc, -bc])
    M0 = np.zeros((nk, nbv, nb, nb), dtype=complex)
    nxt, prv = [], []
    for ib in range(nbv):
        k2, G = wr.neighbours(mesh, steps[ib])
        ph = np.exp(-2j * np.pi * (G @ tau.T))
        M0[:, ib] = np.einsum("kjm,kjn->kmn", Vb.conj(), Vb[k2] * ph[:, :, None])
        nxt.append(k2)
        prv.append(wr.neighbours(mesh, -steps[ib])[0])
    nbr = nxt + prv

    def both(Mp):
        Mm = np.stack([Mp[prv[ib], ib].conj().transpose(0, 2, 1) for ib in range(nbv)], axis=1)
        return np.concatenate([Mp, Mm], axis=1)

    M0all = both(M0)

    def omega_i(Ud):
        tot = 0.0
        for ib in range(2 * nbv):
            Mr = Ud.conj().transpose(0, 2, 1) @ M0all[:, ib] @ Ud[nbr[ib]]
            tot += wall[ib] * np.sum(nw - np.sum(np.abs(Mr) ** 2, axis=(1, 2)))
        return tot / nk

    def select_all(X):
        out = [select(X[q], win[q], frz[q], nw) for q in range(nk)]
        return np.array([o[0] for o in out]), min(o[1] for o in out)

    Ud, gap = select_all(U @ U.conj().transpose(0, 2, 1))
    dis_all = [omega_i(Ud)]
    Zin = None
    for it in range(1, dis_iter + 1):
        Z = np.zeros((nk, nb, nb), dtype=complex)
        for ib in range(2 * nbv):
            T = M0all[:, ib] @ Ud[nbr[ib]]
            Z += wall[ib] * (T @ T.conj().transpose(0, 2, 1))
        Zin = Z if Zin is None else dis_mixing * Z + (1.0 - dis_mixing) * Zin
        Ud, gap = select_all(Zin)
        dis_all.append(omega_i(Ud))
    drows = [0] + [it for it in range(1, dis_iter + 1) if it % check_every == 0 or it == dis_iter]

    # the gauge inside the subspace, then wan_ref's pipeline
    Ap = Ud.conj().transpose(0, 2, 1) @ A
    W, sv, Zh = np.linalg.svd(Ap)
    U0 = Ud @ (W @ Zh)
    ut = Vb @ U0
    Mp = np.stack([U0.conj().transpose(0, 2, 1) @ M0[:, ib] @ U0[nxt[ib]] for ib in range(nbv)], axis=1)
    Uacc = np.tile(np.eye(nw, dtype=complex), (nk, 1, 1))
    sp = wr.spread(both(Mp), wall, ball)
    hist_all = [sp[1] + sp[2] + sp[3]]
    for it in range(max_iter):
        Mall = both(Mp)
        q = sp[6]
        d = np.einsum("kbnn->kbn", Mall)
        Rm = Mall * d.conj()[:, :, None, :]
        Tm = Mall / d[:, :, None, :] * q[:, :, None, :]
        AR = 0.5 * (Rm - Rm.conj().transpose(0, 1, 3, 2))
        ST = (Tm + Tm.conj().transpose(0, 1, 3, 2)) / 2j
        Gk = 4.0 * np.einsum("b,kbmn->kmn", wall, AR - ST)
        E = wr.herm_exp(Gk / (4.0 * np.sum(wall)))
        Uacc = Uacc @ E
        for ib in range(nbv):
            Mp[:, ib] = E.conj().transpose(0, 2, 1) @ Mp[:, ib] @ E[nxt[ib]]
        sp = wr.spread(both(Mp), wall, ball)
        hist_all.append(sp[1] + sp[2] + sp[3])
    rows = [0] + [it for it in range(1, max_iter + 1) if it % check_every == 0 or it == max_iter]
    Ut = U0 @ Uacc
    HW = np.einsum("kbm,kb,kbn->kmn", Ut.conj(), Eb, Ut)
    Rl = wr.torus(mesh) if R is None else np.asarray(R, dtype=int).reshape(-1, dk)
    hop = np.einsum("rk,kmn->rmn", np.exp(-2j * np.pi * (Rl @ k.T)), HW) / nk
    out = dict(centers=sp[0], omega_i=sp[1], omega_od=sp[2], omega_d=sp[3], omega=sp[1] + sp[2] + sp[3], spreads=sp[4],
               sv_min=float(sv.min()), sv_min_projection=float(sv0.min()), history=np.array(hist_all)[rows], hoppings=hop, R_list=Rl,
               gauge=Ut, b_vectors=bc, b_weights=wb, steps=steps, dis_history=np.array(dis_all)[drows], dis_history_all=np.array(dis_all),
               dis_gap_min=float(gap), n_window=win.sum(axis=1), n_frozen=frz.sum(axis=1), frozen_mask=frz, window_mask=win, energies=Eb,
               projector=Ud @ Ud.conj().transpose(0, 2, 1))
    if functions:
        uf = ut @ Uacc
        phase = np.exp(2j * np.pi * np.einsum("rjc,kc->rjk", Rl[:, None, :] + tau[None, :, :], k))
        out["functions"] = np.einsum("rjk,kjn->rjn", phase, uf) / nk
    return out
