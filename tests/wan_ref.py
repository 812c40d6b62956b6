"""NumPy restatement of tb_model.wannier_mesh on the oracle's ham_batch, numpy.linalg.eigh and SVD: the
checker of tests/test_wannier.py.  Every sum over b-vectors runs over the star AND its mirror, explicitly, with
M(k, -b) = M(k - b, b)+ formed as a matrix; the device only ever walks the +b half.

    g~_n(k)[j] = sum amp e^{-2 pi i k.(R + tau_j)}      A = V_bands+ g~      U = A (A+ A)^-1/2      u~ = V_bands U
    M(k, b) = u~(k)+ D_G u~(k + b),  D_G = diag e^{-2 pi i G.tau_j} where k + b leaves the zone by G
    r_n = -(1 / N_k) sum_{k,b} w_b b Im ln M_nn          Omega_I = (1 / N_k) sum w_b (nw - sum_mn |M_mn|^2)
    Omega_OD = (1 / N_k) sum w_b sum_{m != n} |M_mn|^2    Omega_D = (1 / N_k) sum w_b sum_n (Im ln M_nn + b.r_n)^2
    G = 4 sum_b w_b (A[R] - S[T]),  dW = G / (4 sum_b w_b),  U <- U e^{dW},  M(k, b) <- e^{-dW(k)} M e^{dW(k + b)}"""
import numpy as np

from oracle import tb_oracle as orc


def mesh_points(m, mesh):
    return np.asarray(m.k_uniform_mesh(mesh), dtype=float).reshape(-1, m._dim_k)


def state_tau(m):
    """(nsta, dim_k): the reduced position of every state's orbital along the periodic directions."""
    return np.repeat(np.asarray(m._orb, dtype=float)[:, m._per], m._nspin, axis=0)


def bvectors(lat, mesh):
    """(steps, weights, b Cartesian) by the closed-form rule; lat: the periodic lattice vectors as rows."""
    A = np.asarray(lat, dtype=float)
    dk = A.shape[0]
    N = np.asarray(mesh, dtype=float)
    S = (A @ A.T) * np.outer(N, N) / (2.0 * np.pi) ** 2
    rec = 2.0 * np.pi * np.linalg.inv(A @ A.T) @ A
    steps, w = [], []
    for a in range(dk):
        s = np.zeros(dk, dtype=int)
        s[a] = 1
        steps.append(s)
        w.append(0.5 * S[a, a] - 0.5 * (np.sum(np.abs(S[a])) - abs(S[a, a])))
    for a in range(dk):
        for b in range(a + 1, dk):
            if S[a, b] != 0.0:
                s = np.zeros(dk, dtype=int)
                s[a], s[b] = 1, int(np.sign(S[a, b]))
                steps.append(s)
                w.append(0.5 * abs(S[a, b]))
    steps = np.array(steps)
    if min(w) <= 0.0:
        raise ValueError("too skewed")
    return steps, np.array(w), (steps / N[None, :]) @ rec


def trial_terms(m, trial):
    """Per function a list of (amp, state, R over the periodic directions) from any of the accepted forms."""
    dk = m._dim_k
    try:
        arr = np.array(trial)
    except ValueError:
        arr = None
    if arr is not None and arr.dtype != object and arr.ndim == 1:
        return [[(1.0, int(s), np.zeros(dk, dtype=int))] for s in arr]
    if arr is not None and arr.dtype != object and arr.ndim == 2:
        return [[(complex(arr[j, w]), j, np.zeros(dk, dtype=int)) for j in range(arr.shape[0]) if arr[j, w] != 0] for w in range(arr.shape[1])]
    return [[(complex(a), int(s), np.atleast_1d(np.array(R, dtype=int))[m._per]) for a, s, R in fn] for fn in trial]


def torus(mesh):
    axes = [np.arange(-((int(n) - 1) // 2), int(n) // 2 + 1) for n in mesh]
    grid = np.meshgrid(*axes, indexing="ij")
    return np.stack([g.reshape(-1) for g in grid], axis=1)


def neighbours(mesh, step):
    """(index of k + b, G (nk, dk)) for every point in k_uniform_mesh order."""
    mesh = np.asarray(mesh, dtype=int)
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in mesh], indexing="ij"), axis=-1).reshape(-1, mesh.size)
    j = idx + np.asarray(step, dtype=int)[None, :]
    G = np.floor_divide(j, mesh[None, :])
    return np.ravel_multi_index(tuple((j - G * mesh[None, :]).T), tuple(mesh)), G


def herm_exp(dW):
    """e^{dW} of anti-Hermitian dW (batched), exactly unitary: from the eigen-decomposition of i dW."""
    lam, Q = np.linalg.eigh(1j * dW)
    return np.einsum("kij,kj,klj->kil", Q, np.exp(-1j * lam), Q.conj())


def spread(Mall, wall, ball):
    """(centres (nw, dim_r), Omega_I, Omega_OD, Omega_D, spreads (nw,), phi, q) from M over the star and its mirror."""
    nk, nb2, nw, _ = Mall.shape
    d = np.einsum("kbnn->kbn", Mall)
    phi = np.angle(d)
    r = -np.einsum("b,bc,kbn->nc", wall, ball, phi) / nk
    oi = np.sum(wall[None, :] * (nw - np.sum(np.abs(Mall) ** 2, axis=(2, 3)))) / nk
    ood = np.sum(wall[None, :] * (np.sum(np.abs(Mall) ** 2, axis=(2, 3)) - np.sum(np.abs(d) ** 2, axis=2))) / nk
    q = phi + np.einsum("bc,nc->bn", ball, r)[None, :, :]
    od = np.sum(wall[None, :, None] * q ** 2) / nk
    r2 = np.einsum("b,kbn->n", wall, (1.0 - np.abs(d) ** 2) + phi ** 2) / nk
    return r, oi, ood, od, r2 - np.sum(r ** 2, axis=1), phi, q


def run(m, mesh, trial, bands, max_iter=0, check_every=10, R=None, functions=False):
    dk, n = m._dim_k, m._nsta
    mesh = [int(x) for x in mesh]
    k = mesh_points(m, mesh)
    nk = k.shape[0]
    ev, V = np.linalg.eigh(orc.ham_batch(m, k))
    bands = list(bands)
    Vb, Eb = V[:, :, bands], ev[:, bands]
    tau = state_tau(m)
    terms = trial_terms(m, trial)
    nw = len(terms)
    g = np.zeros((nk, n, nw), dtype=complex)
    for w, fn in enumerate(terms):
        for amp, s, Rv in fn:
            g[:, s, w] += amp * np.exp(-2j * np.pi * (k @ (Rv + tau[s])))
    A = np.einsum("kjb,kjw->kbw", Vb.conj(), g)
    W, sv, Zh = np.linalg.svd(A, full_matrices=False)
    U = W @ Zh
    ut = Vb @ U
    steps, wb, bc = bvectors(np.asarray(m._lat, dtype=float)[m._per], mesh)
    nbv = len(wb)
    wall, ball = np.concatenate([wb, wb]), np.concatenate([bc, -bc])
    Mp = np.zeros((nk, nbv, nw, nw), dtype=complex)
    nxt, prv = [], []
    for ib in range(nbv):
        k2, G = neighbours(mesh, steps[ib])
        ph = np.exp(-2j * np.pi * (G @ tau.T))
        Mp[:, ib] = np.einsum("kjm,kjn->kmn", ut.conj(), ut[k2] * ph[:, :, None])
        nxt.append(k2)
        prv.append(neighbours(mesh, -steps[ib])[0])

    def both(Mp):
        Mm = np.stack([Mp[prv[ib], ib].conj().transpose(0, 2, 1) for ib in range(nbv)], axis=1)
        return np.concatenate([Mp, Mm], axis=1)

    Uacc = np.tile(np.eye(nw, dtype=complex), (nk, 1, 1))
    sp = spread(both(Mp), wall, ball)
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
        E = herm_exp(Gk / (4.0 * np.sum(wall)))
        Uacc = Uacc @ E
        for ib in range(nbv):
            Mp[:, ib] = E.conj().transpose(0, 2, 1) @ Mp[:, ib] @ E[nxt[ib]]
        sp = spread(both(Mp), wall, ball)
        hist_all.append(sp[1] + sp[2] + sp[3])
    rows = [0] + [it for it in range(1, max_iter + 1) if it % check_every == 0 or it == max_iter]
    Ut = U @ Uacc
    HW = np.einsum("kbm,kb,kbn->kmn", Ut.conj(), Eb, Ut)
    Rl = torus(mesh) if R is None else np.asarray(R, dtype=int).reshape(-1, dk)
    hop = np.einsum("rk,kmn->rmn", np.exp(-2j * np.pi * (Rl @ k.T)), HW) / nk
    out = dict(centers=sp[0], omega_i=sp[1], omega_od=sp[2], omega_d=sp[3], omega=sp[1] + sp[2] + sp[3], spreads=sp[4],
               sv_min=float(sv.min()), history=np.array(hist_all)[rows], history_all=np.array(hist_all), hoppings=hop, R_list=Rl,
               gauge=Ut, b_vectors=bc, b_weights=wb, steps=steps)
    if functions:
        uf = ut @ Uacc
        phase = np.exp(2j * np.pi * np.einsum("rjc,kc->rjk", Rl[:, None, :] + tau[None, :, :], k))
        out["functions"] = np.einsum("rjk,kjn->rjn", phase, uf) / nk
    return out
