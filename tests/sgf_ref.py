"""NumPy restatement of the surface Green's functions (pythtb_amd.tb_model.surface_green / surface_spectral / surface_dos_mesh):
the principal-layer blocks from cut_piece(2 L) through the oracle's ham_batch, the decimation loop of Lopez Sancho, Lopez Sancho and
Rubio (1985) as DESIGN.md section 18 states it, and numpy.linalg.inv.  Also the independent check: diagonal blocks of the resolvent
of a finite slab.  The checker of tests/test_surface_green.py; pure host code."""
import numpy as np

from helpers import quiet
from oracle import tb_oracle as orc


def principal_layer(m, fin_dir):
    return max([1] + [abs(int(h[3][fin_dir])) for h in m._hoppings])


def kpar(m, k_list):
    """k list of the surface zone as (nk, max(dim_k - 1, 1)); a model with dim_k == 1 has one point."""
    dk = m._dim_k - 1
    if dk == 0:
        return np.zeros((1, 1))
    return np.asarray(k_list, dtype=float).reshape(-1, dk)


def slab_ham(m, cells, fin_dir, k_list):
    """H(k) of cut_piece(cells, fin_dir) on the k list: (nk, cells nsta, cells nsta)."""
    return orc.ham_batch(quiet(m.cut_piece, cells, fin_dir), kpar(m, k_list))


def layer_blocks(m, fin_dir, k_list):
    """(H00, H01), each (nk, N, N): the top-left and top-right blocks of the slab of two principal layers."""
    L = principal_layer(m, fin_dir)
    N = L * m._nsta
    h = slab_ham(m, 2 * L, fin_dir, k_list)
    return h[:, :N, :N], h[:, :N, N:]


def decimate(h00, h01, z, tol=1e-12, max_iter=50):
    """One (k, z) point: (es, et, e, steps, converged) after the stopping rule -- the first step count i, 0 included, with
    max(|alpha|_max, |beta|_max) <= tol max(|H00|_max, |H01|_max); tol = 0: exactly max_iter steps."""
    n = h00.shape[0]
    one = np.identity(n)
    es, et, e = h00.copy(), h00.copy(), h00.copy()
    al, be = h01.copy(), h01.conj().T.copy()
    scale = max(np.abs(h00).max(), np.abs(h01).max())
    steps = 0
    while True:
        if tol > 0.0 and max(np.abs(al).max(), np.abs(be).max()) <= tol * scale:
            return es, et, e, steps, True
        if steps == max_iter:
            return es, et, e, steps, tol == 0.0
        g = np.linalg.inv(z * one - e)
        agb, bga = al @ g @ be, be @ g @ al
        es = es + agb
        et = et + bga
        e = e + agb + bga
        al, be = al @ g @ al, be @ g @ be
        steps += 1


def green(m, k_list, omega, eta, fin_dir, tol=1e-12, max_iter=50):
    """G (3, nk, nw, N, N) for side 0, side 1 and the bulk, and the steps taken (nk, nw)."""
    h00, h01 = layer_blocks(m, fin_dir, k_list)
    nk, n = h00.shape[0], h00.shape[1]
    omega = np.asarray(omega, dtype=float)
    out = np.zeros((3, nk, omega.size, n, n), dtype=complex)
    steps = np.zeros((nk, omega.size), dtype=np.int32)
    one = np.identity(n)
    for ik in range(nk):
        for iw, w in enumerate(omega):
            z = w + 1j * eta
            es, et, e, steps[ik, iw], ok = decimate(h00[ik], h01[ik], z, tol, max_iter)
            if not ok:
                raise Exception("sgf_ref: point (%d, %d) did not converge" % (ik, iw))
            for s, x in enumerate((es, et, e)):
                out[s, ik, iw] = np.linalg.inv(z * one - x)
    return out, steps


def spectral_of(g, nsta, per_state=False):
    """A = -(1 / pi) Im G_ss over the exposed unit cell of G (3, ..., N, N): cell 0, the last cell for side 1."""
    n = g.shape[-1]
    d = -np.imag(np.diagonal(g, axis1=-2, axis2=-1)) / np.pi          # (3, ..., N)
    a = np.stack([d[0][..., :nsta], d[1][..., n - nsta:], d[2][..., :nsta]])
    return a if per_state else a.sum(axis=-1)


def spectral(m, k_list, omega, eta, fin_dir, per_state=False, tol=1e-12, max_iter=50):
    g, steps = green(m, k_list, omega, eta, fin_dir, tol, max_iter)
    return spectral_of(g, m._nsta, per_state), steps


def surface_mesh(m, mesh_size, fin_dir):
    """k_uniform_mesh of the cut model."""
    return orc.k_uniform_mesh(quiet(m.cut_piece, 1, fin_dir), mesh_size)


def dos_mesh(m, mesh_size, omega, eta, fin_dir, per_state=False, tol=1e-12, max_iter=50):
    a, _ = spectral(m, surface_mesh(m, mesh_size, fin_dir), omega, eta, fin_dir, per_state, tol, max_iter)
    return a.mean(axis=1)


def slab_blocks(m, k_list, omega, eta, fin_dir, steps):
    """The direct route (no decimation): with L the principal layer and N = L nsta, the first and the last N x N diagonal block of
    (z - H_slab)^-1 for the slab of L 2^steps cells, and the middle block of the slab of L (2^(steps + 1) - 1) cells:
    (3, nk, nw, N, N) = what `steps` decimation steps give for side 0, side 1 and the bulk."""
    L = principal_layer(m, fin_dir)
    n = L * m._nsta
    omega = np.asarray(omega, dtype=float)
    h_edge = slab_ham(m, L * 2 ** steps, fin_dir, k_list)
    nb = 2 ** (steps + 1) - 1
    h_bulk = slab_ham(m, L * nb, fin_dir, k_list)
    nk = h_edge.shape[0]
    out = np.zeros((3, nk, omega.size, n, n), dtype=complex)
    mid = (nb // 2) * n
    for ik in range(nk):
        for iw, w in enumerate(omega):
            z = w + 1j * eta
            ge = np.linalg.inv(z * np.identity(h_edge.shape[1]) - h_edge[ik])
            gb = np.linalg.inv(z * np.identity(h_bulk.shape[1]) - h_bulk[ik])
            out[0, ik, iw] = ge[:n, :n]
            out[1, ik, iw] = ge[-n:, -n:]
            out[2, ik, iw] = gb[mid:mid + n, mid:mid + n]
    return out


def peaks(a, floor):
    """Indices of the strict local maxima of the 1-D array a that exceed `floor`."""
    a = np.asarray(a)
    i = np.arange(1, a.size - 1)
    return i[(a[i] > a[i - 1]) & (a[i] >= a[i + 1]) & (a[i] > floor)]
