"""tb_model: host-side mirror of PythTB's model class for the k-space hot path.

Same constructor, setters, attribute names and call signatures as the reference
(`pythtb.py:29-560`, `:862-1103`, `:1792-2026`), so scripts written for PythTB
run unchanged; `_gen_ham`, `_sol_ham`, `solve_all` and `solve_one` execute on the
MI355X through libtbk (no CPU path).  The model->model transforms live in
transforms.py, the text report and the sketch plot in report.py / plotting.py.
"""
import copy
import ctypes as C

import numpy as np

from . import _lib

__all__ = ["tb_model", "exciton_reconstruct", "kpm_reconstruct", "kpm_conductivity_reconstruct", "kpm_coefficients", "kpm_fermi_coefficients"]


def _is_int(a):
    return np.issubdtype(type(a), np.integer)        # pythtb.py:3950


def _sweep_args(omega, eta, fermi_level, kT):
    """The checked frequencies of a frequency sweep (`optical_conductivity_mesh`, the photocurrent meshes) as a contiguous
    float array, after the checks of eta, kT and fermi_level that these calls share."""
    w = np.array(omega, dtype=float)
    if w.ndim != 1 or w.size < 1 or w.size > 65536:
        raise Exception("\n\nomega must be a 1-D array of 1..65536 frequencies.")
    if not np.all(np.isfinite(w)):
        raise Exception("\n\nomega must be finite.")
    if not np.isfinite(eta) or not eta > 0.0:
        raise Exception("\n\neta must be finite and > 0.")
    if not np.isfinite(kT) or not kT >= 0.0:
        raise Exception("\n\nkT must be finite and >= 0.")
    if not np.isfinite(fermi_level):
        raise Exception("\n\nfermi_level must be finite.")
    return np.ascontiguousarray(w)


def kpm_reconstruct(mu, energies, bounds, kernel="jackson", lam=4.0):
    """Extension: the kernel-polynomial reconstruction of a density from its Chebyshev moments `mu` `(..., M)` (those of
    `tb_model.kpm_moments` for the same `bounds` = (emin, emax)) at `energies` inside the open interval (emin, emax):

        rho(E) = [g_0 mu_0 + 2 sum_{m >= 1} g_m mu_m T_m(x)] / (pi a sqrt(1 - x^2)),   x = (E - b) / a,

    a = (emax - emin) / 2, b = (emax + emin) / 2; float `(..., nE)`.  kernel: "jackson" (non-negative, resolution ~ pi a / M),
    "lorentz" (g_m = sinh(lam (1 - m / M)) / sinh(lam)) or None (g = 1: the truncated series, with Gibbs oscillations).
    Host NumPy, O(M nE) work; the moments are the product of the device."""
    mu = np.asarray(mu, dtype=float)
    e = np.asarray(energies, dtype=float)
    if mu.ndim < 1 or mu.shape[-1] < 1:
        raise Exception("\n\nkpm_reconstruct: mu must have shape (..., M) with M >= 1")
    if e.ndim != 1:
        raise Exception("\n\nkpm_reconstruct: energies must be a one-dimensional list")
    emin, emax = float(bounds[0]), float(bounds[1])
    if not emax > emin:
        raise Exception("\n\nkpm_reconstruct: bounds must be (emin, emax) with emin < emax")
    if e.size and not (e.min() > emin and e.max() < emax):
        raise Exception("\n\nkpm_reconstruct: energies must lie inside the open interval (%.12g, %.12g)" % (emin, emax))
    M = mu.shape[-1]
    m = np.arange(M, dtype=float)
    if kernel == "jackson":
        q = np.pi / (M + 1.0)
        g = ((M - m + 1.0) * np.cos(q * m) + np.sin(q * m) / np.tan(q)) / (M + 1.0)
    elif kernel == "lorentz":
        g = np.sinh(lam * (1.0 - m / M)) / np.sinh(lam)
    elif kernel is None:
        g = np.ones(M)
    else:
        raise Exception("\n\nkpm_reconstruct: kernel must be \"jackson\", \"lorentz\" or None")
    a, b = 0.5 * (emax - emin), 0.5 * (emax + emin)
    x = (e - b) / a
    w = g * np.where(m == 0, 1.0, 2.0)
    T = np.cos(m[:, None] * np.arccos(x)[None, :])
    return (mu * w) @ T / (np.pi * a * np.sqrt(1.0 - x * x))


def _kpm_kernel(M, kernel, lam, who):
    m = np.arange(M, dtype=float)
    if kernel == "jackson":
        q = np.pi / (M + 1.0)
        return ((M - m + 1.0) * np.cos(q * m) + np.sin(q * m) / np.tan(q)) / (M + 1.0)
    if kernel == "lorentz":
        return np.sinh(lam * (1.0 - m / M)) / np.sinh(lam)
    if kernel is None:
        return np.ones(M)
    raise Exception("\n\n%s: kernel must be \"jackson\", \"lorentz\" or None" % who)


def kpm_conductivity_reconstruct(mu, energies, bounds, kernel="jackson", lam=4.0, kT=0.0, n_quad=None):
    """Extension: the Kubo-Bastin conductivity per sample from double Chebyshev moments `mu` `(..., M, M)` (those of
    `tb_model.kpm_double_moments` for the same `bounds` = (emin, emax)) at the Fermi levels `energies` inside the open
    interval (emin, emax) (Garcia, Covaci, Rappoport, Phys. Rev. Lett. 114, 116602):

        G_ab(E_F) = (2 / (pi^2 a^2)) int_{-1}^{1} dx f(x) (1 - x^2)^{-2} sum_{m,n} Gamma_mn(x) g_m g_n mu_mn / ((1 + d_m0)(1 + d_n0))
        Gamma_mn(x) = (x - i n sqrt(1 - x^2)) e^{i n theta} T_m(x) + (x + i m sqrt(1 - x^2)) e^{-i m theta} T_n(x),   x = cos theta,

    a = (emax - emin) / 2, b = (emax + emin) / 2, g the kernel coefficients of `kpm_reconstruct`, f the Fermi function of
    E = a x + b at temperature kT (kT = 0: the step at E_F); complex `(..., nE)`.  The integral is a Chebyshev-Gauss
    quadrature on the `n_quad` (default 8 M) nodes x_j = cos(pi (j + 1/2) / n_quad) with weights pi sqrt(1 - x_j^2) / n_quad;
    at kT = 0 the nodes with x_j <= x_F.  Host NumPy, O(M^2 n_quad) work per moment set."""
    mu = np.asarray(mu, dtype=complex)
    e = np.asarray(energies, dtype=float)
    if mu.ndim < 2 or mu.shape[-1] < 1 or mu.shape[-1] != mu.shape[-2]:
        raise Exception("\n\nkpm_conductivity_reconstruct: mu must have shape (..., M, M) with M >= 1")
    if e.ndim != 1:
        raise Exception("\n\nkpm_conductivity_reconstruct: energies must be a one-dimensional list")
    emin, emax = float(bounds[0]), float(bounds[1])
    if not emax > emin:
        raise Exception("\n\nkpm_conductivity_reconstruct: bounds must be (emin, emax) with emin < emax")
    if e.size and not (e.min() > emin and e.max() < emax):
        raise Exception("\n\nkpm_conductivity_reconstruct: energies must lie inside the open interval (%.12g, %.12g)" % (emin, emax))
    if not np.isfinite(kT) or kT < 0.0:
        raise Exception("\n\nkpm_conductivity_reconstruct: kT must be finite and >= 0")
    M = mu.shape[-1]
    K = 8 * M if n_quad is None else n_quad
    if not _is_int(K) or K < 1:
        raise Exception("\n\nkpm_conductivity_reconstruct: n_quad must be a positive integer")
    g = _kpm_kernel(M, kernel, lam, "kpm_conductivity_reconstruct")
    g[0] *= 0.5                                             # the factor 1 / (1 + delta_m0)
    a, b = 0.5 * (emax - emin), 0.5 * (emax + emin)
    th = np.pi * (np.arange(K) + 0.5) / K
    x, sq = np.cos(th), np.sin(th)
    m = np.arange(M, dtype=float)
    T = np.cos(m[:, None] * th[None, :])                                               # T_m(x_j)
    A = (x[None, :] - 1j * m[:, None] * sq[None, :]) * np.exp(1j * m[:, None] * th[None, :])   # (x - i n s) e^{i n theta}
    c = mu * (g[:, None] * g[None, :])
    # sum_mn Gamma_mn c_mn = sum_m T_m (c A)_m + sum_n T_n (c^T conj A)_n at every node
    S = np.sum(T * (c @ A), axis=-2) + np.sum(T * (np.swapaxes(c, -1, -2) @ A.conj()), axis=-2)
    S = S * ((np.pi / K) / sq ** 3)                         # the weight pi s / K over (1 - x^2)^2
    if kT > 0.0:
        f = 0.5 * (1.0 - np.tanh(0.5 * ((a * x + b)[:, None] - e[None, :]) / kT))
    else:
        f = (x[:, None] <= ((e - b) / a)[None, :]).astype(float)
    return (2.0 / (np.pi * a) ** 2) * (S @ f)


def kpm_coefficients(f, n_terms, bounds, kernel=None, lam=4.0, n_quad=None):
    """Extension: the Chebyshev coefficients c_m, m < n_terms, of a function f of the energy on `bounds` = (emin, emax), for
    `tb_model.kpm_apply`:

        f(H) ~ sum_m c_m T_m(H~),   c_m = (2 - delta_m0) / K sum_j f(a x_j + b) cos(m theta_j),   x_j = cos theta_j,

    H~ = (H - b) / a, a = (emax - emin) / 2, b = (emax + emin) / 2, by the Chebyshev-Gauss quadrature on the `n_quad` (default
    4 n_terms) nodes theta_j = pi (j + 1/2) / K.  f is called once with the array of node energies; a complex f gives complex
    coefficients.  kernel: None (the truncated series), "jackson" or "lorentz" -- the damping factors g_m of `kpm_reconstruct`
    multiply c_m.  Host NumPy, O(n_terms n_quad) work."""
    if not _is_int(n_terms) or n_terms < 1:
        raise Exception("\n\nkpm_coefficients: n_terms must be a positive integer")
    K = 4 * int(n_terms) if n_quad is None else n_quad
    if not _is_int(K) or K < 1:
        raise Exception("\n\nkpm_coefficients: n_quad must be a positive integer")
    emin, emax = float(bounds[0]), float(bounds[1])
    if not emax > emin:
        raise Exception("\n\nkpm_coefficients: bounds must be (emin, emax) with emin < emax")
    g = _kpm_kernel(int(n_terms), kernel, lam, "kpm_coefficients")
    a, b = 0.5 * (emax - emin), 0.5 * (emax + emin)
    th = np.pi * (np.arange(K) + 0.5) / K
    fx = np.asarray(f(a * np.cos(th) + b))
    if fx.shape != th.shape:
        raise Exception("\n\nkpm_coefficients: f must map an array of energies to an array of the same shape")
    m = np.arange(int(n_terms), dtype=float)
    c = np.cos(m[:, None] * th[None, :]) @ fx * (np.where(m == 0, 1.0, 2.0) / K)
    return c * g


def kpm_fermi_coefficients(fermi_level, n_moments, bounds, kernel="jackson", lam=4.0, kT=0.0):
    """Extension: the Chebyshev coefficients of the occupation, float `(n_moments,)`: with them `tb_model.kpm_apply` applies the
    Fermi projector P = theta(E_F - H) (kT = 0) or the Fermi function of H.  At kT = 0 analytic,

        c_0 = 1 - theta_F / pi,   c_m = -2 sin(m theta_F) / (m pi),   theta_F = arccos((E_F - b) / a),

    at kT > 0 `kpm_coefficients` of the Fermi function; both times the kernel factors g_m ("jackson" by default: the step is
    smoothed over ~ pi a / n_moments and has no Gibbs oscillations).  `fermi_level` must lie inside the open interval of
    `bounds` = (emin, emax); a, b as in `kpm_coefficients`."""
    if not _is_int(n_moments) or n_moments < 1:
        raise Exception("\n\nkpm_fermi_coefficients: n_moments must be a positive integer")
    emin, emax = float(bounds[0]), float(bounds[1])
    if not emax > emin:
        raise Exception("\n\nkpm_fermi_coefficients: bounds must be (emin, emax) with emin < emax")
    if not np.isfinite(fermi_level) or not emin < fermi_level < emax:
        raise Exception("\n\nkpm_fermi_coefficients: fermi_level must lie inside the open interval (%.12g, %.12g)" % (emin, emax))
    if not np.isfinite(kT) or kT < 0.0:
        raise Exception("\n\nkpm_fermi_coefficients: kT must be finite and >= 0")
    if kT > 0.0:
        return kpm_coefficients(lambda e: 0.5 * (1.0 - np.tanh(0.5 * (e - fermi_level) / kT)), n_moments, bounds, kernel, lam)
    g = _kpm_kernel(int(n_moments), kernel, lam, "kpm_fermi_coefficients")
    a, b = 0.5 * (emax - emin), 0.5 * (emax + emin)
    thf = np.arccos((fermi_level - b) / a)
    m = np.arange(1, int(n_moments), dtype=float)
    c = np.empty(int(n_moments))
    c[0] = 1.0 - thf / np.pi
    c[1:] = -2.0 * np.sin(m * thf) / (m * np.pi)
    return c * g


def kpm_window_coefficients(window, n_terms, bounds, kernel="jackson", lam=4.0):
    """Extension: the Chebyshev coefficients of the indicator function of `window` = (e_lo, e_hi), float `(n_terms,)`: with them
    `tb_model.kpm_apply` applies the spectral projector on the window, smoothed by the kernel.  Analytic,

        c_0 = (theta_lo - theta_hi) / pi,   c_m = 2 (sin(m theta_lo) - sin(m theta_hi)) / (m pi),   theta = arccos((e - b) / a),

    times the kernel factors g_m ("jackson" by default: each edge is smoothed over ~ pi a / n_terms, the value at an edge is
    1/2, and there are no Gibbs oscillations).  The window must lie inside the open interval of `bounds` = (emin, emax) with
    e_lo <= e_hi; a, b as in `kpm_coefficients`.  `tb_model.kpm_eigs` filters with these coefficients of its widened window."""
    if not _is_int(n_terms) or n_terms < 1:
        raise Exception("\n\nkpm_window_coefficients: n_terms must be a positive integer")
    emin, emax = float(bounds[0]), float(bounds[1])
    if not emax > emin:
        raise Exception("\n\nkpm_window_coefficients: bounds must be (emin, emax) with emin < emax")
    w = np.array(window, dtype=float)
    if w.shape != (2,) or not np.all(np.isfinite(w)) or w[0] > w[1]:
        raise Exception("\n\nkpm_window_coefficients: window must be (e_lo, e_hi), finite, with e_lo <= e_hi")
    if not (emin < w[0] and w[1] < emax):
        raise Exception("\n\nkpm_window_coefficients: window must lie inside the open interval (%.12g, %.12g)" % (emin, emax))
    g = _kpm_kernel(int(n_terms), kernel, lam, "kpm_window_coefficients")
    a, b = 0.5 * (emax - emin), 0.5 * (emax + emin)
    tlo, thi = np.arccos((w[0] - b) / a), np.arccos((w[1] - b) / a)
    m = np.arange(1, int(n_terms), dtype=float)
    c = np.empty(int(n_terms))
    c[0] = (tlo - thi) / np.pi
    c[1:] = 2.0 * (np.sin(m * tlo) - np.sin(m * thi)) / (m * np.pi)
    return c * g


def _kpm_evolution_coefficients(z):
    """(2 - delta_m0) (-i)^m J_m(z), cut after the last modulus above 1e-17: e^{-i z cos(theta)} = sum_m of these times cos(m theta),
    so its discrete Fourier transform over theta_j = 2 pi j / N gives (-i)^m J_m(z) up to the aliases J_{N -+ m}(z); N is a power of
    two of at least 2 |z| + 128, and large enough that the aliases of the kept terms lie where J has decayed below the cut."""
    z = float(z)
    N = 1 << int(np.ceil(np.log2(2.0 * abs(z) + 40.0 * abs(z) ** (1.0 / 3.0) + 128.0)))
    c = np.fft.fft(np.exp(-1j * z * np.cos(2.0 * np.pi * np.arange(N) / N)))[:N // 2] / N
    c[1:] *= 2.0
    keep = np.nonzero(np.abs(c) > 1e-17)[0]
    return c[:keep[-1] + 1]


class mean_field_result(object):
    """What `tb_model.mean_field_mesh` returns: model, fermi_level, occupations, spin_density, density, R_list, energy, entropy,
    free_energy, band_energy, n_electrons, residuals, history, iterations, converged, resident, field (the parameter vector the
    last iteration produced; `_x` is the one it solved in, which `model` carries and a restart begins from)."""
    pass


class bdg_result(object):
    """What `tb_model.bdg_mesh` returns: model (the Nambu model), normal_model, fermi_level, n_electrons, occupations, pairing,
    anomalous, gap, energy, entropy, free_energy, grand_potential, residuals, history, iterations, converged, field (the parameter
    vector the last iteration produced; `_x` is the one it solved in, which `model` carries and a restart begins from), and on
    request nambu_density and R_list."""
    pass


class exciton_result(object):
    """What `tb_model.exciton_states_mesh` returns: energies `(N_t,)` ascending, dipoles d^a_lambda `(N_t, dim_k)`, gap (the smallest
    transition energy), binding = gap - energies[0], dipole_norm S_ab `(dim_k, dim_k)`, n_occ, valence and conduction (the selected
    bands), mesh, and on request vectors `(N_t, *mesh, nv, nc)`."""

    def polarizability(self, omega, eta, dirs=None):
        """chi_ab(w) = (1/N) sum_lambda conj(d^a_lambda) d^b_lambda / (Omega_lambda - w - i eta), summed on the host:
        `(nw, dim_k, dim_k)`, or `(nw,)` for dirs=(a, b).  omega and eta by the rules of `optical_conductivity_mesh`."""
        w = _sweep_args(omega, eta, 0.0, 0.0)
        dk = self.dipoles.shape[1]
        res = 1.0 / (self.energies[None, :] - w[:, None] - 1j * float(eta))
        if dirs is None:
            return np.einsum("la,lb,wl->wab", np.conj(self.dipoles), self.dipoles, res) / self._nk
        a, b = _exciton_dirs(dirs, dk)
        return (res @ (np.conj(self.dipoles[:, a]) * self.dipoles[:, b])) / self._nk


class exciton_coefficients(object):
    """The Lanczos coefficients of `tb_model.exciton_spectrum_mesh`: alpha and beta `(n_runs, n_steps)`, norm2 `(n_runs,)` (the
    squared norms of the start vectors), n_used `(n_runs,)`, runs (a list of (a, b, kind): kind 0 starts from D^a, 1 from
    D^a + D^b, 2 from D^a + i D^b), dim_k, dirs, n_k.  `exciton_reconstruct` turns them into chi at any frequencies; whoever wants
    Ritz values diagonalises the tridiagonal matrix of a run."""
    pass


class exciton_spectrum(object):
    """What `tb_model.exciton_spectrum_mesh` returns: chi `(nw, dim_k, dim_k)` or `(nw,)`, dipole_norm, gap, n_used, and on request
    coefficients (an `exciton_coefficients`)."""
    pass


def _exciton_dirs(dirs, dk):
    dirs = list(dirs)
    if len(dirs) != 2 or not all(_is_int(d) for d in dirs):
        raise Exception("\n\ndirs must be two integer axes.")
    if min(dirs) < 0 or max(dirs) >= dk:
        raise Exception("\n\nDirection for the polarizability out of bounds.")
    return int(dirs[0]), int(dirs[1])


def exciton_reconstruct(coefficients, omega, eta):
    """chi_ab(w) of `tb_model.exciton_spectrum_mesh` at other frequencies or another eta from its Lanczos coefficients: the
    continued fractions of the runs and the polarisation algebra, on the host, no device call.  The same w gives the same bits
    alone and inside a list."""
    c = coefficients
    if not isinstance(c, exciton_coefficients):
        raise Exception("\n\nexciton_reconstruct needs the coefficients of exciton_spectrum_mesh.")
    w = _sweep_args(omega, eta, 0.0, 0.0)
    dk = c.dim_k
    da, db = (-1, -1) if c.dirs is None else c.dirs
    out = np.zeros((w.size, dk, dk) if da < 0 else (w.size,), dtype=complex)
    alpha, beta = np.ascontiguousarray(c.alpha, dtype=float), np.ascontiguousarray(c.beta, dtype=float)
    _lib.check(_lib.lib.tbk_exciton_reconstruct(dk, da, db, alpha.shape[1], _lib.dptr(alpha), _lib.dptr(beta),
                                                _lib.dptr(np.ascontiguousarray(c.norm2, dtype=float)),
                                                _lib.iptr(np.ascontiguousarray(c.n_used, dtype=np.int32)), int(c.n_k), int(w.size),
                                                _lib.dptr(w), float(eta), _lib.dptr(out.view(float))))
    return out


class wannier_result(object):
    """What `tb_model.wannier_mesh` returns: model, hoppings, R_list, centers, spreads, omega_i, omega_od, omega_d, omega, sv_min,
    history, iterations, converged, b_vectors, b_weights, and on request functions and gauge.  `wannier_disentangle_mesh` adds
    dis_history, dis_iterations, dis_converged, n_window, n_frozen, dis_gap_min and sv_min_projection."""
    pass


class tb_model(object):
    """Tight-binding model in reduced coordinates (reference: pythtb.py:29-184)."""

    def __init__(self, dim_k, dim_r, lat=None, orb=None, per=None, nspin=1):
        if not _is_int(dim_k):
            raise Exception("\n\nArgument dim_k not an integer")
        if dim_k < 0 or dim_k > 4:
            raise Exception("\n\nArgument dim_k out of range. Must be between 0 and 4.")
        if not _is_int(dim_r):
            raise Exception("\n\nArgument dim_r not an integer")
        if dim_r < dim_k or dim_r > 4:
            raise Exception("\n\nArgument dim_r out of range. Must be dim_r>=dim_k and dim_r<=4.")
        self._dim_k = dim_k
        self._dim_r = dim_r

        if lat is None or (isinstance(lat, str) and lat == "unit"):
            self._lat = np.identity(dim_r, float)
            print(" Lattice vectors not specified! I will use identity matrix.")
        else:
            self._lat = np.array(lat, dtype=float)
            if self._lat.shape != (dim_r, dim_r):
                raise Exception("\n\nWrong lat array dimensions")
        if dim_r > 0:
            vol = np.linalg.det(self._lat)
            if np.abs(vol) < 1.0E-6:
                raise Exception("\n\nLattice vectors length/area/volume too close to zero, or zero.")
            if vol < 0.0:
                raise Exception("\n\nLattice vectors need to form right handed system.")

        if orb is None or (isinstance(orb, str) and orb == "bravais"):
            self._norb = 1
            self._orb = np.zeros((1, dim_r))
            print(" Orbital positions not specified. I will assume a single orbital at the origin.")
        elif _is_int(orb):
            self._norb = orb
            self._orb = np.zeros((orb, dim_r))
            print(" Orbital positions not specified. I will assume ", orb, " orbitals at the origin")
        else:
            self._orb = np.array(orb, dtype=float)
            if self._orb.ndim != 2:
                raise Exception("\n\nWrong orb array rank")
            self._norb = self._orb.shape[0]
            if self._orb.shape[1] != dim_r:
                raise Exception("\n\nWrong orb array dimensions")

        if per is None:
            self._per = list(range(self._dim_k))
        else:
            if len(per) != self._dim_k:
                raise Exception("\n\nWrong choice of periodic/infinite direction!")
            self._per = per

        if nspin not in [1, 2]:
            raise Exception("\n\nWrong value of nspin, must be 1 or 2!")
        self._nspin = nspin
        self._assume_position_operator_diagonal = True
        self._nsta = self._norb * self._nspin

        if self._nspin == 1:
            self._site_energies = np.zeros(self._norb, dtype=float)
        else:
            self._site_energies = np.zeros((self._norb, 2, 2), dtype=complex)
        self._site_energies_specified = np.zeros(self._norb, dtype=bool)
        self._hoppings = []
        self._tbk_epoch = 0        # bumped whenever the tables change
        self._tbk_cache = None     # (epoch, device handle)
        self._tbk_surface = {}     # fin_dir -> (fingerprint, cut_piece(2 L, fin_dir)) of the surface Green's functions
        self._tbk_sparse = None    # (edit mark, context, handle of the sparse operator) of the kernel polynomial method

    # ------------------------------------------------------------------ tables
    def _val_to_block(self, val):
        """scalar / (I,sx,sy,sz) 4-vector / 2x2 -> 2x2 block for nspin=2 (pythtb.py:517-560)."""
        if self._nspin == 1:
            return val
        v = np.array(val)
        if v.shape == (2, 2):
            return v
        blk = np.zeros((2, 2), dtype=complex)
        if v.shape == ():
            blk[0, 0] = blk[1, 1] = v
        elif v.shape == (4,):
            blk[0, 0] = v[0] + v[3]
            blk[1, 1] = v[0] - v[3]
            blk[0, 1] = v[1] - 1.0j * v[2]
            blk[1, 0] = v[1] + 1.0j * v[2]
        else:
            raise Exception(
                "\n\nWrong format of the on-site or hopping term. Must be single number, or\n"
                "in the case of a spinfull model can be array of four numbers or 2x2\nmatrix.")
        return blk

    def set_onsite(self, onsite_en, ind_i=None, mode="set"):
        """On-site energies; modes set/reset/add (pythtb.py:186-306)."""
        if ind_i is None:
            if len(onsite_en) != self._norb:
                raise Exception("\n\nWrong number of site energies")
            values = list(onsite_en)
            targets = list(range(self._norb))
        else:
            if ind_i < 0 or ind_i >= self._norb:
                raise Exception("\n\nIndex ind_i out of scope.")
            values = [onsite_en]
            targets = [ind_i]
        for ons in values:
            a = np.array(ons)
            if a.shape == ():
                if np.abs(a - a.conjugate()) > 1.0E-8:
                    raise Exception("\n\nOnsite energy should not have imaginary part!")
            elif a.shape == (4,):
                if np.max(np.abs(a - a.conjugate())) > 1.0E-8:
                    raise Exception("\n\nOnsite energy or Zeeman field should not have imaginary part!")
            elif a.shape == (2, 2):
                if np.max(np.abs(a - a.T.conjugate())) > 1.0E-8:
                    raise Exception("\n\nOnsite matrix should be Hermitian!")
        how = mode.lower()
        if how == "set":
            if ind_i is not None:
                if self._site_energies_specified[ind_i]:
                    raise Exception("\n\nOnsite energy for this site was already specified! "
                                    "Use mode=\"reset\" or mode=\"add\".")
            elif np.any(self._site_energies_specified):
                raise Exception("\n\nSome or all onsite energies were already specified! "
                                "Use mode=\"reset\" or mode=\"add\".")
        elif how not in ("reset", "add"):
            raise Exception("\n\nWrong value of mode parameter")
        for t, ons in zip(targets, values):
            if how == "add":
                self._site_energies[t] += self._val_to_block(ons)
            else:
                self._site_energies[t] = self._val_to_block(ons)
            self._site_energies_specified[t] = True
        self._tbk_epoch += 1

    def set_hop(self, hop_amp, ind_i, ind_j, ind_R=None, mode="set", allow_conjugate_pair=False):
        """Hopping <phi_0i|H|phi_Rj>; stored as [amp, i, j, R] (pythtb.py:308-515)."""
        if self._dim_k != 0 and ind_R is None:
            raise Exception("\n\nNeed to specify ind_R!")
        if self._dim_k == 1 and _is_int(ind_R):
            full = np.zeros(self._dim_r, dtype=int)
            full[self._per] = ind_R
            ind_R = full
        if self._dim_k != 0 and len(ind_R) != self._dim_r:
            raise Exception("\n\nLength of input ind_R vector must equal dim_r! Even if dim_k<dim_r.")
        if ind_i < 0 or ind_i >= self._norb:
            raise Exception("\n\nIndex ind_i out of scope.")
        if ind_j < 0 or ind_j >= self._norb:
            raise Exception("\n\nIndex ind_j out of scope.")
        if ind_i == ind_j:
            if self._dim_k == 0 or all(int(ind_R[k]) == 0 for k in self._per):
                raise Exception("\n\nDo not use set_hop for onsite terms. Use set_onsite instead!")
        r_per = None if self._dim_k == 0 else np.array(ind_R)[self._per]
        if not allow_conjugate_pair:
            for h in self._hoppings:
                if ind_i == h[2] and ind_j == h[1]:
                    if self._dim_k == 0:
                        raise Exception(
                            "\n\nFollowing matrix element was already implicitely specified:\n"
                            "   i=" + str(ind_i) + " j=" + str(ind_j) + "\n"
                            "Remember, specifying <i|H|j> automatically specifies <j|H|i>.  For\n"
                            "consistency, specify all hoppings for a given bond in the same\n"
                            "direction.  (Or, alternatively, see the documentation on the\n"
                            "'allow_conjugate_pair' flag.)\n")
                    if np.all(r_per == -np.array(h[3])[self._per]):
                        raise Exception(
                            "\n\nFollowing matrix element was already implicitely specified:\n"
                            "   i=" + str(ind_i) + " j=" + str(ind_j) + " R=" + str(ind_R) + "\n"
                            "Remember,specifying <i|H|j+R> automatically specifies <j|H|i-R>.  For\n"
                            "consistency, specify all hoppings for a given bond in the same\n"
                            "direction.  (Or, alternatively, see the documentation on the\n"
                            "'allow_conjugate_pair' flag.)\n")
        block = self._val_to_block(hop_amp)
        entry = [block, int(ind_i), int(ind_j)]
        if self._dim_k != 0:
            entry.append(np.array(ind_R))
        match = None                                   # last entry with the same (i,j,R)
        for pos, h in enumerate(self._hoppings):
            if ind_i == h[1] and ind_j == h[2]:
                if self._dim_k == 0 or np.all(r_per == np.array(h[3])[self._per]):
                    match = pos
        how = mode.lower()
        if how == "set":
            if match is not None:
                raise Exception("\n\nHopping energy for this site was already specified! "
                                "Use mode=\"reset\" or mode=\"add\".")
            self._hoppings.append(entry)
        elif how == "reset":
            if match is None:
                self._hoppings.append(entry)
            else:
                self._hoppings[match] = entry
        elif how == "add":
            if match is None:
                self._hoppings.append(entry)
            else:
                self._hoppings[match][0] += entry[0]
        else:
            raise Exception("\n\nWrong value of mode parameter")
        self._tbk_epoch += 1

    def get_num_orbitals(self):
        return self._norb

    def get_orb(self):
        return self._orb.copy()

    def get_lat(self):
        return self._lat.copy()

    def invalidate_device_cache(self):
        """Call after editing `_hoppings` / `_site_energies` in place."""
        self._tbk_epoch += 1

    def __getstate__(self):                      # deepcopy / pickle: drop the device handle
        st = dict(self.__dict__)
        st["_tbk_cache"] = None
        st["_tbk_surface"] = {}
        st["_tbk_sparse"] = None
        return st

    def __del__(self):
        cache = getattr(self, "_tbk_cache", None)
        if cache is not None:
            try:
                _lib.lib.tbk_model_free(cache[2])
            except Exception:
                pass
        sparse = getattr(self, "_tbk_sparse", None)
        if sparse is not None:
            try:
                _lib.lib.tbk_sparse_free(sparse[2])
            except Exception:
                pass

    # ------------------------------------------------------------------ device
    def _flat_tables(self):
        """(orb_per, onsite, hop_i, hop_j, hop_R, hop_amp) in the layout of tbk_model_upload."""
        ns, no, dk = self._nspin, self._norb, self._dim_k
        nh = len(self._hoppings)
        orb_per = np.ascontiguousarray(self._orb[:, self._per], dtype=float).reshape(no, dk)
        onsite = np.zeros((no, ns, ns), dtype=complex)
        if ns == 1:
            onsite[:, 0, 0] = self._site_energies
        else:
            onsite[:] = self._site_energies
        # (whole-column conversions: a Python loop with four NumPy assignments per hopping was 22 us for the 9 hoppings of the
        # Haldane model -- more than the solve a parameter sweep re-uploads the model for)
        hops = self._hoppings
        if nh:
            hop_i = np.fromiter((hp[1] for hp in hops), dtype=np.int32, count=nh)
            hop_j = np.fromiter((hp[2] for hp in hops), dtype=np.int32, count=nh)
            hop_amp = np.empty((nh, ns, ns), dtype=complex)
            if ns == 1:
                hop_amp[:, 0, 0] = [hp[0] for hp in hops]
            else:
                for h, hp in enumerate(hops):
                    hop_amp[h] = hp[0]
            if dk > 0:
                hop_R = np.ascontiguousarray(np.array([hp[3] for hp in hops], dtype=np.int32).reshape(nh, -1)[:, self._per])
            else:
                hop_R = np.zeros((nh, 0), dtype=np.int32)
        else:
            hop_i = np.zeros(0, dtype=np.int32)
            hop_j = np.zeros(0, dtype=np.int32)
            hop_R = np.zeros((0, dk), dtype=np.int32)
            hop_amp = np.zeros((0, ns, ns), dtype=complex)
        return orb_per, onsite, hop_i, hop_j, hop_R, hop_amp

    def _device_model(self):
        ctx = _lib.default_context()
        c = self._tbk_cache
        # the epoch counts edits made through the setters/transforms; the fingerprint also catches scripts
        # that write `_orb` / `_site_energies` / `_hoppings` (length) directly, as some of the reference's do
        mark = (self._tbk_epoch, len(self._hoppings), self._orb.tobytes(), np.asarray(self._site_energies).tobytes())
        if c is not None and c[0] == mark and c[1] is ctx:
            return c[2]
        if c is not None:
            _lib.lib.tbk_model_free(c[2])
            self._tbk_cache = None
        orb_per, onsite, hop_i, hop_j, hop_R, hop_amp = self._flat_tables()
        h = C.c_void_p()
        _lib.check(_lib.lib.tbk_model_upload(
            ctx.handle, self._dim_k, self._norb, self._nspin, _lib.dptr(orb_per),
            _lib.dptr(onsite.view(float)), len(hop_i), _lib.iptr(hop_i), _lib.iptr(hop_j),
            _lib.iptr(hop_R.reshape(-1)) if hop_R.size else None,
            _lib.dptr(hop_amp.view(float)) if hop_amp.size else None, C.byref(h)))
        self._tbk_cache = (mark, ctx, h)
        return h

    # ------------------------------------------------------------------ solve
    def _k_array(self, k_list):
        k = np.asarray(k_list, dtype=float)          # no copy of an array that is already float64
        if k.size == 0:                               # empty list: the reference's loop runs zero times
            return np.zeros((0, self._dim_k), dtype=float)
        if self._dim_k == 1 and k.ndim == 1:
            k = k.reshape(-1, 1)
        if k.ndim != 2 or k.shape[1] != self._dim_k:
            raise Exception("\n\nk-vector of wrong shape!")
        return np.ascontiguousarray(k)

    def _gen_ham(self, k_input=None):
        """H(k) for one k in reduced coordinates (pythtb.py:874-925), built on the device."""
        if k_input is None:
            if self._dim_k != 0:
                raise Exception("\n\nHave to provide a k-vector!")
            k = None
        else:
            kp = np.array(k_input, dtype=float)
            if kp.ndim == 0:
                kp = kp.reshape(1)
            if kp.shape != (self._dim_k,):
                raise Exception("\n\nk-vector of wrong shape!")
            k = np.ascontiguousarray(kp.reshape(1, -1))
        n = self._nsta
        ham = np.zeros((1, n, n), dtype=complex)
        _lib.check(_lib.lib.tbk_gen_ham(self._device_model(), _lib.dptr(k) if self._dim_k else None, 1,
                                        _lib.dptr(ham.view(float))))
        if self._nspin == 1:
            return ham[0]
        return ham[0].reshape(self._norb, 2, self._norb, 2)

    def _sol_ham(self, ham, eig_vectors=False):
        """Eigen-decomposition of one Hamiltonian (pythtb.py:927-953), on the device."""
        n = self._nsta
        hm = np.ascontiguousarray(np.array(ham, dtype=complex).reshape(1, n, n))
        if np.max(hm[0] - hm[0].T.conj()) > 1.0E-9:
            raise Exception("\n\nHamiltonian matrix is not hermitian?!")
        ev = np.zeros((n, 1), dtype=float)
        vec = np.zeros((n, 1, n), dtype=complex) if eig_vectors else None
        _lib.check(_lib.lib.tbk_eigh_batch(_lib.default_context().handle, n, _lib.dptr(hm.view(float)), 1,
                                           _lib.dptr(ev), _lib.dptr(vec.view(float)) if eig_vectors else None))
        if not eig_vectors:
            return ev[:, 0].copy()
        out = vec[:, 0, :]
        if self._nspin == 2:
            out = out.reshape(n, self._norb, 2)
        return ev[:, 0].copy(), out.copy()

    def solve_all(self, k_list=None, eig_vectors=False):
        """Eigenvalues eval[band,k] (and evec[band,k,orb(,spin)]) on a list of k
        (pythtb.py:955-1079): one fused H(k)+eigh launch over the whole list."""
        n = self._nsta
        if k_list is None:
            if self._dim_k != 0:
                raise Exception("\n\nHave to provide a k-vector!")
            nk, k = 1, None
        else:
            k = self._k_array(k_list) if self._dim_k > 0 else None
            nk = len(k_list)
        ev = np.empty((n, nk), dtype=float)                   # filled completely by the device-to-host copies
        vec = np.empty((n, nk, n), dtype=complex) if eig_vectors else None
        if nk > 0:
            _lib.check(_lib.lib.tbk_solve_list(self._device_model(), _lib.dptr(k), nk, _lib.dptr(ev),
                                               _lib.dptr(vec.view(float)) if eig_vectors else None))
        if eig_vectors and self._nspin == 2:
            vec = vec.reshape(n, nk, self._norb, 2)
        if k_list is None:
            return (ev[:, 0], vec[:, 0]) if eig_vectors else ev[:, 0]
        return (ev, vec) if eig_vectors else ev

    def solve_one(self, k_point=None, eig_vectors=False):
        """solve_all for a single k (pythtb.py:1081-1103)."""
        if k_point is None:
            return self.solve_all(eig_vectors=eig_vectors)
        if eig_vectors:
            ev, vec = self.solve_all([k_point], eig_vectors=True)
            return ev[:, 0], vec[:, 0]
        return self.solve_all([k_point])[:, 0]

    # ------------------------------------------------------------------ mesh shortcuts (extensions)
    def _mesh_arg(self, mesh_size):
        mesh = np.array(list(map(round, mesh_size)), dtype=np.int32)     # same checks as k_uniform_mesh
        if mesh.shape != (self._dim_k,):
            print(mesh.shape)
            raise Exception("\n\nIncorrect size of the specified k-mesh!")
        if np.min(mesh) <= 0:
            raise Exception("\n\nMesh must have positive non-zero number of elements.")
        if self._dim_k not in (1, 2, 3):
            raise Exception("\n\nUnsupported dim_k!")
        return np.ascontiguousarray(mesh), int(np.prod(mesh, dtype=np.int64))

    def solve_all_mesh(self, mesh_size, eig_vectors=False):
        """Extension: `solve_all(k_uniform_mesh(mesh_size), eig_vectors)` with the k list generated
        on the device -- the same arrays, minus the 8*dim_k bytes per k-point of upload."""
        mesh, nk = self._mesh_arg(mesh_size)
        n = self._nsta
        ev = np.zeros((n, nk), dtype=float)
        vec = np.zeros((n, nk, n), dtype=complex) if eig_vectors else None
        _lib.check(_lib.lib.tbk_solve_mesh(self._device_model(), _lib.iptr(mesh), _lib.dptr(ev),
                                           _lib.dptr(vec.view(float)) if eig_vectors else None))
        if eig_vectors and self._nspin == 2:
            vec = vec.reshape(n, nk, self._norb, 2)
        return (ev, vec) if eig_vectors else ev

    def dos_mesh(self, mesh_size, bins=50, range=None, per_band=False):
        """Extension: `np.histogram(solve_all(k_uniform_mesh(mesh_size)).flatten(), bins, range)` -- the
        density-of-states reduction of the reference's examples/haldane.py:96-121 -- with the
        eigenvalues kept on the device: (counts, bin_edges), counts int64 `(bins,)`, or
        `(nsta, bins)` with per_band=True.  `bins` is a number of equal-width bins."""
        mesh, nk = self._mesh_arg(mesh_size)
        if not _is_int(bins) or bins < 1:
            raise Exception("\n\ndos_mesh: bins must be a positive integer (equal-width bins)")
        n = self._nsta
        h = self._device_model()
        if range is None:
            lo = np.zeros(n)
            hi = np.zeros(n)
            _lib.check(_lib.lib.tbk_dos_mesh(h, _lib.iptr(mesh), 0, None, None, _lib.dptr(lo), _lib.dptr(hi)))
            range = (lo.min(), hi.max())
        # the edges np.histogram itself would use for this range (incl. its widening of an empty range)
        edges = np.ascontiguousarray(np.histogram_bin_edges(np.zeros(0), bins=int(bins), range=range), dtype=float)
        counts = np.zeros((n, int(bins)), dtype=np.int64)
        _lib.check(_lib.lib.tbk_dos_mesh(h, _lib.iptr(mesh), int(bins), _lib.dptr(edges),
                                         counts.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int64)), None, None))
        return (counts if per_band else counts.sum(axis=0)), edges

    # ------------------------------------------------------------------ Berry curvature (extensions)
    def _gen_dham(self, k_input, dir):
        """Extension: dH/dk_dir for one k in reduced coordinates, with the shapes of `_gen_ham`
        (`(norb, 2, norb, 2)` for spinful models): sum t 2 pi i (R + tau_j - tau_i)_dir e^{2 pi i k.(R + tau_j - tau_i)}."""
        if self._dim_k < 1:
            raise Exception("\n\n_gen_dham needs a model with dim_k >= 1")
        if not _is_int(dir) or dir < 0 or dir >= self._dim_k:
            raise Exception("\n\n_gen_dham: dir must be an axis in [0, dim_k)")
        kp = np.array(k_input, dtype=float)
        if kp.ndim == 0:
            kp = kp.reshape(1)
        if kp.shape != (self._dim_k,):
            raise Exception("\n\nk-vector of wrong shape!")
        k = np.ascontiguousarray(kp.reshape(1, -1))
        n = self._nsta
        out = np.zeros((1, n, n), dtype=complex)
        _lib.check(_lib.lib.tbk_gen_dham(self._device_model(), _lib.dptr(k), 1, int(dir), _lib.dptr(out.view(float))))
        if self._nspin == 1:
            return out[0]
        return out[0].reshape(self._norb, 2, self._norb, 2)

    def _curv_args(self, occ, dirs, what="Berry curvature"):
        """Checked (occ as int32 indices or None, dir0, dir1) of the curvature and orbital-moment calls."""
        if self._dim_k < 2:
            raise Exception("\n\nThe %s needs a model with dim_k >= 2." % what)
        dirs = list(dirs)
        if len(dirs) != 2 or not all(_is_int(d) for d in dirs):
            raise Exception("\n\ndirs must be two integer axes.")
        if dirs[0] == dirs[1]:
            raise Exception("\n\nNeed to specify two different directions for the %s." % what)
        if min(dirs) < 0 or max(dirs) >= self._dim_k:
            raise Exception("\n\nDirection for the %s out of bounds." % what)
        if occ is None:
            return None, int(dirs[0]), int(dirs[1])
        sel = np.arange(self._nsta)[occ]                 # a NumPy fancy index, as wf_array.berry_flux reads it (IndexError)
        sel = np.atleast_1d(sel).ravel()
        if sel.size == 0:
            raise Exception("\n\nocc selects no band.")
        if np.unique(sel).size != sel.size:
            raise Exception("\n\nocc lists a band twice.")
        return np.ascontiguousarray(sel, dtype=np.int32), int(dirs[0]), int(dirs[1])

    @staticmethod
    def _fermi_levels_arg(sel, fermi_levels):
        """Checked Fermi levels of a curvature scan as a float64 array, or None (sel: the band set, exclusive with them)."""
        if fermi_levels is None:
            return None
        if sel is not None:
            raise Exception("\n\nGive either occ or fermi_levels, not both.")
        mu = np.ascontiguousarray(np.array(fermi_levels, dtype=float))
        if mu.ndim != 1 or mu.size < 1 or mu.size > 8192:
            raise Exception("\n\nfermi_levels must be a 1-D array of 1..8192 levels.")
        if not np.all(np.isfinite(mu)):
            raise Exception("\n\nfermi_levels must be finite.")
        return mu

    def berry_curvature(self, k_list, occ=None, dirs=(0, 1)):
        """Extension: the Berry curvature by the Kubo formula at every k of `k_list` (reduced coordinates, as solve_all).

        occ=None: per band, float64 `(nsta, nk)` (the layout of solve_all's eigenvalues),
            Omega_n(k) = -2 Im sum_{m != n} <n|dH_a|m><m|dH_b|n> / (E_n - E_m)^2,  (a, b) = dirs;
            a pair with |E_n - E_m| <= 1e-9 max(1, |E_n|, |E_m|) contributes to neither band.
        occ given (a NumPy index of bands): the gauge-invariant curvature of that band set, `(nk,)`,
            -2 Im sum_{n in occ, m not in occ} (same terms) -- what berry_flux(occ, dirs) measures per plaquette.  It is not
            finite (or huge) where a band of occ touches one outside it, as berry_flux is meaningless there.
        Reduced units: the mean over a uniform (a, b) mesh divided by 2 pi is the Chern number.  The Cartesian curvature of a
        2-D cell of area A (dirs spanning it) is Omega_xy = Omega A / (2 pi)^2, in the length unit of the lattice vectors."""
        sel, d0, d1 = self._curv_args(occ, dirs)
        k = self._k_array(k_list)
        nk = k.shape[0]
        n = self._nsta
        out = np.zeros(nk if sel is not None else (n, nk), dtype=float)
        if nk == 0:
            return out
        _lib.check(_lib.lib.tbk_berry_curv_list(self._device_model(), _lib.dptr(k), nk, d0, d1, _lib.iptr(sel),
                                                0 if sel is None else len(sel), _lib.dptr(out)))
        return out

    def berry_curvature_mesh(self, mesh_size, occ=None, dirs=(0, 1), fermi_levels=None):
        """Extension: means of the Berry curvature over `k_uniform_mesh(mesh_size)` (generated on the device), i.e. BZ
        integrals in reduced units -- divided by 2 pi, the Chern number of a gapped set.

        2-D mesh: occ given -> a float (the band set's integral); occ=None -> per band `(nsta,)`;
            fermi_levels (1-D, at most 8192 values, any order) -> `(nmu,)` in input order,
            I(mu) = mean_k sum_{n: E_n(k) <= mu} Omega_n(k), the T = 0 anomalous-Hall integral (sigma_xy = -(e^2/h) I / 2 pi
            per layer).
        3-D mesh: every result gains a trailing axis over the mesh direction that is not in dirs, one (dirs) plane per slice.
        Curvatures as in `berry_curvature`; the reductions have a fixed order, so two calls give the same bits."""
        sel, d0, d1 = self._curv_args(occ, dirs)
        mesh, nk = self._mesh_arg(mesh_size)
        if self._dim_k not in (2, 3):
            raise Exception("\n\nberry_curvature_mesh needs a 2-D or 3-D mesh.")
        mu = self._fermi_levels_arg(sel, fermi_levels)
        n = self._nsta
        nch = mu.size if mu is not None else (1 if sel is not None else n)
        nslice = 1 if self._dim_k == 2 else int(mesh[3 - d0 - d1])
        out = np.zeros((nch, nslice), dtype=float)
        _lib.check(_lib.lib.tbk_berry_curv_mesh(self._device_model(), _lib.iptr(mesh), d0, d1, _lib.iptr(sel),
                                                0 if sel is None else len(sel), 0 if mu is None else mu.size,
                                                _lib.dptr(mu), _lib.dptr(out)))
        if self._dim_k == 2:
            out = out[:, 0]
            return float(out[0]) if sel is not None else out
        return out[0] if sel is not None else out

    # ------------------------------------------------------------------ quantum geometric tensor (extensions)
    def _qgt_args(self, occ):
        """Checked band set of the quantum-geometry calls (int32 indices or None); `occ` is read as `_curv_args` reads it."""
        if self._dim_k not in (1, 2, 3):
            raise Exception("\n\nThe quantum geometric tensor needs a model with dim_k 1, 2 or 3.")
        if occ is None:
            return None
        sel = np.arange(self._nsta)[occ]                 # a NumPy fancy index (IndexError)
        sel = np.atleast_1d(sel).ravel()
        if sel.size == 0:
            raise Exception("\n\nocc selects no band.")
        if np.unique(sel).size != sel.size:
            raise Exception("\n\nocc lists a band twice.")
        return np.ascontiguousarray(sel, dtype=np.int32)

    def _qgt_assemble(self, raw):
        """Hermitian Q = g - i Omega / 2, `(..., dk, dk)` complex, from the library's `(..., dk^2)` doubles: g_ab for a <= b in
        `np.triu_indices(dk)` order, then Omega_ab for a < b in the same order."""
        dk = self._dim_k
        iu = np.triu_indices(dk)
        io = np.triu_indices(dk, 1)
        ng = len(iu[0])
        q = np.zeros(raw.shape[:-1] + (dk, dk), dtype=complex)
        q[..., iu[0], iu[1]] = raw[..., :ng]
        q[..., iu[1], iu[0]] = raw[..., :ng]
        q[..., io[0], io[1]] -= 0.5j * raw[..., ng:]
        q[..., io[1], io[0]] += 0.5j * raw[..., ng:]
        return q

    def quantum_geometric_tensor(self, k_list, occ=None):
        """Extension: the quantum geometric tensor by the Kubo formula at every k of `k_list` (reduced coordinates, as
        solve_all), over all dk = dim_k axes (1, 2 or 3) at once, complex128.

        occ=None: per band, `(nsta, nk, dk, dk)`,
            Q^n_ab(k) = sum_{m != n} <n|dH_a|m><m|dH_b|n> / (E_n - E_m)^2;
            a pair with |E_n - E_m| <= 1e-9 max(1, |E_n|, |E_m|) contributes to neither band (the rule of `berry_curvature`).
        occ given (a NumPy index of bands): the band set's tensor `(nk, dk, dk)`, the sum over n in occ and m not in occ of the
            same terms (no degeneracy rule) = Tr[P d_aP d_bP]: gauge invariant inside the set, and not finite where the set
            touches a band outside it.
        Q is Hermitian and positive semidefinite, Q = g - i Omega / 2: g_ab = Re Q_ab is the quantum metric (`quantum_metric`) and
        Omega_ab = -2 Im Q_ab is `berry_curvature(..., dirs=(a, b))`.
        There is no Fermi-level scan, on purpose: sum_{n in occ} Q^n is NOT Q^occ for the real part -- the pairs of two
        occupied bands cancel in Omega but count twice in g -- so a scan built from per-band sums would be wrong."""
        sel = self._qgt_args(occ)
        k = self._k_array(k_list)
        nk, n, dk = k.shape[0], self._nsta, self._dim_k
        raw = np.zeros((nk, dk * dk) if sel is not None else (n, nk, dk * dk), dtype=float)
        if nk > 0:
            _lib.check(_lib.lib.tbk_qgt_list(self._device_model(), _lib.dptr(k), nk, _lib.iptr(sel),
                                             0 if sel is None else len(sel), _lib.dptr(raw)))
        return self._qgt_assemble(raw)

    def quantum_metric(self, k_list, occ=None):
        """Extension: the quantum metric g_ab = Re Q_ab of `quantum_geometric_tensor(k_list, occ)` as float64, same shapes:
        `(nsta, nk, dk, dk)` per band or `(nk, dk, dk)` for a band set.  No Fermi-level scan (see there)."""
        return np.ascontiguousarray(self.quantum_geometric_tensor(k_list, occ).real)

    def quantum_geometric_tensor_mesh(self, mesh_size, occ=None, cartesian=False):
        """Extension: the mean of `quantum_geometric_tensor` over the whole `k_uniform_mesh(mesh_size)` (1-, 2- or 3-D, generated
        on the device): complex `(nsta, dk, dk)` per band, `(dk, dk)` for a band set.  -2 Im of its (a, b) entry is the mean
        curvature (2 pi times the Chern number of a gapped set in 2-D).
        cartesian=True returns A^T Q A / (2 pi)^2, `(..., dim_r, dim_r)`, with the A of `drude_weight_mesh` (the periodic
        lattice vectors as rows): its real trace is the band set's gauge-invariant Wannier spread Omega_I per cell, in the
        squared length unit of the lattice vectors.  Fixed-order reductions: two calls give the same bits.  No Fermi-level
        scan (see `quantum_geometric_tensor`)."""
        sel = self._qgt_args(occ)
        if not isinstance(cartesian, (bool, np.bool_)):
            raise Exception("\n\ncartesian must be True or False.")
        mesh, nk = self._mesh_arg(mesh_size)
        n, dk = self._nsta, self._dim_k
        raw = np.zeros((dk * dk,) if sel is not None else (n, dk * dk), dtype=float)
        _lib.check(_lib.lib.tbk_qgt_mesh(self._device_model(), _lib.iptr(mesh), _lib.iptr(sel), 0 if sel is None else len(sel),
                                         _lib.dptr(raw)))
        q = self._qgt_assemble(raw)
        if not cartesian:
            return q
        a = np.array(self._lat, dtype=float)[self._per]               # (dim_k, dim_r)
        return np.einsum("ia,...ij,jb->...ab", a, q, a) / (2.0 * np.pi) ** 2

    # ------------------------------------------------------------------ spin Berry curvature (extensions)
    def _spin_arg(self, spin, what):
        """Checked spin direction of the spin-current calls as a float64 3-vector: 0, 1 or 2 (sigma_x, sigma_y, sigma_z) or a
        finite real 3-vector, used as given."""
        if self._nspin != 2:
            raise Exception("\n\nThe %s needs a spinful model (nspin = 2)." % what)
        if _is_int(spin):
            if spin not in (0, 1, 2):
                raise Exception("\n\nspin must be 0, 1 or 2 (sigma_x, sigma_y, sigma_z) or a real 3-vector.")
            vec = np.zeros(3, dtype=float)
            vec[int(spin)] = 1.0
            return vec
        try:
            if np.iscomplexobj(spin):
                raise TypeError
            vec = np.array(spin, dtype=float)
        except (TypeError, ValueError):
            raise Exception("\n\nspin must be 0, 1 or 2 (sigma_x, sigma_y, sigma_z) or a real 3-vector.")
        if vec.shape != (3,) or not np.all(np.isfinite(vec)):
            raise Exception("\n\nspin must be 0, 1 or 2 (sigma_x, sigma_y, sigma_z) or a finite real 3-vector.")
        return np.ascontiguousarray(vec)

    def _gen_jham(self, k_input, dir, spin=2):
        """Extension: the spin current J = (S dH/dk_dir + dH/dk_dir S) / 2, S = 1_orb (x) s.sigma, for one k in reduced
        coordinates, in `_gen_ham`'s `(norb, 2, norb, 2)` shape (computed on the device; the twin of `_gen_dham`)."""
        vec = self._spin_arg(spin, "spin current")
        if self._dim_k < 1:
            raise Exception("\n\n_gen_jham needs a model with dim_k >= 1")
        if not _is_int(dir) or dir < 0 or dir >= self._dim_k:
            raise Exception("\n\n_gen_jham: dir must be an axis in [0, dim_k)")
        kp = np.array(k_input, dtype=float)
        if kp.ndim == 0:
            kp = kp.reshape(1)
        if kp.shape != (self._dim_k,):
            raise Exception("\n\nk-vector of wrong shape!")
        k = np.ascontiguousarray(kp.reshape(1, -1))
        n = self._nsta
        out = np.zeros((1, n, n), dtype=complex)
        _lib.check(_lib.lib.tbk_gen_jham(self._device_model(), _lib.dptr(k), 1, int(dir), _lib.dptr(vec),
                                         _lib.dptr(out.view(float))))
        return out[0].reshape(self._norb, 2, self._norb, 2)

    def spin_berry_curvature(self, k_list, spin=2, occ=None, dirs=(0, 1)):
        """Extension: the spin Berry curvature of a spinful model by the Kubo formula at every k of `k_list` -- `berry_curvature`
        with the first velocity replaced by the spin current J^a = (S dH_a + dH_a S) / 2, S = 1_orb (x) s.sigma:

            Omega^s_n(k) = -2 Im sum_{m != n} <n|J^a|m><m|dH_b|n> / (E_n - E_m)^2,  (a, b) = dirs.

        `spin`: 0, 1 or 2 for sigma_x, sigma_y, sigma_z, or a finite real 3-vector s (used as given, not normalised; the result
        is linear in it).  Shapes, `occ` and the degeneracy rule as in `berry_curvature`: `(nsta, nk)` per band, `(nk,)` for a
        band set (pairs inside the set cancel, as for the charge curvature)."""
        vec = self._spin_arg(spin, "spin Berry curvature")
        sel, d0, d1 = self._curv_args(occ, dirs, "spin Berry curvature")
        k = self._k_array(k_list)
        nk = k.shape[0]
        out = np.zeros(nk if sel is not None else (self._nsta, nk), dtype=float)
        if nk == 0:
            return out
        _lib.check(_lib.lib.tbk_spin_curv_list(self._device_model(), _lib.dptr(k), nk, d0, d1, _lib.iptr(sel),
                                               0 if sel is None else len(sel), _lib.dptr(vec), _lib.dptr(out)))
        return out

    def spin_hall_conductivity_mesh(self, mesh_size, spin=2, occ=None, dirs=(0, 1), fermi_levels=None):
        """Extension: means of `spin_berry_curvature` over `k_uniform_mesh(mesh_size)` (generated on the device), with every
        rule of `berry_curvature_mesh`: a float for a band set, `(nsta,)` per band, `(nmu,)` for `fermi_levels`
        (I^s(mu) = mean_k sum_{n: E_n(k) <= mu} Omega^s_n(k), 1..8192 finite levels in any order, returned in input order;
        either occ or fermi_levels, not both), and a trailing slice axis for 3-D meshes.

        Units: with spin hbar sigma / 2 and the sign convention of `berry_curvature_mesh`, the spin Hall conductivity is
        sigma^s_ab = (e / 4 pi) I^s / (2 pi) per layer; for a model that conserves S_z, I^s / (2 pi) = C_up - C_down.
        `spin` as in `spin_berry_curvature`.  Fixed-order reductions: two calls give the same bits."""
        vec = self._spin_arg(spin, "spin Hall conductivity")
        sel, d0, d1 = self._curv_args(occ, dirs, "spin Hall conductivity")
        mesh, nk = self._mesh_arg(mesh_size)
        if self._dim_k not in (2, 3):
            raise Exception("\n\nspin_hall_conductivity_mesh needs a 2-D or 3-D mesh.")
        mu = self._fermi_levels_arg(sel, fermi_levels)
        nch = mu.size if mu is not None else (1 if sel is not None else self._nsta)
        nslice = 1 if self._dim_k == 2 else int(mesh[3 - d0 - d1])
        out = np.zeros((nch, nslice), dtype=float)
        _lib.check(_lib.lib.tbk_spin_curv_mesh(self._device_model(), _lib.iptr(mesh), d0, d1, _lib.iptr(sel),
                                               0 if sel is None else len(sel), 0 if mu is None else mu.size,
                                               _lib.dptr(mu), _lib.dptr(vec), _lib.dptr(out)))
        if self._dim_k == 2:
            out = out[:, 0]
            return float(out[0]) if sel is not None else out
        return out[0] if sel is not None else out

    def optical_conductivity_mesh(self, mesh_size, omega, eta, fermi_level=0.0, kT=0.0, dirs=None, cartesian=False):
        """Extension: the interband optical conductivity tensor by the Kubo formula, averaged over the whole
        `k_uniform_mesh(mesh_size)` (1-, 2- or 3-D, generated on the device):

            S_ab(w) = (i / N_k) sum_k sum_{n != m} [(f_m - f_n) / (E_m - E_n)] V^a_nm V^b_mn / (E_m - E_n - w - i eta)

        k reduced, H the matrix of `_gen_ham`, V^a = dH/dk_a (`_gen_dham`), E_n and |n> the eigenpairs of `solve_all`,
        f_n = [E_n <= fermi_level] for kT = 0, else 1 / (1 + exp((E_n - fermi_level) / kT)).  Pairs with
        |E_m - E_n| <= 1e-9 max(1, |E_n|, |E_m|) are left out (interband only, no Drude term); eta > 0 is a constant
        Lorentzian half-width; time dependence e^{-i w t}; no spin-degeneracy factor.

        omega: 1-D, 1..65536 finite frequencies in any order.  dirs=None -> complex `(nw, dim_k, dim_k)`; dirs=(a, b)
        (a == b allowed) -> `(nw,)`, the component S_ab.  Re S_aa >= 0 (passive), S(-w) = conj S(w), and S_ab = S_ba with
        time reversal.  DC limit: at w = 0, eta -> 0, Re (S_ab - S_ba) / 2 = -I(mu) of `berry_curvature_mesh(mesh,
        dirs=(a, b), fermi_levels=[mu])` (the slice mean for a 3-D mesh); the error shrinks as eta^2.
        cartesian=True (dirs=None only) returns sigma = A^T S A / ((2 pi)^2 V_c), `(nw, dim_r, dim_r)`, in units of
        e^2/hbar x length^(2 - dim_k), A = the periodic lattice vectors as rows, V_c = sqrt(det(A A^T)); spinless graphene
        gives Re sigma_xx -> 1/8 at small w.  A one-state model, or kT = 0 with the Fermi level below or above every
        level, gives exact zeros.  Fixed reduction order: two calls give the same bits.  The pairs left out here -- the
        intraband (Drude) weight of a metal at kT > 0 -- are `drude_weight_mesh`."""
        if self._dim_k not in (1, 2, 3):
            raise Exception("\n\noptical_conductivity_mesh needs a model with dim_k 1, 2 or 3.")
        mesh, nk = self._mesh_arg(mesh_size)
        w = _sweep_args(omega, eta, fermi_level, kT)
        if dirs is None:
            d0 = d1 = -1
        else:
            dirs = list(dirs)
            if len(dirs) != 2 or not all(_is_int(d) for d in dirs):
                raise Exception("\n\ndirs must be two integer axes.")
            if min(dirs) < 0 or max(dirs) >= self._dim_k:
                raise Exception("\n\nDirection for the optical conductivity out of bounds.")
            if cartesian:
                raise Exception("\n\ncartesian=True returns the whole tensor: give dirs=None.")
            d0, d1 = int(dirs[0]), int(dirs[1])
        dk = self._dim_k
        out = np.zeros((w.size, dk, dk) if d0 < 0 else (w.size,), dtype=complex)
        if self._nsta > 1:
            _lib.check(_lib.lib.tbk_optical_cond_mesh(self._device_model(), _lib.iptr(mesh), int(w.size), _lib.dptr(w),
                                                      float(eta), float(fermi_level), float(kT), d0, d1,
                                                      _lib.dptr(out.view(float))))
        if not cartesian:
            return out
        a = np.array(self._lat, dtype=float)[self._per]               # (dim_k, dim_r)
        vc = np.sqrt(np.linalg.det(a @ a.T))
        return np.einsum("ia,wij,jb->wab", a, out, a) / ((2.0 * np.pi) ** 2 * vc)

    def _q_list_arg(self, q_list):
        """(q, single) of the susceptibility calls: the checked q list as a contiguous `(nq, dim_k)` array; single: it was one
        `(dim_k,)` point."""
        q = np.array(q_list, dtype=float)
        single = q.ndim == 1
        if single:
            q = q.reshape(1, -1)
        if q.ndim != 2 or q.shape[1] != self._dim_k or q.shape[0] < 1 or q.shape[0] > 65536:
            raise Exception("\n\nq_list must have shape (nq, dim_k) with 1..65536 points, or (dim_k,).")
        if not np.all(np.isfinite(q)):
            raise Exception("\n\nq_list must be finite.")
        return np.ascontiguousarray(q), single

    def susceptibility_mesh(self, mesh_size, q_list, omega=None, eta=None, fermi_level=0.0, kT=0.0, matrix_elements=True):
        """Extension: the bare (Lindhard) susceptibility at momentum transfer q, averaged over the whole
        `k_uniform_mesh(mesh_size)` (1-, 2- or 3-D, generated on the device).  Dynamic (`omega` and `eta > 0` given):

            chi0(q, w) = -(1 / N_k) sum_k sum_{n,m} [f(E_n(k)) - f(E_m(k+q))] |M_nm(k,q)|^2 / (w + i eta + E_n(k) - E_m(k+q))
            M_nm(k,q)  = sum_j conj(u_n(k)[j]) u_m(k+q)[j]        (= <psi_nk| e^{-i q.r} |psi_m,k+q>, r at the orbital positions)

        k and q reduced, E_n and u_n the eigenpairs of `solve_all` (the matrix of `_gen_ham`, whose phases carry the orbital
        positions: u is the cell-periodic part), f = [E <= fermi_level] for kT = 0, else the Fermi function.  All n^2 ordered
        pairs take part, n = m (intraband) included; nothing is left out (every term is finite for eta > 0); no
        spin-degeneracy factor.  Sign: Re chi0(q, 0) >= 0 and Im chi0(q, w > 0) >= 0.  Units: per unit cell and per energy.

        Static (`omega=None`; `eta` must then be None): the exact eta -> 0, w = 0 limit, float `(nq,)`,

            chi0(q) = (1 / N_k) sum_k sum_{n,m} L_nm |M_nm|^2,    L = -(f_n - f_m) / (E_n - E_m)

        with L = 0 where f_n = f_m at kT = 0, and L = (sinh h / h) / (2 kT (cosh h + cosh u)), h = (E_m(k+q) - E_n(k)) / 2kT,
        u = ((E_n + E_m) / 2 - fermi_level) / kT at kT > 0: smooth through E_n = E_m, where it is -f'(E).  The dynamic form at
        any eta > 0 and w = 0 DROPS the terms with E_n(k) = E_m(k+q) exactly (a nested Fermi surface on a commensurate mesh,
        q = 0): their numerator vanishes before the denominator does.  The static mode keeps them -- that is why it exists.

        q_list: `(nq, dim_k)`, 1 <= nq <= 65536, or `(dim_k,)` for one q (the leading axis of the result is then dropped);
        finite, any real values (a `k_path`, a `k_uniform_mesh`, incommensurate points).  omega: 1-D, 1..65536 finite
        frequencies in any order, nq * nw <= 2**22; the result is complex `(nq, nw)`.  matrix_elements=False replaces
        |M|^2 by 1: the band-only Lindhard (nesting) function, from eigenvalue-only solves.

        chi0(q = 0, w) = 0 to rounding (charge conservation).  Two symmetries one might expect do NOT hold in general:
        chi0(-q, -w) = conj chi0(q, w) holds only for q commensurate with the mesh (for other q the discrete k sum is not
        invariant under the shift k -> k - q), and chi0(q + G) = chi0(q) holds only when every orbital sits on a lattice
        point (otherwise e^{-i q.r} gives a form factor).  At kT = 0 a Fermi level below or above every level gives exact
        zeros.  Fixed reduction order: two calls give the same bits, and a q gives the same bits alone and inside a longer
        q_list.  Each q costs a second eigen-solve of the mesh, the larger part of a static map's time; no timing is claimed
        beyond the measured cases of DESIGN.md section 26."""
        if self._dim_k not in (1, 2, 3):
            raise Exception("\n\nsusceptibility_mesh needs a model with dim_k 1, 2 or 3.")
        mesh, nk = self._mesh_arg(mesh_size)
        q, single = self._q_list_arg(q_list)
        nq = q.shape[0]
        flags = 1 if matrix_elements else 0
        if omega is None:
            if eta is not None:
                raise Exception("\n\nThe static mode (omega=None) is the eta -> 0 limit: eta must be None.")
            _sweep_args([0.0], 1.0, fermi_level, kT)
            out = np.zeros(nq, dtype=float)
            _lib.check(_lib.lib.tbk_susceptibility_mesh(self._device_model(), _lib.iptr(mesh), nq, _lib.dptr(q), 0, None, 0.0,
                                                        float(fermi_level), float(kT), flags, _lib.dptr(out)))
        else:
            if eta is None:
                raise Exception("\n\nThe dynamic mode (omega given) needs eta > 0.")
            w = _sweep_args(omega, eta, fermi_level, kT)
            if nq * w.size > 2 ** 22:
                raise Exception("\n\nnq * nw must be at most 2**22: split q_list or omega.")
            out = np.zeros((nq, w.size), dtype=complex)
            _lib.check(_lib.lib.tbk_susceptibility_mesh(self._device_model(), _lib.iptr(mesh), nq, _lib.dptr(q), int(w.size),
                                                        _lib.dptr(w), float(eta), float(fermi_level), float(kT), flags,
                                                        _lib.dptr(out.view(float))))
        return out[0] if single else out

    def susceptibility_matrix_mesh(self, mesh_size, q_list, omega=None, eta=None, fermi_level=0.0, kT=0.0, states=None,
                                   interaction=None, return_det=False):
        """Extension: the orbital-resolved bare susceptibility and the RPA on top of it.  Every convention of
        `susceptibility_mesh` (k and q reduced, the eigenpairs of `solve_all`, f = [E <= fermi_level] or the Fermi function, all
        n^2 ordered pairs, no spin factor, the mean over `k_uniform_mesh(mesh_size)` generated on the device, any real q), with
        the orbital index kept:

            chi0_ab(q, w) = -(1 / N_k) sum_k sum_{n,m} [f(E_n(k)) - f(E_m(k+q))] A_a conj(A_b) / (w + i eta + E_n(k) - E_m(k+q))
            A_a(k, q)     = conj(u_n(k)[a]) u_m(k+q)[a]

        complex `(nq, nw, na, na)`; static (`omega=None`, `eta=None`): chi0_ab(q) = (1 / N_k) sum_k sum_{n,m} L_nm A_a conj(A_b)
        with the weight L of `susceptibility_mesh`, complex `(nq, na, na)`: Hermitian and positive semidefinite, but not real in
        general.  A single `(dim_k,)` q drops the leading axis.  The sum over a, b of ALL states is the scalar chi0 of
        `susceptibility_mesh`.  At q = 0 every row and column sum of the dynamic matrix vanishes (charge conservation per
        orbital); the static ones at kT > 0 do not (the intraband -f' term stays).

        states: the indices a -- STATE indices 0 .. nsta - 1, components of the eigenvector in the layout of
        `solve_one(..., eig_vectors=True)` (a spinful model has 2 norb of them, orbital-major).  None: all states (nsta <= 16);
        else 1..16 distinct integers in [0, nsta) in any order (no negative indices); the a, b axes follow the order given.
        nq * max(nw, 1) * na^2 <= 2**22.

        interaction: None returns chi0.  A finite complex `(na, na)` matrix V, or `(nq, na, na)` for a V(q), not necessarily
        Hermitian, returns `(chi0, chi_rpa)` with chi_rpa = (1 - chi0 V)^-1 chi0 per (q, w), and with `return_det=True`
        `(chi0, chi_rpa, det)`, det = det(1 - chi0 V), complex `(nq,)` or `(nq, nw)`: the generalized Stoner criterion, whose
        zeros in w are the collective modes.  With chi0 per spin, as here, the transverse spin channel of an on-site Hubbard U
        is V = U * identity, the charge channel V = -U * identity (-(U + 2 V(q)) with an extended term).  The solve is an LU
        with partial pivoting on the device.  A pivot that is exactly 0 does NOT raise: that matrix of chi_rpa is NaN and its
        det is 0 -- the Stoner point itself is a legitimate input.  The eigenvalues of chi0 V, if wanted, are one line on the
        host: `np.linalg.eigvals(chi0 @ V)`.

        Fixed reduction order: two calls give the same bits, a q gives the same bits alone and inside a longer q_list, and chi0
        has the same bits with and without an interaction.  Each q costs a second eigen-solve of the mesh; the measured cases
        are in DESIGN.md section 28."""
        if self._dim_k not in (1, 2, 3):
            raise Exception("\n\nsusceptibility_matrix_mesh needs a model with dim_k 1, 2 or 3.")
        mesh, nk = self._mesh_arg(mesh_size)
        q, single = self._q_list_arg(q_list)
        nq = q.shape[0]
        if omega is None:
            if eta is not None:
                raise Exception("\n\nThe static mode (omega=None) is the eta -> 0 limit: eta must be None.")
            _sweep_args([0.0], 1.0, fermi_level, kT)
            w, nw, eta = None, 0, 0.0
        else:
            if eta is None:
                raise Exception("\n\nThe dynamic mode (omega given) needs eta > 0.")
            w = _sweep_args(omega, eta, fermi_level, kT)
            nw = int(w.size)
        if states is None:
            if self._nsta > 16:
                raise Exception("\n\nstates=None means all states, which needs nsta <= 16: give states (1..16 state indices).")
            sel = np.arange(self._nsta, dtype=np.int32)
        else:
            st = np.asarray(states)
            if st.ndim != 1 or st.size < 1 or st.size > 16 or not np.issubdtype(st.dtype, np.integer):
                raise Exception("\n\nstates must be a list of 1..16 integer state indices.")
            if st.min() < 0 or st.max() >= self._nsta or np.unique(st).size != st.size:
                raise Exception("\n\nstates must be distinct indices in [0, nsta).")
            sel = np.ascontiguousarray(st, dtype=np.int32)
        na = int(sel.size)
        if nq * max(nw, 1) * na * na > 2 ** 22:
            raise Exception("\n\nnq * max(nw, 1) * na^2 must be at most 2**22: split q_list or omega.")
        v, nvq = None, 0
        if interaction is None:
            if return_det:
                raise Exception("\n\nreturn_det=True needs an interaction.")
        else:
            try:
                v = np.array(interaction, dtype=complex)
            except (TypeError, ValueError):
                raise Exception("\n\ninteraction must be a complex (na, na) or (nq, na, na) array.")
            if v.shape not in ((na, na), (nq, na, na)):
                raise Exception("\n\ninteraction must have shape (na, na) or (nq, na, na).")
            if not np.all(np.isfinite(v)):
                raise Exception("\n\ninteraction must be finite.")
            v = np.ascontiguousarray(v.reshape(-1, na, na))
            nvq = v.shape[0]
        shape = (nq, na, na) if w is None else (nq, nw, na, na)
        chi0 = np.zeros(shape, dtype=complex)
        chi = np.zeros(shape, dtype=complex) if v is not None else None
        det = np.zeros(shape[:-2], dtype=complex) if return_det else None
        _lib.check(_lib.lib.tbk_susceptibility_matrix_mesh(
            self._device_model(), _lib.iptr(mesh), nq, _lib.dptr(q), nw, _lib.dptr(w), float(eta), float(fermi_level), float(kT), na,
            _lib.iptr(sel), None if v is None else _lib.dptr(v.view(float)), nvq, _lib.dptr(chi0.view(float)),
            None if chi is None else _lib.dptr(chi.view(float)), None if det is None else _lib.dptr(det.view(float))))
        out = (chi0,) if v is None else ((chi0, chi, det) if return_det else (chi0, chi))
        if single:
            out = tuple(x[0] for x in out)
        return out[0] if v is None else out

    # ------------------------------------------------------------------ occupied states: N, E, S, the Fermi level, the density matrix
    def _occ_args(self, what, mesh_size, kT):
        """(mesh, N_k, kT) of the occupied-state calls: dim_k 1, 2 or 3, the mesh of `_mesh_arg`, kT finite and >= 0."""
        if self._dim_k not in (1, 2, 3):
            raise Exception("\n\n%s needs a model with dim_k 1, 2 or 3." % what)
        mesh, nk = self._mesh_arg(mesh_size)
        try:
            kT = float(kT)
        except (TypeError, ValueError):
            raise Exception("\n\nkT must be finite and >= 0.")
        if not np.isfinite(kT) or not kT >= 0.0:
            raise Exception("\n\nkT must be finite and >= 0.")
        return mesh, nk, kT

    def thermodynamics_mesh(self, mesh_size, fermi_levels, kT=0.0):
        """Extension: the electron count, the band energy and the electronic entropy per cell as means over
        `k_uniform_mesh(mesh_size)` (1-, 2- or 3-D, generated on the device), for many Fermi levels at once: float `(3, nmu)`,

            N(mu) = (1 / N_k) sum_{k,n} f        E(mu) = (1 / N_k) sum f E_n        S(mu) = -(1 / N_k) sum [f ln f + (1 - f) ln(1 - f)]

        with E_n(k) the eigenvalues of `solve_all`, f = [E <= mu] for kT = 0, else the Fermi function.  No spin-degeneracy
        factor: a state counts once (a spinful model has 2 norb of them).  fermi_levels: 1-D, 1..8192 finite values in any
        order (repeats allowed; each gets its own value), or a scalar (the last axis is then dropped).  S in units of k_B; it
        is exactly 0 at kT = 0, where N is an integer count divided by N_k.  Eigenvalues only, kept on the device; fixed-order
        sums: two calls give the same bits."""
        mesh, nk, kT = self._occ_args("thermodynamics_mesh", mesh_size, kT)
        mu = np.array(fermi_levels, dtype=float)
        scalar = mu.ndim == 0
        if scalar:
            mu = mu.reshape(1)
        if mu.ndim != 1 or mu.size < 1 or mu.size > 8192:
            raise Exception("\n\nfermi_levels must be a scalar or a 1-D array of 1..8192 levels.")
        if not np.all(np.isfinite(mu)):
            raise Exception("\n\nfermi_levels must be finite.")
        mu = np.ascontiguousarray(mu)
        out = np.zeros((3, mu.size), dtype=float)
        _lib.check(_lib.lib.tbk_thermodynamics_mesh(self._device_model(), _lib.iptr(mesh), int(mu.size), _lib.dptr(mu), kT,
                                                    _lib.dptr(out)))
        return out[:, 0] if scalar else out

    def fermi_level_mesh(self, mesh_size, n_electrons, kT=0.0, return_edges=False):
        """Extension: the Fermi level that puts `n_electrons` electrons per cell into the levels of `k_uniform_mesh(mesh_size)`
        (no spin factor: a state holds one electron).  n_electrons: a scalar, or 1-D with 1..64 values (a doping scan); the
        result has the same shape.  The mesh is solved ONCE per call, whatever the number of fillings, and the selection runs
        on the device (a bisection on the integer key of a double: 64 passes over the resident levels, for all fillings at once).

        kT = 0: c = n_electrons * N_k must lie within 1e-6 of an integer in [1, nsta N_k - 1].  With all levels of the mesh
        sorted, e_0 <= e_1 <= ..., the result is mu = (e_{c-1} + e_c) / 2, from the device's own eigenvalues;
        return_edges=True returns (mu, edges) with edges `(2,)` or `(nfill, 2)` = (e_{c-1}, e_c): the band edges of an
        insulator.  EQUAL edges mean that the Fermi level cuts a group of degenerate levels (a metal whose Fermi surface passes
        through mesh points, e.g. the half-filled square lattice): `thermodynamics_mesh` at that mu then counts MORE than c,
        the whole group.  Nothing is hidden: compare the edges.

        kT > 0: any real 0 < n_electrons < nsta; the result is the first double at which the occupation sum reaches
        n_electrons, |N(mu) - n_electrons| <= 1e-12 nsta.  Inside a gap at kT much smaller than the gap, N(mu) is flat to
        rounding, and mu is only as determined as N is: any level of the plateau satisfies the bound, and which one is returned
        is decided by the last bits of the sum (the same ones every call).  return_edges needs kT = 0.

        Fixed-order sums: the result is reproducible bit for bit, and a filling gives the same bits alone and in a list."""
        mesh, nk, kT = self._occ_args("fermi_level_mesh", mesh_size, kT)
        nel = np.array(n_electrons, dtype=float)
        scalar = nel.ndim == 0
        if scalar:
            nel = nel.reshape(1)
        if nel.ndim != 1 or nel.size < 1 or nel.size > 64:
            raise Exception("\n\nn_electrons must be a scalar or a 1-D array of 1..64 values.")
        if not np.all(np.isfinite(nel)):
            raise Exception("\n\nn_electrons must be finite.")
        if return_edges and kT > 0.0:
            raise Exception("\n\nreturn_edges needs kT = 0: the levels on both sides of the Fermi level exist at kT = 0 only.")
        n = self._nsta
        if kT > 0.0:
            if not (np.all(nel > 0.0) and np.all(nel < n)):
                raise Exception("\n\nn_electrons must lie in the open interval (0, %d) at kT > 0." % n)
        else:
            c = nel * nk
            if np.any(np.abs(c - np.round(c)) > 1e-6):
                raise Exception("\n\nn_electrons times the %d mesh points must be an integer at kT = 0." % nk)
            if np.any(np.round(c) < 1) or np.any(np.round(c) > n * nk - 1):
                raise Exception("\n\nn_electrons must select between 1 and %d of the %d levels at kT = 0." % (n * nk - 1, n * nk))
        nel = np.ascontiguousarray(nel)
        mu = np.zeros(nel.size, dtype=float)
        edges = np.zeros((nel.size, 2), dtype=float) if return_edges else None
        _lib.check(_lib.lib.tbk_fermi_level_mesh(self._device_model(), _lib.iptr(mesh), int(nel.size), _lib.dptr(nel), kT,
                                                 _lib.dptr(mu), _lib.dptr(edges) if return_edges else None))
        res = float(mu[0]) if scalar else mu
        if return_edges:
            return res, (edges[0] if scalar else edges)
        return res

    def _R_list_arg(self, R_list):
        """(R, single) of the real-space calls: the checked lattice vectors as a contiguous int32 `(nR, dim_k)` array, 1 <= nR <=
        4096 and |R_a| < 2**30 (None: R = 0); single: it was None or one `(dim_k,)` vector."""
        dk = self._dim_k
        Rf = np.zeros(dk) if R_list is None else np.array(R_list)
        if Rf.dtype == object or not (np.issubdtype(Rf.dtype, np.integer) or np.issubdtype(Rf.dtype, np.floating)):
            raise Exception("\n\nR_list must hold integers.")
        single = Rf.ndim == 1
        if single:
            Rf = Rf.reshape(1, -1)
        if Rf.ndim != 2 or Rf.shape[1] != dk or Rf.shape[0] < 1 or Rf.shape[0] > 4096:
            raise Exception("\n\nR_list must have shape (nR, dim_k) with 1..4096 lattice vectors, or (dim_k,).")
        if not np.all(np.isfinite(Rf)) or np.any(Rf != np.round(Rf)):
            raise Exception("\n\nR_list must hold integers.")
        if np.any(np.abs(Rf) >= 2 ** 30):
            raise Exception("\n\nR_list: every component must be below 2**30 in magnitude.")
        return np.ascontiguousarray(Rf, dtype=np.int32), single

    def density_matrix_mesh(self, mesh_size, fermi_level, kT=0.0, R_list=None):
        """Extension: the one-particle density matrix in real space, as a mean over `k_uniform_mesh(mesh_size)` (1-, 2- or 3-D,
        generated on the device): complex `(nR, nsta, nsta)`,

            P(k)    = sum_n f(E_n(k)) u_n(k) u_n(k)^+
            D_ij(R) = (1 / N_k) sum_k P_ij(k) e^{-2 pi i k.(R + tau_j - tau_i)} = <i,0| rho |j,R> = <c+_{j,R} c_{i,0}>

        with the eigenpairs of `solve_all` and f as in `thermodynamics_mesh` (no spin factor).  Index layout and phase
        convention are those of `set_hop(amp, i, j, R)`: D is the thermal average of the operator whose hopping table is t, so
        D_ii(0) is the occupation of state i, sum_i D_ii(0) = N(mu), D_ji(-R) = conj D_ij(R), and the band energy is
        E(mu) = Re sum conj(t_ij(R)) D_ij(R) over the whole table (both directions of every hop, on-site terms at R = 0, spin
        blocks included).  For an insulator at kT = 0, D is the projector onto the occupied bands on the torus of the mesh.

        R_list: `(nR, dim_k)` integers with |R_a| < 2**30, 1 <= nR <= 4096 and nR * nsta**2 <= 2**22; `(dim_k,)` alone drops
        the leading axis; None is R = 0 (`(nsta, nsta)`).  Spinful models return `(nR, norb, 2, norb, 2)`, as `_gen_ham`
        does.  The phase e^{-2 pi i k.R} is formed from exact integers: an R equal to a period of the mesh gives D(0) bit for
        bit (the mesh cannot tell them apart).  The eigenvectors never leave the device.  At kT = 0 a Fermi level within
        rounding of an eigenvalue makes that state's occupation depend on the last bits; take `fermi_level_mesh`'s midpoint.
        Fixed-order sums: two calls give the same bits, and an R gives the same bits alone and inside a longer list."""
        mesh, nk, kT = self._occ_args("density_matrix_mesh", mesh_size, kT)
        try:
            fermi_level = float(fermi_level)
        except (TypeError, ValueError):
            raise Exception("\n\nfermi_level must be one finite number.")
        if not np.isfinite(fermi_level):
            raise Exception("\n\nfermi_level must be finite.")
        n = self._nsta
        R, single = self._R_list_arg(R_list)
        nR = R.shape[0]
        if nR * n * n > 2 ** 22:
            raise Exception("\n\nnR * nsta**2 must be at most 2**22: split R_list.")
        out = np.zeros((nR, n, n), dtype=complex)
        _lib.check(_lib.lib.tbk_density_matrix_mesh(self._device_model(), _lib.iptr(mesh), fermi_level, kT, nR, _lib.iptr(R),
                                                    _lib.dptr(out.view(float))))
        if self._nspin == 2:
            out = out.reshape(nR, self._norb, 2, self._norb, 2)
        return out[0] if single else out

    # ------------------------------------------------------------------ self-consistent Hartree-Fock (extension)
    def _mf_entries(self, what, interaction, U):
        """The state-indexed interaction of `mean_field_mesh`, for the call `what`: (ab (nint, 2) int32, R (nint, dim_k) int32,
        V (nint,) float).  Orbital entries act on total densities (all four spin pairs on a spinful model); U adds
        (o up, o down, R = 0)."""
        ns, no, dk = self._nspin, self._norb, self._dim_k
        ab, Rs, Vs = [], [], []
        if interaction is None and U is None:
            raise Exception("\n\n%s needs an interaction list, U, or both." % what)
        for ent in (interaction if interaction is not None else []):
            try:
                V, i, j, R = ent
                V = float(V)
            except (TypeError, ValueError):
                raise Exception("\n\ninteraction must be a list of (V, i, j, R) with real V.")
            if not np.isfinite(V):
                raise Exception("\n\ninteraction: V must be finite.")
            if not (_is_int(i) and _is_int(j)) or i < 0 or i >= no or j < 0 or j >= no:
                raise Exception("\n\ninteraction: orbital index out of scope.")
            Rf = np.array(R)
            if Rf.shape != (self._dim_r,) or Rf.dtype == object or np.any(Rf != np.round(Rf)):
                raise Exception("\n\ninteraction: R must hold dim_r integers, as in set_hop.")
            Rp = np.array(Rf, dtype=np.int64)[self._per]
            if np.any(np.abs(Rp) >= 2 ** 30):
                raise Exception("\n\ninteraction: every component of R must be below 2**30 in magnitude.")
            if i == j and not np.any(Rp):
                if ns == 2:
                    raise Exception("\n\ninteraction: (i, i, R = 0) on a spinful model: that is U.")
                raise Exception("\n\ninteraction: (i, i, R = 0) is a self-interaction.")
            for s in range(ns):
                for t in range(ns):
                    ab.append((i * ns + s, j * ns + t))
                    Rs.append(Rp)
                    Vs.append(V)
        if U is not None:
            if ns != 2:
                raise Exception("\n\nU needs a spinful model (nspin = 2).")
            Uv = np.array(U, dtype=float)
            if Uv.ndim == 0:
                Uv = np.full(no, float(Uv))
            if Uv.shape != (no,) or not np.all(np.isfinite(Uv)):
                raise Exception("\n\nU must be a finite scalar or one value per orbital.")
            for o in range(no):
                ab.append((2 * o, 2 * o + 1))
                Rs.append(np.zeros(dk, dtype=np.int64))
                Vs.append(float(Uv[o]))
        if not ab:
            raise Exception("\n\n%s needs an interaction list, U, or both." % what)
        seen = set()
        for (a, b), R in zip(ab, Rs):
            k1, k2 = (a, b) + tuple(int(x) for x in R), (b, a) + tuple(int(-x) for x in R)
            if k1 in seen or k2 in seen:
                raise Exception("\n\ninteraction: a bond is given once and means the symmetric pair; one was given twice.")
            seen.add(k1)
        return (np.ascontiguousarray(ab, dtype=np.int32), np.ascontiguousarray(np.array(Rs).reshape(len(ab), dk), dtype=np.int32),
                np.ascontiguousarray(Vs, dtype=float))

    def _scf_args(self, what, nsta_max, n_electrons, fermi_level, filling_rule, history, max_iter, check_every, mixing, tol):
        """The argument checks `mean_field_mesh` and `bdg_mesh` share: (filling, mixing, tol) as floats.  The rule that ties
        n_electrons to the mesh is the caller's: filling_rule(filling) raises where it is broken, and is asked where it always
        was, behind the checks of the filling itself and before those of the loop."""
        if self._nsta > nsta_max:
            raise Exception("\n\n%s: at most %d states." % (what, nsta_max))
        if (n_electrons is None) == (fermi_level is None):
            raise Exception("\n\n%s needs exactly one of n_electrons and fermi_level." % what)
        try:
            filling = float(n_electrons if n_electrons is not None else fermi_level)
        except (TypeError, ValueError):
            raise Exception("\n\nn_electrons / fermi_level must be one finite number.")
        if not np.isfinite(filling):
            raise Exception("\n\nn_electrons / fermi_level must be finite.")
        if n_electrons is not None:
            filling_rule(filling)
        if not _is_int(history) or history < 0 or history > 8:
            raise Exception("\n\nhistory must be an integer in 0..8.")
        if not _is_int(max_iter) or max_iter < 1 or max_iter > 65536:
            raise Exception("\n\nmax_iter must be an integer in 1..65536.")
        if not _is_int(check_every) or check_every < 1:
            raise Exception("\n\ncheck_every must be an integer >= 1.")
        mixing, tol = float(mixing), float(tol)
        if not 0.0 < mixing <= 1.0:
            raise Exception("\n\nmixing must satisfy 0 < mixing <= 1.")
        if not (np.isfinite(tol) and tol >= 0.0):
            raise Exception("\n\ntol must be finite and >= 0.")
        return filling, mixing, tol

    def _mf_layout(self, what, ab, Rs):
        """The layout of the parameters as include/tbk.h has it: (touched states ascending, state -> parameter of its occupation,
        their number, the distinct lattice vectors: R = 0 first, then in order of first appearance; at most 4096)."""
        touched = sorted(set(ab.reshape(-1).tolist()))
        occ_par = {a: p for p, a in enumerate(touched)}
        Rl = [tuple([0] * self._dim_k)]
        for R in Rs:
            if tuple(int(x) for x in R) not in Rl:
                Rl.append(tuple(int(x) for x in R))
        if len(Rl) > 4096:
            raise Exception("\n\n%s: at most 4096 distinct lattice vectors." % what)
        return touched, occ_par, len(touched), Rl

    @staticmethod
    def _mf_table_args(tables, mesh, ab, Rs, Vs):
        """The arguments tbk_mean_field_mesh and tbk_bdg_mesh take from orb to int_V: the flattened tables of the bare model, the mesh
        and the state-indexed interaction."""
        orb_per, onsite, hop_i, hop_j, hop_R, hop_amp = tables
        return (_lib.dptr(orb_per), _lib.dptr(onsite.view(float)), len(hop_i), _lib.iptr(hop_i), _lib.iptr(hop_j),
                _lib.iptr(hop_R.reshape(-1)) if hop_R.size else None, _lib.dptr(hop_amp.view(float)) if hop_amp.size else None,
                _lib.iptr(mesh), len(Vs), _lib.iptr(ab.reshape(-1)), _lib.iptr(Rs.reshape(-1)), _lib.dptr(Vs))

    def _scf_result(self, what, res, info, nR, res_hist, occ_hist, x_in, x_out, key):
        """The fields every self-consistent result carries: residuals, history, iterations, converged, field, _x, _key."""
        if int(info[2]) != nR or int(info[3]) != len(x_in):
            raise Exception("\n\n%s: the library laid out %d lattice vectors and %d parameters, not %d and %d."
                            % (what, info[2], info[3], nR, len(x_in)))
        its, ns, no, n = int(info[0]), self._nspin, self._norb, self._nsta
        res.residuals = res_hist[:its].copy()
        res.history = occ_hist[:its].reshape((its, no, 2) if ns == 2 else (its, n)).copy()
        res.iterations, res.converged = its, bool(info[1])
        res.field, res._x, res._key = x_out, x_in, key
        return its

    def mean_field_mesh(self, mesh_size, interaction=None, n_electrons=None, fermi_level=None, kT=0.0, U=None, start=None, fock=True,
                        mixing=0.5, history=4, tol=1e-10, max_iter=200, check_every=1):
        """Extension: unrestricted Hartree-Fock for a density-density interaction, iterated to self-consistency on
        `k_uniform_mesh(mesh_size)` with the whole loop on the device.

            H_int = 1/2 sum_{a,b,R} V_ab(R) n_{a,0} n_{b,R}        (a, b states; V_ab(R) = V_ba(-R) real, V_aa(0) = 0)

        With D_ij(R) = <c+_{j,R} c_{i,0}> of `density_matrix_mesh`: the on-site energy of state a gets sum_{b,R} V_ab(R) n_b
        (Hartree) and, with fock=True, the entry (a, b, R) of the hopping table gets -V_ab(R) D_ab(R), its mirror the conjugate
        (on the Hubbard pair this is the spin-flip element of the on-site block).  interaction: a list of (V, i, j, R) in
        orbital indices and full-dimension R as in `set_hop`, a bond given once; on a spinful model it couples the total
        densities.  U: scalar or one value per orbital, U n_up n_down (nspin = 2).  Exactly one of n_electrons (the rules of
        `fermi_level_mesh`) and fermi_level.  start: None (the field of the non-interacting model at the same filling), an
        array of occupations `(nsta,)` / `(norb, 2)`, the on-site spin densities `(norb, 2, 2)`, or an earlier result (restart).
        mixing 0 < alpha <= 1; history 0: x <- x + alpha r; history m in 1..8: Anderson mixing over the last m (x, r) pairs after
        m linear steps.  tol on max |r| (0: exactly max_iter iterations); the host looks at the residual every check_every
        iterations and at nothing else.

        Returns a `mean_field_result`: model (a copy of this model with the field of the last iteration added; this model is
        not edited), fermi_level, occupations `(norb,)` / `(norb, 2)`, spin_density `(norb, 2, 2)` on spinful models,
        density `(nR, nsta, nsta)` with R_list `(nR, dim_k)`, energy = <H_0> + <H_int> per cell in the Hartree-Fock state,
        entropy, free_energy, residuals (one per iteration), history (the occupations after every iteration), iterations,
        converged (False is not an exception).  `density` is D of the last iteration, i.e. of `model` at `fermi_level`.
        Fixed-order sums: two calls give the same bits, and max_iter = k gives the first k history rows of a longer run."""
        mesh, nk, kT = self._occ_args("mean_field_mesh", mesh_size, kT)
        ns, no, dk, n = self._nspin, self._norb, self._dim_k, self._nsta
        def filling_rule(filling):
            if kT > 0.0:
                if not 0.0 < filling < n:
                    raise Exception("\n\nn_electrons must lie in the open interval (0, %d) at kT > 0." % n)
            else:
                c = filling * nk
                if abs(c - round(c)) > 1e-6:
                    raise Exception("\n\nn_electrons times the %d mesh points must be an integer at kT = 0." % nk)
                if round(c) < 1 or round(c) > n * nk - 1:
                    raise Exception("\n\nn_electrons must select between 1 and %d of the %d levels at kT = 0." % (n * nk - 1, n * nk))

        filling, mixing, tol = self._scf_args("mean_field_mesh", 2048, n_electrons, fermi_level, filling_rule, history, max_iter,
                                              check_every, mixing, tol)
        ab, Rs, Vs = self._mf_entries("mean_field_mesh", interaction, U)
        nint = len(Vs)
        fock = bool(fock)
        touched, occ_par, nocc, Rl = self._mf_layout("mean_field_mesh", ab, Rs)
        npar = nocc + (2 * nint if fock else 0)
        nR = len(Rl)
        if nR * n * n > 2 ** 22:
            raise Exception("\n\nmean_field_mesh: nR * nsta**2 must be at most 2**22.")
        if npar > 2 ** 20:
            raise Exception("\n\nmean_field_mesh: at most 2**20 mean-field parameters.")
        key = (ab.tobytes(), Rs.tobytes(), Vs.tobytes(), fock, n)
        x0 = None
        if isinstance(start, mean_field_result):
            if start._key != key:
                raise Exception("\n\nstart: the result belongs to another model size, interaction or fock setting.")
            x0 = np.array(start._x, dtype=float)
        elif start is not None:
            st = np.array(start, dtype=complex)
            x0 = np.zeros(npar)
            if ns == 2 and st.shape == (no, 2, 2):
                occ = np.real(np.einsum("oss->os", st)).reshape(n)
                if fock:
                    for e in range(nint):
                        a, b = int(ab[e, 0]), int(ab[e, 1])
                        if a // 2 == b // 2 and not np.any(Rs[e]):
                            x0[nocc + 2 * e] = st[a // 2, a % 2, b % 2].real
                            x0[nocc + 2 * e + 1] = st[a // 2, a % 2, b % 2].imag
            elif st.size == n and st.shape in ((n,), (no, ns)):
                occ = np.real(st).reshape(n)
            else:
                raise Exception("\n\nstart must be None, occupations of shape (nsta,) or (norb, nspin), spin densities (norb, 2, 2), "
                                "or an earlier result.")
            for a in touched:
                x0[occ_par[a]] = occ[a]
        if x0 is not None and not np.all(np.isfinite(x0)):
            raise Exception("\n\nstart must be finite.")
        ctx = _lib.default_context()
        x_in, x_out, mu = np.zeros(npar), np.zeros(npar), np.zeros(1)
        dens = np.zeros((nR, n, n), dtype=complex)
        R_out = np.zeros((nR, dk), dtype=np.int32)
        energies = np.zeros(5)
        res_hist, occ_hist = np.zeros(max_iter), np.zeros((max_iter, n))
        info = np.zeros(5, dtype=np.int32)
        _lib.check(_lib.lib.tbk_mean_field_mesh(
            ctx.handle, dk, no, ns, *self._mf_table_args(self._flat_tables(), mesh, ab, Rs, Vs), int(fock),
            int(n_electrons is not None), filling, kT, 0 if x0 is None else 1, None if x0 is None else _lib.dptr(x0), mixing,
            int(history), tol, int(max_iter), int(check_every), _lib.dptr(x_in), _lib.dptr(x_out), _lib.dptr(mu),
            _lib.dptr(dens.view(float)), _lib.iptr(R_out.reshape(-1)), _lib.dptr(energies), _lib.dptr(res_hist), _lib.dptr(occ_hist),
            _lib.iptr(info)))
        res = mean_field_result()
        self._scf_result("mean_field_mesh", res, info, nR, res_hist, occ_hist, x_in, x_out, key)
        res.model = self._mf_model(ab, Rs, Vs, fock, occ_par, nocc, x_in)
        res.fermi_level = float(mu[0])
        d0 = dens[0]
        occ = np.real(np.diagonal(d0)).copy()
        res.occupations = occ.reshape(no, 2) if ns == 2 else occ
        res.spin_density = np.array([d0[2 * o:2 * o + 2, 2 * o:2 * o + 2] for o in range(no)]) if ns == 2 else None
        res.density, res.R_list = dens, R_out
        res.energy, res.entropy, res.free_energy = float(energies[0]), float(energies[1]), float(energies[2])
        res.band_energy, res.n_electrons = float(energies[3]), float(energies[4])
        res.resident = bool(info[4])
        return res

    def _mf_model(self, ab, Rs, Vs, fock, occ_par, nocc, x):
        """A copy of this model with the mean field of the parameter vector x added through set_onsite / set_hop(mode="add")."""
        ns, no, dk = self._nspin, self._norb, self._dim_k
        m = copy.deepcopy(self)
        site = np.zeros((no, ns, ns), dtype=complex)
        hops = {}
        for e in range(len(Vs)):
            a, b, V = int(ab[e, 0]), int(ab[e, 1]), float(Vs[e])
            site[a // ns, a % ns, a % ns] += V * x[occ_par[b]]
            site[b // ns, b % ns, b % ns] += V * x[occ_par[a]]
            if not fock:
                continue
            amp = -V * (x[nocc + 2 * e] + 1j * x[nocc + 2 * e + 1])
            if a // ns == b // ns and not np.any(Rs[e]):           # the on-site spin-flip element
                site[a // ns, a % ns, b % ns] += amp
                site[a // ns, b % ns, a % ns] += np.conj(amp)
                continue
            blk = hops.setdefault((a // ns, b // ns) + tuple(int(r) for r in Rs[e]), np.zeros((ns, ns), dtype=complex))
            blk[a % ns, b % ns] += amp
        for o in range(no):
            if np.any(site[o]):
                m.set_onsite(site[o] if ns == 2 else float(site[o, 0, 0].real), o, mode="add")
        for (i, j, *R), blk in hops.items():
            Rf = np.zeros(self._dim_r, dtype=int)
            Rf[self._per] = R
            m.set_hop(blk if ns == 2 else complex(blk[0, 0]), i, j, Rf, mode="add", allow_conjugate_pair=True)
        return m

    # ------------------------------------------------------------------ excitons: Tamm-Dancoff BSE (extension)
    def _exciton_args(self, what, mesh_size, interaction, U, fermi_level, valence, conduction):
        """The checked arguments the three exciton calls share: (mesh, N_k, ab, Rs, Vs, mu, (nv, vsel), (nc, csel))."""
        mesh, nk, _ = self._occ_args(what, mesh_size, 0.0)
        if self._nsta > 2048:
            raise Exception("\n\n%s: at most 2048 states." % what)
        try:
            mu = float(fermi_level)
        except (TypeError, ValueError):
            raise Exception("\n\nfermi_level must be one finite number.")
        if not np.isfinite(mu):
            raise Exception("\n\nfermi_level must be finite.")
        ab, Rs, Vs = self._mf_entries(what, interaction, U)
        sel = []
        for name, arg, kind in (("valence", valence, "occupied"), ("conduction", conduction, "empty")):
            if arg is None:
                sel.append((0, None))
            elif _is_int(arg):
                if arg < 1:
                    raise Exception("\n\n%s: no %s band selected." % (name, kind))
                if arg > 16:
                    raise Exception("\n\n%s: at most 16 bands." % name)
                sel.append((int(arg), None))
            else:
                idx = list(arg)
                if len(idx) < 1:
                    raise Exception("\n\n%s: no %s band selected." % (name, kind))
                if len(idx) > 16:
                    raise Exception("\n\n%s: at most 16 bands." % name)
                if not all(_is_int(b) for b in idx) or min(idx) < 0 or max(idx) >= self._nsta or len(set(idx)) != len(idx):
                    raise Exception("\n\n%s must be an integer or a list of distinct band indices." % name)
                sel.append((len(idx), np.ascontiguousarray(sorted(idx), dtype=np.int32)))
        return mesh, nk, ab, Rs, Vs, mu, sel[0], sel[1]

    def exciton_apply_mesh(self, mesh_size, interaction=None, U=None, fermi_level=0.0, valence=None, conduction=None, direct=True,
                           exchange=True, vectors=None):
        """Extension: the exciton Hamiltonian of the Tamm-Dancoff Bethe-Salpeter equation applied to vectors, without forming its
        matrix.  The bands are this model's (`mean_field_mesh(...).model` for time-dependent Hartree-Fock; a bare model treats
        its bands as quasi-particle energies and `interaction` as the screened interaction), an insulator at kT = 0: the same
        number of levels at or below `fermi_level` at every point of `k_uniform_mesh(mesh_size)`.  interaction and U are those of
        `mean_field_mesh`.  With transitions t = (k, v, c), Delta_t = E_c(k) - E_v(k), E both directions (a, b, R) of every bond,
        d_e = R + tau_b - tau_a and N = N_k:

            H_ex = Delta + K^x - K^d
            K^d_tt' = (1/N) sum_e V_e e^{2 pi i (k-k').d_e} conj(u_ck[a]) u_c'k'[a] u_vk[b] conj(u_v'k'[b])   (direct, from Fock)
            K^x_tt' = (1/N) sum_e V_e conj(u_ck[a]) u_vk[a] conj(u_v'k'[b]) u_c'k'[b]                        (exchange, from Hartree)

        direct=False / exchange=False drops a term (the response of a fock=False mean field is direct=False).  States are
        spin-orbitals; no spin-degeneracy factor.  valence / conduction: an int m (the top m occupied / bottom m empty bands), a
        list of band indices, or None (all); at most 16 each.  vectors: `(nb, *mesh, nv, nc)` with nb in 1..16, or
        `(*mesh, nv, nc)`, in the gauge of the eigenvectors `solve_all` returns.  Returns (H_ex X in the shape of vectors, gaps
        `(*mesh, nv, nc)`).  One application is two sweeps over the selected eigenvectors, O(N_k) work.  Two calls give the same
        bits, and a vector gives the same bits alone and inside any block.  Not covered: finite-momentum excitons (q != 0), the
        non-TDA matrix, separate screened and bare interactions, kT > 0 and metals, several GPUs."""
        what = "exciton_apply_mesh"
        mesh, nk, ab, Rs, Vs, mu, (nv, vsel), (nc, csel) = self._exciton_args(what, mesh_size, interaction, U, fermi_level, valence,
                                                                             conduction)
        if vectors is None:
            raise Exception("\n\nexciton_apply_mesh needs vectors of shape (nb, *mesh, nv, nc) or (*mesh, nv, nc).")
        x = np.array(vectors, dtype=complex)
        dk, ms = self._dim_k, tuple(int(v) for v in mesh)
        single = x.ndim == dk + 2
        if single:
            x = x[None]
        if x.ndim != dk + 3 or x.shape[1:dk + 1] != ms or not 1 <= x.shape[0] <= 16 or x.shape[-1] < 1 or x.shape[-2] < 1:
            raise Exception("\n\nvectors must have shape (nb, *mesh, nv, nc) with nb in 1..16, or (*mesh, nv, nc).")
        if not np.all(np.isfinite(x)):
            raise Exception("\n\nvectors must be finite.")
        x = np.ascontiguousarray(x)
        out = np.zeros_like(x)
        gaps = np.zeros(x.shape[1:])
        info = np.zeros(3, dtype=np.int32)
        _lib.check(_lib.lib.tbk_exciton_apply_mesh(
            self._device_model(), _lib.iptr(mesh), len(Vs), _lib.iptr(ab.reshape(-1)), _lib.iptr(Rs.reshape(-1)), _lib.dptr(Vs), mu, nv,
            _lib.iptr(vsel), nc, _lib.iptr(csel), int(bool(direct)), int(bool(exchange)), x.shape[0], x.shape[-2], x.shape[-1],
            _lib.dptr(x.view(float)), _lib.dptr(out.view(float)), _lib.dptr(gaps), _lib.iptr(info)))
        return (out[0] if single else out), gaps

    def exciton_states_mesh(self, mesh_size, interaction=None, U=None, fermi_level=0.0, valence=None, conduction=None, direct=True,
                            exchange=True, return_vectors=False):
        """Extension: the exciton states of `exciton_apply_mesh`'s H_ex by the dense path, for N_t = N_k nv nc <= 2048: H_ex is
        formed by applying the operator to unit vectors in blocks of 16 and diagonalised on the device.  Returns an
        `exciton_result`: energies (ascending), dipoles d^a_lambda = <A^lambda|D^a> with D^a_t = <u_ck|dH/dk_a|u_vk> / Delta_t
        (`_gen_dham`'s derivative, the length gauge), gap, binding = gap - energies[0], dipole_norm S_ab = (1/N) <D^a|D^b>, and with
        return_vectors the eigenvectors `(N_t, *mesh, nv, nc)`; its `polarizability(omega, eta, dirs)` sums
        chi_ab(w) = (1/N) sum_lambda conj(d^a) d^b / (Omega - w - i eta).  The resonant conductivity is -i w chi.  Not covered:
        finite-momentum excitons, the non-TDA matrix, a Cartesian tensor, kT > 0 and metals; low-lying states beyond the dense
        limit (the Lanczos coefficients of `exciton_spectrum_mesh` give Ritz values)."""
        what = "exciton_states_mesh"
        mesh, nk, ab, Rs, Vs, mu, (nv, vsel), (nc, csel) = self._exciton_args(what, mesh_size, interaction, U, fermi_level, valence,
                                                                             conduction)
        dk = self._dim_k
        if nk > 2048:
            raise Exception("\n\nexciton_states_mesh: at most 2048 transitions on the dense path; use exciton_spectrum_mesh.")
        cap = min(2048, nk * min(16, self._nsta) ** 2)               # room for N_t, whatever the selection resolves to
        energies, dip = np.zeros(cap), np.zeros((cap, dk), dtype=complex)
        sab, scal, info = np.zeros((dk, dk), dtype=complex), np.zeros(2), np.zeros(3, dtype=np.int32)
        vec = np.zeros(cap * cap, dtype=complex) if return_vectors else None
        _lib.check(_lib.lib.tbk_exciton_states_mesh(
            self._device_model(), _lib.iptr(mesh), len(Vs), _lib.iptr(ab.reshape(-1)), _lib.iptr(Rs.reshape(-1)), _lib.dptr(Vs), mu, nv,
            _lib.iptr(vsel), nc, _lib.iptr(csel), int(bool(direct)), int(bool(exchange)), cap, _lib.dptr(energies),
            _lib.dptr(dip.view(float)), _lib.dptr(sab.view(float)), None if vec is None else _lib.dptr(vec.view(float)),
            _lib.dptr(scal), _lib.iptr(info)))
        nocc, nv, nc = int(info[0]), int(info[1]), int(info[2])
        nt = nk * nv * nc
        res = exciton_result()
        res.energies, res.dipoles = energies[:nt].copy(), dip[:nt].copy()
        res.gap, res.binding, res.dipole_norm = float(scal[0]), float(scal[0] - energies[0]), sab
        res.n_occ, res.mesh, res._nk = nocc, mesh.copy(), nk
        res.valence = [int(b) for b in vsel] if vsel is not None else list(range(nocc - nv, nocc))
        res.conduction = [int(b) for b in csel] if csel is not None else list(range(nocc, nocc + nc))
        res.vectors = vec[:nt * nt].reshape((nt,) + tuple(int(v) for v in mesh) + (nv, nc)).copy() if return_vectors else None
        return res

    def exciton_spectrum_mesh(self, mesh_size, interaction=None, U=None, fermi_level=0.0, valence=None, conduction=None, direct=True,
                              exchange=True, omega=None, eta=None, dirs=None, n_steps=256, return_coefficients=False):
        """Extension: the polarizability chi_ab(w) = (1/N) <D^a| (H_ex - w - i eta)^-1 |D^b> of `exciton_apply_mesh`'s H_ex by the
        Haydock recursion, for up to 2**24 transitions (the selected eigenvectors stay on the device: N_k nsta (nv + nc) <= 2**26).
        Diagonal components are Lanczos runs started from D^a; an off-diagonal pair adds the runs from D^a + D^b and D^a + i D^b,
        dim_k**2 runs for the tensor, all carried as one block through the same applications with the whole loop on the
        device.  A run whose beta falls below 1e-10 of the largest |alpha| so far (at least the largest transition energy) has
        exhausted its invariant subspace and ends there (n_used); it is not restarted.  The continued fraction is evaluated on the
        host: `exciton_reconstruct(coefficients, omega, eta)` gives another frequency list for nothing.  omega, eta by the rules of
        `optical_conductivity_mesh`; dirs=None -> `(nw, dim_k, dim_k)`, dirs=(a, b) -> `(nw,)`, bitwise the tensor's entry.
        Returns an `exciton_spectrum` with chi, dipole_norm, gap, n_used and, on request, coefficients.  Two calls give the same
        bits; n_steps = k gives the first k coefficients of a longer run.  Not covered: finite-momentum excitons, the non-TDA
        matrix, a Cartesian tensor, kT > 0 and metals, several GPUs; eigenpairs come from the coefficients (Ritz values)."""
        what = "exciton_spectrum_mesh"
        mesh, nk, ab, Rs, Vs, mu, (nv, vsel), (nc, csel) = self._exciton_args(what, mesh_size, interaction, U, fermi_level, valence,
                                                                             conduction)
        if omega is None or eta is None:
            raise Exception("\n\nexciton_spectrum_mesh needs omega and eta.")
        w = _sweep_args(omega, eta, 0.0, 0.0)
        dk = self._dim_k
        da, db = (-1, -1) if dirs is None else _exciton_dirs(dirs, dk)
        if not _is_int(n_steps) or n_steps < 1 or n_steps > 65536:
            raise Exception("\n\nn_steps must be an integer in 1..65536.")
        if da < 0:
            runs = [(a, a, 0) for a in range(dk)] + [(a, b, kind) for a in range(dk) for b in range(a + 1, dk) for kind in (1, 2)]
        elif da == db:
            runs = [(da, da, 0)]
        else:
            runs = [(da, da, 0), (db, db, 0), (da, db, 1), (da, db, 2)]
        nr = len(runs)
        alpha, beta = np.zeros((nr, n_steps)), np.zeros((nr, n_steps))
        norm2, n_used = np.zeros(nr), np.zeros(nr, dtype=np.int32)
        sab, scal, info = np.zeros((dk, dk), dtype=complex), np.zeros(2), np.zeros(3, dtype=np.int32)
        _lib.check(_lib.lib.tbk_exciton_spectrum_mesh(
            self._device_model(), _lib.iptr(mesh), len(Vs), _lib.iptr(ab.reshape(-1)), _lib.iptr(Rs.reshape(-1)), _lib.dptr(Vs), mu, nv,
            _lib.iptr(vsel), nc, _lib.iptr(csel), int(bool(direct)), int(bool(exchange)), da, db, int(n_steps), _lib.dptr(alpha),
            _lib.dptr(beta), _lib.dptr(norm2), _lib.iptr(n_used), _lib.dptr(sab.view(float)), _lib.dptr(scal), _lib.iptr(info)))
        co = exciton_coefficients()
        co.alpha, co.beta, co.norm2, co.n_used, co.runs = alpha, beta, norm2, n_used, runs
        co.dim_k, co.dirs, co.n_k = dk, (None if da < 0 else (da, db)), nk
        res = exciton_spectrum()
        res.chi = exciton_reconstruct(co, w, eta)
        res.dipole_norm, res.gap, res.n_used = sab, float(scal[0]), n_used.copy()
        res.coefficients = co if return_coefficients else None
        return res

    # ------------------------------------------------------------------ Bogoliubov-de Gennes superconductivity (extension)
    def _state_table(self):
        """The state-level table {(a, b, R over the periodic directions): t_ab(R)}: on-site blocks at R = 0 and both directions of
        every hop (a = orbital * nspin + spin)."""
        ns, dk = self._nspin, self._dim_k
        tab = {}
        zero = (0,) * dk
        for o in range(self._norb):
            blk = np.array(self._site_energies[o], dtype=complex).reshape(ns, ns)
            for s in range(ns):
                for t in range(ns):
                    if blk[s, t] != 0.0:
                        tab[(o * ns + s, o * ns + t) + zero] = tab.get((o * ns + s, o * ns + t) + zero, 0.0) + complex(blk[s, t])
        for hop in self._hoppings:
            blk = np.array(hop[0], dtype=complex).reshape(ns, ns)
            R = tuple(int(x) for x in np.array(hop[3], dtype=int)[self._per]) if dk > 0 else ()
            mR = tuple(-x for x in R)
            for s in range(ns):
                for t in range(ns):
                    a, b = hop[1] * ns + s, hop[2] * ns + t
                    tab[(a, b) + R] = tab.get((a, b) + R, 0.0) + complex(blk[s, t])
                    tab[(b, a) + mR] = tab.get((b, a) + mR, 0.0) + complex(np.conj(blk[s, t]))
        return tab

    def _pairing_arg(self, pairing):
        """The checked pairing list of `nambu_model`: [(Delta, a, b, R over the periodic directions)]."""
        n, dk = self._nsta, self._dim_k
        out, seen = [], set()
        for ent in (pairing if pairing is not None else []):
            try:
                D, a, b, R = ent
                D = complex(D)
            except (TypeError, ValueError):
                raise Exception("\n\npairing must be a list of (Delta, a, b, R) with complex Delta.")
            if not (np.isfinite(D.real) and np.isfinite(D.imag)):
                raise Exception("\n\npairing: Delta must be finite.")
            if not (_is_int(a) and _is_int(b)) or a < 0 or a >= n or b < 0 or b >= n:
                raise Exception("\n\npairing: state index out of scope.")
            Rf = np.array(R)
            if Rf.shape != (self._dim_r,) or Rf.dtype == object or np.any(Rf != np.round(Rf)):
                raise Exception("\n\npairing: R must hold dim_r integers, as in set_hop.")
            Rp = tuple(int(x) for x in np.array(Rf, dtype=np.int64)[self._per]) if dk > 0 else ()
            if any(abs(x) >= 2 ** 30 for x in Rp):
                raise Exception("\n\npairing: every component of R must be below 2**30 in magnitude.")
            if a == b and not any(Rp):
                raise Exception("\n\npairing: (a, a, R = 0) vanishes by antisymmetry.")
            k1, k2 = (int(a), int(b)) + Rp, (int(b), int(a)) + tuple(-x for x in Rp)
            if k1 in seen or k2 in seen:
                raise Exception("\n\npairing: an entry is given once and means the antisymmetric pair; one was given twice.")
            seen.add(k1)
            out.append((D, int(a), int(b), Rp))
        return out

    def nambu_model(self, fermi_level, pairing=None):
        """Extension: the Bogoliubov-de Gennes (Nambu) model of this model, a new spinless `tb_model` with 2 nsta orbitals; this
        model is not edited.  With Psi_k = (c_k, c+_{-k}) and H = 1/2 sum_k Psi+_k H_BdG(k) Psi_k + const,

            H_BdG(k) = [[h(k) - mu, Delta(k)], [Delta(k)+, -h(-k)^T + mu]]

        Particle orbital a is state a of this model (orbital * nspin + spin, the index of `density_matrix_mesh`) at that
        orbital's position, hole orbital nsta + a sits at the same position.  With t_ab(R) the state-level hopping table: the
        particle block is t with fermi_level subtracted on the diagonal; the hole block is the hop (a -> b, R) with amplitude
        -conj(t_ab(R)) and the on-site energy -eps_a + fermi_level, which is -h(-k)^T with the orbital positions in the phases,
        inversion symmetry or not.  pairing: a list of (Delta, a, b, R) -- complex Delta, state indices, full-dimension R as
        in `set_hop` -- each meaning Delta c+_{a,0} c+_{b,R} + h.c.: the hop (a -> nsta + b, R) with amplitude Delta and its
        antisymmetric mirror (b -> nsta + a, -R) with -Delta.  An entry and its mirror given twice is refused, and so is
        (a, a, R = 0), which vanishes.  nsta <= 1024.

        The density matrix of the result at Fermi level 0 holds every expectation value: n_a = D_aa(0), <c+_{b,R} c_{a,0}> =
        D_ab(R), F_ab(R) = <c_{b,R} c_{a,0}> = D_{a,nsta+b}(R), and the hole block is delta - conj(D_ab(R)).  Every call that
        takes a `tb_model` takes it: `berry_phase` of a topological superconductor, `cut_piece` for Majorana end states, the
        quasi-particle DOS."""
        n, dk = self._nsta, self._dim_k
        if n > 1024:
            raise Exception("\n\nnambu_model: at most 1024 states.")
        try:
            mu = float(fermi_level)
        except (TypeError, ValueError):
            raise Exception("\n\nfermi_level must be one finite number.")
        if not np.isfinite(mu):
            raise Exception("\n\nfermi_level must be finite.")
        pair = self._pairing_arg(pairing)
        zero = (0,) * dk
        tab = {}
        for key, amp in self._state_table().items():
            a, b, R = key[0], key[1], key[2:]
            tab[key] = tab.get(key, 0.0) + amp
            hk = (n + a, n + b) + R
            tab[hk] = tab.get(hk, 0.0) - np.conj(amp)
        for a in range(n):
            tab[(a, a) + zero] = tab.get((a, a) + zero, 0.0) - mu
            tab[(n + a, n + a) + zero] = tab.get((n + a, n + a) + zero, 0.0) + mu
        for D, a, b, R in pair:
            mR = tuple(-x for x in R)
            for key, amp in (((a, n + b) + R, D), ((b, n + a) + mR, -D), ((n + b, a) + mR, np.conj(D)), ((n + a, b) + R, -np.conj(D))):
                tab[key] = tab.get(key, 0.0) + amp
        return self._model_from_state_table(tab, 2)

    def _model_from_state_table(self, tab, copies):
        """A spinless tb_model with `copies` * nsta orbitals -- copy c of state a at the position of a's orbital -- from a
        Hermitian state-level table {(a, b, R): amplitude}; exact zeros are dropped."""
        dk, ns = self._dim_k, self._nspin
        orb = np.tile(np.repeat(self._orb, ns, axis=0), (copies, 1))
        m = tb_model(dk, self._dim_r, self._lat.copy(), orb, per=list(self._per), nspin=1)
        N = orb.shape[0]
        zero = (0,) * dk
        ons = np.zeros(N)
        for key in sorted(tab):
            amp = complex(tab[key])
            a, b, R = key[0], key[1], key[2:]
            if a == b and R == zero:
                ons[a] = amp.real
                continue
            if amp == 0.0 or (a, b) + R > (b, a) + tuple(-x for x in R):   # (the mirror is implied)
                continue
            entry = [amp, a, b]
            if dk > 0:
                Rf = np.zeros(self._dim_r, dtype=int)
                Rf[self._per] = R
                entry.append(Rf)
            m._hoppings.append(entry)
        m.set_onsite(list(ons))
        m._tbk_epoch += 1
        return m

    def density_matrix_pairs_mesh(self, mesh_size, fermi_level, kT=0.0, pairs=None):
        """Extension: selected entries of `density_matrix_mesh` -- the complex vector D_{i_p j_p}(R_p) for a list `pairs` of up to
        2**20 triples (i, j, R): state indices and a lattice vector over the periodic directions (`(dim_k,)` integers,
        |R_a| < 2**30; None is R = 0).  Definition, phase, occupation rule and chunking are those of `density_matrix_mesh`, but
        no matrix is formed: a triple costs one weighted sum over the bands per k point, which is what a self-consistency loop
        consumes (a handful of bond orders and occupations instead of nR nsta**2 entries).  Repeated triples are allowed.
        Fixed-order sums and a partition that does not depend on the list: two calls give the same bits, and a triple gives
        the same bits alone and inside any list."""
        mesh, nk, kT = self._occ_args("density_matrix_pairs_mesh", mesh_size, kT)
        try:
            fermi_level = float(fermi_level)
        except (TypeError, ValueError):
            raise Exception("\n\nfermi_level must be one finite number.")
        if not np.isfinite(fermi_level):
            raise Exception("\n\nfermi_level must be finite.")
        n, dk = self._nsta, self._dim_k
        if pairs is None:
            raise Exception("\n\ndensity_matrix_pairs_mesh needs a list of (i, j, R) triples.")
        pairs = list(pairs)
        if len(pairs) < 1 or len(pairs) > 2 ** 20:
            raise Exception("\n\npairs must hold 1..2**20 triples (i, j, R).")
        ij = np.zeros((len(pairs), 2), dtype=np.int32)
        Rs = np.zeros((len(pairs), dk), dtype=np.int32)
        for p, ent in enumerate(pairs):
            try:
                i, j, R = ent
            except (TypeError, ValueError):
                raise Exception("\n\npairs must hold triples (i, j, R).")
            if not (_is_int(i) and _is_int(j)) or i < 0 or i >= n or j < 0 or j >= n:
                raise Exception("\n\npairs: state index out of scope.")
            Rf = np.zeros(dk) if R is None else np.array(R)
            if Rf.shape != (dk,) or Rf.dtype == object or not np.all(np.isfinite(Rf.astype(float))) or np.any(Rf != np.round(Rf)):
                raise Exception("\n\npairs: R must hold dim_k integers.")
            if np.any(np.abs(Rf) >= 2 ** 30):
                raise Exception("\n\npairs: every component of R must be below 2**30 in magnitude.")
            ij[p] = (i, j)
            Rs[p] = Rf
        out = np.zeros(len(pairs), dtype=complex)
        _lib.check(_lib.lib.tbk_density_matrix_pairs_mesh(self._device_model(), _lib.iptr(mesh), fermi_level, kT, len(pairs),
                                                          _lib.iptr(ij.reshape(-1)), _lib.iptr(Rs.reshape(-1)), _lib.dptr(out.view(float))))
        return out

    def bdg_mesh(self, mesh_size, interaction=None, n_electrons=None, fermi_level=None, kT=0.0, U=None, hartree=True, fock=False,
                 pairing=True, start=None, pairing_seed=0.1, mu_start=None, mu_step=1.0, mixing=0.5, history=4, tol=1e-10,
                 max_iter=200, check_every=1, return_density=False):
        """Extension: self-consistent Bogoliubov-de Gennes mean-field theory of the density-density interaction of
        `mean_field_mesh` (the same `interaction` / `U`), iterated on `k_uniform_mesh(mesh_size)` with the whole loop on the
        device.  An entry (V, a, b, R) -- the bond and its mirror -- is decoupled in up to three channels on the Nambu model of
        `nambu_model`: hartree (the on-site energy of a gets sum V n_b), fock (the entry (a, b, R) gets -V D_ab(R)) and pairing
        (Delta_ab(R) = V F_ab(R), F_ab(R) = <c_{b,R} c_{a,0}>, on the hop (a -> nsta + b, R) and -Delta on its mirror).

        The unknown is the real vector x: the occupations of the touched states (ascending), Re and Im of D_ab(R) per entry
        with fock, Re and Im of F_ab(R) per entry with pairing, and -- with n_electrons given -- mu last.  Exactly one of
        n_electrons (any value in (0, nsta): N is continuous in a paired state) and fermi_level.  With n_electrons the chemical
        potential is iterated with the field: x_out[mu] = x_in[mu] + mu_step (n_electrons - N_out).  start: None (occupations
        n_electrons / nsta, or 1/2 at a given fermi_level; D = 0; every F = pairing_seed, since F = 0 is always a fixed point;
        mu = mu_start, by default the mean bare on-site energy plus the mean Hartree shift of the start occupations), an array
        of occupations `(nsta,)` / `(norb, nspin)`, or an earlier `bdg_result` (restart).  mixing, history, tol, max_iter and
        check_every as in `mean_field_mesh`; for attractive interactions the mu update makes plain linear mixing unstable, use
        history >= 1.

        Returns a `bdg_result`: model (the Nambu `tb_model` of the last x_in: feed it to any other call), normal_model (this
        model with the Hartree and Fock field, no mu), fermi_level, n_electrons, occupations, pairing (the list of
        (Delta, a, b, R) `nambu_model` takes), anomalous (the F values), gap (min |E_n(k)| over the mesh), energy = <H - mu N> +
        mu N, entropy, free_energy = energy - kT entropy, grand_potential = free_energy - mu N, residuals, history (the
        occupations after every iteration), iterations, converged (False is not an exception), field (the x the last
        iteration produced); with return_density=True nambu_density `(nR, 2 nsta, 2 nsta)` and R_list, the whole density
        matrix of `model` at Fermi level 0 from one closing pass of `density_matrix_mesh`.  Fixed-order sums: two calls give
        the same bits, and max_iter = k gives the first k history rows of a longer run."""
        mesh, nk, kT = self._occ_args("bdg_mesh", mesh_size, kT)
        ns, no, dk, n = self._nspin, self._norb, self._dim_k, self._nsta
        def filling_rule(filling):
            if not 0.0 < filling < n:
                raise Exception("\n\nn_electrons must lie in the open interval (0, %d)." % n)

        filling, mixing, tol = self._scf_args("bdg_mesh", 1024, n_electrons, fermi_level, filling_rule, history, max_iter, check_every,
                                              mixing, tol)
        have_nel = n_electrons is not None
        mu_step, seed = float(mu_step), float(pairing_seed)
        if not (np.isfinite(mu_step) and mu_step > 0.0):
            raise Exception("\n\nmu_step must be finite and > 0.")
        if not np.isfinite(seed):
            raise Exception("\n\npairing_seed must be finite.")
        hartree, fock, pairing = bool(hartree), bool(fock), bool(pairing)
        if not (hartree or fock or pairing):
            raise Exception("\n\nbdg_mesh: every channel is switched off.")
        ab, Rs, Vs = self._mf_entries("bdg_mesh", interaction, U)
        nint = len(Vs)
        touched, occ_par, nocc, Rl = self._mf_layout("bdg_mesh", ab, Rs)
        par_d = nocc if fock else -1
        par_f = nocc + (2 * nint if fock else 0) if pairing else -1
        npar = nocc + 2 * nint * (int(fock) + int(pairing)) + int(have_nel)
        par_mu = npar - 1 if have_nel else -1
        nR = len(Rl)
        if npar > 2 ** 20:
            raise Exception("\n\nbdg_mesh: at most 2**20 mean-field parameters.")
        if return_density and nR * 4 * n * n > 2 ** 22:
            raise Exception("\n\nbdg_mesh: with return_density, nR * (2 nsta)**2 must be at most 2**22.")
        key = (ab.tobytes(), Rs.tobytes(), Vs.tobytes(), hartree, fock, pairing, have_nel, n)
        eps = np.array([np.real(np.array(self._site_energies[a // ns]).reshape(ns, ns)[a % ns, a % ns]) for a in range(n)])
        if isinstance(start, bdg_result):
            if start._key != key:
                raise Exception("\n\nstart: the result belongs to another model size, interaction, channel or filling setting.")
            x0 = np.array(start._x, dtype=float)
        else:
            if start is None:
                occ = np.full(n, filling / n if have_nel else 0.5)
            else:
                st = np.array(start, dtype=float)
                if not (st.size == n and st.shape in ((n,), (no, ns))):
                    raise Exception("\n\nstart must be None, occupations of shape (nsta,) or (norb, nspin), or an earlier result.")
                occ = st.reshape(n)
            x0 = np.zeros(npar)
            for a in touched:
                x0[occ_par[a]] = occ[a]
            if pairing:
                x0[par_f:par_f + 2 * nint:2] = seed
            if have_nel:
                if mu_start is None:
                    shift = np.zeros(n)
                    if hartree:
                        for e in range(nint):
                            a, b = int(ab[e, 0]), int(ab[e, 1])
                            shift[a] += Vs[e] * occ[b]
                            shift[b] += Vs[e] * occ[a]
                    x0[par_mu] = float(np.mean(eps) + np.mean(shift))
                else:
                    x0[par_mu] = float(mu_start)
        if not np.all(np.isfinite(x0)):
            raise Exception("\n\nstart must be finite.")
        bare = self.nambu_model(0.0 if have_nel else filling)
        ctx = _lib.default_context()
        x_in, x_out = np.zeros(npar), np.zeros(npar)
        energies = np.zeros(7)
        res_hist, occ_hist = np.zeros(max_iter), np.zeros((max_iter, n))
        info = np.zeros(5, dtype=np.int32)
        _lib.check(_lib.lib.tbk_bdg_mesh(
            ctx.handle, dk, n, *self._mf_table_args(bare._flat_tables(), mesh, ab, Rs, Vs), int(hartree), int(fock),
            int(pairing), int(have_nel), filling, kT, _lib.dptr(x0), mu_step, mixing, int(history), tol, int(max_iter),
            int(check_every), _lib.dptr(x_in), _lib.dptr(x_out), _lib.dptr(energies), _lib.dptr(res_hist), _lib.dptr(occ_hist),
            _lib.iptr(info)))
        res = bdg_result()
        its = self._scf_result("bdg_mesh", res, info, nR, res_hist, occ_hist, x_in, x_out, key)
        mu_in = float(energies[5])
        y = x_in.copy()
        if not hartree:
            y[:nocc] = 0.0                                         # (_mf_model adds V n_b for every entry)
        res.normal_model = self._mf_model(ab, Rs, Vs, fock, occ_par, nocc, y)
        res.pairing, res.anomalous = [], np.zeros(0, dtype=complex)
        if pairing:
            F_in = x_in[par_f:par_f + 2 * nint:2] + 1j * x_in[par_f + 1:par_f + 2 * nint:2]
            res.anomalous = x_out[par_f:par_f + 2 * nint:2] + 1j * x_out[par_f + 1:par_f + 2 * nint:2]
            for e in range(nint):
                Rf = np.zeros(self._dim_r, dtype=int)
                Rf[self._per] = Rs[e]
                res.pairing.append((complex(Vs[e] * F_in[e]), int(ab[e, 0]), int(ab[e, 1]), Rf))
        res.model = res.normal_model.nambu_model(mu_in, res.pairing)
        res.fermi_level, res.n_electrons = mu_in, float(energies[4])
        occ = occ_hist[its - 1].copy()
        res.occupations = occ.reshape(no, 2) if ns == 2 else occ
        res.gap = float(energies[6])
        res.energy, res.entropy, res.free_energy, res.grand_potential = (float(energies[0]), float(energies[1]), float(energies[2]),
                                                                         float(energies[3]))
        res.nambu_density, res.R_list = None, None
        if return_density:
            res.R_list = np.ascontiguousarray(Rl, dtype=np.int32).reshape(nR, dk)
            res.nambu_density = res.model.density_matrix_mesh(mesh_size, 0.0, kT, res.R_list)
        return res

    # ------------------------------------------------------------------ Wannier functions (extension)
    def _wannier_bvectors(self, mesh, b_vectors="star"):
        """b_vectors="shells": the shell search of `_wannier_shells`.  "star" (the default): the b-vector star of `wannier_mesh` in closed form: (steps (nbv, dim_k) int32 in {-1, 0, 1}, weights (nbv,), b (nbv, dim_r)
        Cartesian).  With S_ab = N_a N_b (a_a . a_b) / (2 pi)^2: the step +beta_a / N_a with weight S_aa / 2 - sum_{b != a} |S_ab| / 2,
        and for every pair a < b with S_ab != 0 the diagonal beta_a / N_a + sign(S_ab) beta_b / N_b with weight |S_ab| / 2, so that
        2 sum_b w_b b b^T is the identity on the span of the periodic lattice vectors (the mirror -b of every step is implied)."""
        if not (isinstance(b_vectors, str) and b_vectors in ("star", "shells")):
            raise Exception("\n\nb_vectors must be \"star\" or \"shells\".")
        if b_vectors == "shells":
            return self._wannier_shells(mesh)
        dk = self._dim_k
        A = self._lat[self._per]                                   # (dim_k, dim_r)
        gram = A @ A.T
        N = np.array(mesh, dtype=float)
        S = gram * np.outer(N, N) / (2.0 * np.pi) ** 2
        rec = 2.0 * np.pi * np.linalg.solve(gram, A)               # beta_a, rows: beta_a . a_b = 2 pi delta_ab
        steps, weights = [], []
        for a in range(dk):
            w = 0.5 * S[a, a] - 0.5 * sum(abs(S[a, b]) for b in range(dk) if b != a)
            if not w > 0.0:
                raise Exception("\n\nwannier_mesh: the mesh is too skewed for the closed-form b-vector star (the weight of the step "
                                "along axis %d is %.6g); choose mesh sizes that make the steps beta_a / N_a more nearly orthogonal." % (a, w))
            s = [0] * dk
            s[a] = 1
            steps.append(s)
            weights.append(w)
        for a in range(dk):
            for b in range(a + 1, dk):
                if S[a, b] != 0.0:
                    s = [0] * dk
                    s[a], s[b] = 1, (1 if S[a, b] > 0.0 else -1)
                    steps.append(s)
                    weights.append(0.5 * abs(S[a, b]))
        steps = np.ascontiguousarray(steps, dtype=np.int32).reshape(len(weights), dk)
        bcart = (steps / N[None, :]) @ rec
        return steps, np.ascontiguousarray(weights, dtype=float), np.ascontiguousarray(bcart)

    def _wannier_shells(self, mesh):
        """The b-vector star by a search over shells, for lattices whose closed-form star has a vanishing weight (fcc, bcc).  The
        candidates are the nonzero steps in {-1, 0, 1}^dim_k, one of every +-pair (the one whose first nonzero component is +1),
        sorted by |b| and then by descending step tuple, grouped into shells by length (relative tolerance 1e-9).  Shells are added
        shortest first, a shell that does not raise the rank of the system skipped; one weight per shell, by least squares on the
        upper triangle of 2 sum_b w_b b b^T = 1; the first set with residual below 1e-12 and every weight positive is taken.  At
        most 6 vectors (the kernels' cap).  Returns what `_wannier_bvectors` returns."""
        dk = self._dim_k
        A = self._lat[self._per]
        N = np.array(mesh, dtype=float)
        rec = 2.0 * np.pi * np.linalg.solve(A @ A.T, A)
        cand = []
        for idx in np.ndindex(*([3] * dk)):
            s = [1 - i for i in idx]                               # descending tuples: (1, 1, 1) first
            nz = [x for x in s if x != 0]
            if nz and nz[0] == 1:
                cand.append(s)
        cand = np.array(cand, dtype=np.int32).reshape(-1, dk)
        bc = (cand / N[None, :]) @ rec
        ln = np.sqrt(np.sum(bc ** 2, axis=1))
        order = np.argsort(ln, kind="stable")
        shells = []
        for i in order:
            if shells and abs(ln[i] - ln[shells[-1][0]]) <= 1e-9 * ln[shells[-1][0]]:
                shells[-1].append(int(i))
            else:
                shells.append([int(i)])
        shells = [sorted(sh) for sh in shells]                     # inside a shell: the candidates' own order, not rounding's
        iu = np.triu_indices(self._dim_r)
        target = np.eye(self._dim_r)[iu]
        cols, chosen = [], []
        for sh in shells:
            col = 2.0 * np.einsum("bi,bj->ij", bc[sh], bc[sh])[iu]
            trial = cols + [col]
            mat = np.array(trial).T
            if np.linalg.matrix_rank(mat / np.linalg.norm(mat, axis=0)[None, :], tol=1e-9) < len(trial):
                continue
            if sum(len(c) for c in chosen) + len(sh) > 6:
                break
            cols, chosen = trial, chosen + [sh]
            w = np.linalg.lstsq(mat, target, rcond=None)[0]
            if np.max(np.abs(mat @ w - target)) < 1e-12 and np.all(w > 0.0):
                pick = [i for c in chosen for i in c]
                weights = np.concatenate([[w[j]] * len(c) for j, c in enumerate(chosen)])
                return (np.ascontiguousarray(cand[pick], dtype=np.int32).reshape(len(pick), dk), np.ascontiguousarray(weights, dtype=float),
                        np.ascontiguousarray(bc[pick]))
        raise Exception("\n\nwannier_mesh: the mesh is too skewed: no b-vector star of positive weights was found within 6 vectors with "
                        "steps in {-1, 0, 1}.")

    def _wannier_torus(self, mesh):
        """One lattice vector per class of the torus of the mesh: R_a in -floor((N_a - 1) / 2) .. floor(N_a / 2), row-major."""
        axes = [np.arange(-((int(n) - 1) // 2), int(n) // 2 + 1) for n in mesh]
        grid = np.meshgrid(*axes, indexing="ij")
        return np.ascontiguousarray(np.stack([g.reshape(-1) for g in grid], axis=1), dtype=np.int32)

    def _wannier_args(self, mesh_size, trial, bands, max_iter, tol, check_every, R_list, b_vectors="star"):
        """The checked arguments of `wannier_mesh` in the layout of tbk_wannier_mesh."""
        if self._dim_k not in (1, 2, 3):
            raise Exception("\n\nwannier_mesh needs a model with dim_k 1, 2 or 3.")
        if self._dim_r != self._dim_k:
            raise Exception("\n\nwannier_mesh needs a model that is periodic in every direction (dim_k == dim_r).")
        mesh, nk = self._mesh_arg(mesh_size)
        if np.min(mesh) < 3:
            raise Exception("\n\nwannier_mesh: every mesh size must be at least 3 (the steps +b and -b must reach different points).")
        n, dk = self._nsta, self._dim_k
        if n > 2048:
            raise Exception("\n\nwannier_mesh: at most 2048 states.")
        try:
            sel = np.atleast_1d(np.array(bands)).ravel()
        except Exception:
            raise Exception("\n\nbands must be a list of band indices.")
        if sel.size < 1 or not all(_is_int(b) for b in sel.tolist()):
            raise Exception("\n\nbands must be a list of band indices.")
        if sel.size > 32:
            raise Exception("\n\nwannier_mesh: at most 32 bands.")
        if np.min(sel) < 0 or np.max(sel) >= n:
            raise Exception("\n\nbands: index out of range.")
        if np.unique(sel).size != sel.size:
            raise Exception("\n\nbands lists a band twice.")
        sel = np.ascontiguousarray(sel, dtype=np.int32)
        # the trial functions as term lists
        terms = []
        tr = trial
        as_arr = None
        try:
            as_arr = np.array(tr)
        except Exception:
            as_arr = None
        if as_arr is not None and as_arr.dtype != object and as_arr.ndim == 1 and as_arr.size >= 1 \
                and all(_is_int(s) for s in as_arr.tolist()):
            for s in as_arr.tolist():
                terms.append([(1.0 + 0.0j, int(s), np.zeros(dk, dtype=np.int64))])
        elif as_arr is not None and as_arr.dtype != object and as_arr.ndim == 2 and np.issubdtype(as_arr.dtype, np.number):
            if as_arr.shape[0] != n or as_arr.shape[1] < 1:
                raise Exception("\n\ntrial: a matrix of amplitudes must have shape (nsta, nw).")
            mat = np.array(as_arr, dtype=complex)
            if not np.all(np.isfinite(mat)):
                raise Exception("\n\ntrial: amplitudes must be finite.")
            for w in range(mat.shape[1]):
                nz = np.nonzero(mat[:, w])[0]
                if nz.size == 0:
                    raise Exception("\n\ntrial: function %d is zero." % w)
                terms.append([(complex(mat[j, w]), int(j), np.zeros(dk, dtype=np.int64)) for j in nz])
        else:
            try:
                for fnc in tr:
                    lst = []
                    for amp, s, R in fnc:
                        amp = complex(amp)
                        Rf = np.array(R)
                        if dk == 1 and Rf.ndim == 0:
                            Rf = Rf.reshape(1)
                        if Rf.shape != (self._dim_r,) or Rf.dtype == object or np.any(Rf != np.round(Rf)):
                            raise Exception("\n\ntrial: R must hold dim_r integers, as in set_hop.")
                        if not _is_int(s):
                            raise Exception("\n\ntrial: a state index must be an integer.")
                        lst.append((amp, int(s), np.array(Rf, dtype=np.int64)[self._per]))
                    if not lst:
                        raise Exception("\n\ntrial: a function without terms.")
                    terms.append(lst)
            except (TypeError, ValueError):
                raise Exception("\n\ntrial must be a list of state indices, a complex (nsta, nw) matrix, or per function a list of "
                                "(amp, state, R) terms.")
        nw = len(terms)
        if nw < 1:
            raise Exception("\n\ntrial: at least one function.")
        if nw > 16:
            raise Exception("\n\nwannier_mesh: at most 16 trial functions.")
        if nw > sel.size:
            raise Exception("\n\nwannier_mesh: more trial functions (%d) than bands (%d)." % (nw, sel.size))
        tptr, tstate, tR, tamp = [0], [], [], []
        for lst in terms:
            for amp, s, R in lst:
                if s < 0 or s >= n:
                    raise Exception("\n\ntrial: state index out of range.")
                if not np.isfinite(amp):
                    raise Exception("\n\ntrial: amplitudes must be finite.")
                if np.any(np.abs(R) >= 2 ** 30):
                    raise Exception("\n\ntrial: every component of R must be below 2**30 in magnitude.")
                tstate.append(s)
                tR.append(R)
                tamp.append(amp)
            tptr.append(len(tstate))
        if nk * n * nw > 2 ** 26:
            raise Exception("\n\nwannier_mesh: N_k * nsta * nw = %d complex numbers stay resident (at most 2**26): coarsen the mesh."
                            % (nk * n * nw))
        if not _is_int(max_iter) or max_iter < 0 or max_iter > 65536:
            raise Exception("\n\nmax_iter must be an integer in 0..65536.")
        if not _is_int(check_every) or check_every < 1:
            raise Exception("\n\ncheck_every must be an integer >= 1.")
        try:
            tol = float(tol)
        except (TypeError, ValueError):
            raise Exception("\n\ntol must be finite and >= 0.")
        if not (np.isfinite(tol) and tol >= 0.0):
            raise Exception("\n\ntol must be finite and >= 0.")
        if R_list is None:
            R, r_user = self._wannier_torus(mesh), 0
        else:
            R, single = self._R_list_arg(R_list)
            r_user = 1
        if R.shape[0] * nw * nw > 2 ** 26:
            raise Exception("\n\nwannier_mesh: nR * nw**2 must be at most 2**26: give an R_list.")
        steps, weights, bcart = self._wannier_bvectors(mesh, b_vectors)
        return dict(mesh=mesh, nk=nk, bands=sel, nw=nw, tptr=np.ascontiguousarray(tptr, dtype=np.int32),
                    tstate=np.ascontiguousarray(tstate, dtype=np.int32),
                    tR=np.ascontiguousarray(np.array(tR).reshape(len(tstate), dk), dtype=np.int32),
                    tamp=np.ascontiguousarray(tamp, dtype=complex), max_iter=int(max_iter), tol=tol, check_every=int(check_every),
                    R=R, r_user=r_user, steps=steps, weights=weights, bcart=bcart)

    def wannier_mesh(self, mesh_size, trial, bands, max_iter=0, tol=0.0, check_every=10, R_list=None, return_functions=False,
                     return_gauge=False, b_vectors="star"):
        """Extension: projected and maximally localised Wannier functions of the bands `bands` on `k_uniform_mesh(mesh_size)`
        (1-, 2- or 3-D, every N_a >= 3), with the whole loop on the device.

        trial: nw <= 16 functions as a list of state indices, a complex `(nsta, nw)` matrix of home-cell amplitudes, or per function
        a list of `(amp, state, R)` terms with R as in `set_hop` (states of a spinful model are orbital * 2 + spin, the order of
        `_gen_ham`).  bands: nw <= nb <= 32 distinct band indices, the same at every k.  With the cell-periodic eigenvectors of
        `solve_all`: g~_n(k)[j] = sum amp e^{-2 pi i k.(R + tau_j)}, A = V_bands+ g~, U = A (A+ A)^-1/2 (Loewdin), u~ = V_bands U.  The
        call raises when the smallest singular value of A over the mesh is below 1e-8 -- what the band of a Chern insulator does to
        any trial function.  The overlaps M(k, b) = <u~(k)|u~(k + b)> run over the closed-form b-vector star of
        `_wannier_bvectors`; centres, the spread Omega = Omega_I + Omega_OD + Omega_D and the steepest-descent step (alpha = 1)
        are those of Marzari and Vanderbilt, PRB 56, 12847.  max_iter = 0 is the projection alone; otherwise up to max_iter
        steps, the host reading the change of Omega every check_every steps and stopping when its modulus is below tol > 0.

        Returns a `wannier_result`: model (an ordinary `tb_model` of nw orbitals at the centres with the hoppings
        t_mn(R) = (1 / N_k) sum_k e^{-2 pi i k.R} [U_tot+ E U_tot]_mn; R over one representative per class of the torus of the
        mesh, an entry at R_a = N_a / 2 of an even axis split in halves between +-N_a / 2, or over R_list, at most 4096
        vectors), hoppings `(nR, nw, nw)` with R_list `(nR, dim_k)` (the raw table), centers `(nw, dim_r)` Cartesian, spreads
        `(nw,)`, omega_i, omega_od, omega_d, omega, sv_min, history (Omega of the projection, then at every check), iterations,
        converged, b_vectors `(nbv, dim_r)`, b_weights; with return_functions, functions `(nR, nsta, nw)`:
        w_n(R, j) = (1 / N_k) sum_k e^{2 pi i k.(R + tau_j)} u~_n(k)[j]; with return_gauge, gauge `(N_k, nb, nw)`: U_tot.
        b_vectors="shells" takes the star from the shell search of `_wannier_shells` (fcc, bcc) instead of the closed form.
        Fixed-order sums: two calls give the same bits, and max_iter = m gives the first rows of the history of a longer run."""
        a = self._wannier_args(mesh_size, trial, bands, max_iter, tol, check_every, R_list, b_vectors)
        mesh, nk, nw, R = a["mesh"], a["nk"], a["nw"], a["R"]
        n, dk, nb, nR, nbv = self._nsta, self._dim_k, a["bands"].size, a["R"].shape[0], a["weights"].size
        if return_functions and nR * n * nw > 2 ** 26:
            raise Exception("\n\nwannier_mesh: the functions take nR * nsta * nw complex numbers (at most 2**26): give an R_list.")
        bgram = np.ascontiguousarray(a["bcart"] @ a["bcart"].T)
        hop = np.zeros((nR, nw, nw), dtype=complex)
        sums = np.zeros(21 + 16 * 6)
        hist = np.zeros(a["max_iter"] + 1)
        fns = np.zeros((nR, n, nw), dtype=complex) if return_functions else None
        gauge = np.zeros((nk, nb, nw), dtype=complex) if return_gauge else None
        info = np.zeros(5, dtype=np.int32)
        _lib.check(_lib.lib.tbk_wannier_mesh(
            self._device_model(), _lib.iptr(mesh), int(nb), _lib.iptr(a["bands"]), int(nw), len(a["tstate"]), _lib.iptr(a["tptr"]),
            _lib.iptr(a["tstate"]), _lib.iptr(a["tR"].reshape(-1)), _lib.dptr(a["tamp"].view(float)), int(nbv),
            _lib.iptr(a["steps"].reshape(-1)), _lib.dptr(a["weights"]), _lib.dptr(bgram.reshape(-1)), a["max_iter"], a["tol"],
            a["check_every"], int(nR), int(a["r_user"]), _lib.iptr(R.reshape(-1)), _lib.dptr(hop.view(float)), _lib.dptr(sums),
            _lib.dptr(hist), _lib.dptr(fns.view(float)) if return_functions else None,
            _lib.dptr(gauge.view(float)) if return_gauge else None, _lib.iptr(info)))
        return self._wannier_result(a, int(info[0]), bool(info[1]), hop, sums, hist, fns, gauge)

    def _wannier_result(self, a, its, converged, hop, sums, hist, fns, gauge):
        """The `wannier_result` of a call from its checked arguments and what the device returned."""
        mesh, nk, nw, R, nbv = a["mesh"], a["nk"], a["nw"], a["R"], a["weights"].size
        res = wannier_result()
        res.omega_i, res.omega_od, res.omega_d, res.omega = (float(x) for x in sums[:4])
        res.spreads = sums[4:4 + nw].copy()
        res.sv_min = float(sums[20])
        s1 = sums[21:21 + nw * nbv].reshape(nw, nbv)
        res.centers = -(2.0 / nk) * (s1 * a["weights"][None, :]) @ a["bcart"]
        rows = [0] + [it for it in range(1, its + 1) if it % a["check_every"] == 0 or it == its]
        res.history = hist[rows].copy()
        res.iterations, res.converged = its, converged
        res.b_vectors, res.b_weights = a["bcart"], a["weights"]
        res.hoppings, res.R_list = hop, R
        res.model = self._wannier_model(mesh, hop, R, res.centers, split=not a["r_user"])
        if fns is not None:
            res.functions = fns
        if gauge is not None:
            res.gauge = gauge
        return res

    def wannier_disentangle_mesh(self, mesh_size, trial, bands, window=None, frozen=None, dis_iter=200, dis_mixing=1.0, dis_tol=0.0,
                                 max_iter=0, tol=0.0, check_every=10, R_list=None, return_functions=False, return_gauge=False,
                                 b_vectors="star"):
        """Extension: disentangled Wannier functions with energy windows (Souza, Marzari and Vanderbilt, PRB 65, 035109) on
        `k_uniform_mesh(mesh_size)`, the whole loop on the device.  trial, bands, max_iter, tol, check_every, R_list,
        return_functions, return_gauge and b_vectors mean what they mean in `wannier_mesh`; `bands` (nw <= nb <= 32, the same at
        every k) is the outermost candidate set.

        window=(lo, hi): of those bands only the ones with lo <= E_n(k) <= hi take part at k (None: all); the call raises, naming
        the k, where fewer than nw do.  frozen=(lo, hi): window bands inside it are kept in the subspace whole; the call raises,
        naming the k, where more than nw are.  The start is the projected subspace U = A (A+ A)^-1/2 (rows outside the window
        zero) with the frozen states forced in: the frozen unit vectors, then the nw - n_frozen leading eigenvectors of U U+ on the
        free indices (in the window, not frozen).  Iteration: Z(k) = sum_{+-b} w_b T T+, T = M0(k, b) U_dis(k + b) from the
        previous iteration at every k, Z_in = dis_mixing Z + (1 - dis_mixing) Z_in, the leading eigenvectors of Z_in on the free
        indices; dis_iter iterations (0..65536; 0: the start alone), the host reading the change of Omega_I every check_every
        iterations and stopping when its modulus is below dis_tol > 0.  Then the gauge U0 = U_dis A' (A'+ A')^-1/2, A' = U_dis+ A,
        and `wannier_mesh`'s spread, descent (max_iter), model and functions.  The frozen eigenvalues are eigenvalues of the
        result model at every mesh point.

        Returns `wannier_mesh`'s `wannier_result` (sv_min: the smallest singular value of A' over the mesh) with dis_history
        (Omega_I of the start, then at every check), dis_iterations, dis_converged, n_window and n_frozen `(N_k,)`, dis_gap_min (the
        smallest gap over k, at the last iteration, between the last selected and the first rejected eigenvalue of Z; inf where
        nothing is rejected), sv_min_projection (of the nb x nw projection); gauge `(N_k, nb, nw)` has zero rows for bands outside
        the window.  Beyond `wannier_mesh`'s caps: N_k * nsta * nb <= 2**26 and N_k * nbv * nb**2 <= 2**26 stay resident.
        Fixed-order sums: two calls give the same bits, and a shorter dis_iter or max_iter gives the first rows of a longer run."""
        def pair(x, name):
            if x is None:
                return None
            try:
                v = np.array(x, dtype=float).ravel()
            except (TypeError, ValueError):
                v = np.zeros(0)
            if v.size != 2 or not np.all(np.isfinite(v)) or v[0] > v[1]:
                raise Exception("\n\n%s must be None or a finite pair (lo, hi) with lo <= hi." % name)
            return np.ascontiguousarray(v)
        window, frozen = pair(window, "window"), pair(frozen, "frozen")
        if not _is_int(dis_iter) or dis_iter < 0 or dis_iter > 65536:
            raise Exception("\n\ndis_iter must be an integer in 0..65536.")
        try:
            dis_mixing, dis_tol = float(dis_mixing), float(dis_tol)
        except (TypeError, ValueError):
            raise Exception("\n\ndis_mixing and dis_tol must be numbers.")
        if not (dis_mixing > 0.0 and dis_mixing <= 1.0):
            raise Exception("\n\ndis_mixing must lie in (0, 1].")
        if not (np.isfinite(dis_tol) and dis_tol >= 0.0):
            raise Exception("\n\ndis_tol must be finite and >= 0.")
        a = self._wannier_args(mesh_size, trial, bands, max_iter, tol, check_every, R_list, b_vectors)
        mesh, nk, nw, R = a["mesh"], a["nk"], a["nw"], a["R"]
        n, dk, nb, nR, nbv = self._nsta, self._dim_k, a["bands"].size, a["R"].shape[0], a["weights"].size
        if nk * n * nb > 2 ** 26:
            raise Exception("\n\nwannier_disentangle_mesh: N_k * nsta * nb = %d complex numbers of candidate states stay resident "
                            "(at most 2**26): coarsen the mesh." % (nk * n * nb))
        if nk * nbv * nb * nb > 2 ** 26:
            raise Exception("\n\nwannier_disentangle_mesh: N_k * nbv * nb**2 = %d complex numbers of overlaps stay resident "
                            "(at most 2**26): coarsen the mesh." % (nk * nbv * nb * nb))
        if return_functions and nR * n * nw > 2 ** 26:
            raise Exception("\n\nwannier_disentangle_mesh: the functions take nR * nsta * nw complex numbers (at most 2**26): give an R_list.")
        bgram = np.ascontiguousarray(a["bcart"] @ a["bcart"].T)
        hop = np.zeros((nR, nw, nw), dtype=complex)
        sums = np.zeros(21 + 16 * 6)
        hist = np.zeros(a["max_iter"] + 1)
        dsums = np.zeros(2)
        dhist = np.zeros(int(dis_iter) + 1)
        nwin = np.zeros(nk, dtype=np.int32)
        nfrz = np.zeros(nk, dtype=np.int32)
        fns = np.zeros((nR, n, nw), dtype=complex) if return_functions else None
        gauge = np.zeros((nk, nb, nw), dtype=complex) if return_gauge else None
        info = np.zeros(5, dtype=np.int32)
        _lib.check(_lib.lib.tbk_wannier_dis_mesh(
            self._device_model(), _lib.iptr(mesh), int(nb), _lib.iptr(a["bands"]), int(nw), len(a["tstate"]), _lib.iptr(a["tptr"]),
            _lib.iptr(a["tstate"]), _lib.iptr(a["tR"].reshape(-1)), _lib.dptr(a["tamp"].view(float)), int(nbv),
            _lib.iptr(a["steps"].reshape(-1)), _lib.dptr(a["weights"]), _lib.dptr(bgram.reshape(-1)),
            _lib.dptr(window) if window is not None else None, _lib.dptr(frozen) if frozen is not None else None, int(dis_iter),
            dis_mixing, dis_tol, a["max_iter"], a["tol"], a["check_every"], int(nR), int(a["r_user"]), _lib.iptr(R.reshape(-1)),
            _lib.dptr(hop.view(float)), _lib.dptr(sums), _lib.dptr(hist), _lib.dptr(dsums), _lib.dptr(dhist), _lib.iptr(nwin),
            _lib.iptr(nfrz), _lib.dptr(fns.view(float)) if return_functions else None,
            _lib.dptr(gauge.view(float)) if return_gauge else None, _lib.iptr(info)))
        res = self._wannier_result(a, int(info[0]), bool(info[1]), hop, sums, hist, fns, gauge)
        dits = int(info[2])
        rows = [0] + [it for it in range(1, dits + 1) if it % a["check_every"] == 0 or it == dits]
        res.dis_history = dhist[rows].copy()
        res.dis_iterations, res.dis_converged = dits, bool(info[3])
        res.n_window, res.n_frozen = nwin, nfrz
        res.sv_min_projection, res.dis_gap_min = float(dsums[0]), float(dsums[1])
        return res

    def _wannier_model(self, mesh, hop, R, centers, split):
        """The tb_model of the Wannier functions: nw orbitals at the centres (reduced coordinates), on-site terms the real diagonal
        of t(0), every other entry of the table a hopping.  split: an entry at R_a = N_a / 2 of an even axis goes in halves to
        +-N_a / 2, so that the table is Hermitian.  A pair (m, n, R) and its mirror (n, m, -R) are stored once, as their mean."""
        nw, dk = hop.shape[1], self._dim_k
        red = np.linalg.solve(self._lat.T, np.array(centers, dtype=float).T).T
        m = tb_model(dk, self._dim_r, self._lat.copy(), red, per=list(self._per), nspin=1)
        table = {}
        for r in range(R.shape[0]):
            Rv = [int(x) for x in R[r]]
            images = [([], 1.0)]
            for d in range(dk):
                if split and mesh[d] % 2 == 0 and Rv[d] == mesh[d] // 2:
                    images = [(pre + [s * Rv[d]], w * 0.5) for pre, w in images for s in (1, -1)]
                else:
                    images = [(pre + [Rv[d]], w) for pre, w in images]
            for Ri, w in images:
                key = tuple(Ri)
                table[key] = table.get(key, 0.0) + w * hop[r]
        zero = tuple([0] * dk)
        if zero in table:
            m.set_onsite([float(table[zero][i, i].real) for i in range(nw)])
        hops = []
        for key in sorted(table):
            neg = tuple(-x for x in key)
            if key < neg:
                continue                                           # its mirror carries the pair
            t = table[key]
            tm = table.get(neg)
            for i in range(nw):
                for j in range(nw):
                    if key == zero and i >= j:
                        continue
                    amp = t[i, j] if tm is None or key == zero else 0.5 * (t[i, j] + np.conj(tm[j, i]))
                    if key == zero:
                        amp = 0.5 * (t[i, j] + np.conj(t[j, i]))
                    Rf = np.zeros(self._dim_r, dtype=int)
                    Rf[self._per] = key
                    hops.append([complex(amp), i, j, Rf])
        for key in sorted(table):                                   # vectors whose mirror is not in a caller's list
            neg = tuple(-x for x in key)
            if key < neg and neg not in table:
                t = table[key]
                for i in range(nw):
                    for j in range(nw):
                        Rf = np.zeros(self._dim_r, dtype=int)
                        Rf[self._per] = key
                        hops.append([complex(t[i, j]), i, j, Rf])
        m._hoppings.extend(hops)
        m._tbk_epoch += 1
        return m

    # ------------------------------------------------------------------ the lattice Green's function and local impurities (extensions)
    def _gf_args(self, what, mesh_size, omega, eta):
        """(mesh, N_k, omega, scalar, eta) of the Green's-function calls: dim_k 1, 2 or 3, the mesh of `_mesh_arg`, omega a scalar
        or 1-D with 1..65536 finite values, eta one finite number > 0."""
        if self._dim_k not in (1, 2, 3):
            raise Exception("\n\n%s needs a model with dim_k 1, 2 or 3." % what)
        mesh, nk = self._mesh_arg(mesh_size)
        if nk >= 2 ** 31:
            raise Exception("\n\n%s: the mesh must have fewer than 2**31 points." % what)
        w, scalar, eta = self._omega_eta_arg(omega, eta)
        return mesh, nk, w, scalar, eta

    @staticmethod
    def _omega_eta_arg(omega, eta):
        """(omega as a contiguous 1-D float array, whether it was a scalar, eta): omega a scalar or 1-D with 1..65536 finite values,
        eta one finite number > 0."""
        try:
            w = np.array(omega, dtype=float)
        except (TypeError, ValueError):
            raise Exception("\n\nomega must be a scalar or a 1-D array of 1..65536 finite frequencies.")
        scalar = w.ndim == 0
        if scalar:
            w = w.reshape(1)
        if w.ndim != 1 or w.size < 1 or w.size > 65536:
            raise Exception("\n\nomega must be a scalar or a 1-D array of 1..65536 finite frequencies.")
        if not np.all(np.isfinite(w)):
            raise Exception("\n\nomega must be finite.")
        try:
            eta = float(eta)
        except (TypeError, ValueError):
            raise Exception("\n\neta must be one finite number > 0.")
        if not np.isfinite(eta) or not eta > 0.0:
            raise Exception("\n\neta must be finite and > 0 (the retarded function).")
        return np.ascontiguousarray(w), scalar, eta

    def _gf_states_arg(self, states):
        """The selection of the Green's-function calls as int32 state indices, or None for all states: 1..32 distinct integers in
        [-nsta, nsta), negative ones counted from the end."""
        if states is None:
            return None
        st = np.asarray(states)
        if st.ndim != 1 or st.size < 1 or st.size > 32 or not np.issubdtype(st.dtype, np.integer):
            raise Exception("\n\nstates must be None or a list of 1..32 integer state indices.")
        if st.min() < -self._nsta or st.max() >= self._nsta:
            raise Exception("\n\nstates must be indices in [-nsta, nsta).")
        st = np.where(st < 0, st + self._nsta, st)
        if np.unique(st).size != st.size:
            raise Exception("\n\nstates must be distinct.")
        return np.ascontiguousarray(st, dtype=np.int32)

    def _gf_impurity_args(self, mesh, sites, potential):
        """(site states int32 (ns,), site lattice vectors int32 (ns, dim_k), V complex (ns, ns)) of the impurity calls."""
        dk, n = self._dim_k, self._nsta
        try:
            pairs = [(s, np.array(R)) for s, R in sites]
        except (TypeError, ValueError):
            raise Exception("\n\nsites must be a list of 1..16 pairs (state index, R).")
        if len(pairs) < 1 or len(pairs) > 16:
            raise Exception("\n\nsites must be a list of 1..16 pairs (state index, R).")
        st = np.zeros(len(pairs), dtype=np.int32)
        Rs = np.zeros((len(pairs), dk), dtype=np.int32)
        for a, (s, R) in enumerate(pairs):
            if not _is_int(s) or s < -n or s >= n:
                raise Exception("\n\nsites: the state index of site %d must be an integer in [-nsta, nsta)." % a)
            if R.shape != (dk,) or R.dtype == object or not (np.issubdtype(R.dtype, np.integer) or np.issubdtype(R.dtype, np.floating)) \
                    or not np.all(np.isfinite(R)) or np.any(R != np.round(R)) or np.any(np.abs(R) >= 2 ** 30):
                raise Exception("\n\nsites: R of site %d must hold dim_k integers below 2**30 in magnitude." % a)
            st[a] = s + n if s < 0 else s
            Rs[a] = R
        key = [(int(st[a]),) + tuple(int(x) for x in np.mod(Rs[a], mesh)) for a in range(len(pairs))]
        if len(set(key)) != len(key):
            raise Exception("\n\nsites: two sites coincide modulo the mesh (they are one site of its torus).")
        ns = len(pairs)
        try:
            v = np.array(potential, dtype=complex)
        except (TypeError, ValueError):
            raise Exception("\n\npotential must be a Hermitian (ns, ns) matrix or ns real on-site shifts.")
        if v.shape == (ns,):
            if np.any(v.imag != 0.0):
                raise Exception("\n\npotential: the on-site shifts must be real.")
            v = np.diag(v)
        if v.shape != (ns, ns):
            raise Exception("\n\npotential must be a Hermitian (ns, ns) matrix or ns real on-site shifts.")
        if not np.all(np.isfinite(v)):
            raise Exception("\n\npotential must be finite.")
        if np.max(np.abs(v - v.conj().T)) > 1e-12 * max(np.max(np.abs(v)), 0.0):
            raise Exception("\n\npotential must be Hermitian.")
        return st, np.ascontiguousarray(Rs), np.ascontiguousarray(v)

    def green_function_mesh(self, mesh_size, omega, eta, R_list=None, states=None):
        """Extension: the retarded real-space Green's function of the bulk crystal, resolved in energy, as a mean over
        `k_uniform_mesh(mesh_size)` (1-, 2- or 3-D, generated on the device): complex `(nw, nR, nsta, nsta)`,

            G_ij(R, w) = (1 / N_k) sum_k sum_n u_n,i(k) conj(u_n,j(k)) / (w + i eta - E_n(k)) e^{-2 pi i k.(R + tau_j - tau_i)}
                       = <i,0| (w + i eta - H)^-1 |j,R>

        with the eigenpairs of `solve_all`.  Index layout and phase convention are exactly those of `density_matrix_mesh` and of
        `set_hop(amp, i, j, R)`; `density_matrix_mesh` is the w-integrated special case (its weight f(E_n) is 1 / (z - E_n) here).

        G is EXACTLY the Green's function of the torus of the mesh: with H_T the Hamiltonian whose block from cell c to cell
        c + R (mod mesh_size) is the hopping table t(R), `inv(z - H_T)[(0, i), (R, j)]` equals the formula above.  The
        infinite-crystal limit needs eta above the level spacing of the mesh; below it G shows the discrete levels of the torus.
        Degenerate levels need no care: G is a function of H.  conj(G_ij(R, w + i eta)) = G_ji(-R, w - i eta).

        omega: a scalar (the w axis is dropped), or 1-D with 1..65536 finite values in any order, repeats allowed.  eta: one
        finite number > 0.  R_list: as `density_matrix_mesh` -- `(nR, dim_k)` integers with |R_a| < 2**30, 1 <= nR <= 4096;
        `(dim_k,)` alone drops the axis; None is R = 0.  states: None for all states, or 1..32 distinct state indices (negative
        ones count from the end): the result is then the `(na, na)` block G_{s_a s_b} at a cost of nsta na^2 per point and
        frequency instead of nsta^3 -- one site of a 512-state supercell is affordable.  Spinful models with states=None return
        `(..., norb, 2, norb, 2)`.  nw * nR * na^2 <= 2**22.

        The phase e^{-2 pi i k.R} is formed from exact integers: an R equal to a period of the mesh gives the bits of R = 0.  The
        partition of the work depends on (mesh, nsta, dim_k) alone and every sum has a fixed order: two calls give the same
        bits, and a frequency, an R or a selection gives the same bits alone and inside a longer omega or R_list.  The
        eigenvectors never leave the device."""
        mesh, nk, w, scalar, eta = self._gf_args("green_function_mesh", mesh_size, omega, eta)
        R, single = self._R_list_arg(R_list)
        sel = self._gf_states_arg(states)
        n = self._nsta
        na = n if sel is None else int(sel.size)
        nw, nR = int(w.size), R.shape[0]
        if nw * nR * na * na > 2 ** 22:
            raise Exception("\n\nnw * nR * na^2 must be at most 2**22: split omega or R_list.")
        out = np.zeros((nw, nR, na, na), dtype=complex)
        _lib.check(_lib.lib.tbk_green_function_mesh(self._device_model(), _lib.iptr(mesh), nw, _lib.dptr(w), eta, nR, _lib.iptr(R),
                                                    0 if sel is None else na, _lib.iptr(sel), _lib.dptr(out.view(float))))
        if sel is None and self._nspin == 2:
            out = out.reshape(nw, nR, self._norb, 2, self._norb, 2)
        if single:
            out = out[:, 0]
        return out[0] if scalar else out

    def impurity_t_matrix_mesh(self, mesh_size, omega, eta, sites, potential, return_det=False):
        """Extension: the exact T-matrix of a local impurity in the bulk crystal (no supercell).  sites: a list of 1..16 pairs
        `(state index, R)`, R holding dim_k integers; two sites that coincide modulo the mesh raise (they are one site of the
        torus).  potential: a finite Hermitian complex `(ns, ns)` matrix V between the sites, or a 1-D real array of ns on-site
        shifts.  With G of `green_function_mesh` on the same mesh,

            g_ab(w) = G_{i_a i_b}(R_b - R_a, w)        T(w) = V (1 - g(w) V)^-1

        Returns T, complex `(nw, ns, ns)` (`(ns, ns)` for a scalar omega); with return_det=True `(T, det)`, det = det(1 - g V),
        complex `(nw,)`: its zeros in a gap are the bound states of the impurity.  The full Green's function with the impurity is
        G + G T G.  The solve is an LU with partial pivoting per frequency on the device.  A singular 1 - g V (a pivot that is
        exactly 0) raises an error that names the frequency; it is never a NaN result.  Bit-reproducible as `green_function_mesh`."""
        mesh, nk, w, scalar, eta = self._gf_args("impurity_t_matrix_mesh", mesh_size, omega, eta)
        st, Rs, v = self._gf_impurity_args(mesh, sites, potential)
        nw, ns = int(w.size), int(st.size)
        t = np.zeros((nw, ns, ns), dtype=complex)
        det = np.zeros(nw, dtype=complex) if return_det else None
        _lib.check(_lib.lib.tbk_impurity_t_matrix_mesh(self._device_model(), _lib.iptr(mesh), nw, _lib.dptr(w), eta, ns, _lib.iptr(st),
                                                       _lib.iptr(Rs), _lib.dptr(v.view(float)), _lib.dptr(t.view(float)),
                                                       None if det is None else _lib.dptr(det.view(float))))
        if scalar:
            return (t[0], det[0]) if return_det else t[0]
        return (t, det) if return_det else t

    def impurity_ldos_mesh(self, mesh_size, omega, eta, sites, potential, R_list=None, states=None):
        """Extension: the local density of states around the impurity of `impurity_t_matrix_mesh`: `(ldos0, dldos)`,

            ldos0[w, a]    = -(1 / pi) Im G_{s_a s_a}(0, w)                                         float (nw, na)
            dldos[w, r, a] = -(1 / pi) Im sum_{bc} G_{s_a i_b}(R_b - R_r) T_bc G_{i_c s_a}(R_r - R_c)    float (nw, nR, na)

        ldos0 is the bulk LDOS of state s_a (the same in every cell, Lorentzian-broadened by eta), dldos the change in the cell
        R_r of R_list: the Friedel ripple, and over a grid of R a quasi-particle interference map.  R_list and states (the probe
        states s_a; None: all states, which needs nsta <= 32) as `green_function_mesh`; a scalar omega, a single R or R_list=None
        drop their axes.  The G blocks are computed into device scratch and contracted there; only the two real results come
        back.  Internally the lattice vectors are the differences between probe cells and sites, reduced modulo the mesh (it
        cannot tell them apart) and de-duplicated, nR_int of them, and the selection is the union of the probe and site states,
        na_int of them.  Caps: nR_int <= 16384, nw * nR_int * na_int^2 <= 2**23 and nw * nR * na <= 2**24 -- a 64 x 64 map of R
        around one site of a 2-state model at 16 frequencies fits in one call; beyond them the call raises (split omega or
        R_list).  A singular 1 - g V raises as in `impurity_t_matrix_mesh`."""
        mesh, nk, w, scalar, eta = self._gf_args("impurity_ldos_mesh", mesh_size, omega, eta)
        st, Rs, v = self._gf_impurity_args(mesh, sites, potential)
        R, single = self._R_list_arg(R_list)
        sel = self._gf_states_arg(states)
        n = self._nsta
        if sel is None and n > 32:
            raise Exception("\n\nstates=None means all states, which needs nsta <= 32: give states (1..32 state indices).")
        na = n if sel is None else int(sel.size)
        nw, nR, ns = int(w.size), R.shape[0], int(st.size)
        # the internal problem, as the library forms it: differences reduced modulo the mesh, kept once
        d = (Rs[None, :, :].astype(np.int64) - R[:, None, :].astype(np.int64)).reshape(-1, self._dim_k)
        pd = (Rs[None, :, :].astype(np.int64) - Rs[:, None, :].astype(np.int64)).reshape(-1, self._dim_k)
        nint = np.unique(np.mod(np.concatenate([np.zeros((1, self._dim_k), dtype=np.int64), d, -d, pd]), mesh), axis=0).shape[0]
        naint = np.union1d(st, np.arange(n) if sel is None else sel).size
        if nint > 16384 or nw * nint * naint * naint > 2 ** 23 or nw * nR * na > 2 ** 24:
            raise Exception("\n\nimpurity_ldos_mesh: %d internal lattice vectors and %d internal states at %d frequencies are beyond "
                            "the caps (nR_int <= 16384, nw * nR_int * na_int^2 <= 2**23, nw * nR * na <= 2**24): split omega or R_list."
                            % (nint, naint, nw))
        ldos0 = np.zeros((nw, na), dtype=float)
        dldos = np.zeros((nw, nR, na), dtype=float)
        _lib.check(_lib.lib.tbk_impurity_ldos_mesh(self._device_model(), _lib.iptr(mesh), nw, _lib.dptr(w), eta, ns, _lib.iptr(st),
                                                   _lib.iptr(Rs), _lib.dptr(v.view(float)), nR, _lib.iptr(R), 0 if sel is None else na,
                                                   _lib.iptr(sel), _lib.dptr(ldos0), _lib.dptr(dldos)))
        if single:
            dldos = dldos[:, 0]
        return (ldos0[0], dldos[0]) if scalar else (ldos0, dldos)

    # ------------------------------------------------------------------ band unfolding (extensions)
    def _unfold_args(self, what, k_list, sc_red_lat, prim_index, prim_orb, dense=True):
        """The checked arguments of the unfolding calls, made on the supercell model: (k (nk, dim_k) primitive reduced, K = S_per k
        the supercell's, group int32 (nsta,) with -1 for states that project on nothing, ng, the count of states per group (ng,),
        delta (norb, dim_k) or None, N_c)."""
        if self._dim_k not in (1, 2, 3):
            raise Exception("\n\n%s needs a model with dim_k 1, 2 or 3." % what)
        if dense and self._nsta > _lib.MAX_NSTA:
            raise Exception("\n\n%s: the supercell has %d states, beyond the dense solver's %d: use kpm_unfolded_spectral."
                            % (what, self._nsta, _lib.MAX_NSTA))
        try:
            k = np.array(k_list, dtype=float)
        except (TypeError, ValueError):
            raise Exception("\n\nk_list must be (nk, dim_k) k-points in the reduced coordinates of the primitive cell.")
        if self._dim_k == 1 and k.ndim == 1:
            k = k.reshape(-1, 1)
        if k.ndim != 2 or k.shape[1] != self._dim_k or k.shape[0] < 1:
            raise Exception("\n\nk_list must be (nk, dim_k) k-points in the reduced coordinates of the primitive cell.")
        if not np.all(np.isfinite(k)):
            raise Exception("\n\nk_list must be finite.")
        S = np.array(sc_red_lat)                                   # the rules of make_supercell
        if S.shape != (self._dim_r, self._dim_r):
            raise Exception("\n\nDimension of sc_red_lat array must be dim_r*dim_r")
        if S.dtype == object or not np.issubdtype(S.dtype, np.integer):
            raise Exception("\n\nsc_red_lat array elements must be integers")
        for i in range(self._dim_r):
            for j in range(self._dim_r):
                if i == j and i not in self._per and S[i, j] != 1:
                    raise Exception("\n\nDiagonal elements of sc_red_lat for non-periodic directions must equal 1.")
                if i != j and (i not in self._per or j not in self._per) and S[i, j] != 0:
                    raise Exception("\n\nOff-diagonal elements of sc_red_lat for non-periodic directions must equal 0.")
        det = np.linalg.det(S.astype(float))
        if not det > 1.0E-6:
            raise Exception("\n\nsc_red_lat must have a positive determinant (a right handed super-cell of non-zero volume).")
        nc = int(round(det))
        norb, nspin = self._norb, self._nspin
        if prim_index is None:
            if norb % nc != 0:
                raise Exception("\n\nprim_index: the model has %d orbitals, not a multiple of the %d primitive cells of sc_red_lat "
                                "(orbitals were removed or added): give prim_index, the primitive orbital of every orbital." % (norb, nc))
            pi = np.arange(norb) % (norb // nc)
        else:
            pi = np.asarray(prim_index)
            if pi.dtype == object or pi.ndim != 1 or pi.shape[0] != norb or not np.issubdtype(pi.dtype, np.integer):
                raise Exception("\n\nprim_index must be None or %d integers (one per orbital): the primitive orbital, or -1." % norb)
            if pi.min() < -1:
                raise Exception("\n\nprim_index: entries must be >= -1 (-1: an orbital that projects on nothing).")
            if pi.max() < 0:
                raise Exception("\n\nprim_index: at least one orbital must belong to a primitive orbital.")
            pi = pi.astype(np.int64)
        n_prim = int(pi.max()) + 1
        ng = n_prim * nspin
        if ng > 64:
            raise Exception("\n\nprim_index: %d primitive orbitals x %d spin components are ng = %d groups (at most 64)." % (n_prim, nspin, ng))
        group = np.where(pi[:, None] >= 0, pi[:, None] * nspin + np.arange(nspin)[None, :], -1).reshape(-1)
        group = np.ascontiguousarray(group, dtype=np.int32)
        count = np.bincount(group[group >= 0], minlength=ng)
        per = list(self._per)
        delta = None
        if prim_orb is not None:
            try:
                po = np.array(prim_orb, dtype=float)
            except (TypeError, ValueError):
                raise Exception("\n\nprim_orb must be None or a float array (n_prim, dim_r) = (%d, %d)." % (n_prim, self._dim_r))
            if po.shape != (n_prim, self._dim_r):
                raise Exception("\n\nprim_orb must be None or a float array (n_prim, dim_r) = (%d, %d)." % (n_prim, self._dim_r))
            if not np.all(np.isfinite(po)):
                raise Exception("\n\nprim_orb must be finite.")
            d = (self._orb @ S.astype(float))[:, per] - po[np.maximum(pi, 0)][:, per]
            d -= np.round(d)
            d[pi < 0] = 0.0
            delta = np.ascontiguousarray(d)
        K = np.ascontiguousarray(k @ S[np.ix_(per, per)].astype(float).T)
        return np.ascontiguousarray(k), K, group, ng, count, delta, nc

    def unfolded_bands(self, k_list, sc_red_lat, prim_index=None, prim_orb=None, per_state=False):
        """Extension: the bands of a supercell unfolded into the Brillouin zone of the primitive cell (the "effective band
        structure").  The call is made ON THE SUPERCELL MODEL -- the result of `make_supercell(sc_red_lat)`, edited at will
        (`set_onsite(mode="add")`, `remove_orb`, moved orbitals, added ones).  Returns `(evals, weights)`: `evals` float
        `(nsta, nk)` as `solve_all` returns it, `weights` float `(nsta, nk)`, or `(nsta, nk, ng)` with per_state=True,

            W_n,g(k) = (1 / N_c) | sum_{j in g} e^{2 pi i k.delta_j} u_n[j] |^2,      weights = sum_g W_n,g

        the weight of eigenstate n of H_sc(K) on the normalised primitive Bloch sum |k,g> of group g.

        k_list: `(nk, dim_k)` in the reduced coordinates of the PRIMITIVE cell.  sc_red_lat: the integer matrix S given to
        `make_supercell` (same rules; det > 0), N_c = det S.  The supercell is solved at K = S k (the periodic block of S),
        the same Cartesian vector, passed to the solver as is and not reduced modulo 1.  prim_index: for every supercell
        orbital the primitive orbital it is an image of, or -1 for an adatom or interstitial that projects on nothing;
        None is `arange(norb) % (norb // N_c)`, the order `make_supercell` produces (it raises when norb is no multiple of
        N_c, as after `remove_orb`).  Spinful models: state (j, s) belongs to group g = prim_index[j] * 2 + s, ng = 2 n_prim.
        prim_orb: None for an undistorted supercell (every delta_j = 0, no phase is formed), or the `(n_prim, dim_r)` orbital
        positions of the primitive cell; delta_j = orb[j] S - prim_orb[prim_index[j]], minus its rounding, along the periodic
        directions, is the displacement of orbital j from the nearest lattice image of its ideal site (so `to_home` does
        not matter).  nsta <= 2048 (beyond: `kpm_unfolded_spectral`), ng <= 64, nsta * nk * ng <= 2**24.

        sum_n W_n,g = (orbitals of group g) / N_c: 1 without vacancies.  With the identity supercell and
        `prim_index = arange(norb)`, W_n,g = |u_n[g]|^2: orbital-projected ("fat") bands of any model.

        Every sum has a fixed order and the partition of the work depends on (nsta, ng) alone: two calls give the same
        bits, and the projection adds no dependence on a point's position, chunk or neighbours -- a k-point gives the same
        bits alone and inside a longer list wherever the eigen-solver takes the same route for both (it picks its method
        from nsta and the number of points of a launch, as for `solve_all`).  The eigenvectors never leave the device."""
        k, K, group, ng, _, delta, nc = self._unfold_args("unfolded_bands", k_list, sc_red_lat, prim_index, prim_orb)
        n, nk = self._nsta, k.shape[0]
        ngo = ng if per_state else 1
        if n * nk * ngo > 2 ** 24:
            raise Exception("\n\nnsta * nk * ng must be at most 2**24: split k_list or omega.")
        ev = np.empty((n, nk), dtype=float)
        wt = np.empty((n, nk, ngo), dtype=float)
        _lib.check(_lib.lib.tbk_unfold_bands_list(self._device_model(), _lib.dptr(K), nk, ng, _lib.iptr(group),
                                                  None if delta is None else _lib.dptr(k), _lib.dptr(delta), 1.0 / nc,
                                                  1 if per_state else 0, _lib.dptr(ev), _lib.dptr(wt)))
        return ev, (wt if per_state else wt[:, :, 0])

    def unfolded_spectral(self, k_list, omega, eta, sc_red_lat, prim_index=None, prim_orb=None, per_state=False):
        """Extension: the spectral function of a supercell in the Brillouin zone of the primitive cell (the ARPES-like map),
        float `(nk, nw)`, or `(nk, nw, ng)` with per_state=True,

            A_g(k, w) = sum_n W_n,g(k) (eta / pi) / ((w - E_n)^2 + eta^2) = -(1 / pi) Im <k,g| (w + i eta - H_sc)^-1 |k,g>
            A(k, w)   = sum_g A_g(k, w)

        with the eigenpairs of H_sc(K = S k) and the weights of `unfolded_bands`, whose arguments k_list, sc_red_lat,
        prim_index and prim_orb it shares; it is called on the supercell model.  For an unedited supercell A_g is the
        spectral function of the primitive model, sum_m |u_m[g](k)|^2 L_eta(w - E_m(k)); k and k + any integer vector give the
        same A.  omega: a scalar (the w axis is dropped), or 1-D with 1..65536 finite values in any order, repeats allowed.
        eta: one finite number > 0.  nsta <= 2048, ng <= 64, nk * nw * ng <= 2**24 (split k_list or omega beyond).

        The Lorentzian is formed once per (band, frequency) and feeds every group; bands are added in index order.  Two
        calls give the same bits; a frequency gives the same bits alone and inside a longer list, in any place of it; a
        k-point does as in `unfolded_bands` (wherever the eigen-solver takes the same route for both list lengths).  The
        eigenvectors never leave the device: nk * nw * ng doubles come back instead of nk * nsta^2 complex components."""
        k, K, group, ng, _, delta, nc = self._unfold_args("unfolded_spectral", k_list, sc_red_lat, prim_index, prim_orb)
        w, scalar, eta = self._omega_eta_arg(omega, eta)
        nk, nw = k.shape[0], int(w.size)
        ngo = ng if per_state else 1
        if nk * nw * ngo > 2 ** 24:
            raise Exception("\n\nnk * nw * ng must be at most 2**24: split k_list or omega.")
        out = np.empty((nk, nw, ngo), dtype=float)
        _lib.check(_lib.lib.tbk_unfold_spectral_list(self._device_model(), _lib.dptr(K), nk, ng, _lib.iptr(group),
                                                     None if delta is None else _lib.dptr(k), _lib.dptr(delta), 1.0 / nc, nw,
                                                     _lib.dptr(w), eta, 1 if per_state else 0, _lib.dptr(out)))
        if not per_state:
            out = out[:, :, 0]
        return out[:, 0] if scalar else out

    def kpm_unfolded_spectral(self, k_list, energies, n_moments, sc_red_lat, prim_index=None, prim_orb=None, per_state=False,
                              kernel="jackson", bounds=None):
        """Extension: `unfolded_spectral` for supercells of any size (beyond the 2048 states of the dense solver) by the kernel
        polynomial method, float `(nk, nE)` or `(nk, nE, ng)`: A_g(k, E) = <k,g| delta(E - H_sc(K)) |k,g> from `kpm_moments`
        with the primitive Bloch sums as start vectors -- v_j = e^{-2 pi i k.delta_j} / sqrt(N_c) on the members of group g --
        multiplied back by <v|v> and reconstructed by `kpm_reconstruct` (energies, kernel and bounds as there; the
        resolution is that of the kernel, ~ pi a / n_moments for "jackson", not a Lorentzian of given eta).  Without
        prim_orb the start vectors do not depend on k and one `kpm_moments` call covers the list; else one call per k-point.
        k_list, sc_red_lat, prim_index, prim_orb as `unfolded_bands`.  Host glue over the sparse path: no dense matrix."""
        k, K, group, ng, count, delta, nc = self._unfold_args("kpm_unfolded_spectral", k_list, sc_red_lat, prim_index, prim_orb,
                                                              dense=False)
        nk, n, nspin = k.shape[0], self._nsta, self._nspin
        live = np.flatnonzero(count > 0)                           # (a group without members has A = 0 and no start vector)
        member = (group[None, :] == live[:, None]).astype(float)   # (nlive, nsta)
        norm = count[live] / float(nc)                              # <v|v>
        e = np.asarray(energies, dtype=float)
        if delta is None:
            mu, bnd = self.kpm_moments(n_moments, K, vectors=(member / np.sqrt(nc)).astype(complex), bounds=bounds)
        else:
            mu, bnd = None, None
            for q in range(nk):
                ph = np.repeat(np.exp(-2.0j * np.pi * (delta @ k[q])), nspin)
                mq, bnd = self.kpm_moments(n_moments, K[q:q + 1], vectors=np.ascontiguousarray(member * ph[None, :] / np.sqrt(nc)),
                                           bounds=bounds)
                if mu is None:
                    mu = np.empty((nk,) + mq.shape[1:], dtype=float)
                mu[q] = mq[0]
        a = kpm_reconstruct(mu * norm[None, :, None], e, bnd, kernel)   # (nk, nlive, nE)
        out = np.zeros((nk, e.size, ng), dtype=float)
        out[:, :, live] = np.transpose(a, (0, 2, 1))
        return out if per_state else out.sum(axis=2)

    # ------------------------------------------------------------------ the linear tetrahedron method (extensions)
    def _tetra_mesh_arg(self, what, mesh_size):
        if self._dim_k not in (1, 2, 3):
            raise Exception("\n\n%s needs a model with dim_k 1, 2 or 3." % what)
        mesh, nk = self._mesh_arg(mesh_size)
        if nk >= 2 ** 31:
            raise Exception("\n\n%s: the mesh must have fewer than 2**31 points." % what)
        return mesh, nk

    def tetrahedron_dos_mesh(self, mesh_size, energies, per_band=False, states=None):
        """Extension: the density of states g(E) and its integral N(E) per cell by the linear tetrahedron method (Bloechl, Jepsen,
        Andersen, PRB 49, 16223) on `k_uniform_mesh(mesh_size)` (1-, 2- or 3-D, periodic, generated on the device):
        `(dos, idos)`, each float `(nE,)`, or `(nsta, nE)` with per_band=True (a "band" is the sorted index of `solve_all`).

        Each mesh cell with origin o is cut along the fixed diagonal o -> o + (1, .., 1): in 3-D six tetrahedra, one per
        permutation (a, b, c) of the axes, with corners o, o + e_a, o + e_a + e_b, o + (1, 1, 1); in 2-D the two triangles
        (o, o + e_0, o + e_0 + e_1) and (o, o + e_1, o + e_0 + e_1); in 1-D the segment.  Every band is interpolated linearly
        inside a simplex, and theta(E - e), delta(E - e) are integrated in closed form: a continuous g(E) with its van Hove
        kinks, and an N(E) that converges like 1 / N^2 with the mesh.  The level at E counts as occupied (f = [e <= E]); a band
        that is flat over a simplex adds a step to N and nothing to g.  The fixed diagonal breaks the lattice's point symmetry
        slightly (the shortest diagonal is not chosen).  No spin factor: N above the spectrum is nsta.

        energies: 1-D, 1..65536 finite values in any order (repeats allowed).  Each result holds at most 2**22 values.

        states: None, or 1..16 distinct STATE indices in [0, nsta), read as `susceptibility_matrix_mesh` reads its `states`.
        With it a third array is returned, the projected DOS g_a(E) = sum d_i(E) |u_b(k_i)[a]|^2 over simplices, bands and
        corners: `(nsel, nE)`, or `(nsel, nsta, nE)` with per_band=True.  It costs a second solve with eigenvectors, which stay
        on the device.  Over ALL states it sums to g(E).  Where bands are degenerate at a mesh point the split of g_a between
        them follows the solver's choice of eigenvectors; their sum does not.

        Fixed-order sums: two calls give the same bits, and an energy gives the same bits alone and inside a longer list."""
        mesh, nk = self._tetra_mesh_arg("tetrahedron_dos_mesh", mesh_size)
        try:
            en = np.array(energies, dtype=float)
        except (TypeError, ValueError):
            raise Exception("\n\nenergies must be a 1-D array of 1..65536 finite values.")
        if en.ndim != 1 or en.size < 1 or en.size > 65536:
            raise Exception("\n\nenergies must be a 1-D array of 1..65536 finite values.")
        if not np.all(np.isfinite(en)):
            raise Exception("\n\nenergies must be finite.")
        en = np.ascontiguousarray(en)
        n, nE = self._nsta, int(en.size)
        nb = n if per_band else 1
        if nb * nE > 2 ** 22:
            raise Exception("\n\nnsta * nE must be at most 2**22 with per_band=True: split energies.")
        sel = None
        if states is not None:
            st = np.asarray(states)
            if st.ndim != 1 or st.size < 1 or st.size > 16 or not np.issubdtype(st.dtype, np.integer):
                raise Exception("\n\nstates must be a list of 1..16 integer state indices.")
            if st.min() < 0 or st.max() >= n or np.unique(st).size != st.size:
                raise Exception("\n\nstates must be distinct indices in [0, nsta).")
            sel = np.ascontiguousarray(st, dtype=np.int32)
            if sel.size * nb * nE > 2 ** 22:
                raise Exception("\n\nThe projected DOS holds at most 2**22 values: split energies or states.")
        dos = np.zeros((nb, nE), dtype=float)
        idos = np.zeros((nb, nE), dtype=float)
        pdos = None if sel is None else np.zeros((sel.size, nb, nE), dtype=float)
        _lib.check(_lib.lib.tbk_tetrahedron_dos_mesh(self._device_model(), _lib.iptr(mesh), nE, _lib.dptr(en), int(bool(per_band)),
                                                     0 if sel is None else int(sel.size), _lib.iptr(sel), _lib.dptr(dos),
                                                     _lib.dptr(idos), _lib.dptr(pdos)))
        if not per_band:
            dos, idos = dos[0], idos[0]
            pdos = None if pdos is None else pdos[:, 0]
        return (dos, idos) if pdos is None else (dos, idos, pdos)

    def tetrahedron_weights_mesh(self, mesh_size, fermi_level, correction=False, derivative=False):
        """Extension: the occupation weights of the linear tetrahedron method at `fermi_level`, float `(nsta, N_k)` in the order
        of `k_uniform_mesh(mesh_size)`: entry (b, k) is the sum of w_i(mu) over every simplex that has mesh point k as its
        corner i (the simplices and conventions of `tetrahedron_dos_mesh`), so that

            sum_{b,k} w[b, k] X_b(k) = the tetrahedron integral of theta(mu - E_b) X_b over the zone, per cell

        for any X given on the mesh; sum_k w[b] is the band's N(mu).  derivative=True gives the sum of d_i(mu) = dw_i / dmu
        instead: the weights of a Fermi-surface integral, sum_k of which is the band's g(mu).  correction=True (dim_k = 3 only,
        not together with derivative) adds Bloechl's curvature correction (1 / 40) g_T(mu) sum_j (e_j - e_i) per tetrahedron,
        which sums to zero over the corners: N is unchanged.  Eigenvalues only.  Two calls give the same bits."""
        mesh, nk = self._tetra_mesh_arg("tetrahedron_weights_mesh", mesh_size)
        try:
            fermi_level = float(fermi_level)
        except (TypeError, ValueError):
            raise Exception("\n\nfermi_level must be one finite number.")
        if not np.isfinite(fermi_level):
            raise Exception("\n\nfermi_level must be finite.")
        if correction and self._dim_k != 3:
            raise Exception("\n\ncorrection=True needs dim_k = 3: the curvature correction is that of tetrahedra.")
        if correction and derivative:
            raise Exception("\n\ncorrection=True applies to the occupation weights, not to derivative=True.")
        if self._nsta * nk > 2 ** 31:
            raise Exception("\n\nnsta * N_k must be at most 2**31 weights.")
        out = np.zeros((self._nsta, nk), dtype=float)
        _lib.check(_lib.lib.tbk_tetrahedron_weights_mesh(self._device_model(), _lib.iptr(mesh), fermi_level, int(bool(correction)),
                                                         int(bool(derivative)), _lib.dptr(out)))
        return out

    def tetrahedron_fermi_level_mesh(self, mesh_size, n_electrons):
        """Extension: the T = 0 Fermi level that puts `n_electrons` electrons per cell (one real number, no spin factor) into
        the tetrahedron-method N(E) of `tetrahedron_dos_mesh`, from ONE eigen-solve of the mesh.

        If n_electrons is within 1e-9 of an integer m in [1, nsta - 1] and band m - 1 lies wholly below band m
        (max_k E_{m-1} < min_k E_m on the mesh), the result is the middle of that gap.  Otherwise 0 < n_electrons < nsta is
        required, and the result is the first double at which the device's own N(mu) reaches n_electrons, found by rounds of up
        to 256 trial energies per launch between the lowest and the highest level of the mesh (eight or nine rounds).  Unlike
        `fermi_level_mesh` at kT = 0 the level of a metal does not jump from mesh level to mesh level.  Where N is flat (touching
        bands at an integer filling, a Dirac point) mu is only as determined as N is.  Two calls give the same bits."""
        mesh, nk = self._tetra_mesh_arg("tetrahedron_fermi_level_mesh", mesh_size)
        try:
            nel = float(n_electrons)
        except (TypeError, ValueError):
            raise Exception("\n\nn_electrons must be one finite number.")
        if not np.isfinite(nel):
            raise Exception("\n\nn_electrons must be finite.")
        if not 0.0 < nel < self._nsta:
            raise Exception("\n\nn_electrons must lie in the open interval (0, %d)." % self._nsta)
        mu = np.zeros(1, dtype=float)
        _lib.check(_lib.lib.tbk_tetrahedron_fermi_level_mesh(self._device_model(), _lib.iptr(mesh), nel, _lib.dptr(mu)))
        return float(mu[0])

    # ------------------------------------------------------------------ shift and injection photocurrents (extensions)
    def _gen_ddham(self, k_input, dir0, dir1):
        """Extension: d^2 H / dk_dir0 dk_dir1 for one k in reduced coordinates, with the shapes of `_gen_ham` (`(norb, 2, norb, 2)`
        for spinful models): sum t (2 pi i)^2 (R + tau_j - tau_i)_dir0 (R + tau_j - tau_i)_dir1 e^{2 pi i k.(R + tau_j - tau_i)}.
        The twin of `_gen_dham`; dir0 == dir1 is allowed."""
        if self._dim_k < 1:
            raise Exception("\n\n_gen_ddham needs a model with dim_k >= 1")
        for d in (dir0, dir1):
            if not _is_int(d) or d < 0 or d >= self._dim_k:
                raise Exception("\n\n_gen_ddham: dir0 and dir1 must be axes in [0, dim_k)")
        kp = np.array(k_input, dtype=float)
        if kp.ndim == 0:
            kp = kp.reshape(1)
        if kp.shape != (self._dim_k,):
            raise Exception("\n\nk-vector of wrong shape!")
        k = np.ascontiguousarray(kp.reshape(1, -1))
        n = self._nsta
        out = np.zeros((1, n, n), dtype=complex)
        _lib.check(_lib.lib.tbk_gen_ddham(self._device_model(), _lib.dptr(k), 1, int(dir0), int(dir1),
                                          _lib.dptr(out.view(float))))
        if self._nspin == 1:
            return out[0]
        return out[0].reshape(self._norb, 2, self._norb, 2)

    def _dirs3_arg(self, dirs, what):
        """Checked (a, b, c) of the photocurrent calls: three integer axes in [0, dim_k), repeats allowed."""
        dirs = list(dirs)
        if len(dirs) != 3 or not all(_is_int(d) for d in dirs):
            raise Exception("\n\ndirs must be three integer axes.")
        if min(dirs) < 0 or max(dirs) >= self._dim_k:
            raise Exception("\n\nDirection for the %s out of bounds." % what)
        return int(dirs[0]), int(dirs[1]), int(dirs[2])

    def shift_current(self, k_list, occ, dirs):
        """Extension: the k-resolved shift-current transition strength at every k of `k_list` (reduced coordinates, as
        solve_all), float64 `(nk,)`:

            sum_{n in occ, m not in occ, G(n) != G(m)} Im X^{abc}_nm,   X^{abc}_nm = r^b_mn r^c_nm;a + r^c_mn r^b_nm;a,

        (a, b, c) = dirs (axes may repeat), `occ` a NumPy index of bands as in `berry_curvature`.  r^b_nm = -i V^b_nm / E_nm
        is the interband connection and r^b_nm;a its generalized derivative by the sum rule of `shift_current_mesh`, with
        the same groups G.  Needs dim_k >= 1."""
        if self._dim_k < 1:
            raise Exception("\n\nThe shift current needs a model with dim_k >= 1.")
        a, b, c = self._dirs3_arg(dirs, "shift current")
        sel = np.atleast_1d(np.arange(self._nsta)[occ]).ravel()
        if sel.size == 0:
            raise Exception("\n\nocc selects no band.")
        if np.unique(sel).size != sel.size:
            raise Exception("\n\nocc lists a band twice.")
        sel = np.ascontiguousarray(sel, dtype=np.int32)
        k = self._k_array(k_list)
        nk = k.shape[0]
        out = np.zeros(nk, dtype=float)
        if nk == 0 or self._nsta == 1:
            return out
        _lib.check(_lib.lib.tbk_shift_list(self._device_model(), _lib.dptr(k), nk, a, b, c, _lib.iptr(sel), len(sel),
                                           _lib.dptr(out)))
        return out

    def _photocurrent_mesh(self, kind, what, mesh_size, omega, eta, fermi_level, kT, dirs, cartesian):
        if self._dim_k not in (1, 2, 3):
            raise Exception("\n\n%s needs a model with dim_k 1, 2 or 3." % what)
        mesh, nk = self._mesh_arg(mesh_size)
        w = _sweep_args(omega, eta, fermi_level, kT)
        if dirs is None:
            a = b = c = -1
        else:
            a, b, c = self._dirs3_arg(dirs, "photocurrent")
            if cartesian:
                raise Exception("\n\ncartesian=True returns the whole tensor: give dirs=None.")
        dk = self._dim_k
        out = np.zeros((w.size, dk, dk, dk) if a < 0 else (w.size,), dtype=complex if kind else float)
        if self._nsta > 1:
            _lib.check(_lib.lib.tbk_photocurrent_mesh(self._device_model(), _lib.iptr(mesh), int(kind), int(w.size),
                                                      _lib.dptr(w), float(eta), float(fermi_level), float(kT), a, b, c,
                                                      _lib.dptr(out.view(float))))
        if not cartesian:
            return out
        lat = np.array(self._lat, dtype=float)[self._per]             # (dim_k, dim_r)
        vc = np.sqrt(np.linalg.det(lat @ lat.T))
        pref = (0.5 * np.pi if kind == 0 else 1.0) / ((2.0 * np.pi) ** 3 * vc)
        return pref * np.einsum("ax,by,cz,wabc->wxyz", lat, lat, lat, out)

    def shift_current_mesh(self, mesh_size, omega, eta, fermi_level=0.0, kT=0.0, dirs=None, cartesian=False):
        """Extension: the shift-current response -- the interband second-order (bulk photovoltaic) response to linearly
        polarised light -- averaged over the whole `k_uniform_mesh(mesh_size)` (1-, 2- or 3-D, generated on the device):

            K_abc(w) = mean_k sum_{E_m > E_n, G(n) != G(m)} (f_n - f_m) Im X^{abc}_nm D(E_m - E_n, w)
            X^{abc}_nm = r^b_mn r^c_nm;a + r^c_mn r^b_nm;a
            D(eps, w) = (eta / pi) [1 / ((eps - w)^2 + eta^2) + 1 / ((eps + w)^2 + eta^2)]

        k reduced, H the matrix of `_gen_ham`, V^a = dH/dk_a (`_gen_dham`), W^{ab} = d^2H/dk_a dk_b (`_gen_ddham`), E_n and
        |n> the eigenpairs of `solve_all`, E_nm = E_n - E_m, f as in `optical_conductivity_mesh`.  G(n) is the group of band
        n: a maximal run of consecutive levels, each within 1e-9 max(1, |E|, |E'|) of its predecessor (the rule of
        `anomalous_transport_mesh`).  r^b_nm = -i V^b_nm / E_nm for G(n) != G(m) and 0 inside a group, and the generalized
        derivative follows from the sum rule

            r^b_nm;a = (i / E_nm) [T^{ba}_nm / E_nm - W^{ba}_nm + sum_{p not in G(n) u G(m)} (V^b_np V^a_pm / E_pm - V^a_np V^b_pm / E_np)]
            T^{ba}_nm = sum_{p in G(n)} (V^a_np V^b_pm + V^b_np V^a_pm) - sum_{p in G(m)} (V^b_np V^a_pm + V^a_np V^b_pm)

        (groups of one: T^{ba}_nm = V^b_nm D^a_nm + V^a_nm D^b_nm, D^a_nm = V^a_nn - V^a_mm, the sum rule of Sipe and
        Shkrebtii, Phys. Rev. B 61, 5337 (2000)).  The sums over (n in G1, m in G2) do not depend on the solver's choice of
        eigenvectors inside a group -- Kramers points, spin-doubled models.  For a model whose in-group velocity blocks are
        not multiples of the identity at every k (PT-symmetric antiferromagnets with spin-orbit coupling), nothing beyond
        that independence has been validated.

        omega, eta, fermi_level, kT: the rules of `optical_conductivity_mesh`.  dirs=None -> real `(nw, dim_k, dim_k, dim_k)`;
        dirs=(a, b, c) (axes may repeat) -> `(nw,)`.  K is symmetric in b <-> c and even in w, and vanishes with inversion
        symmetry.  cartesian=True (dirs=None only) returns
        sigma^{xyz} = (pi / 2) sum_abc A_ax A_by A_cz K_abc / ((2 pi)^3 V_c), `(nw, dim_r, dim_r, dim_r)`, in units of
        e^3/hbar^2 x length^(3 - dim_k), A and V_c as in `optical_conductivity_mesh`; for b = c this is the standard
        sigma^{abb} = (pi e^3 / hbar^2) int [dk] sum f_nm Im[r^b_mn r^b_nm;a] delta(w_mn - w).  No spin-degeneracy factor.  A
        one-state model, or kT = 0 with the Fermi level below or above every level, gives exact zeros.  Fixed reduction
        order: two calls give the same bits."""
        return self._photocurrent_mesh(0, "shift_current_mesh", mesh_size, omega, eta, fermi_level, kT, dirs, cartesian)

    def injection_current_mesh(self, mesh_size, omega, eta, fermi_level=0.0, kT=0.0, dirs=None, cartesian=False):
        """Extension: the injection-current response, with the signature, the conventions and the groups G of
        `shift_current_mesh`:

            N_abc(w) = mean_k sum_{E_m > E_n, G(n) != G(m)} (f_n - f_m) Y^{abc}_nm D(E_m - E_n, w)
            Y^{abc}_nm = sum_{m' in G(m)} V^a_mm' r^c_m'n r^b_nm - sum_{n' in G(n)} r^c_mn V^a_nn' r^b_n'm

        (groups of one: Y^{abc}_nm = (V^a_mm - V^a_nn) r^b_nm r^c_mn).  Complex, `(nw, dim_k, dim_k, dim_k)` or `(nw,)`;
        N_acb = conj N_abc.  Re N is the linear (magnetic) injection, which vanishes with time reversal; Im N is the
        circular injection, which needs broken inversion.  Physical prefactor: the injection rate of the current is
        d j^a / dt = eta^{abc}(w) E_b(w) E_c(-w) with eta^{abc} = (pi e^3 / 2 hbar^2) int [dk] sum_{nm} f_nm D^a_mn r^c_mn r^b_nm
        delta(w_mn - w), D^a_mn = V^a_mm - V^a_nn: the product form of Sipe and Shkrebtii, Phys. Rev. B 61, 5337 (2000),
        eq. (57), whose commutator [r^c_mn, r^b_nm] keeps the part antisymmetric in b <-> c (2i Im N, the circular
        injection); the symmetric part is the magnetic injection.  So eta^{abc} = (pi e^3 / 2 hbar^2) N_abc after the
        reduced-to-Cartesian transform.  cartesian=True (dirs=None only)
        applies the rank-3 transform of `shift_current_mesh` without the pi / 2:
        sum_abc A_ax A_by A_cz N_abc / ((2 pi)^3 V_c).  The same documented limit for in-group velocity blocks applies."""
        return self._photocurrent_mesh(1, "injection_current_mesh", mesh_size, omega, eta, fermi_level, kT, dirs, cartesian)

    # ------------------------------------------------------------------ orbital magnetization (extensions)
    def orbital_moment(self, k_list, occ=None, dirs=(0, 1)):
        """Extension: the orbital moment by the Kubo formula at every k of `k_list` (reduced coordinates, as solve_all).

        (a, b) = dirs, V^d = dH/dk_d (`_gen_dham`), E_n and |n> the eigenpairs of `solve_all`, P_nm = Im V^a_nm V^b_mn.
        occ=None: per band, float64 `(nsta, nk)`, m_n(k) = sum_{m != n} P_nm / (E_m - E_n); a pair with
            |E_n - E_m| <= 1e-9 max(1, |E_n|, |E_m|) contributes to neither band (the rule of `berry_curvature`).  A two-state
            model has m_0 = m_1 = (E_0 - E_1) Omega_0 / 2, Omega_0 of `berry_curvature`.
        occ given (a NumPy index of bands): the gauge-invariant sum of that band set, `(nk,)`, LC(k) + IC(k) with
            LC = sum_{n in occ, m not in occ} P_nm E_m / (E_n - E_m)^2 and IC = (same) P_nm E_n / (E_n - E_m)^2 (no
            degeneracy rule).  Its mean over a mesh is the band-set part of `orbital_magnetization_mesh`.
        Reduced units (energy x the reduced curvature); `orbital_magnetization_mesh` gives the conversion."""
        sel, d0, d1 = self._curv_args(occ, dirs, "orbital moment")
        k = self._k_array(k_list)
        nk = k.shape[0]
        out = np.zeros(nk if sel is not None else (self._nsta, nk), dtype=float)
        if nk == 0:
            return out
        _lib.check(_lib.lib.tbk_orb_moment_list(self._device_model(), _lib.dptr(k), nk, d0, d1, _lib.iptr(sel),
                                                0 if sel is None else len(sel), _lib.dptr(out)))
        return out

    def orbital_magnetization_mesh(self, mesh_size, occ=None, fermi_levels=None, kT=0.0, dirs=(0, 1)):
        """Extension: the orbital magnetization by the Kubo formula, as means over `k_uniform_mesh(mesh_size)` (2-D or 3-D,
        generated on the device).  Give exactly one of occ and fermi_levels.

        occ given: float64 `(3,)` = (mean LC, mean IC, mean Omega_occ) of `orbital_moment(occ=...)`'s terms, with
            Omega_occ = -2 sum_{n in occ, m not in occ} P_nm / (E_n - E_m)^2 (`berry_curvature_mesh(occ)`).  For mu in the gap
            above the set, M(mu) = LC + IC + mu Omega_occ, so dM/dmu = 2 pi C (the Streda formula).
        fermi_levels (1-D, 1..8192 finite values, any order): M(mu), `(nmu,)` in input order,
            kT = 0:  M(mu) = mean_k sum_{n: E_n <= mu} [m_n + (mu - E_n) Omega_n] = A(mu) + mu I(mu), m_n of `orbital_moment`,
                     Omega_n of `berry_curvature`, I(mu) of `berry_curvature_mesh(fermi_levels=...)`.  Pairs of occupied bands
                     cancel only in exact arithmetic, so near-degenerate occupied pairs cost precision, as in that scan.
            kT > 0:  M(mu, T) = mean_k sum_n [f_n m_n + g_n Omega_n], f_n = 1 / (1 + e^x), g_n = kT ln(1 + e^-x),
                     x = (E_n - mu) / kT (Xiao et al., PRL 97, 026603); it tends to the kT = 0 form as kT -> 0.
        3-D mesh: every result gains a trailing axis over the mesh direction that is not in dirs, one plane per slice (a sheet
        value per slice).
        Units and sign: for dirs = (0, 1) of a 2-D cell with a1 x a2 along +z, the orbital magnetization per area of particles
        of charge q is M_z = -(q / hbar) M / (2 pi)^2, with M in the model's energy unit.  The reductions have a fixed order,
        so two calls give the same bits."""
        sel, d0, d1 = self._curv_args(occ, dirs, "orbital magnetization")
        mesh, nk = self._mesh_arg(mesh_size)
        if self._dim_k not in (2, 3):
            raise Exception("\n\norbital_magnetization_mesh needs a 2-D or 3-D mesh.")
        kT = float(kT)
        if not np.isfinite(kT) or not kT >= 0.0:
            raise Exception("\n\nkT must be finite and >= 0.")
        if (sel is None) == (fermi_levels is None):
            raise Exception("\n\nGive exactly one of occ and fermi_levels.")
        if kT > 0.0 and fermi_levels is None:
            raise Exception("\n\nkT > 0 needs fermi_levels.")
        mu = None
        if fermi_levels is not None:
            mu = np.ascontiguousarray(np.array(fermi_levels, dtype=float))
            if mu.ndim != 1 or mu.size < 1 or mu.size > 8192:
                raise Exception("\n\nfermi_levels must be a 1-D array of 1..8192 levels.")
            if not np.all(np.isfinite(mu)):
                raise Exception("\n\nfermi_levels must be finite.")
        nch = 3 if sel is not None else mu.size
        nslice = 1 if self._dim_k == 2 else int(mesh[3 - d0 - d1])
        out = np.zeros((nch, nslice), dtype=float)
        _lib.check(_lib.lib.tbk_orb_mag_mesh(self._device_model(), _lib.iptr(mesh), d0, d1, _lib.iptr(sel),
                                             0 if sel is None else len(sel), 0 if mu is None else mu.size, _lib.dptr(mu), kT,
                                             _lib.dptr(out)))
        return out[:, 0] if self._dim_k == 2 else out

    # ------------------------------------------------------------------ Fermi-surface transport (extensions)
    @staticmethod
    def _thermal_args(fermi_levels, kT):
        """Checked (levels as a float64 array, kT) of the thermal scans: 1..8192 finite levels in any order, kT finite and > 0."""
        try:
            kT = float(kT)
        except (TypeError, ValueError):
            raise Exception("\n\nkT must be finite and > 0.")
        if not np.isfinite(kT) or not kT > 0.0:
            raise Exception("\n\nkT must be finite and > 0.")
        mu = np.array(fermi_levels, dtype=float)
        if mu.ndim != 1 or mu.size < 1 or mu.size > 8192:
            raise Exception("\n\nfermi_levels must be a 1-D array of 1..8192 levels.")
        if not np.all(np.isfinite(mu)):
            raise Exception("\n\nfermi_levels must be finite.")
        return np.ascontiguousarray(mu), kT

    def band_velocity(self, k_list, dirs=None):
        """Extension: the band velocities v^c_n(k) = <n|dH/dk_c|n> at every k of `k_list` (reduced coordinates, as solve_all;
        dim_k >= 1), |n> the eigenvectors of `solve_all` and dH/dk_c of `_gen_dham`.

        dirs=None: every axis, float64 `(dim_k, nsta, nk)`; dirs an integer axis: `(nsta, nk)`.
        For an isolated band this is the derivative of `solve_all`'s eigenvalue with respect to the reduced k_c
        (Hellmann-Feynman).  It is the raw diagonal element: inside a group of degenerate levels (the pair rule of
        `berry_curvature` applied to neighbouring levels) the eigenvectors are the solver's choice, and only the sum of the
        group's velocities is defined -- `anomalous_transport_mesh` and `drude_weight_mesh` use the group forms.
        Cartesian velocities are v A / (2 pi) with A the periodic lattice vectors as rows."""
        if self._dim_k < 1:
            raise Exception("\n\nThe band velocity needs a model with dim_k >= 1.")
        if dirs is not None and (not _is_int(dirs) or dirs < 0 or dirs >= self._dim_k):
            raise Exception("\n\ndirs must be None (every axis) or one integer axis in [0, dim_k).")
        k = self._k_array(k_list)
        nk = k.shape[0]
        n, dk = self._nsta, self._dim_k
        out = np.zeros((dk, n, nk) if dirs is None else (n, nk), dtype=float)
        if nk == 0:
            return out
        _lib.check(_lib.lib.tbk_band_velocity_list(self._device_model(), _lib.dptr(k), nk, -1 if dirs is None else int(dirs),
                                                   _lib.dptr(out)))
        return out

    def anomalous_transport_mesh(self, mesh_size, fermi_levels, kT, dirs=(0, 1)):
        """Extension: the thermal anomalous-Hall and Nernst integrals and the Berry curvature dipole, as means over
        `k_uniform_mesh(mesh_size)` (2-D or 3-D, generated on the device), for many Fermi levels at once.

        fermi_levels: 1-D, 1..8192 finite values in any order; kT finite and > 0.  With x = (E_n - mu) / kT,
        f = 1 / (1 + e^x), s = -f ln f - (1 - f) ln(1 - f) and Omega_n of `berry_curvature(dirs=dirs)`, the tuple
        (hall, nernst, dipole), each in input order of the levels:
            hall `(nmu,)`           = mean_k sum_n f_n Omega_n
            nernst `(nmu,)`         = mean_k sum_n s_n Omega_n
            dipole `(dim_k, nmu)`   = mean_k sum_n (-df/dE)_n Omega_n vbar^c_n,  c = 0 .. dim_k - 1,
        vbar^c_n the mean of <m|dH/dk_c|m> over the group of levels degenerate with n (`band_velocity` for an isolated band): a
        group's sum does not depend on the solver's eigenvectors, e.g. at the Kramers points of a time-reversal-symmetric model.
        3-D mesh: every result gains a trailing axis over the mesh direction that is not in dirs, one plane per slice.
        Identities: dipole[c] = mean_k sum_n f_n dOmega_n/dk_c (integration by parts), d nernst / d mu = d hall / d kT, and
        hall -> `berry_curvature_mesh(fermi_levels=...)` as kT -> 0 (nernst and dipole -> 0 in a gap).  A time-reversal-symmetric
        model has hall = nernst = 0 and, without inversion, a dipole; a C3-symmetric 2-D model has no dipole.
        Units, in the sign convention of `berry_curvature_mesh`: sigma_xy = -(e^2/h) hall / (2 pi) per layer; the anomalous
        Nernst (Peltier) coefficient alpha_xy = -(k_B e / h) nernst / (2 pi), i.e. alpha_xy / sigma_xy = (k_B / e) nernst / hall
        (Xiao et al., PRL 97, 026603); the Cartesian dipole of a 2-D cell with dirs
        spanning it is D_x = dipole A / (2 pi)^2 (a length), A the periodic lattice vectors as rows.
        Fixed-order reductions: two calls give the same bits."""
        _, d0, d1 = self._curv_args(None, dirs, "anomalous transport")
        mesh, nk = self._mesh_arg(mesh_size)
        if self._dim_k not in (2, 3):
            raise Exception("\n\nanomalous_transport_mesh needs a 2-D or 3-D mesh.")
        mu, kT = self._thermal_args(fermi_levels, kT)
        dk = self._dim_k
        nslice = 1 if dk == 2 else int(mesh[3 - d0 - d1])
        out = np.zeros((2 + dk, mu.size, nslice), dtype=float)
        _lib.check(_lib.lib.tbk_anom_transport_mesh(self._device_model(), _lib.iptr(mesh), d0, d1, int(mu.size), _lib.dptr(mu), kT,
                                                    _lib.dptr(out)))
        if dk == 2:
            out = out[:, :, 0]
        return out[0], out[1], out[2:]

    def drude_weight_mesh(self, mesh_size, fermi_levels, kT, cartesian=False):
        """Extension: the Drude weight tensor, the mean over the whole `k_uniform_mesh(mesh_size)` (1-, 2- or 3-D, generated on
        the device), for many Fermi levels at once: float64 `(nmu, dim_k, dim_k)` in input order of the levels,

            D_cd(mu) = mean_k sum_n (-df/dE)_n w^{cd}_n,   w^{cd}_n = sum_{m in G(n)} Re <n|dH/dk_c|m><m|dH/dk_d|n>,

        G(n) the group of levels degenerate with n (w = v^c_n v^d_n of `band_velocity` for an isolated band), f the Fermi
        function at kT > 0 (finite); fermi_levels 1-D, 1..8192 finite values in any order.  The pairs inside a group are
        exactly the ones `optical_conductivity_mesh` leaves out, so D is its intraband complement: real, symmetric, with a
        non-negative diagonal, and D_cd = mean_k sum_n f_n d^2 E_n / dk_c dk_d for non-degenerate bands.
        cartesian=True returns A^T D A / ((2 pi)^2 V_c), `(nmu, dim_r, dim_r)`, with the A and V_c of
        `optical_conductivity_mesh`: the weight of sigma(w) = i D / (w + i 0) in e^2/hbar x length^(2 - dim_k).
        Fixed-order reductions: two calls give the same bits."""
        if self._dim_k not in (1, 2, 3):
            raise Exception("\n\ndrude_weight_mesh needs a model with dim_k 1, 2 or 3.")
        if not isinstance(cartesian, (bool, np.bool_)):
            raise Exception("\n\ncartesian must be True or False.")
        mesh, nk = self._mesh_arg(mesh_size)
        mu, kT = self._thermal_args(fermi_levels, kT)
        dk = self._dim_k
        tri = np.zeros((mu.size, dk * (dk + 1) // 2), dtype=float)
        _lib.check(_lib.lib.tbk_drude_mesh(self._device_model(), _lib.iptr(mesh), int(mu.size), _lib.dptr(mu), kT, _lib.dptr(tri)))
        out = np.zeros((mu.size, dk, dk), dtype=float)
        iu = np.triu_indices(dk)
        out[:, iu[0], iu[1]] = tri
        out[:, iu[1], iu[0]] = tri
        if not cartesian:
            return out
        a = np.array(self._lat, dtype=float)[self._per]               # (dim_k, dim_r)
        vc = np.sqrt(np.linalg.det(a @ a.T))
        return np.einsum("ia,wij,jb->wab", a, out, a) / ((2.0 * np.pi) ** 2 * vc)

    # ------------------------------------------------------------------ real-time propagation under a uniform field (extensions)
    def _shift_dt_args(self, what, shift, dt):
        """(shift as a contiguous float64 `(nt + 1, dim_k)` array, nt, dt) of the propagation calls: dim_k 1, 2 or 3, 1 <= nt <=
        65536, every shift finite, dt finite and > 0."""
        if self._dim_k not in (1, 2, 3):
            raise Exception("\n\n%s needs a model with dim_k 1, 2 or 3." % what)
        try:
            kap = np.array(shift, dtype=float)
        except (TypeError, ValueError):
            raise Exception("\n\nshift must be a real array of shape (nt + 1, dim_k).")
        if self._dim_k == 1 and kap.ndim == 1:
            kap = kap.reshape(-1, 1)
        if kap.ndim != 2 or kap.shape[1] != self._dim_k:
            raise Exception("\n\nshift must have shape (nt + 1, dim_k): the shift of k at the times j * dt, j = 0 .. nt.")
        if kap.shape[0] < 2 or kap.shape[0] > 65537:
            raise Exception("\n\nshift must hold the shifts at nt + 1 times with 1 <= nt <= 65536.")
        if not np.all(np.isfinite(kap)):
            raise Exception("\n\nshift must be finite.")
        try:
            dt = float(dt)
        except (TypeError, ValueError):
            raise Exception("\n\ndt must be finite and > 0.")
        if not np.isfinite(dt) or not dt > 0.0:
            raise Exception("\n\ndt must be finite and > 0.")
        return np.ascontiguousarray(kap), kap.shape[0] - 1, dt

    _TD_STATE_CAP = 2 ** 26

    def propagate_mesh(self, mesh_size, shift, dt, occ=None, fermi_level=None, kT=0.0, cartesian=False, return_populations=False,
                       return_k_populations=False):
        """Extension: the crystal in a uniform time-dependent field, propagated in real time on `k_uniform_mesh(mesh_size)` (1-, 2-
        or 3-D, generated on the device): `(current (nt + 1, dim_k), energy (nt + 1,))` per cell, hbar = e = 1.

        Velocity gauge: the field is a rigid shift of every k-point, k -> k + shift(t); `shift` `(nt + 1, dim_k)` holds it at the
        times t_j = j * dt in reduced coordinates (kappa = -A(t) . a_i / 2 pi for a vector potential A and an electron of charge
        -1; `laser_shift` builds common pulses).  H and dH/dk_a are the matrices of `_gen_ham` and `_gen_dham`.
        Start: the eigenvectors of `solve_all` at k + shift[0] -- the bands `occ` (a NumPy index, as `berry_curvature` reads it),
        each with weight 1, or every band with the Fermi weight f_n of (`fermi_level`, `kT`) in the conventions of
        `thermodynamics_mesh` (no spin factor; f = [E <= mu] at kT = 0).  Exactly one of occ / fermi_level must be given.
        States whose weight is exactly 0 are not carried.
        Step j -> j + 1: psi <- V exp(-i E dt) V^+ psi with the eigenpairs of H(k + (shift[j] + shift[j + 1]) / 2), the exponential
        midpoint rule: exactly unitary, second order in dt, independent of the solver's basis inside a degenerate group.
        At every t_j, j = 0 included:
            current[j, a] = (1 / N_k) sum_k sum_n f_n <psi_n| dH/dk_a (k + shift[j]) |psi_n>,    energy[j] = the same with H.
        cartesian=True maps the current as `band_velocity` documents: J A / (2 pi), `(nt + 1, dim_r)`.  With shift advancing by a
        reciprocal vector along axis a over the run, int J_b dt / (2 pi) of a filled band is its pumped charge.

        return_populations / return_k_populations append pop `(nsta,)` and kpop `(nsta, N_k)`: p_n(k) = sum_m f_m
        |<u_n(k + shift[-1])|psi_m>|^2 with the eigenvectors of `solve_all` at the last time, and its mesh mean.  Inside a group
        of degenerate levels the eigenvectors are the solver's choice and only the group's sum is defined, as for `band_velocity`.

        The states stay on the device for the whole call: N_k * nprop * nsta <= 2**26 (nprop = the bands of occ, or nsta).
        Fixed-order sums: two calls give the same bits, and the leading nt' + 1 shifts alone give the bits of the first nt' + 1
        entries."""
        kap, nt, dt = self._shift_dt_args("propagate_mesh", shift, dt)
        mesh, nk = self._mesh_arg(mesh_size)
        if (occ is None) == (fermi_level is None):
            raise Exception("\n\nGive exactly one of occ (a band set) and fermi_level (Fermi weights).")
        if not isinstance(cartesian, (bool, np.bool_)):
            raise Exception("\n\ncartesian must be True or False.")
        n, dk = self._nsta, self._dim_k
        sel, mu = None, 0.0
        if occ is not None:
            sel = np.atleast_1d(np.arange(n)[occ]).ravel()
            if sel.size == 0:
                raise Exception("\n\nocc selects no band.")
            if np.unique(sel).size != sel.size:
                raise Exception("\n\nocc lists a band twice.")
            sel = np.ascontiguousarray(sel, dtype=np.int32)
            kT = 0.0
        else:
            try:
                mu = float(fermi_level)
            except (TypeError, ValueError):
                raise Exception("\n\nfermi_level must be one finite number.")
            if not np.isfinite(mu):
                raise Exception("\n\nfermi_level must be finite.")
            try:
                kT = float(kT)
            except (TypeError, ValueError):
                raise Exception("\n\nkT must be finite and >= 0.")
            if not np.isfinite(kT) or not kT >= 0.0:
                raise Exception("\n\nkT must be finite and >= 0.")
        nprop = n if sel is None else int(sel.size)
        if nk * nprop * n > self._TD_STATE_CAP:
            raise Exception("\n\npropagate_mesh keeps N_k * nprop * nsta = %d complex numbers on the device (at most 2**26): "
                            "coarsen the mesh or select fewer bands (occ)." % (nk * nprop * n))
        cur = np.zeros((nt + 1, dk), dtype=float)
        en = np.zeros(nt + 1, dtype=float)
        want = bool(return_populations) or bool(return_k_populations)
        pop = np.zeros(n, dtype=float) if want else None
        kpop = np.zeros((n, nk), dtype=float) if want else None
        _lib.check(_lib.lib.tbk_propagate_mesh(self._device_model(), _lib.iptr(mesh), nt, _lib.dptr(kap), dt,
                                               0 if sel is None else len(sel), _lib.iptr(sel), mu, kT, _lib.dptr(cur), _lib.dptr(en),
                                               _lib.dptr(pop), _lib.dptr(kpop)))
        if cartesian:
            cur = cur @ np.array(self._lat, dtype=float)[self._per] / (2.0 * np.pi)
        out = (cur, en)
        if return_populations:
            out += (pop,)
        if return_k_populations:
            out += (kpop,)
        return out

    def floquet_propagator(self, k_list, shift, dt):
        """Extension: the propagator of the steps of `propagate_mesh` at every k of `k_list` (reduced coordinates, as solve_all),
        started from the identity: complex `(nk, nsta, nsta)`,

            U(k) = prod_j exp(-i H(k + (shift[j] + shift[j + 1]) / 2) dt),   j = nt - 1 .. 0 from the left,   U[k, i, j] = <i|U|j>,

        exactly unitary.  Spinful models return `(nk, norb, 2, norb, 2)`, as `_gen_ham` does.  nk * nsta**2 <= 2**26."""
        kap, nt, dt = self._shift_dt_args("floquet_propagator", shift, dt)
        try:
            k = np.array(k_list, dtype=float)
        except (TypeError, ValueError):
            raise Exception("\n\nk_list must be a real array of shape (nk, dim_k).")
        if self._dim_k == 1 and k.ndim == 1:
            k = k.reshape(-1, 1)
        if k.ndim != 2 or k.shape[1] != self._dim_k or k.shape[0] < 1 or not np.all(np.isfinite(k)):
            raise Exception("\n\nk_list must have shape (nk, dim_k) with at least one k-point, all finite.")
        k = np.ascontiguousarray(k)
        nk, n = k.shape[0], self._nsta
        if nk * n * n > self._TD_STATE_CAP:
            raise Exception("\n\nfloquet_propagator keeps nk * nsta**2 = %d complex numbers on the device (at most 2**26): split k_list."
                            % (nk * n * n))
        out = np.zeros((nk, n, n), dtype=complex)
        _lib.check(_lib.lib.tbk_propagator_list(self._device_model(), _lib.dptr(k), nk, nt, _lib.dptr(kap), dt, _lib.dptr(out.view(float))))
        if self._nspin == 2:
            out = out.reshape(nk, self._norb, 2, self._norb, 2)
        return out

    def floquet_bands(self, k_list, shift, dt):
        """Extension: the quasi-energies of a periodically driven model, float `(nsta, nk)` (the layout of `solve_all`), ascending,

            eps_n(k) = -arg(lambda_n) / T  in  (-pi / T, pi / T],   T = nt * dt,   lambda_n the eigenvalues of `floquet_propagator`.

        The propagator is built on the device; the eigenvalues of the small unitary matrices are taken on the host with NumPy -- a
        reconstruction step like `kpm_reconstruct`, not a device computation.  The quasi-energies mean something only if the
        caller's shift is periodic over the window, shift(t + T) = shift(t).  In convention II a shift by a reciprocal vector
        gives a unitarily equivalent H (conjugated by the orbital phases e^{2 pi i G.tau}), not an equal one: a window over which
        shift advances by a reciprocal vector is periodic only up to that transformation."""
        kap, nt, dt = self._shift_dt_args("floquet_bands", shift, dt)
        u = self.floquet_propagator(k_list, kap, dt)
        nk, n = u.shape[0], self._nsta
        period = nt * dt
        lam = np.linalg.eigvals(u.reshape(nk, n, n))
        eps = -np.angle(lam) / period
        eps = np.where(eps <= -np.pi / period, eps + 2.0 * np.pi / period, eps)     # (arg = +pi -> the upper edge)
        return np.ascontiguousarray(np.sort(eps, axis=1).T)

    def laser_shift(self, times, amplitude, omega, phase=0.0, envelope="sin2"):
        """Extension, a host convenience: the shift kappa(t) `(len(times), dim_k)` of a laser pulse for `propagate_mesh` and the
        Floquet calls,

            kappa_a(t) = env(t) [Re(amplitude_a) cos(omega t + phase) + Im(amplitude_a) sin(omega t + phase)].

        amplitude `(dim_k,)` in reduced coordinates: real for linear polarisation, complex for elliptic -- a (1, 1j) is the
        circular pulse a (cos, sin).  envelope "flat": env = 1; "sin2": env = sin^2(pi (t - t_0) / (t_end - t_0)) over the span of
        `times`, which vanishes with its derivative at both ends.  times: 1-D, at least two finite values (propagate_mesh wants
        them equally spaced from 0: j * dt)."""
        if self._dim_k not in (1, 2, 3):
            raise Exception("\n\nlaser_shift needs a model with dim_k 1, 2 or 3.")
        try:
            t = np.array(times, dtype=float)
            amp = np.array(amplitude, dtype=complex)
            omega, phase = float(omega), float(phase)
        except (TypeError, ValueError):
            raise Exception("\n\nlaser_shift: times, amplitude, omega and phase must be numbers.")
        if t.ndim != 1 or t.size < 2 or not np.all(np.isfinite(t)):
            raise Exception("\n\ntimes must be a 1-D array of at least two finite values.")
        if amp.ndim == 0 and self._dim_k == 1:
            amp = amp.reshape(1)
        if amp.shape != (self._dim_k,) or not np.all(np.isfinite(amp)):
            raise Exception("\n\namplitude must be a finite (dim_k,) vector (complex for elliptic polarisation).")
        if not np.isfinite(omega) or not np.isfinite(phase):
            raise Exception("\n\nomega and phase must be finite.")
        if envelope == "flat":
            env = np.ones_like(t)
        elif envelope == "sin2":
            if not t[-1] > t[0]:
                raise Exception("\n\ntimes must increase for the sin2 envelope.")
            env = np.sin(np.pi * (t - t[0]) / (t[-1] - t[0])) ** 2
        else:
            raise Exception("\n\nenvelope must be 'sin2' or 'flat'.")
        arg = omega * t + phase
        return env[:, None] * (np.cos(arg)[:, None] * amp.real[None, :] + np.sin(arg)[:, None] * amp.imag[None, :])

    # ------------------------------------------------------------------ position operator
    def ignore_position_operator_offdiagonal(self):
        self._assume_position_operator_diagonal = True

    def _position_dir_check(self, dir):
        if dir in self._per:
            raise Exception("Can not compute position matrix elements along periodic direction!")
        if dir < 0 or dir >= self._dim_r:
            raise Exception("Direction out of range!")
        if self._assume_position_operator_diagonal == False:  # noqa: E712
            raise Exception("\n\nPosition-operator objects of Wannier90 models need "
                            "my_model.ignore_position_operator_offdiagonal()")

    def _position_call(self, evec, dir, want_x, want_c, want_w, orbital, wfs=None):
        """Shared driver of position_matrix/expectation/hwf.  `evec` is one point
        [band,orb(,spin)] or a batch [point,band,orb(,spin)] (extension).  With
        wfs = (device handle, point indices or None, occ) the states are read from a
        resident wf_array instead and `evec` is ignored (always batched)."""
        self._position_dir_check(dir)
        ncomp = self._norb * self._nspin
        pos = np.ascontiguousarray(np.repeat(self._orb[:, dir], self._nspin), dtype=float)   # pythtb.py:2078-2083
        if wfs is None:
            ev = np.array(evec, dtype=complex)
            tail = 2 if self._nspin == 2 else 1
            batched = ev.ndim == tail + 2
            if ev.ndim not in (tail + 1, tail + 2) or ev.shape[-tail:] != ((self._norb, 2) if tail == 2 else (self._norb,)):
                raise Exception("\n\nWrong shape of the eigenvector array")
            nsub = ev.shape[-tail - 1]
            nk = ev.shape[0] if batched else 1
            flat = np.ascontiguousarray(ev.reshape(nk, nsub, ncomp))
        else:
            handle, pts, occ, npts_all = wfs
            batched = True
            nsub = len(occ)
            nk = npts_all if pts is None else len(pts)
        xmat = np.zeros((nk, nsub, nsub), dtype=complex) if want_x else None
        hwfc = np.zeros((nk, nsub), dtype=float) if want_c else None
        width = ncomp if orbital else nsub
        hwf = np.zeros((nk, nsub, width), dtype=complex) if want_w else None
        outs = (_lib.dptr(xmat.view(float)) if want_x else None, _lib.dptr(hwfc),
                _lib.dptr(hwf.view(float)) if want_w else None, 1 if orbital else 0)
        if wfs is None:
            _lib.check(_lib.lib.tbk_position_hwf(
                _lib.default_context().handle, _lib.dptr(flat.view(float)), nk, nsub, ncomp, _lib.dptr(pos), *outs))
        else:
            import ctypes as C
            occ32 = np.ascontiguousarray(occ, dtype=np.int32)
            p64 = None if pts is None else np.ascontiguousarray(pts, dtype=np.int64)
            _lib.check(_lib.lib.tbk_wfs_position_hwf(
                handle, None if p64 is None else p64.ctypes.data_as(C.POINTER(C.c_int64)), nk, _lib.iptr(occ32), nsub,
                _lib.dptr(pos), *outs))
        if want_w and orbital and self._nspin == 2:
            hwf = hwf.reshape(nk, nsub, self._norb, 2)
        pick = (lambda a: a) if batched else (lambda a: None if a is None else a[0])
        return pick(xmat), pick(hwfc), pick(hwf)

    def position_matrix(self, evec, dir, _wfs=None):
        """X_mn = <u_m| r_dir |u_n> for the states `evec` of one k-point (pythtb.py:2034-2098)."""
        xmat, _, _ = self._position_call(evec, dir, True, False, False, False, _wfs)
        herm = xmat - np.swapaxes(xmat.conj(), -1, -2)
        if np.max(herm) > 1.0E-9:
            raise Exception("\n\n Position matrix is not hermitian?!")
        return xmat

    def position_expectation(self, evec, dir, _wfs=None):
        """Diagonal of the position matrix (pythtb.py:2100-2141)."""
        xmat = self.position_matrix(evec, dir, _wfs)
        return np.array(np.real(np.diagonal(xmat, axis1=-2, axis2=-1)), dtype=float)

    def position_hwf(self, evec, dir, hwf_evec=False, basis="orbital", _wfs=None):
        """Hybrid Wannier centres (and functions) = eigen-decomposition of the position
        matrix (pythtb.py:2143-2279)."""
        if not hwf_evec:
            _, hwfc, _ = self._position_call(evec, dir, False, True, False, False, _wfs)
            return hwfc
        which = basis.lower().strip()
        if which in ("wavefunction", "bloch"):
            orbital = False
        elif which == "orbital":
            orbital = True
        else:
            raise Exception("\n\nBasis must be either 'wavefunction', 'bloch', or 'orbital'")
        _, hwfc, hwf = self._position_call(evec, dir, False, True, True, orbital, _wfs)
        return (hwfc, hwf)

    # ------------------------------------------------------------------ surface Green's functions (extensions)
    def _surface_dir(self, fin_dir):
        """Checked fin_dir of the surface calls: a periodic lattice direction, as `cut_piece` takes it."""
        if self._dim_k == 0:
            raise Exception("\n\nSurface Green's functions need a model with dim_k >= 1.")
        if not _is_int(fin_dir) or fin_dir < 0 or fin_dir >= self._dim_r:
            raise Exception("\n\nfin_dir must be a lattice direction in [0, dim_r).")
        if list(self._per).count(fin_dir) != 1:
            raise Exception("\n\nCan not make model finite along this direction!")
        return int(fin_dir)

    def principal_layer(self, fin_dir):
        """Extension: L = max(1, max |R_fin_dir| over the hoppings), the number of unit cells along `fin_dir` in one
        principal layer: layers of L cells couple to their nearest neighbours only."""
        d = self._surface_dir(fin_dir)
        return max([1] + [abs(int(h[3][d])) for h in self._hoppings])

    def _surface_cut(self, fin_dir):
        """(device handle of cut_piece(2 L, fin_dir), L, N = L nsta); the cut model is built once per state of the tables."""
        d = self._surface_dir(fin_dir)
        L = self.principal_layer(d)
        N = L * self._nsta
        if N > 128:
            raise _lib.TbkError("\n\nA principal layer of %d states (L = %d cells of %d): the decimation kernels of this "
                                "build take at most 128." % (N, L, self._nsta))
        mark = (self._tbk_epoch, len(self._hoppings), self._orb.tobytes(), np.asarray(self._site_energies).tobytes())
        c = self._tbk_surface.get(d)
        if c is None or c[0] != mark:
            import contextlib
            import io
            with contextlib.redirect_stdout(io.StringIO()):
                cut = self.cut_piece(2 * L, d)
            c = (mark, cut)
            self._tbk_surface[d] = c
        return c[1], L, N

    def _surface_k(self, k_list, one=False):
        """k list of the surface zone, `(nk, dim_k - 1)`; a model with dim_k == 1 has no k and one point."""
        dk = self._dim_k - 1
        if dk == 0:
            if k_list is not None and np.asarray(k_list, dtype=float).size != 0:
                raise Exception("\n\nk-vector of wrong shape!")
            return None, 1
        if k_list is None:
            raise Exception("\n\nHave to provide a k-vector!")
        k = np.array(k_list, dtype=float)
        if one:
            if k.ndim == 0:
                k = k.reshape(1)
            if k.shape != (dk,):
                raise Exception("\n\nk-vector of wrong shape!")
            k = k.reshape(1, dk)
        elif dk == 1 and k.ndim == 1:
            k = k.reshape(-1, 1)
        if k.ndim != 2 or k.shape[1] != dk or k.shape[0] < 1:
            raise Exception("\n\nk-vector of wrong shape!")
        if not np.all(np.isfinite(k)):
            raise Exception("\n\nk must be finite.")
        return np.ascontiguousarray(k), k.shape[0]

    @staticmethod
    def _surface_args(omega, eta, tol, max_iter):
        w = np.array(omega, dtype=float)
        if w.ndim != 1 or w.size < 1 or w.size > 65536:
            raise Exception("\n\nomega must be a 1-D array of 1..65536 frequencies.")
        if not np.all(np.isfinite(w)):
            raise Exception("\n\nomega must be finite.")
        if not np.isfinite(eta) or not eta > 0.0:
            raise Exception("\n\neta must be finite and > 0.")
        if not np.isfinite(tol) or not tol >= 0.0:
            raise Exception("\n\ntol must be finite and >= 0.")
        if not _is_int(max_iter) or max_iter < 0 or max_iter > 64:
            raise Exception("\n\nmax_iter must be an integer in 0..64.")
        return np.ascontiguousarray(w)

    def _gen_layer_blocks(self, k_point, fin_dir):
        """Extension: `(H00, H01)`, each complex `(N, N)`, N = L nsta: the top-left and top-right blocks of
        `cut_piece(2 L, fin_dir)._gen_ham(k_point)`, built on the device.  H00 is the Hamiltonian of one principal layer
        (state `cell * nsta + state`, spin innermost), H01 couples it to the next layer toward +fin_dir; `k_point` holds the
        reduced coordinates of the remaining periodic directions (None for dim_k == 1)."""
        cut, L, N = self._surface_cut(fin_dir)
        k, _ = self._surface_k(k_point, one=True)
        h00 = np.zeros((1, N, N), dtype=complex)
        h01 = np.zeros((1, N, N), dtype=complex)
        _lib.check(_lib.lib.tbk_surface_blocks(cut._device_model(), N, _lib.dptr(k), 1, _lib.dptr(h00.view(float)),
                                               _lib.dptr(h01.view(float))))
        return h00[0], h01[0]

    def surface_green(self, k_list, omega, eta, fin_dir, side, tol=1e-12, max_iter=50):
        """Extension: the retarded Green's function of the semi-infinite crystal by iterative decimation (Lopez Sancho,
        Lopez Sancho and Rubio 1985) on the principal layer of `_gen_layer_blocks`, z = omega + i eta:

            side 0   the crystal fills cells >= 0 along fin_dir, cell 0 exposed:  G = [z - H00 - H01 G H01^+]^-1
            side 1   the crystal fills cells <= 0, the last cell of the layer exposed:  G = [z - H00 - H01^+ G H01]^-1
            side 2   bulk:  G = [z - H00 - H01 G_0 H01^+ - H01^+ G_1 H01]^-1

        Returns complex `(nk, nw, N, N)`; meant for a few points (whole matrices).  k_list: points of the surface zone,
        `(nk, dim_k - 1)`, the coordinates `cut_piece(., fin_dir)`'s model takes (None for dim_k == 1: one point).
        omega: 1-D, 1..65536 finite values in any order; eta > 0.  A point stops at the first step count i (0 included)
        with max(|alpha|_max, |beta|_max) <= tol max(|H00|_max, |H01|_max); tol=0 takes exactly max_iter (0..64) steps, after
        which G is a diagonal block of the resolvent of the slab of L 2^i cells (L (2^(i+1) - 1) for the bulk).  Raises when
        a point misses a non-zero tol.  The value at a point does not depend on the rest of the call (same bits)."""
        if side not in (0, 1, 2) or not _is_int(side):
            raise Exception("\n\nside must be 0, 1 or 2 (bulk).")
        cut, L, N = self._surface_cut(fin_dir)
        k, nk = self._surface_k(k_list)
        w = self._surface_args(omega, eta, tol, max_iter)
        out = np.zeros((nk, w.size, N, N), dtype=complex)
        _lib.check(_lib.lib.tbk_surface_green_list(cut._device_model(), N, self._nsta, _lib.dptr(k), nk, int(w.size), _lib.dptr(w),
                                                   float(eta), float(tol), int(max_iter), 0, int(side),
                                                   _lib.dptr(out.view(float)), None))
        return out

    def surface_spectral(self, k_list, omega, eta, fin_dir, per_state=False, tol=1e-12, max_iter=50, return_info=False):
        """Extension: the spectral functions A = -(1 / pi) Im sum_s G_ss of the two surfaces and the bulk, float
        `(3, nk, nw)` with rows side 0, side 1, bulk of `surface_green`; the sum runs over the states of the exposed unit
        cell (cell 0 of the layer; the last cell for side 1).  per_state=True: `(3, nk, nw, nsta)`, the diagonal itself.
        return_info=True: `(A, steps)` with steps int32 `(nk, nw)`, the decimation steps each point took.  Arguments and
        stopping rule as `surface_green`.  Each side and the bulk come out separately and without a finite-size gap, at the
        cost of matrices of one principal layer per (k, omega): what a ribbon of `cut_piece` cells diagonalised at every k
        approximates."""
        cut, L, N = self._surface_cut(fin_dir)
        k, nk = self._surface_k(k_list)
        w = self._surface_args(omega, eta, tol, max_iter)
        ns = self._nsta
        out = np.zeros((3, nk, w.size, ns) if per_state else (3, nk, w.size), dtype=float)
        info = np.zeros((nk, w.size), dtype=np.int32) if return_info else None
        _lib.check(_lib.lib.tbk_surface_green_list(cut._device_model(), N, ns, _lib.dptr(k), nk, int(w.size), _lib.dptr(w),
                                                   float(eta), float(tol), int(max_iter), 2 if per_state else 1, 0,
                                                   _lib.dptr(out), _lib.iptr(info)))
        return (out, info) if return_info else out

    def surface_dos_mesh(self, mesh_size, omega, eta, fin_dir, per_state=False, tol=1e-12, max_iter=50):
        """Extension: the mean of `surface_spectral` over the uniform mesh of the surface zone -- the `k_uniform_mesh`
        points of `cut_piece(., fin_dir)`'s model, generated on the device: `(3, nw)`, or `(3, nw, nsta)` with
        per_state=True.  Needs dim_k >= 2.  Fixed-order sums on the device: two calls give the same bits."""
        d = self._surface_dir(fin_dir)
        if self._dim_k < 2:
            raise Exception("\n\nsurface_dos_mesh needs a model with dim_k >= 2.")
        mesh = np.array(list(map(round, mesh_size)), dtype=np.int32)
        if mesh.shape != (self._dim_k - 1,):
            raise Exception("\n\nIncorrect size of the specified k-mesh!")
        if np.min(mesh) <= 0:
            raise Exception("\n\nMesh must have positive non-zero number of elements.")
        w = self._surface_args(omega, eta, tol, max_iter)
        cut, L, N = self._surface_cut(d)
        ns = self._nsta
        out = np.zeros((3, w.size, ns) if per_state else (3, w.size), dtype=float)
        _lib.check(_lib.lib.tbk_surface_dos_mesh(cut._device_model(), N, ns, _lib.iptr(np.ascontiguousarray(mesh)), int(w.size),
                                                 _lib.dptr(w), float(eta), float(tol), int(max_iter), 1 if per_state else 0,
                                                 _lib.dptr(out)))
        return out

    # ------------------------------------------------------------------ Landauer transmission (extensions)
    def lead_self_energy(self, k_list, omega, eta, fin_dir, side, tol=1e-12, max_iter=50):
        """Extension: the self-energy a pristine semi-infinite lead of this crystal puts on the layer it touches, from the
        decimation of `surface_green` (same arguments, stopping rule and sides):

            side 0   Sigma_R = H01 G_0 H01^+   the lead fills the layers toward +fin_dir, its first layer exposed
            side 1   Sigma_L = H01^+ G_1 H01   the lead fills the layers toward -fin_dir, its last layer exposed

        Returns complex `(nk, nw, N, N)`; whole matrices, meant for a few points."""
        if side not in (0, 1) or not _is_int(side):
            raise Exception("\n\nside must be 0 or 1.")
        cut, L, N = self._surface_cut(fin_dir)
        k, nk = self._surface_k(k_list)
        w = self._surface_args(omega, eta, tol, max_iter)
        out = np.zeros((nk, w.size, N, N), dtype=complex)
        _lib.check(_lib.lib.tbk_lead_self_energy_list(cut._device_model(), N, _lib.dptr(k), nk, int(w.size), _lib.dptr(w),
                                                      float(eta), float(tol), int(max_iter), int(side),
                                                      _lib.dptr(out.view(float)), None))
        return out

    def _landauer_device(self, device, fin_dir):
        """Checked `device` of the transmission calls: the number M of principal layers it holds (host checks only)."""
        d = self._surface_dir(fin_dir)
        L = self.principal_layer(d)
        if not isinstance(device, tb_model):
            raise Exception("\n\ndevice must be a tb_model.")
        if (device._dim_r != self._dim_r or device._nspin != self._nspin or device._lat.shape != self._lat.shape
                or not np.array_equal(device._lat, self._lat)):
            raise Exception("\n\ndevice must share the lattice and nspin of the model.")
        if list(device._per) != [p for p in self._per if p != d]:
            raise Exception("\n\ndevice must be finite along fin_dir and periodic along the other periodic directions.")
        nl = L * self._norb
        M = device._norb // nl
        if device._norb % nl != 0 or M < 1 or M > 1024:
            raise Exception("\n\ndevice must hold 1..1024 principal layers of %d orbitals." % nl)
        want = np.tile(self._orb, (M * L, 1))                  # the orbitals of cut_piece(M L, fin_dir), by its own arithmetic
        want[:, d] += np.repeat(np.arange(M * L, dtype=float), self._norb)
        if not np.abs(device._orb - want).max() <= 1e-12:
            raise Exception("\n\ndevice orbitals must be those of cut_piece(%d, fin_dir)." % (M * L))
        for h in device._hoppings:
            la, lb = sorted((h[1] // nl, h[2] // nl))
            if lb - la > 1:
                raise Exception("\n\ndevice couples layers %d and %d: only neighbouring principal layers may couple."
                                % (la + 1, lb + 1))
        return M

    def _gen_device_blocks(self, k_point, fin_dir, device):
        """Extension: `(D, U)`, complex `(M, N, N)` and `(M - 1, N, N)`: the diagonal blocks D_i and the upper blocks
        U_i = H_{i,i+1} of `device._gen_ham(k_point)` in layers of N = L nsta states, built on the device; the counterpart
        of `_gen_layer_blocks` for the scattering region of `transmission`."""
        cut, L, N = self._surface_cut(fin_dir)
        M = self._landauer_device(device, fin_dir)
        k, _ = self._surface_k(k_point, one=True)
        D = np.zeros((1, M, N, N), dtype=complex)
        U = np.zeros((1, max(M - 1, 0), N, N), dtype=complex)
        _lib.check(_lib.lib.tbk_landauer_blocks(device._device_model(), N, M, _lib.dptr(k), 1, _lib.dptr(D.view(float)),
                                                _lib.dptr(U.view(float)) if M > 1 else None))
        return D[0], U[0]

    def transmission(self, k_list, omega, eta, fin_dir, device=None, tol=1e-12, max_iter=50, return_info=False):
        """Extension: the Landauer transmission T(k, omega) = Tr[Gamma_R G Gamma_L G^+] (Caroli / Fisher-Lee) of a scattering
        region between two pristine semi-infinite leads of this crystal, float `(nk, nw)`; the conductance is e^2 / h times
        T (per spin channel kept in the model).  Gamma = i (Sigma - Sigma^+) with the self-energies of `lead_self_energy`,
        G the retarded Green's function of the region with both self-energies, z = omega + i eta in the leads and in the
        region alike.

        device: a `tb_model` with the geometry of `self.cut_piece(M * L, fin_dir)`, L = `principal_layer(fin_dir)`,
        M = 1..1024, which the caller has edited (on-site shifts, changed or added hoppings); it may couple neighbouring
        principal layers only.  The left lead continues it below layer 1, the right lead above layer M, both with the
        crystal's own H01.  device=None: one pristine principal layer.  The work per point is a recursive Green's function
        sweep over the M layers on matrices of one layer (N <= 128).  k_list, omega, eta, tol, max_iter as `surface_green`;
        return_info=True: `(T, steps)` with steps int32 `(nk, nw)`, the decimation steps of the leads.  The value at a point
        does not depend on the rest of the call (same bits)."""
        cut, L, N = self._surface_cut(fin_dir)
        M = 1 if device is None else self._landauer_device(device, fin_dir)
        k, nk = self._surface_k(k_list)
        w = self._surface_args(omega, eta, tol, max_iter)
        out = np.zeros((nk, w.size), dtype=float)
        info = np.zeros((nk, w.size), dtype=np.int32) if return_info else None
        _lib.check(_lib.lib.tbk_transmission_list(cut._device_model(), None if device is None else device._device_model(), N, M,
                                                  _lib.dptr(k), nk, int(w.size), _lib.dptr(w), float(eta), float(tol),
                                                  int(max_iter), _lib.dptr(out), _lib.iptr(info)))
        return (out, info) if return_info else out

    def conductance_mesh(self, mesh_size, omega, eta, fin_dir, device=None, tol=1e-12, max_iter=50):
        """Extension: the mean of `transmission` over the uniform mesh of the surface zone -- the `k_uniform_mesh` points of
        `cut_piece(., fin_dir)`'s model, generated on the device: float `(nw,)`, the conductance per transverse cell in
        units of e^2 / h.  Needs dim_k >= 2.  Fixed-order sums on the device: two calls give the same bits."""
        d = self._surface_dir(fin_dir)
        if self._dim_k < 2:
            raise Exception("\n\nconductance_mesh needs a model with dim_k >= 2.")
        mesh = np.array(list(map(round, mesh_size)), dtype=np.int32)
        if mesh.shape != (self._dim_k - 1,):
            raise Exception("\n\nIncorrect size of the specified k-mesh!")
        if np.min(mesh) <= 0:
            raise Exception("\n\nMesh must have positive non-zero number of elements.")
        w = self._surface_args(omega, eta, tol, max_iter)
        cut, L, N = self._surface_cut(d)
        M = 1 if device is None else self._landauer_device(device, d)
        out = np.zeros(w.size, dtype=float)
        _lib.check(_lib.lib.tbk_transmission_mesh(cut._device_model(), None if device is None else device._device_model(), N, M,
                                                  _lib.iptr(np.ascontiguousarray(mesh)), int(w.size), _lib.dptr(w), float(eta),
                                                  float(tol), int(max_iter), _lib.dptr(out)))
        return out

    # ------------------------------------------------------------------ kernel polynomial method (extensions)
    def _sparse_model(self):
        """The sparse (CSR) operator of this model on the device: any number of states, no dense upload.  Cached with the edit
        mark of `_device_model` and freed with it."""
        ctx = _lib.default_context()
        c = getattr(self, "_tbk_sparse", None)
        mark = (self._tbk_epoch, len(self._hoppings), self._orb.tobytes(), np.asarray(self._site_energies).tobytes())
        if c is not None and c[0] == mark and c[1] is ctx:
            return c[2]
        if c is not None:
            _lib.lib.tbk_sparse_free(c[2])
            self._tbk_sparse = None
        orb_per, onsite, hop_i, hop_j, hop_R, hop_amp = self._flat_tables()
        h = C.c_void_p()
        _lib.check(_lib.lib.tbk_sparse_upload(
            ctx.handle, self._dim_k, self._norb, self._nspin, _lib.dptr(orb_per),
            _lib.dptr(onsite.view(float)), len(hop_i), _lib.iptr(hop_i), _lib.iptr(hop_j),
            _lib.iptr(hop_R.reshape(-1)) if hop_R.size else None,
            _lib.dptr(hop_amp.view(float)) if hop_amp.size else None, C.byref(h)))
        self._tbk_sparse = (mark, ctx, h)
        return h

    def _kpm_k(self, k_list):
        if k_list is None:
            if self._dim_k != 0:
                raise Exception("\n\nHave to provide a k-vector!")
            return None, 1
        if self._dim_k == 0:
            raise Exception("\n\nA model with dim_k = 0 takes no k_list.")
        k = self._k_array(k_list)
        if len(k) < 1:
            raise Exception("\n\nkpm: empty k_list")
        return k, len(k)

    def _kpm_bounds(self, bounds, sp):
        if bounds is None:
            g = np.zeros(2)
            _lib.check(_lib.lib.tbk_sparse_info(sp, None, None, None, _lib.dptr(g)))
            pad = 0.01 * (g[1] - g[0]) if g[1] > g[0] else 1.0
            return float(g[0] - pad), float(g[1] + pad)
        return bounds

    @staticmethod
    def _kpm_bounds_arg(bounds):
        if bounds is None:
            return None
        b = np.array(bounds, dtype=float)
        if b.shape != (2,) or not np.all(np.isfinite(b)) or not b[1] > b[0]:
            raise Exception("\n\nkpm: bounds must be (emin, emax), finite, with emin < emax")
        return float(b[0]), float(b[1])

    def kpm_vectors(self, n_vectors, seed=0, first=0):
        """Extension: the random-phase start vectors e^{i phi} of `kpm_moments`, complex `(n_vectors, nsta)`: vectors number
        first .. first + n_vectors - 1 of `seed`.  Element i of vector g is a pure function of (seed, g, i), generated on the
        device; `kpm_moments` uses the numbers q * n_vectors + v at the k-point with index q."""
        if not _is_int(n_vectors) or n_vectors < 1:
            raise Exception("\n\nkpm_vectors: n_vectors must be a positive integer")
        if not _is_int(seed) or not 0 <= seed < 2 ** 64 or not _is_int(first) or first < 0:
            raise Exception("\n\nkpm_vectors: seed must be an integer in [0, 2^64), first a non-negative integer")
        out = np.empty((int(n_vectors), self._nsta), dtype=complex)
        _lib.check(_lib.lib.tbk_kpm_vectors(self._sparse_model(), int(seed), int(first), int(n_vectors), _lib.dptr(out.view(float))))
        return out

    def _kpm_start(self, who, vectors, n_vectors, seed, states):
        """Checked start vectors of the moment calls: (vectors or None, int32 states or None, nvec)."""
        if vectors is not None and states is not None:
            raise Exception("\n\n%s: give either vectors or states, not both" % who)
        n = self._nsta
        vec = st = None
        if vectors is not None:
            vec = np.asarray(vectors)
            if vec.dtype != np.complex128 or vec.ndim != 2 or vec.shape[0] < 1 or vec.shape[1] != n:
                raise Exception("\n\n%s: vectors must be a complex128 array of shape (nvec, %d)" % (who, n))
            vec = np.ascontiguousarray(vec)
            nvec = vec.shape[0]
        elif states is not None:
            st = np.array(list(states))
            if st.ndim != 1 or st.size < 1 or not np.issubdtype(st.dtype, np.integer):
                raise Exception("\n\n%s: states must be a non-empty list of integers" % who)
            if st.min() < 0 or st.max() >= n:
                raise Exception("\n\n%s: state index out of range [0, %d)" % (who, n))
            st = np.ascontiguousarray(st, dtype=np.int32)
            nvec = st.size
        else:
            if not _is_int(n_vectors) or n_vectors < 1:
                raise Exception("\n\n%s: n_vectors must be a positive integer" % who)
            nvec = int(n_vectors)
        if not _is_int(seed) or not 0 <= seed < 2 ** 64:
            raise Exception("\n\n%s: seed must be an integer in [0, 2^64)" % who)
        return vec, st, nvec

    def kpm_moments(self, n_moments, k_list=None, vectors=None, n_vectors=8, seed=0, states=None, bounds=None):
        """Extension: Chebyshev moments mu_m = <v|T_m(H~(k))|v> / <v|v>, m < n_moments, of the rescaled sparse Hamiltonian
        H~ = (H - b) / a, a = (emax - emin) / 2, b = (emax + emin) / 2 (the kernel polynomial method; Weisse et al., Rev. Mod.
        Phys. 78, 275) -- for models of any size: nothing is diagonalised and no dense matrix is built.  Returns
        `(mu, (emin, emax))`, mu float `(nk, nvec, n_moments)`, without the k axis when k_list is None (dim_k = 0 only).

        Start vectors, exactly one of: `vectors` complex128 `(nvec, nsta)`; `states`, state indices (unit vectors: the local
        density of states); otherwise `n_vectors` random-phase vectors of `seed` (those `kpm_vectors` returns).
        bounds=None: the Gershgorin interval of the hopping table widened by 1 % of its width on each side.  Bounds that do
        not contain the spectrum make the recursion diverge: the call raises, naming them.  n_moments moments cost
        n_moments / 2 sparse products per block of 8 vectors; fixed-order sums on the device: two calls give the same bits."""
        if not _is_int(n_moments) or n_moments < 1:
            raise Exception("\n\nkpm_moments: n_moments must be a positive integer")
        vec, st, nvec = self._kpm_start("kpm_moments", vectors, n_vectors, seed, states)
        bounds = self._kpm_bounds_arg(bounds)
        k, nk = self._kpm_k(k_list)
        sp = self._sparse_model()
        emin, emax = self._kpm_bounds(bounds, sp)
        mu = np.empty((nk, nvec, int(n_moments)), dtype=float)
        _lib.check(_lib.lib.tbk_kpm_moments(sp, _lib.dptr(k), nk, int(n_moments), emin, emax, nvec,
                                            None if vec is None else _lib.dptr(vec.view(float)), _lib.iptr(st), int(seed),
                                            _lib.dptr(mu)))
        return (mu[0] if k_list is None else mu), (emin, emax)

    def kpm_dos(self, energies, n_moments, k_list=None, n_vectors=8, seed=0, kernel="jackson", bounds=None, return_error=False,
                states=None):
        """Extension: the density of states per state rho(E) (integral 1) by the kernel polynomial method: the stochastic
        trace over `n_vectors` random-phase vectors per k-point, averaged over `k_list`, reconstructed by `kpm_reconstruct`.
        return_error=True: `(rho, err)` with the standard error of the mean over the k x vector samples.  states (a list of
        state indices) replaces the random vectors by unit vectors; `range(nsta)` is the exact trace."""
        mu, bnd = self.kpm_moments(n_moments, k_list, n_vectors=n_vectors, seed=seed, states=states, bounds=bounds)
        samples = mu.reshape(-1, mu.shape[-1])
        rho = kpm_reconstruct(samples.mean(axis=0), energies, bnd, kernel)
        if not return_error:
            return rho
        each = kpm_reconstruct(samples, energies, bnd, kernel)
        ns = each.shape[0]
        err = each.std(axis=0, ddof=1) / np.sqrt(ns) if ns > 1 else np.full(rho.shape, np.nan)
        return rho, err

    def kpm_ldos(self, energies, states, n_moments, k_list=None, kernel="jackson", bounds=None):
        """Extension: the local density of states rho_i(E) = sum_n |<i|n>|^2 delta(E - E_n) of the states `states`, averaged
        over `k_list`, float `(len(states), nE)`: `kpm_moments` with unit start vectors, then `kpm_reconstruct`."""
        if states is None:
            raise Exception("\n\nkpm_ldos: states must be a non-empty list of integers")
        mu, bnd = self.kpm_moments(n_moments, k_list, states=states, bounds=bounds)
        if k_list is not None:
            mu = mu.mean(axis=0)
        return kpm_reconstruct(mu, energies, bnd, kernel)

    def kpm_double_moments(self, n_moments, dirs, k_list, vectors=None, n_vectors=8, seed=0, states=None, bounds=None):
        """Extension: the double Chebyshev moments of the Kubo-Bastin conductivity on the sparse operator, for models of any
        size with a periodic axis (dim_k = 0 raises):

            mu_mn = <v| V^a T_m(H~(k)) V^b T_n(H~(k)) |v> / <v|v>,   m, n < n_moments,   (a, b) = dirs (a == b allowed),

        H~ = (H - b) / a, a = (emax - emin) / 2, b = (emax + emin) / 2 as in `kpm_moments`, V^a = dH/dk_a in reduced
        coordinates for a periodic axis a in [0, dim_k): the matrix `_gen_dham(k, a)` returns.  Returns `(mu, (emin, emax))`,
        mu complex `(nk, nvec, n_moments, n_moments)`.  Start vectors, bounds and the random-vector numbering (q * nvec + v at
        the k-point with index q) as in `kpm_moments`.  3 n_moments sparse products per block of 8 vectors, a contraction of
        n_moments^2 nsta multiply-adds per vector and a device workspace of n_moments * nsta * 128 bytes; fixed-order sums:
        two calls give the same bits.  Bounds that do not contain the spectrum raise, naming the Gershgorin interval."""
        if not _is_int(n_moments) or n_moments < 1:
            raise Exception("\n\nkpm_double_moments: n_moments must be a positive integer")
        if self._dim_k < 1:
            raise Exception("\n\nkpm_double_moments needs a model with dim_k >= 1: the velocity operator is dH/dk.")
        dirs = list(dirs)
        if len(dirs) != 2 or not all(_is_int(d) for d in dirs):
            raise Exception("\n\nkpm_double_moments: dirs must be two integer axes.")
        if min(dirs) < 0 or max(dirs) >= self._dim_k:
            raise Exception("\n\nkpm_double_moments: dirs must be axes in [0, dim_k)")
        vec, st, nvec = self._kpm_start("kpm_double_moments", vectors, n_vectors, seed, states)
        bounds = self._kpm_bounds_arg(bounds)
        k, nk = self._kpm_k(k_list)
        sp = self._sparse_model()
        emin, emax = self._kpm_bounds(bounds, sp)
        M = int(n_moments)
        mu = np.empty((nk, nvec, M, M), dtype=complex)
        _lib.check(_lib.lib.tbk_kpm_double_moments(sp, _lib.dptr(k), nk, M, emin, emax, int(dirs[0]), int(dirs[1]), nvec,
                                                   None if vec is None else _lib.dptr(vec.view(float)), _lib.iptr(st), int(seed),
                                                   _lib.dptr(mu.view(float))))
        return mu, (emin, emax)

    def kpm_conductivity(self, energies, n_moments, dirs, k_list, n_vectors=8, seed=0, kernel="jackson", bounds=None, kT=0.0,
                         return_error=False, states=None):
        """Extension: the DC conductivity sigma_ab(E_F), (a, b) = dirs, at the Fermi levels `energies` by the Chebyshev
        expansion of the Kubo-Bastin formula, the longitudinal (a == b) and the Hall component alike, float `(nE,)`:

            sigma_ab(E_F) = nsta * Re mean_samples G_ab(E_F),

        G_ab of `kpm_conductivity_reconstruct` from `kpm_double_moments`, the samples being the `n_vectors` random-phase
        vectors per k-point of `k_list` (the stochastic trace).  Reduced coordinates: V^a = dH/dk_a as in
        `optical_conductivity_mesh`; for dim_k = 2 sigma_ab is the sheet conductance of the model's cell in units of e^2/h
        (no spin-degeneracy factor), and the Cartesian tensor is A^T sigma A / V_c in units of e^2/h x length^(2 - dim_k),
        A = the periodic lattice vectors as rows, V_c = sqrt(det(A A^T)).  Sign: in a gap sigma_01 = -C, C the Chern number
        of the occupied bands as `berry_curvature_mesh(mesh, occ, dirs=(0, 1)) / (2 pi)` gives it -- the sign of its
        docstring's sigma_xy = -(e^2/h) I / 2 pi.  return_error=True: `(sigma, err)` with the standard error of the mean over
        the k x vector samples.  states (a list of state indices) replaces the random vectors by unit vectors;
        `range(nsta)` is the exact trace.  The resolution is ~ pi a / n_moments (Jackson kernel): a plateau needs a gap
        several times that."""
        mu, bnd = self.kpm_double_moments(n_moments, dirs, k_list, n_vectors=n_vectors, seed=seed, states=states, bounds=bounds)
        samples = mu.reshape(-1, mu.shape[-2], mu.shape[-1])
        n = self._nsta
        sigma = n * kpm_conductivity_reconstruct(samples.mean(axis=0), energies, bnd, kernel, kT=kT).real
        if not return_error:
            return sigma
        each = n * kpm_conductivity_reconstruct(samples, energies, bnd, kernel, kT=kT).real
        ns = each.shape[0]
        err = each.std(axis=0, ddof=1) / np.sqrt(ns) if ns > 1 else np.full(sigma.shape, np.nan)
        return sigma, err

    def kpm_apply(self, coeffs, k_list=None, vectors=None, n_vectors=8, seed=0, states=None, bounds=None):
        """Extension: a function of the sparse Hamiltonian applied to vectors by its Chebyshev series,

            out_s = sum_m coeffs[s][m] T_m(H~(k)) v,   H~ = (H - b) / a,   a = (emax - emin) / 2,   b = (emax + emin) / 2,

        for models of any size: nothing is diagonalised.  `coeffs` `(nset, ncoef)`, real or complex, holds one coefficient set
        per row -- `kpm_fermi_coefficients` (the Fermi projector), `kpm_coefficients` (any function of the energy); all sets
        share the ncoef - 1 sparse products per block of 8 vectors.  Returns `(out, (emin, emax))`, out complex
        `(nk, nset, nvec, nsta)`, without the k axis when k_list is None (dim_k = 0 only) and without the set axis for 1-D
        `coeffs`; not divided by <v|v>.  Start vectors, bounds and the random-vector numbering (q * nvec + v at the k-point with
        index q) as in `kpm_moments`; the coefficients must belong to the same bounds.  Bounds that do not contain the spectrum
        raise, naming the Gershgorin interval.  Fixed-order sums on the device: two calls give the same bits."""
        c = np.asarray(coeffs)
        if c.ndim not in (1, 2) or c.size < 1 or not (np.issubdtype(c.dtype, np.number) and c.dtype != bool):
            raise Exception("\n\nkpm_apply: coeffs must be a non-empty numeric array of shape (ncoef,) or (nset, ncoef)")
        c2 = np.ascontiguousarray(np.atleast_2d(c), dtype=complex)
        if not np.all(np.isfinite(c2)):
            raise Exception("\n\nkpm_apply: coeffs must be finite")
        vec, st, nvec = self._kpm_start("kpm_apply", vectors, n_vectors, seed, states)
        bounds = self._kpm_bounds_arg(bounds)
        k, nk = self._kpm_k(k_list)
        sp = self._sparse_model()
        emin, emax = self._kpm_bounds(bounds, sp)
        nset, ncoef = c2.shape
        out = np.empty((nk, nset, nvec, self._nsta), dtype=complex)
        _lib.check(_lib.lib.tbk_kpm_apply_series(sp, _lib.dptr(k), nk, ncoef, nset, _lib.dptr(c2.view(float)), emin, emax, nvec,
                                                 None if vec is None else _lib.dptr(vec.view(float)), _lib.iptr(st), int(seed),
                                                 _lib.dptr(out.view(float))))
        if c.ndim == 1:
            out = out[:, 0]
        return (out[0] if k_list is None else out), (emin, emax)

    def kpm_evolve(self, times, k_list=None, vectors=None, states=None, bounds=None):
        """Extension: the time evolution e^{-i H(k) t} |v> of the supplied `vectors` (complex128 `(nvec, nsta)`) or of the unit
        vectors at `states`, for every t of `times` (hbar = 1), by the Chebyshev series with the coefficients
        c_m(t) = (2 - delta_m0) (-i)^m J_m(a t) e^{-i b t} (Tal-Ezer, Kosloff, J. Chem. Phys. 81, 3967): one coefficient set per
        time through `kpm_apply`, so all times share one run of ~ a max|t| + 10 (a max|t|)^(1/3) sparse products.  The series is
        cut where |c_m| falls below 1e-17: the result is e^{-iHt} v to rounding, and the norm is kept.  Returns
        `(psi, (emin, emax))`, psi complex `(nk, nt, nvec, nsta)`, without the k axis when k_list is None (dim_k = 0 only) and
        without the time axis for a scalar `times`."""
        t = np.asarray(times, dtype=float)
        if t.ndim not in (0, 1) or t.size < 1 or not np.all(np.isfinite(t)):
            raise Exception("\n\nkpm_evolve: times must be a finite number or a non-empty one-dimensional list of them")
        if vectors is None and states is None:
            raise Exception("\n\nkpm_evolve: give the vectors or the states to evolve")
        bounds = self._kpm_bounds(self._kpm_bounds_arg(bounds), self._sparse_model())
        a, b = 0.5 * (bounds[1] - bounds[0]), 0.5 * (bounds[1] + bounds[0])
        sets = [_kpm_evolution_coefficients(a * ti) * np.exp(-1j * b * ti) for ti in t.reshape(-1)]
        c = np.zeros((len(sets), max(len(s) for s in sets)), dtype=complex)
        for row, s in zip(c, sets):
            row[:len(s)] = s
        return self.kpm_apply(c if t.ndim else c[0], k_list, vectors=vectors, states=states, bounds=bounds)

    def local_chern_marker(self, fermi_level, n_moments, states=None, dirs=(0, 1), kernel="jackson", bounds=None):
        """Extension: the local Chern marker of Bianco and Resta (Phys. Rev. B 84, 241106) of an open sample (dim_k = 0),

            c(s) = 4 pi Im <s| P r_a P r_b P |s>,   (a, b) = dirs,

        at the states `states` (default: all), float `(nstates,)`: a Chern number resolved in real space, for flakes, domain
        walls and disorder.  P is the Fermi projector as the Chebyshev series of `kpm_fermi_coefficients(fermi_level,
        n_moments, bounds, kernel)` on the sparse operator; r_a, r_b are the reduced coordinates of the orbitals along the
        axes a, b in [0, dim_r) (`cut_piece` keeps them unwrapped; in reduced coordinates the cell has area 1).
        2 (n_moments - 1) sparse products per block of 8 states, everything on the device; two calls give the same bits.

        - The sum of c(s) over the states of one cell deep in the bulk is the Chern number of the occupied bands as
          `berry_curvature_mesh(mesh, occ, dirs) / (2 pi)` of the periodic model gives it; dirs=(b, a) gives the negative.
        - The sum over a whole open sample is NOT a Chern number: with the exact projector it vanishes (the edge
          compensates the bulk), and with the series it is dominated by the edge states inside the gap, which no finite
          n_moments resolves.  Use bulk cells.
        - The resolution in energy is ~ pi a / n_moments (Jackson kernel), as in `kpm_conductivity`: the gap has to be
          several times that."""
        if self._dim_k != 0:
            raise Exception("\n\nlocal_chern_marker needs an open sample: cut_piece every periodic direction (dim_k = 0).")
        dirs = list(dirs)
        if len(dirs) != 2 or not all(_is_int(d) for d in dirs):
            raise Exception("\n\nlocal_chern_marker: dirs must be two integer axes.")
        if min(dirs) < 0 or max(dirs) >= self._dim_r or dirs[0] == dirs[1]:
            raise Exception("\n\nlocal_chern_marker: dirs must be two different axes in [0, dim_r)")
        if not _is_int(n_moments) or n_moments < 1:
            raise Exception("\n\nlocal_chern_marker: n_moments must be a positive integer")
        n = self._nsta
        _, st, nvec = self._kpm_start("local_chern_marker", None, 1, 0, range(n) if states is None else states)
        bounds = self._kpm_bounds_arg(bounds)
        sp = self._sparse_model()
        emin, emax = self._kpm_bounds(bounds, sp)
        c = np.ascontiguousarray(kpm_fermi_coefficients(fermi_level, n_moments, (emin, emax), kernel), dtype=float)
        da = np.ascontiguousarray(np.repeat(self._orb[:, dirs[0]], self._nspin), dtype=float)
        db = np.ascontiguousarray(np.repeat(self._orb[:, dirs[1]], self._nspin), dtype=float)
        out = np.empty(nvec, dtype=complex)
        _lib.check(_lib.lib.tbk_kpm_marker(sp, len(c), _lib.dptr(c), emin, emax, _lib.dptr(da), _lib.dptr(db), nvec, _lib.iptr(st),
                                           _lib.dptr(out.view(float))))
        return 4.0 * np.pi * out.imag

    def kpm_eigs(self, window, n_search=64, k_point=None, degree=None, tol=1e-10, max_iter=40, seed=0, bounds=None,
                 return_info=False):
        """Extension: all eigenvalues and eigenvectors of the sparse H(k) inside `window` = (e_lo, e_hi), for models of any size
        (edge states of a flake or ribbon past the dense limit of `solve_all`): Chebyshev-filtered subspace iteration (Pieper
        et al., J. Comput. Phys. 325, 226) on the operator of `kpm_moments`.  The dense model is never built.  Returns
        `(evals, evecs)`: evals float `(m,)` ascending, evecs complex `(m, norb)` (`(m, norb, 2)` for nspin = 2) -- the layout
        of `solve_one(k_point, eig_vectors=True)`, orthonormal; m = 0 is a valid answer.

        The contract: the call returns every eigenpair with e_lo <= E <= e_hi, or it raises -- never a part of them.
        `n_search` random-phase vectors of `seed` are filtered with the series of `kpm_window_coefficients` (Jackson kernel,
        `degree` + 1 terms) of the window widened by 2 pi a / degree on each side, orthonormalised, and rotated to Ritz
        vectors, until every pair inside the window has |H x - E x| <= tol a, a = (emax - emin) / 2.  `n_search` (a multiple of
        8, at most the number of states rounded down to 8 and 2048) must exceed the number of states in the WIDENED window:
        `nsta * kpm_dos` integrated over it estimates that number.  When as many Ritz vectors pass the filter as the subspace has
        directions the call raises ("raise n_search"): states could be missing.  It also raises when `max_iter` filter
        applications (at least 2) do not reach `tol`; a larger `degree` separates the window from its neighbours faster.

        degree=None: ceil(8 a / (e_hi - e_lo)) clipped to [64, 4096] -- chosen from a NumPy prototype of the algorithm (3 to 13
        filter applications on flakes and chains of 63 to 2112 states), not from a timing.  bounds as in `kpm_moments`
        (None: the Gershgorin interval widened by 1 %; bounds that do not contain the spectrum raise).  k_point: one k-vector,
        None for dim_k = 0.  return_info=True adds a dict: `residuals` `(m,)`, `applications`, `rank`, `strong` (pairs with
        filter norm >= 1/2), `returned`, `degree`, `bounds`.  Fixed-order sums on the device: two calls give the same bits."""
        w = np.array(window, dtype=float)
        if w.shape != (2,) or not np.all(np.isfinite(w)) or w[0] > w[1]:
            raise Exception("\n\nkpm_eigs: window must be (e_lo, e_hi), finite, with e_lo <= e_hi")
        n = self._nsta
        top = min(n - n % 8, 2048)
        if not _is_int(n_search) or n_search < 8 or n_search % 8 != 0 or n_search > top:
            raise Exception("\n\nkpm_eigs: n_search must be a multiple of 8 in [8, %d] for this model of %d states" % (top, n))
        if degree is not None and (not _is_int(degree) or not 2 <= degree <= 65536):
            raise Exception("\n\nkpm_eigs: degree must be an integer in [2, 65536] or None")
        if not np.isfinite(tol) or not tol > 0.0:
            raise Exception("\n\nkpm_eigs: tol must be positive")
        if not _is_int(max_iter) or max_iter < 2:
            raise Exception("\n\nkpm_eigs: max_iter must be an integer of at least 2")
        if not _is_int(seed) or not 0 <= seed < 2 ** 64:
            raise Exception("\n\nkpm_eigs: seed must be an integer in [0, 2^64)")
        bounds = self._kpm_bounds_arg(bounds)
        k, _ = self._kpm_k(None if k_point is None else [k_point])
        sp = self._sparse_model()
        emin, emax = self._kpm_bounds(bounds, sp)
        if not (emin < w[0] and w[1] < emax):
            raise Exception("\n\nkpm_eigs: window must lie inside the open interval of the bounds (%.12g, %.12g)" % (emin, emax))
        if degree is None:
            width = w[1] - w[0]
            degree = 4096 if width <= 0.0 else int(min(4096, max(64, np.ceil(4.0 * (emax - emin) / width))))
        ns = int(n_search)
        nfound = C.c_int(0)
        ev = np.zeros(ns)
        vec = np.empty((ns, n), dtype=complex)
        res = np.zeros(ns)
        inf = np.zeros(4, dtype=np.int32)
        _lib.check(_lib.lib.tbk_kpm_eigs(sp, _lib.dptr(k), float(w[0]), float(w[1]), emin, emax, ns, int(degree), float(tol),
                                         int(max_iter), int(seed), C.byref(nfound), _lib.dptr(ev), _lib.dptr(vec.view(float)),
                                         _lib.dptr(res), _lib.iptr(inf)))
        m = nfound.value
        evals, evecs = ev[:m].copy(), vec[:m].copy()
        if self._nspin == 2:
            evecs = evecs.reshape(m, self._norb, 2)
        if not return_info:
            return evals, evecs
        return evals, evecs, dict(residuals=res[:m].copy(), applications=int(inf[0]), rank=int(inf[1]), strong=int(inf[2]),
                                  returned=int(inf[3]), degree=int(degree), bounds=(emin, emax))

    # ------------------------------------------------------------------ k generators (host)
    def k_uniform_mesh(self, mesh_size):
        """Gamma-containing uniform mesh, last index fastest (pythtb.py:1792-1861)."""
        use = np.array(list(map(round, mesh_size)), dtype=int)
        if use.shape != (self._dim_k,):
            print(use.shape)
            raise Exception("\n\nIncorrect size of the specified k-mesh!")
        if np.min(use) <= 0:
            raise Exception("\n\nMesh must have positive non-zero number of elements.")
        if self._dim_k not in (1, 2, 3):
            raise Exception("\n\nUnsupported dim_k!")
        idx = np.indices(tuple(use)).reshape(self._dim_k, -1).T
        # a plain ndarray like the reference's; C-contiguous, so solve_all hands it to the device as is.  (solve_all always
        # solves the k list it is GIVEN; the device-generated mesh is the explicit extension solve_all_mesh.)
        return np.divide(idx, use.astype(float), order='C')

    def k_path(self, kpts, nk, report=True):
        """Piecewise-linear path through `kpts` with `nk` points, spaced by the
        Cartesian metric (pythtb.py:1863-2026).  Returns (k_vec, k_dist, k_node)."""
        if isinstance(kpts, str):
            named = {"full": [[0.0], [0.5], [1.0]], "fullc": [[-0.5], [0.0], [0.5]], "half": [[0.0], [0.5]]}
            nodes = np.array(named[kpts]) if kpts in named else np.array(kpts)
        else:
            nodes = np.array(kpts)
        if nodes.ndim == 1 and self._dim_k == 1:
            nodes = nodes.reshape(-1, 1)
        if nodes.shape[1] != self._dim_k:
            print('input k-space dimension is', nodes.shape[1])
            print('k-space dimension taken from model is', self._dim_k)
            raise Exception("\n\nk-space dimensions do not match")
        if nk < nodes.shape[0]:
            raise Exception("\n\nMust have more points in the path than number of nodes.")
        n_nodes = nodes.shape[0]
        lat_per = np.copy(self._lat)[self._per]
        k_metric = np.linalg.inv(np.dot(lat_per, lat_per.T))
        k_node = np.zeros(n_nodes, dtype=float)
        for s in range(1, n_nodes):
            dk = nodes[s] - nodes[s - 1]
            k_node[s] = k_node[s - 1] + np.sqrt(np.dot(dk, np.dot(k_metric, dk)))
        node_index = [0]
        for s in range(1, n_nodes - 1):
            node_index.append(int(round(k_node[s] / k_node[-1] * (nk - 1))))
        node_index.append(nk - 1)
        k_dist = np.zeros(nk, dtype=float)
        k_vec = np.zeros((nk, self._dim_k), dtype=float)
        k_vec[0] = nodes[0]
        for s in range(1, n_nodes):
            lo, hi = node_index[s - 1], node_index[s]
            if hi == lo:        # two nodes on one path index: the reference's 0/0 (pythtb.py:1991)
                raise ZeroDivisionError("float division by zero")
            frac = (np.arange(lo, hi + 1) - lo).astype(float) / float(hi - lo)
            k_dist[lo:hi + 1] = k_node[s - 1] + frac * (k_node[s] - k_node[s - 1])
            k_vec[lo:hi + 1] = nodes[s - 1] + frac[:, None] * (nodes[s] - nodes[s - 1])
        if report:
            if self._dim_k == 1:
                print(' Path in 1D BZ defined by nodes at ' + str(nodes.flatten()))
            else:
                print('----- k_path report begin ----------')
                keep = np.get_printoptions()
                np.set_printoptions(precision=5)
                print('real-space lattice vectors\n', lat_per)
                print('k-space metric tensor\n', k_metric)
                print('internal coordinates of nodes\n', nodes)
                if lat_per.shape[0] == lat_per.shape[1]:
                    rec = np.linalg.inv(lat_per).T
                    print('reciprocal-space lattice vectors\n', rec)
                    print('cartesian coordinates of nodes\n', np.tensordot(nodes, rec, axes=1))
                print('list of segments:')
                for s in range(1, n_nodes):
                    seg = str(round(k_node[s] - k_node[s - 1], 5)).rjust(7)
                    print('  length = ' + seg + '  from ', nodes[s - 1], ' to ', nodes[s])
                print('node distance list:', k_node)
                print('node index list:   ', np.array(node_index))
                np.set_printoptions(precision=keep["precision"])
                print('----- k_path report end ------------')
            print()
        return (k_vec, k_dist, k_node)


from . import plotting as _plotting  # noqa: E402
from . import report as _report  # noqa: E402
from . import transforms as _transforms  # noqa: E402

_transforms.install(tb_model)
tb_model.display = _report.display
tb_model.visualize = _plotting.visualize
