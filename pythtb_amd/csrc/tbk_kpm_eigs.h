// tbk_kpm_eigs.h -- the host-only parts of the windowed eigensolver on the sparse operator (tbk_kpm_eigs.hip):
// the filter coefficients, the argument checks, the workspace layout and the dense algebra of the subspace between two device
// passes.  No device call in this file: check/kpm_eigs_check.cpp runs all of it under the host sanitizers.
#pragma once
#include <cmath>
#include <cstring>
#include <vector>
#include "tbk_kpm.h"

#define KPME_GRAM_WG 256      // workgroups of the Gram kernel per block pair (grid-stride over the row tiles beyond that)
#define KPME_GRAM_ROWS 64     // rows of one of its tiles: 16 per wavefront
#define KPME_GRAM_PAIRS 64    // block pairs per launch: their partial sums take at most 32 MiB
#define KPME_PANEL 256        // rows of the rotation matrix staged in LDS at a time (x 8 columns x 16 bytes = 32 KiB)
#define KPME_MAX_SEARCH 2048  // the dense solver's limit
#define KPME_MAX_DEGREE 65536
#define KPME_DROP 1e-12       // directions of the Gram matrix at or below this fraction of its largest eigenvalue are dropped

// The window the filter is built for: [e_lo - delta, e_hi + delta], delta = 2 pi a / degree (twice the width over which the
// Jackson kernel smooths an edge, so that the filter is >= 1/2 on all of [e_lo, e_hi]), clipped to the open interval (emin, emax).
static inline void kpm_eigs_widened(double e_lo, double e_hi, double emin, double emax, int degree, double* w_lo, double* w_hi) {
    const double a = 0.5 * (emax - emin), delta = 2.0 * M_PI * a / degree, eps = 1e-9 * a;
    *w_lo = std::max(e_lo - delta, emin + eps);
    *w_hi = std::min(e_hi + delta, emax - eps);
}

// c[m], m <= degree: the Jackson-damped Chebyshev coefficients of the indicator of the widened window,
// c_0 = (th_lo - th_hi) / pi, c_m = 2 (sin m th_lo - sin m th_hi) / (m pi), th = arccos((e - b) / a)
static inline void kpm_eigs_coefficients(double e_lo, double e_hi, double emin, double emax, int degree, double* c) {
    const double a = 0.5 * (emax - emin), b = 0.5 * (emax + emin);
    double w_lo, w_hi;
    kpm_eigs_widened(e_lo, e_hi, emin, emax, degree, &w_lo, &w_hi);
    const double tl = acos((w_lo - b) / a), th = acos((w_hi - b) / a);
    const int M = degree + 1;
    const double q = M_PI / (M + 1.0);
    for (int m = 0; m < M; ++m) {
        const double g = ((M - m + 1.0) * cos(q * m) + sin(q * m) / tan(q)) / (M + 1.0);
        c[m] = g * (m == 0 ? (tl - th) / M_PI : 2.0 * (sin(m * tl) - sin(m * th)) / (m * M_PI));
    }
}

static int kpm_eigs_check_args(const tbk_sparse* sp, const double* k, double e_lo, double e_hi, double emin, double emax, int n_search,
                               int degree, double tol, int max_iter, const int* n_found, const double* eval, const double* evec,
                               const int32_t* info) {
    TBK_REQUIRE(sp && n_found && eval && evec && info, TBK_EINVAL, "tbk_kpm_eigs: null argument");
    TBK_REQUIRE(sp->dim_k == 0 || k, TBK_EINVAL, "tbk_kpm_eigs: null k-point for a model with dim_k = %d", sp->dim_k);
    TBK_REQUIRE(std::isfinite(emin) && std::isfinite(emax) && emax > emin, TBK_EINVAL, "tbk_kpm_eigs: bounds (%g, %g)", emin, emax);
    TBK_REQUIRE(std::isfinite(e_lo) && std::isfinite(e_hi) && e_lo <= e_hi, TBK_EINVAL, "tbk_kpm_eigs: empty window (%g, %g)", e_lo, e_hi);
    TBK_REQUIRE(emin < e_lo && e_hi < emax, TBK_EINVAL, "tbk_kpm_eigs: the window (%g, %g) is not inside the bounds (%.17g, %.17g)", e_lo,
                e_hi, emin, emax);
    const int top = std::min(sp->nsta - sp->nsta % KPM_NV, KPME_MAX_SEARCH);
    TBK_REQUIRE(n_search >= KPM_NV && n_search % KPM_NV == 0 && n_search <= top, TBK_EINVAL,
                "tbk_kpm_eigs: n_search=%d must be a multiple of %d in [%d, %d] (%d states)", n_search, KPM_NV, KPM_NV, top, sp->nsta);
    TBK_REQUIRE(degree >= 2 && degree <= KPME_MAX_DEGREE, TBK_EINVAL, "tbk_kpm_eigs: degree=%d (2 .. %d)", degree, KPME_MAX_DEGREE);
    TBK_REQUIRE(std::isfinite(tol) && tol > 0.0, TBK_EINVAL, "tbk_kpm_eigs: tol=%g", tol);
    TBK_REQUIRE(max_iter >= 2, TBK_EINVAL, "tbk_kpm_eigs: max_iter=%d (at least two filter applications are made)", max_iter);
    return TBK_OK;
}

// The device workspace of a call: X, Y, HY as n_search / 8 blocks [row][8]; the buffers of one series; the Gram partial sums and
// sums; the dense problem (matrix, eigenvalues, eigenvectors), the rotation matrix, the Ritz values and the residual sums.
struct KpmEigsWork {
    int n, ns, nb, degree, dim_k, gram_wg, pair_chunk;
    int64_t nnz, npairs;
    KpmPlan P;
    cd *val = nullptr, *X = nullptr, *Y = nullptr, *HY = nullptr, *cur = nullptr, *prev = nullptr, *coef = nullptr, *rot = nullptr,
       *eig_h = nullptr, *eig_v = nullptr;
    double *part = nullptr, *dots = nullptr, *rec = nullptr, *gpart = nullptr, *gram = nullptr, *theta = nullptr, *res = nullptr,
           *eig_e = nullptr, *k_dev = nullptr;
    KpmEigsWork(const tbk_sparse* sp, int n_search, int degree_)
        : n(sp->nsta), ns(n_search), nb(n_search / KPM_NV), degree(degree_), dim_k(sp->dim_k), nnz(sp->nnz), P(kpm_plan(sp->nsta, degree_)) {
        npairs = (int64_t)nb * (nb + 1) / 2;
        gram_wg = (int)std::min<int64_t>(((int64_t)n + KPME_GRAM_ROWS - 1) / KPME_GRAM_ROWS, KPME_GRAM_WG);
        pair_chunk = (int)std::min<int64_t>(npairs, KPME_GRAM_PAIRS);
    }
    size_t block_len() const { return (size_t)n * KPM_NV; }
    void carve(KpmCarve& c) {
        constexpr int NV = KPM_NV, NC = 2 * NV;
        c.take(val, dim_k > 0 ? (size_t)nnz : 0);
        c.take(X, (size_t)nb * block_len());
        c.take(Y, (size_t)nb * block_len());
        c.take(HY, (size_t)nb * block_len());
        c.take(cur, block_len());
        c.take(prev, block_len());
        c.take(coef, (size_t)degree + 1);
        c.take(part, P.part_len());
        c.take(dots, (size_t)(degree + 1) * NC);
        c.take(rec, (size_t)KPMS_GUARD);
        c.take(gpart, (size_t)pair_chunk * 4 * NV * NV * gram_wg);
        c.take(gram, (size_t)npairs * 4 * NV * NV);
        c.take(rot, (size_t)ns * ns);
        c.take(eig_h, (size_t)ns * ns);
        c.take(eig_v, (size_t)ns * ns);
        c.take(eig_e, (size_t)ns);
        c.take(theta, (size_t)ns);
        c.take(res, (size_t)nb * NC);
        c.take(k_dev, (size_t)std::max(dim_k, 1));
    }
};

// G and A (ns x ns, row-major, exactly Hermitian) from the sums of the upper block triangle: gram[pair][4][8][8], the components
// (Re G, Im G, Re A, Im A) of block (p, q), p <= q, element (i, j); pairs in the order (0,0), (0,1) .. (0,nb-1), (1,1) ...
static inline void kpm_eigs_assemble(int nb, const double* gram, cd* G, cd* A) {
    constexpr int NV = KPM_NV, BL = NV * NV;
    const int ns = nb * NV;
    int64_t pair = 0;
    for (int p = 0; p < nb; ++p)
        for (int q = p; q < nb; ++q, ++pair) {
            const double* s = gram + pair * 4 * BL;
            for (int i = 0; i < NV; ++i)
                for (int j = (p == q ? i : 0); j < NV; ++j) {
                    const int r = p * NV + i, c = q * NV + j, e = i * NV + j;
                    cd g{s[e], s[BL + e]}, h{s[2 * BL + e], s[3 * BL + e]};
                    if (r == c) g.y = h.y = 0.0;
                    G[(size_t)r * ns + c] = g;
                    A[(size_t)r * ns + c] = h;
                    G[(size_t)c * ns + r] = cconj(g);
                    A[(size_t)c * ns + r] = cconj(h);
                }
        }
}

// The directions kept of eigh(G) = U lam U^H (lam ascending, U[d][i] = component i of direction d): those with
// lam > KPME_DROP lam_max, in ascending order.  wh[r][i] = U[d_r][i] / sqrt(lam_r): the rows of Wh^T.  Returns the rank.
static inline int kpm_eigs_whiten(int ns, const double* lam, const cd* U, cd* wh) {
    double top = 0.0;
    for (int d = 0; d < ns; ++d)
        if (lam[d] > top) top = lam[d];
    int rank = 0;
    if (!(top > 0.0) || !std::isfinite(top)) return 0;
    for (int d = 0; d < ns; ++d) {
        if (!(lam[d] > KPME_DROP * top)) continue;
        const double s = 1.0 / sqrt(lam[d]);
        for (int i = 0; i < ns; ++i) wh[(size_t)rank * ns + i] = cscale(U[(size_t)d * ns + i], s);
        ++rank;
    }
    return rank;
}

// B = Wh^H A Wh (rank x rank, row-major, made exactly Hermitian); tmp: rank x ns
static inline void kpm_eigs_project(int ns, int rank, const cd* A, const cd* wh, cd* tmp, cd* B) {
    for (int s = 0; s < rank; ++s)          // tmp[s][i] = sum_j A[i][j] Wh[j][s]
        for (int i = 0; i < ns; ++i) {
            cd t{0.0, 0.0};
            for (int j = 0; j < ns; ++j) cfma(t, A[(size_t)i * ns + j], wh[(size_t)s * ns + j]);
            tmp[(size_t)s * ns + i] = t;
        }
    for (int r = 0; r < rank; ++r)
        for (int s = r; s < rank; ++s) {
            cd t{0.0, 0.0}, u{0.0, 0.0};
            for (int i = 0; i < ns; ++i) {
                cfmac(t, wh[(size_t)r * ns + i], tmp[(size_t)s * ns + i]);
                cfmac(u, wh[(size_t)s * ns + i], tmp[(size_t)r * ns + i]);
            }
            cd h{0.5 * (t.x + u.x), 0.5 * (t.y - u.y)};
            if (r == s) h.y = 0.0;
            B[(size_t)r * rank + s] = h;
            B[(size_t)s * rank + r] = cconj(h);
        }
}

// rot[i][s] = sum_r Wh[i][r] W[r][s] for s < rank, zero beyond (ns x ns, row-major: row = column of Y, column = column of X);
// Wv[s][r] = component r of Ritz vector s
static inline void kpm_eigs_rotation(int ns, int rank, const cd* wh, const cd* Wv, cd* rot) {
    std::memset((void*)rot, 0, (size_t)ns * ns * sizeof(cd));
    for (int s = 0; s < rank; ++s)
        for (int r = 0; r < rank; ++r) {
            const cd w = Wv[(size_t)s * rank + r];
            for (int i = 0; i < ns; ++i) cfma(rot[(size_t)i * ns + s], wh[(size_t)r * ns + i], w);
        }
}

// The stop test on the Ritz pairs of the previous iteration (theta, resid: the first `rank` entries) with the filter norms tau of
// this one: strong = tau >= 1/2, selected = strong and e_lo <= theta <= e_hi.  sel[]: the indices selected, ascending in theta.
struct KpmEigsVerdict {
    int nstrong = 0, nsel = 0;
    double worst = 0.0;       // the largest residual of a selected pair
    bool converged = false;   // every selected pair has resid <= limit
    bool room = false;        // nstrong < rank: the subspace holds more than the window's states
};
static inline KpmEigsVerdict kpm_eigs_verdict(int rank, const double* theta, const double* resid, const double* tau, double e_lo,
                                              double e_hi, double limit, int* sel) {
    KpmEigsVerdict v;
    v.converged = true;
    for (int j = 0; j < rank; ++j) {
        if (!(tau[j] >= 0.5)) continue;
        ++v.nstrong;
        if (!(theta[j] >= e_lo && theta[j] <= e_hi)) continue;
        int at = v.nsel++;
        while (at > 0 && theta[sel[at - 1]] > theta[j]) {       // insertion: the Ritz values arrive ascending already
            sel[at] = sel[at - 1];
            --at;
        }
        sel[at] = j;
        if (!(resid[j] <= limit)) v.converged = false;          // a NaN misses every limit
        if (!(resid[j] <= v.worst) && v.worst == v.worst) v.worst = resid[j];
    }
    v.room = v.nstrong < rank;
    return v;
}
