// tbk_orbmag.hip -- orbital moments and orbital magnetization by the Kubo formula on k lists and uniform meshes (DESIGN.md
// section 13).
//
// k reduced, H the convention-II matrix of tbk_gen_ham, V^d = d_d H (tbk_gen_dham), E_n and |n> the eigenpairs of the solver,
// (a, b) = (dir0, dir1), P_nm = Im V^a_nm V^b_mn, Delta_nm = E_n - E_m:
//   moment (1)       m_n = sum_{m != n} P_nm / (E_m - E_n), beside Omega_n = -2 sum_{m != n} P_nm / Delta^2 (tbk_curv.hip); a pair with
//                    |Delta| <= 1e-9 max(1, |E_n|, |E_m|) contributes to neither
//   band set (2)     over n in occ, m not in occ (no degeneracy rule): LC = sum P_nm E_m / Delta^2, IC = sum P_nm E_n / Delta^2,
//                    Omega_occ = -2 sum P_nm / Delta^2
//   T = 0 scan (3)   M(mu) = mean_k sum_{E_n <= mu} [m_n + (mu - E_n) Omega_n] = A(mu) + mu I(mu), A the same sum of m_n - E_n Omega_n
//   kT > 0 (4)       M(mu, T) = mean_k sum_n [f_n m_n + g_n Omega_n], f = 1 / (1 + e^x), g = kT ln(1 + e^-x), x = (E_n - mu) / kT
//
// Forms, routed as in tbk_curv.hip:
//   n = 2     one lane per k from curv2_point (no eigen-solve): m_0 = m_1 = (E_0 - E_1) Omega_0 / 2.  On a mesh the lane feeds the
//             plane and T = 0 reductions directly; for kT > 0 it writes the (E, m, Omega) records.
//   n != 2    chunks of kOrbChunkBytes of eigenvectors through the solver, then up to 32 states k_orb_lds (k_curv_lds with two
//             accumulators per (point, band) lane, three for a band set); from 33 states k_curv_wsp's W^d and k_orb_contract.
// Reductions: k_orb_plane (the three band-set sums in one pass), k_orb_fermi (the bins of k_curv_fermi for two quantities), k_orb_kt
// (levels across lanes, records read as wave-uniform values, sums in registers), k_orb_rows.  Every partition depends on the mesh,
// n and the number of levels alone, and nothing uses atomics: two calls give the same bits.
#include <math.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>
#include "tbk_dham.h"

static const size_t kOrbChunkBytes = (size_t)32 << 20;   // eigenvectors per chunk (the budget of section 11)
static const int kOrbWin = 2048;                         // levels per LDS window of k_orb_fermi (two quantities: 32 KiB of bins)
static const int kOrbKtTile = 256;                       // levels per workgroup of k_orb_kt (one per lane)
static const int kOrbKtGroupsMax = 1024;                 // k-groups of k_orb_kt at most

// ---------------------------------------------------------------- n = 2: closed form in registers
// list form: out[2][nk] = m (occ_sign == 0), or out[nk] = LC + IC of the band set {0} (occ_sign = +1) or {1} (-1)
__global__ __launch_bounds__(256) void k_orb2_list(const ModelView mv, const int64_t nk, const double* __restrict__ k, const int d0,
                                                   const int d1, const int occ_sign, double* __restrict__ out) {
    const int64_t ik = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (ik >= nk) return;
    double kk[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) kk[d] = d < mv.dim_k ? k[ik * mv.dim_k + d] : 0.0;
    const Curv2 c = curv2_point(mv, kk, d0, d1);
    if (occ_sign == 0) {
        const double w = c.degenerate ? 0.0 : 0.5 * (c.e0 - c.e1) * c.om;
        out[ik] = w;
        out[nk + ik] = w;
    } else {
        out[ik] = -0.5 * (c.e0 + c.e1) * (occ_sign > 0 ? c.om : -c.om);   // P / Delta^2 = -Omega_occ / 2, times E_0 + E_1
    }
}

// Sources of per-point values for the reductions.  band(): Omega_ch (degeneracy rule), a = m_ch - E_ch Omega_ch and E_ch;
// set(): (LC, IC, Omega_occ) of the band set.
struct Orb2Src {
    ModelView mv;
    int d0, d1, occ_sign;
    __device__ __forceinline__ Curv2 at(const PlaneArgs& P, const int (&ii)[3]) const {
        double kk[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int d = 0; d < 3; ++d)
            if (d < mv.dim_k) kk[d] = (double)ii[d] / (double)P.N[d];   // k_uniform_mesh's point, bit for bit
        return curv2_point(mv, kk, d0, d1);
    }
    __device__ __forceinline__ double band(const PlaneArgs& P, const int (&ii)[3], int64_t, const int ch, double& e, double& a) const {
        const Curv2 c = at(P, ii);
        e = ch ? c.e1 : c.e0;
        const double w = c.degenerate ? 0.0 : c.om;
        const double o = ch ? -w : w;
        a = -0.5 * (c.e0 + c.e1) * o;   // sum_m P_nm (E_n + E_m) / Delta^2
        return o;
    }
    __device__ __forceinline__ void set(const PlaneArgs& P, const int (&ii)[3], int64_t, double& lc, double& ic, double& om) const {
        const Curv2 c = at(P, ii);
        om = occ_sign > 0 ? c.om : -c.om;   // the manifold value of tbk_curv.hip, bit for bit
        const double h = -0.5 * om;
        lc = h * (occ_sign > 0 ? c.e1 : c.e0);
        ic = h * (occ_sign > 0 ? c.e0 : c.e1);
    }
};
struct OrbArraySrc {
    const double* ev;   // [n][npts] (per band)
    const double* mm;
    const double* om;
    const double* st;   // [3][npts] (band set)
    __device__ __forceinline__ double band(const PlaneArgs& P, const int (&)[3], const int64_t idx, const int ch, double& e,
                                           double& a) const {
        const int64_t i = (int64_t)ch * P.npts + idx;
        e = ev[i];
        const double o = om[i];
        a = mm[i] - e * o;
        return o;
    }
    __device__ __forceinline__ void set(const PlaneArgs& P, const int (&)[3], const int64_t idx, double& lc, double& ic,
                                        double& om) const {
        lc = st[idx];
        ic = st[P.npts + idx];
        om = st[2 * P.npts + idx];
    }
};

// n = 2 records for kT > 0: ev, mm, om [2][npts] of every mesh point (degenerate pairs: m = Omega = 0)
__global__ __launch_bounds__(256) void k_orb2_records(const ModelView mv, const PlaneArgs P, const int d0, const int d1,
                                                      double* __restrict__ ev, double* __restrict__ mm, double* __restrict__ om) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= P.npts) return;
    int ii[3];
    const int64_t i01 = idx / P.N[2];
    ii[2] = (int)(idx - i01 * P.N[2]);
    ii[0] = (int)(i01 / P.N[1]);
    ii[1] = (int)(i01 - (int64_t)ii[0] * P.N[1]);
    const Orb2Src src{mv, d0, d1, 0};
    const Curv2 c = src.at(P, ii);
    const double w = c.degenerate ? 0.0 : c.om;
    const double m = c.degenerate ? 0.0 : 0.5 * (c.e0 - c.e1) * c.om;
    ev[idx] = c.e0;
    ev[P.npts + idx] = c.e1;
    mm[idx] = m;
    mm[P.npts + idx] = m;
    om[idx] = w;
    om[P.npts + idx] = -w;
}

// ---------------------------------------------------------------- reductions
// band-set plane sums: blockIdx.x = g of gx, blockIdx.y = slice s (and every gridDim.y after it); part[s][c][gx], c = LC, IC, Omega.
// Each sum runs in k_curv_plane's order (and the Omega sum is its manifold sum, bit for bit).
template <class Src>
__global__ __launch_bounds__(256) void k_orb_plane(const Src src, const PlaneArgs P, double* __restrict__ part) {
    __shared__ double red[3][4];
    for (int s = blockIdx.y; s < P.nslice; s += gridDim.y) {
        double acc[3] = {0.0, 0.0, 0.0};
        for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < P.nplane; p += (int64_t)gridDim.x * 256) {
            int ii[3];
            const int64_t idx = plane_point(P, s, p, ii);
            double lc, ic, om;
            src.set(P, ii, idx, lc, ic, om);
            acc[0] += lc;
            acc[1] += ic;
            acc[2] += om;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double t = block_sum(acc[c], red[c]);
            if (threadIdx.x == 0) part[((int64_t)s * 3 + c) * gridDim.x + blockIdx.x] = t;
        }
        __syncthreads();                                          // (red is reused by the next slice)
    }
}

// T = 0 scan: every (point, band) item of slice s adds (Omega_n, m_n - E_n Omega_n) to the bins of the first sorted level
// mu_j >= E_n -- k_curv_fermi with two quantities.  blockIdx.x = g of gx, blockIdx.y = slice, blockIdx.z = window of kOrbWin
// levels.  part[s][j][2][gx]
template <class Src>
__global__ __launch_bounds__(256) void k_orb_fermi(const Src src, const PlaneArgs P, const int nb, const double* __restrict__ mu,
                                                   const int nmu, double* __restrict__ part) {
    __shared__ double bins[2][kOrbWin];
    __shared__ double tw[2][256];
    __shared__ int tb[256];
    for (int s = blockIdx.y; s < P.nslice; s += gridDim.y) {
        const int w0 = blockIdx.z * kOrbWin, wn = min(kOrbWin, nmu - w0);
        for (int j = threadIdx.x; j < kOrbWin; j += 256) bins[0][j] = bins[1][j] = 0.0;
        const int per = (wn + 255) / 256;
        const int lo = threadIdx.x * per, hi = min(wn, lo + per);
        const int64_t total = P.nplane * nb;
        for (int64_t t0 = (int64_t)blockIdx.x * 256; t0 < total; t0 += (int64_t)gridDim.x * 256) {
            const int64_t it = t0 + threadIdx.x;
            int bin = -1;
            double w = 0.0, a = 0.0;
            if (it < total) {
                const int64_t p = it / nb;
                const int band = (int)(it - p * nb);
                int ii[3];
                const int64_t idx = plane_point(P, s, p, ii);
                double e;
                w = src.band(P, ii, idx, band, e, a);
                int l = 0, r = nmu;                  // first j with mu[j] >= e (nmu: above every level; NaN: nowhere)
                while (l < r) {
                    const int m = (l + r) >> 1;
                    if (mu[m] < e) l = m + 1;
                    else r = m;
                }
                bin = e == e ? l - w0 : -1;
            }
            __syncthreads();                         // the previous tile's items are consumed
            tb[threadIdx.x] = bin;
            tw[0][threadIdx.x] = w;
            tw[1][threadIdx.x] = a;
            __syncthreads();
            for (int q = 0; q < 256; ++q) {
                const int b = tb[q];
                if (b >= lo && b < hi) {
                    bins[0][b] += tw[0][q];
                    bins[1][b] += tw[1][q];
                }
            }
        }
        __syncthreads();
        for (int j = threadIdx.x; j < wn; j += 256) {
            double* o = part + ((int64_t)s * nmu + w0 + j) * 2 * gridDim.x + blockIdx.x;
            o[0] = bins[0][j];
            o[gridDim.x] = bins[1][j];
        }
        __syncthreads();                                           // (bins are reused by the next slice)
    }
}

// kT > 0 scan.  Workgroup (tile of kOrbKtTile levels, k-group g, slice s): lane t takes level j = tile + t and walks the records
// (E, m, Omega) of the plane points [g nplane / G, (g + 1) nplane / G) of slice s, every band of a point in order; a record's
// address depends on the workgroup and the loop alone, so it is read as a wave-uniform value.  Per (record, level) one exp, one
// log1p and one division:  t = e^{-|x|},  f = 1 / (1 + t) (x < 0) or t / (1 + t),  g = kT log1p(t) (x >= 0) or
// mu - E + kT log1p(t).  part[s][j][G]
__global__ __launch_bounds__(256) void k_orb_kt(const PlaneArgs P, const int nb, const double* __restrict__ ev,
                                                const double* __restrict__ mm, const double* __restrict__ om,
                                                const double* __restrict__ mu, const int nmu, const double kT, const int G,
                                                double* __restrict__ part) {
    const int base = blockIdx.x * kOrbKtTile;
    if (base + (int)(threadIdx.x & ~63u) >= nmu) return;            // a wavefront without a level (uniform)
    const int j = base + threadIdx.x, g = blockIdx.y;
    const double u = j < nmu ? mu[j] : 0.0;
    const double ikT = 1.0 / kT;
    const int64_t p0 = (int64_t)g * P.nplane / G, p1 = (int64_t)(g + 1) * P.nplane / G;
    for (int s = blockIdx.z; s < P.nslice; s += gridDim.z) {
        double acc = 0.0;
        for (int64_t p = p0; p < p1; ++p) {
            int ii[3];
            const int64_t idx = plane_point(P, s, p, ii);
            for (int b = 0; b < nb; ++b) {
                const int64_t i = (int64_t)b * P.npts + idx;
                const double e = ev[i], m = mm[i], o = om[i];
                const double x = (e - u) * ikT;
                const double t = exp(-fabs(x));
                const double r = 1.0 / (1.0 + t);
                const double l = kT * log1p(t);
                const bool up = x >= 0.0;
                const double f = up ? t * r : r;
                const double gg = up ? l : (u - e) + l;
                acc = fma(f, m, fma(gg, o, acc));
            }
        }
        if (j < nmu) part[((int64_t)s * nmu + j) * G + g] = acc;
    }
}

// out[r] = sum_g part[r][g] in a fixed order (one workgroup per row)
__global__ __launch_bounds__(256) void k_orb_rows(const double* __restrict__ part, const int gx, double* __restrict__ out) {
    __shared__ double red[4];
    const double* p = part + (int64_t)blockIdx.x * gx;
    double acc = 0.0;
    for (int g = threadIdx.x; g < gx; g += 256) acc += p[g];
    const double t = block_sum(acc, red);
    if (threadIdx.x == 0) out[blockIdx.x] = t;
}

// ---------------------------------------------------------------- n != 2: contraction of the solver's eigenvectors
// Up to 32 states: k_curv_lds's kernel -- P points per workgroup, U, d_{d0} H, d_{d1} H and T in LDS, V^{d0} formed in LDS, V^{d1}
// on the fly -- whose (point, band) lane keeps Omega's and m's weights of the same P_nm (per band: mm[b], om[b] and ev[b] at
// [nfull] stride, om and ev nullable) or the band's shares of LC, IC and Omega_occ, which the workgroup sums per point into
// st[c][nfull] (c = LC, IC, Omega; Omega_occ as k_curv_lds forms it, bit for bit).
#define ORB_LDS_CD 4096
static inline int orb_lds_points(int n) { return std::max(1, std::min(64, ORB_LDS_CD / (4 * n * n))); }
__global__ __launch_bounds__(256) void k_orb_lds(const ModelView mv, const double* __restrict__ k, const cd* __restrict__ evec,
                                                 const double* __restrict__ eval, const int64_t nk, const int d0, const int d1,
                                                 const int P, const int* __restrict__ occ, const int64_t first, const int64_t nfull,
                                                 double* __restrict__ mm, double* __restrict__ om, double* __restrict__ ev,
                                                 double* __restrict__ st) {
    __shared__ cd L[ORB_LDS_CD];
    const int n = mv.nsta, nn = n * n;
    const int64_t ik0 = (int64_t)blockIdx.x * P;
    const int np = (int)std::min<int64_t>(P, nk - ik0);
    cd* U = L;
    cd* D = L + P * nn;
    cd* T = L + 2 * P * nn;
    cd* X = L + 3 * P * nn;
    for (int e = threadIdx.x; e < np * nn; e += 256) {
        const int p = e / nn, r = e - p * nn, b = r / n, i = r - b * n;
        U[e] = evec[((int64_t)b * nk + ik0 + p) * n + i];
        D[e] = cd{0.0, 0.0};
        X[e] = cd{0.0, 0.0};
    }
    __syncthreads();
    for (int e = threadIdx.x; e < np * mv.nnz; e += 256) {
        const int p = e / mv.nnz;
        const int4 z4 = mv.nz[e - p * mv.nnz];
        const int a = z4.x & 0xffff, b = z4.x >> 16;
        double kk[4];
        cd z[4];
        k_phases(mv, k, ik0 + p, kk, z);
        cd h, v0, v1;
        dham_terms(mv, a, b, z4.y, z4.z, kk, z, d0, d1, h, v0, v1);
        D[p * nn + a * n + b] = v0;
        D[p * nn + b * n + a] = cconj(v0);
        X[p * nn + a * n + b] = v1;
        X[p * nn + b * n + a] = cconj(v1);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < np * nn; e += 256) {            // T = D U^T
        const int p = e / nn, r = e - p * nn, i = r / n, c = r - i * n;
        const cd* dr = D + p * nn + i * n;
        const cd* uc = U + p * nn + c * n;
        cd acc{0.0, 0.0};
        for (int j = 0; j < n; ++j) cfma(acc, dr[j], uc[j]);
        T[e] = acc;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < np * nn; e += 256) {            // D := V^{d0} = conj(U) T   (reads U, T only)
        const int p = e / nn, r = e - p * nn, b = r / n, c = r - b * n;
        const cd* ub = U + p * nn + b * n;
        const cd* tc = T + p * nn + c;
        cd acc{0.0, 0.0};
        for (int i = 0; i < n; ++i) cfmac(acc, ub[i], tc[i * n]);
        D[e] = acc;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < np * nn; e += 256) {            // T := X U^T
        const int p = e / nn, r = e - p * nn, i = r / n, c = r - i * n;
        const cd* xr = X + p * nn + i * n;
        const cd* uc = U + p * nn + c * n;
        cd acc{0.0, 0.0};
        for (int j = 0; j < n; ++j) cfma(acc, xr[j], uc[j]);
        T[e] = acc;
    }
    __syncthreads();
    double* share = (double*)X;                                    // (X is dead: the band shares of (2), 3 np n <= 2 P n^2 doubles)
    for (int e = threadIdx.x; e < np * n; e += 256) {
        const int p = e / n, b = e - p * n;
        const int64_t ik = ik0 + p;
        const double eb = eval[(int64_t)b * nk + ik];
        const cd* ub = U + p * nn + b * n;
        const cd* va = D + p * nn + b * n;
        const cd* tp = T + p * nn;
        double acc = 0.0, acm = 0.0;                               // sum P / Delta^2; sum P / (E_m - E_b) or sum P E_m / Delta^2
        if (!occ || occ[b]) {
            for (int m = 0; m < n; ++m) {
                if (m == b) continue;
                const double em = eval[(int64_t)m * nk + ik];
                const double de = eb - em;
                if (occ) {
                    if (occ[m]) continue;
                } else if (!(fabs(de) > 1e-9 * fmax(1.0, fmax(fabs(eb), fabs(em))))) {
                    continue;
                }
                cd vb{0.0, 0.0};
                for (int i = 0; i < n; ++i) cfmac(vb, ub[i], tp[i * n + m]);
                const cd a = va[m];
                const double pr = a.y * vb.x - a.x * vb.y;         // Im V^a_bm V^b_mb = Im V^a_bm conj(V^b_bm)
                const double w = pr / (de * de);
                acc += w;
                if (occ) acm += w * em;
                else acm += pr / (em - eb);
            }
        }
        const double o = -2.0 * acc;
        if (occ) {
            share[3 * e] = acm;
            share[3 * e + 1] = eb * acc;
            share[3 * e + 2] = o;
        } else {
            const int64_t i = (int64_t)b * nfull + first + ik;
            mm[i] = acm;
            if (om) om[i] = o;
            if (ev) ev[i] = eb;
        }
    }
    if (occ) {
        __syncthreads();
        for (int p = threadIdx.x; p < np; p += 256) {
            double s0 = 0.0, s1 = 0.0, s2 = 0.0;
            for (int b = 0; b < n; ++b) {
                const double* sh = share + 3 * (p * n + b);
                s0 += sh[0];
                s1 += sh[1];
                s2 += sh[2];
            }
            st[first + ik0 + p] = s0;
            st[nfull + first + ik0 + p] = s1;
            st[2 * nfull + first + ik0 + p] = s2;
        }
    }
}

// 33..2048 states, one lane per (ik, band b) on k_curv_wsp's W^d: V^d_{b,m} = sum_i conj(u_b[i]) W^d[i][m], the two weights of
// k_orb_lds.  Per band: mm/om/ev [b][first + ik] as k_orb_lds; band set: tmp[ik][b][3], summed per point by k_orb_occ_sum.
__global__ __launch_bounds__(256) void k_orb_contract(const cd* __restrict__ evec, const double* __restrict__ eval,
                                                      const cd* __restrict__ wt, const int64_t nk, const int n,
                                                      const int* __restrict__ occ, const int64_t first, const int64_t nfull,
                                                      double* __restrict__ mm, double* __restrict__ om, double* __restrict__ ev,
                                                      double* __restrict__ tmp) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nk * n) return;
    const int64_t ik = idx / n;
    const int b = (int)(idx - ik * n);
    const int64_t nn = (int64_t)n * n;
    const cd* u = evec + ((int64_t)b * nk + ik) * n;
    const cd* w0 = wt + (2 * ik) * nn;
    const cd* w1 = w0 + nn;
    const double eb = eval[(int64_t)b * nk + ik];
    double acc = 0.0, acm = 0.0;
    if (!occ || occ[b]) {
        for (int m = 0; m < n; ++m) {
            if (m == b) continue;
            const double em = eval[(int64_t)m * nk + ik];
            const double de = eb - em;
            if (occ) {
                if (occ[m]) continue;
            } else if (!(fabs(de) > 1e-9 * fmax(1.0, fmax(fabs(eb), fabs(em))))) {
                continue;
            }
            cd va{0.0, 0.0}, vb{0.0, 0.0};
            for (int i = 0; i < n; ++i) {
                cfmac(va, u[i], w0[(int64_t)i * n + m]);
                cfmac(vb, u[i], w1[(int64_t)i * n + m]);
            }
            const double pr = va.y * vb.x - va.x * vb.y;           // Im V^a_bm V^b_mb = Im V^a_bm conj(V^b_bm)
            const double w = pr / (de * de);
            acc += w;
            if (occ) acm += w * em;
            else acm += pr / (em - eb);
        }
    }
    const double o = -2.0 * acc;
    if (occ) {
        double* t = tmp + 3 * idx;
        t[0] = acm;
        t[1] = eb * acc;
        t[2] = o;
    } else {
        const int64_t i = (int64_t)b * nfull + first + ik;
        mm[i] = acm;
        if (om) om[i] = o;
        if (ev) ev[i] = eb;
    }
}

__global__ __launch_bounds__(256) void k_orb_occ_sum(const double* __restrict__ tmp, const int64_t nk, const int n,
                                                     const int64_t nfull, double* __restrict__ st) {
    const int64_t ik = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (ik >= nk) return;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int b = 0; b < n; ++b) {
        const double* t = tmp + 3 * (ik * n + b);
        s0 += t[0];
        s1 += t[1];
        s2 += t[2];
    }
    st[ik] = s0;
    st[nfull + ik] = s1;
    st[2 * nfull + ik] = s2;
}

// ---------------------------------------------------------------- host side
static inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
static inline unsigned nblk(int64_t threads) { return (unsigned)((threads + 255) / 256); }

// the argument checks of tbk_curv.hip; *mask (n entries) = 1 for the bands of occ
static int orb_check(const char* fn, tbk_model* m, int dir0, int dir1, const int32_t* occ, int nocc, std::vector<int>& mask) {
    TBK_REQUIRE(m, TBK_EINVAL, "%s: null model", fn);
    TBK_REQUIRE(m->dim_k >= 2, TBK_EINVAL, "%s: the orbital moment needs dim_k >= 2 (the model has %d)", fn, m->dim_k);
    TBK_REQUIRE(dir0 >= 0 && dir0 < m->dim_k && dir1 >= 0 && dir1 < m->dim_k && dir0 != dir1, TBK_EINVAL,
                "%s: dirs (%d, %d) must be two different axes in [0, %d)", fn, dir0, dir1, m->dim_k);
    const int n = m->nsta;
    mask.clear();
    if (occ) {
        TBK_REQUIRE(nocc >= 1 && nocc <= n, TBK_EINVAL, "%s: nocc=%d (1..%d)", fn, nocc, n);
        mask.assign(n, 0);
        for (int i = 0; i < nocc; ++i) {
            TBK_REQUIRE(occ[i] >= 0 && occ[i] < n, TBK_EINVAL, "%s: occ[%d]=%d outside [0, %d)", fn, i, occ[i], n);
            TBK_REQUIRE(!mask[occ[i]], TBK_EINVAL, "%s: band %d appears twice in occ", fn, occ[i]);
            mask[occ[i]] = 1;
        }
    } else {
        TBK_REQUIRE(nocc == 0, TBK_EINVAL, "%s: nocc=%d without occ", fn, nocc);
    }
    return TBK_OK;
}

// The n != 2 pipeline over points [0, nk): k from k_all (list) or generated from `mesh`, in chunks.  Per band: mm[n][nk]
// (+ om, ev [n][nk] when set); band set: st[3][nk].  `work` is scratch behind the caller's buffers.
struct OrbWork {
    size_t bytes;
    int64_t chunk;
};
static OrbWork orb_work_size(int n, int dim_k, int64_t nk, bool manifold) {
    const size_t vb = (size_t)n * n * sizeof(cd);
    int64_t chunk = std::max<int64_t>(1, (int64_t)(kOrbChunkBytes / vb));
    chunk = std::min<int64_t>(chunk, std::max<int64_t>(nk, 1));
    const bool wide = n > 32;
    size_t b = al256((size_t)chunk * dim_k * sizeof(double)) + al256((size_t)chunk * n * sizeof(double)) + al256((size_t)chunk * vb) +
               (wide ? al256(2 * (size_t)chunk * vb) : 0) + al256((size_t)n * sizeof(int)) +
               (wide && manifold ? al256(3 * (size_t)chunk * n * sizeof(double)) : 0);
    return OrbWork{b, chunk};
}
static int orb_general(tbk_model* m, const double* k_all_dev, const int32_t* mesh, int64_t nk, int d0, int d1,
                       const std::vector<int>& mask, unsigned char* work, const OrbWork& cw, double* mm, double* om, double* ev,
                       double* st) {
    tbk_ctx* ctx = m->ctx;
    const int n = m->nsta, dk = m->dim_k;
    const int64_t chunk = cw.chunk;
    const size_t vb = (size_t)n * n * sizeof(cd);
    const bool wide = n > 32;
    unsigned char* p = work;
    double* kc = (double*)p;
    p += al256((size_t)chunk * dk * sizeof(double));
    double* ec = (double*)p;
    p += al256((size_t)chunk * n * sizeof(double));
    cd* vc = (cd*)p;
    p += al256((size_t)chunk * vb);
    cd* wt = (cd*)p;
    p += wide ? al256(2 * (size_t)chunk * vb) : 0;
    int* occ_dev = (int*)p;
    p += al256((size_t)n * sizeof(int));
    double* tmp = (double*)p;
    const bool manifold = !mask.empty();
    const int* occ_arg = manifold ? (const int*)occ_dev : (const int*)nullptr;
    if (manifold) TBK_HIP(hipMemcpyAsync(occ_dev, mask.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    for (int64_t first = 0; first < nk; first += chunk) {
        const int64_t cnt = std::min<int64_t>(chunk, nk - first);
        const double* kp;
        if (mesh) {
            int rc = tbk_k_uniform_mesh_range_dev(ctx, dk, mesh, first, cnt, kc);
            if (rc) return rc;
            kp = kc;
        } else {
            kp = k_all_dev + first * dk;
        }
        int rc = tbk_solve_list_dev_checked(m, kp, cnt, ec, (double*)vc);
        if (rc) return rc;
        if (!wide) {
            const int P = orb_lds_points(n);
            ProfScope ps(ctx, "orb_lds");
            hipLaunchKernelGGL(k_orb_lds, dim3((unsigned)((cnt + P - 1) / P)), dim3(256), 0, ctx->stream, m->view, kp, (const cd*)vc,
                               (const double*)ec, cnt, d0, d1, P, occ_arg, first, nk, mm, om, ev, st);
            TBK_HIP(hipGetLastError());
            continue;
        }
        {
            ProfScope ps(ctx, "orb_wsp");
            hipLaunchKernelGGL(k_curv_wsp, dim3((unsigned)cnt, (unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, m->view, kp,
                               (const cd*)vc, cnt, d0, d1, wt);
            TBK_HIP(hipGetLastError());
        }
        {
            ProfScope ps(ctx, "orb_contract");
            hipLaunchKernelGGL(k_orb_contract, dim3(nblk(cnt * n)), dim3(256), 0, ctx->stream, (const cd*)vc, (const double*)ec,
                               (const cd*)wt, cnt, n, occ_arg, first, nk, mm, om, ev, tmp);
            TBK_HIP(hipGetLastError());
        }
        if (manifold) {
            ProfScope ps(ctx, "orb_occ_sum");
            hipLaunchKernelGGL(k_orb_occ_sum, dim3(nblk(cnt)), dim3(256), 0, ctx->stream, (const double*)tmp, cnt, n, nk, st + first);
            TBK_HIP(hipGetLastError());
        }
    }
    return TBK_OK;
}

extern "C" int tbk_orb_moment_list(tbk_model* m, const double* k, int64_t nk, int dir0, int dir1, const int32_t* occ, int nocc,
                                   double* out) {
    std::vector<int> mask;
    int rc = orb_check("tbk_orb_moment_list", m, dir0, dir1, occ, nocc, mask);
    if (rc) return rc;
    TBK_REQUIRE(nk >= 0 && out && (k || nk == 0), TBK_EINVAL, "tbk_orb_moment_list: bad k list or output");
    const int n = m->nsta, dk = m->dim_k;
    const bool manifold = occ != nullptr;
    const int64_t nout = manifold ? nk : (int64_t)n * nk;
    if (nk == 0) return TBK_OK;
    if (n < 2 || (manifold && nocc == n)) {   // no pair to sum
        std::fill(out, out + nout, 0.0);
        return TBK_OK;
    }
    tbk_ctx* ctx = m->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    const int64_t ndev = manifold && n != 2 ? 3 * nk : nout;   // a band set of the n != 2 path: st[3][nk]
    const size_t kb = al256((size_t)nk * dk * sizeof(double)), ob = al256((size_t)ndev * sizeof(double));
    const OrbWork cw = n == 2 ? OrbWork{0, 0} : orb_work_size(n, dk, nk, manifold);
    void* base = nullptr;
    rc = tbk_ctx_scratch(ctx, 256 + kb + ob + cw.bytes, &base);
    if (rc) return rc;
    unsigned char* p = (unsigned char*)base + 256;
    double* k_dev = (double*)p;
    double* o_dev = (double*)(p + kb);
    TBK_HIP(hipMemcpyAsync(k_dev, k, (size_t)nk * dk * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (n == 2) {
        ProfScope ps(ctx, "orb2_list");
        const int sign = manifold ? (mask[0] ? 1 : -1) : 0;
        hipLaunchKernelGGL(k_orb2_list, dim3(nblk(nk)), dim3(256), 0, ctx->stream, m->view, nk, (const double*)k_dev, dir0, dir1, sign,
                           o_dev);
        TBK_HIP(hipGetLastError());
    } else {
        rc = orb_general(m, k_dev, nullptr, nk, dir0, dir1, mask, p + kb + ob, cw, manifold ? nullptr : o_dev, nullptr, nullptr,
                         manifold ? o_dev : nullptr);
        if (rc) return rc;
    }
    if (manifold && n != 2) {                 // LC + IC
        std::vector<double> lcic((size_t)2 * nk);
        TBK_HIP(hipMemcpyAsync(lcic.data(), o_dev, (size_t)2 * nk * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        TBK_HIP(hipStreamSynchronize(ctx->stream));
        for (int64_t i = 0; i < nk; ++i) out[i] = lcic[(size_t)i] + lcic[(size_t)(nk + i)];
        return TBK_OK;
    }
    TBK_HIP(hipMemcpyAsync(out, o_dev, (size_t)nout * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    return TBK_OK;
}

extern "C" int tbk_orb_mag_mesh(tbk_model* m, const int32_t* mesh, int dir0, int dir1, const int32_t* occ, int nocc, int nmu,
                                const double* mu, double kT, double* out) {
    std::vector<int> mask;
    int rc = orb_check("tbk_orb_mag_mesh", m, dir0, dir1, occ, nocc, mask);
    if (rc) return rc;
    TBK_REQUIRE(mesh && out, TBK_EINVAL, "tbk_orb_mag_mesh: null argument");
    TBK_REQUIRE(m->dim_k == 2 || m->dim_k == 3, TBK_EINVAL, "tbk_orb_mag_mesh: dim_k=%d (meshes of 2 or 3 dimensions)", m->dim_k);
    TBK_REQUIRE(nmu >= 0 && nmu <= 8192 && (nmu == 0 || mu), TBK_EINVAL, "tbk_orb_mag_mesh: nmu=%d (0..8192 levels)", nmu);
    TBK_REQUIRE((nmu > 0) != (occ != nullptr), TBK_EINVAL, "tbk_orb_mag_mesh: give exactly one of a band set and Fermi levels");
    TBK_REQUIRE(std::isfinite(kT) && kT >= 0.0, TBK_EINVAL, "tbk_orb_mag_mesh: kT must be finite and >= 0");
    TBK_REQUIRE(kT == 0.0 || nmu > 0, TBK_EINVAL, "tbk_orb_mag_mesh: kT > 0 needs Fermi levels");
    for (int j = 0; j < nmu; ++j)
        TBK_REQUIRE(std::isfinite(mu[j]), TBK_EINVAL, "tbk_orb_mag_mesh: Fermi level %d is not finite", j);
    const int n = m->nsta, dk = m->dim_k;
    PlaneArgs P{};
    int64_t npts = 1;
    for (int d = 0; d < 3; ++d) {
        if (d < dk) TBK_REQUIRE(mesh[d] >= 1, TBK_EINVAL, "tbk_orb_mag_mesh: mesh[%d]=%d", d, mesh[d]);
        P.N[d] = d < dk ? mesh[d] : 1;
        npts *= P.N[d];
    }
    P.da = dir0;
    P.db = dir1;
    P.dc = dk == 3 ? 3 - dir0 - dir1 : -1;
    P.nplane = (int64_t)P.N[dir0] * P.N[dir1];
    P.npts = npts;
    const int nslice = P.dc >= 0 ? P.N[P.dc] : 1;
    P.nslice = nslice;
    const bool manifold = occ != nullptr, hot = kT > 0.0;
    const int nch = manifold ? 3 : nmu;
    const int64_t nout = (int64_t)nch * nslice;
    if (n < 2 || (manifold && nocc == n)) {   // no pair to sum
        std::fill(out, out + nout, 0.0);
        return TBK_OK;
    }
    tbk_ctx* ctx = m->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    // T = 0: levels sorted on the host (ties by index) for the bins; results come back in input order
    std::vector<int> ord(nmu);
    std::iota(ord.begin(), ord.end(), 0);
    if (!hot) std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return mu[x] < mu[y]; });
    std::vector<double> mus(nmu);
    for (int j = 0; j < nmu; ++j) mus[j] = mu[ord[j]];
    // partial layouts and counts: the grid shapes depend on the mesh shape, n and nmu alone
    int gx;
    int64_t nrows;
    if (manifold) {
        gx = (int)std::max<int64_t>(1, std::min<int64_t>((P.nplane + 2047) / 2048, 1024));   // k_curv_plane's
        nrows = (int64_t)nslice * 3;
    } else if (!hot) {
        const int64_t tiles = (P.nplane * n + 255) / 256;
        const int64_t cap = std::max<int64_t>(1, ((int64_t)1 << 22) / ((int64_t)nslice * nmu * 2));
        gx = (int)std::max<int64_t>(1, std::min<int64_t>({(tiles + 7) / 8, 512, cap}));
        nrows = (int64_t)nslice * nmu * 2;
    } else {
        const int64_t cap = std::max<int64_t>(1, ((int64_t)1 << 22) / ((int64_t)nslice * nmu));
        gx = (int)std::max<int64_t>(1, std::min<int64_t>({(P.nplane * n + 1023) / 1024, (int64_t)kOrbKtGroupsMax, cap}));
        nrows = (int64_t)nslice * nmu;
    }
    const size_t partb = al256((size_t)nrows * gx * sizeof(double)), rowb = al256((size_t)nrows * sizeof(double));
    const size_t mub = al256((size_t)std::max(nmu, 1) * sizeof(double));
    const bool general = n != 2;
    // per-point arrays: band set st[3][npts] (n != 2); per band ev, mm, om [n][npts] (n != 2, or n = 2 with kT > 0)
    const size_t stb = general && manifold ? al256((size_t)3 * npts * sizeof(double)) : 0;
    const size_t recb = (general && !manifold) || hot ? al256((size_t)n * npts * sizeof(double)) : 0;
    const OrbWork cw = general ? orb_work_size(n, dk, npts, manifold) : OrbWork{0, 0};
    void* base = nullptr;
    rc = tbk_ctx_scratch(ctx, 256 + partb + rowb + mub + stb + 3 * recb + cw.bytes, &base);
    if (rc) return rc;
    unsigned char* p = (unsigned char*)base + 256;
    double* part = (double*)p;
    p += partb;
    double* rows = (double*)p;
    p += rowb;
    double* mu_dev = (double*)p;
    p += mub;
    double* st_dev = stb ? (double*)p : nullptr;
    p += stb;
    double* ev_dev = recb ? (double*)p : nullptr;
    double* mm_dev = recb ? (double*)(p + recb) : nullptr;
    double* om_dev = recb ? (double*)(p + 2 * recb) : nullptr;
    p += 3 * recb;
    unsigned char* work = p;
    if (nmu) TBK_HIP(hipMemcpyAsync(mu_dev, mus.data(), (size_t)nmu * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    auto reduce = [&](auto src) -> int {
        if (manifold) {
            ProfScope ps(ctx, n == 2 ? "orb2_plane" : "orb_plane");
            hipLaunchKernelGGL(k_orb_plane<decltype(src)>, dim3(gx, (unsigned)std::min(nslice, 65535)), dim3(256), 0, ctx->stream, src,
                               P, part);
            TBK_HIP(hipGetLastError());
        } else {
            ProfScope ps(ctx, n == 2 ? "orb2_fermi" : "orb_fermi");
            const unsigned nwin = (unsigned)((nmu + kOrbWin - 1) / kOrbWin);
            hipLaunchKernelGGL(k_orb_fermi<decltype(src)>, dim3(gx, (unsigned)std::min(nslice, 65535), nwin), dim3(256), 0, ctx->stream,
                               src, P, n, (const double*)mu_dev, nmu, part);
            TBK_HIP(hipGetLastError());
        }
        return TBK_OK;
    };
    if (general) {
        rc = orb_general(m, nullptr, mesh, npts, dir0, dir1, mask, work, cw, mm_dev, om_dev, ev_dev, st_dev);
        if (rc) return rc;
    } else if (hot) {
        ProfScope ps(ctx, "orb2_records");
        hipLaunchKernelGGL(k_orb2_records, dim3(nblk(npts)), dim3(256), 0, ctx->stream, m->view, P, dir0, dir1, ev_dev, mm_dev, om_dev);
        TBK_HIP(hipGetLastError());
    }
    if (hot) {
        ProfScope ps(ctx, "orb_kt");
        const unsigned ntile = (unsigned)((nmu + kOrbKtTile - 1) / kOrbKtTile);
        hipLaunchKernelGGL(k_orb_kt, dim3(ntile, (unsigned)gx, (unsigned)std::min(nslice, 65535)), dim3(256), 0, ctx->stream, P, n,
                           (const double*)ev_dev, (const double*)mm_dev, (const double*)om_dev, (const double*)mu_dev, nmu, kT, gx,
                           part);
        TBK_HIP(hipGetLastError());
    } else if (general) {
        rc = reduce(OrbArraySrc{ev_dev, mm_dev, om_dev, st_dev});
    } else {
        rc = reduce(Orb2Src{m->view, dir0, dir1, manifold ? (mask[0] ? 1 : -1) : 0});
    }
    if (rc) return rc;
    {
        ProfScope ps(ctx, "orb_rows");
        hipLaunchKernelGGL(k_orb_rows, dim3((unsigned)nrows), dim3(256), 0, ctx->stream, (const double*)part, gx, rows);
        TBK_HIP(hipGetLastError());
    }
    std::vector<double> sums((size_t)nrows);
    TBK_HIP(hipMemcpyAsync(sums.data(), rows, (size_t)nrows * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    const double inv = 1.0 / (double)P.nplane;
    // out[ch][s]: the Python shapes (nch,) for a 2-D mesh, (nch, nslice) for a 3-D one
    for (int s = 0; s < nslice; ++s) {
        if (manifold) {
            for (int c = 0; c < 3; ++c) out[(size_t)c * nslice + s] = sums[(size_t)s * 3 + c] * inv;
        } else if (hot) {
            for (int j = 0; j < nmu; ++j) out[(size_t)j * nslice + s] = sums[(size_t)s * nmu + j] * inv;
        } else {
            double ai = 0.0, aa = 0.0;             // I(mu_j), A(mu_j): prefix sums of the bins over the sorted levels
            for (int j = 0; j < nmu; ++j) {
                ai += sums[((size_t)s * nmu + j) * 2];
                aa += sums[((size_t)s * nmu + j) * 2 + 1];
                out[(size_t)ord[j] * nslice + s] = aa * inv + mus[j] * (ai * inv);
            }
        }
    }
    return TBK_OK;
}
