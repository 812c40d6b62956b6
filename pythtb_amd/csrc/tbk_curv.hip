// tbk_curv.hip -- Berry curvature by the Kubo formula on k lists and uniform meshes.
//
// k in reduced coordinates, H the convention-II matrix of tbk_gen_ham: H_ab(k) = sum_t amp_t exp(2 pi i k.(R_t + tau_b - tau_a)).
//   velocity      d_d H_ab(k) = sum_t amp_t 2 pi i (R_t + tau_b - tau_a)_d exp(2 pi i k.(R_t + tau_b - tau_a))
//   per band (1)  Omega_n = -2 Im sum_{m != n} V^a_nm V^b_mn / (E_n - E_m)^2,  V^d_nm = <n| d_d H |m>;
//                 a pair with |E_n - E_m| <= 1e-9 max(1, |E_n|, |E_m|) contributes nothing to either band
//   manifold (2)  Omega_occ = -2 Im sum_{n in occ, m not in occ} V^a_nm V^b_mn / (E_n - E_m)^2   (no degeneracy rule)
//
// Two forms:
//   n = 2     one lane per k, H = d0 + d.sigma and d_a d, d_b d in registers: Omega_0 = d.(d_a d x d_b d) / (2 |d|^3) = -Omega_1,
//             no eigen-solve.  On a mesh the lane generates its own k and feeds the plane / Fermi reductions directly.
//   n != 2    chunks of at most kCurvChunkBytes of eigenvectors: the device k generator (mesh form), the eigen-solver with vectors
//             (tbk_solve_list_dev_checked), then up to 32 states ONE kernel with several points' U, d H and products in LDS
//             (k_curv_lds); from 33 states W^d = d_d H U^T from the sparse slots (k_curv_wsp) and a lane per (k, band) contraction.
// Reductions are fixed-shape trees (per-workgroup partials in a grid-stride order that depends on the mesh shape alone, then one
// workgroup per output): two calls on the same input give the same bits.  No floating-point atomics anywhere.
#include <math.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>
#include "tbk_dham.h"

// bytes of eigenvectors per chunk of the n != 2 path: fixed, so that the chunking -- and with it every result -- does not depend
// on the machine.  (From 33 states the chunk's W takes 2x this beside it.)
static const size_t kCurvChunkBytes = (size_t)32 << 20;
static const int kFermiWin = 4096;   // Fermi levels per LDS window of k_curv_fermi (32 KiB of bins)

// dense d_{d0} H and d_{d1} H of nk points from the non-empty slots: the n x n matrices of point ik at out0 + ik pstride and
// out1 + ik pstride (zeroed by the caller); out1 nullable
__global__ __launch_bounds__(256) void k_curv_dham(const ModelView mv, const int64_t nk, const double* __restrict__ k, const int d0,
                                                   const int d1, const int64_t pstride, cd* __restrict__ out0, cd* __restrict__ out1) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nk * mv.nnz) return;
    const int64_t ik = idx / mv.nnz;
    const int4 e = mv.nz[(int)(idx - ik * mv.nnz)];
    const int a = e.x & 0xffff, b = e.x >> 16, n = mv.nsta;
    double kk[4];
    cd z[4];
    k_phases(mv, k, ik, kk, z);
    cd h, v0, v1;
    dham_terms(mv, a, b, e.y, e.z, kk, z, d0, d1, h, v0, v1);
    cd* o0 = out0 + ik * pstride;
    o0[a * n + b] = v0;
    o0[b * n + a] = cconj(v0);
    if (out1) {
        cd* o1 = out1 + ik * pstride;
        o1[a * n + b] = v1;
        o1[b * n + a] = cconj(v1);
    }
}

// ---------------------------------------------------------------- n = 2: closed form in registers (curv2_point, tbk_dham.h)
// list form: out[2][nk] per band (occ_sign == 0) or out[nk] = occ_sign * Omega_0 (the manifold of band 0: +1, of band 1: -1)
__global__ __launch_bounds__(256) void k_curv2_list(const ModelView mv, const int64_t nk, const double* __restrict__ k, const int d0,
                                                    const int d1, const int occ_sign, double* __restrict__ out) {
    const int64_t ik = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (ik >= nk) return;
    double kk[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) kk[d] = d < mv.dim_k ? k[ik * mv.dim_k + d] : 0.0;
    const Curv2 c = curv2_point(mv, kk, d0, d1);
    if (occ_sign == 0) {
        const double w = c.degenerate ? 0.0 : c.om;
        out[ik] = w;
        out[nk + ik] = -w;
    } else {
        out[ik] = occ_sign > 0 ? c.om : -c.om;
    }
}

// ---------------------------------------------------------------- mesh planes (PlaneArgs, plane_point: tbk_dham.h)
// sources of per-point values for the reductions.  band(): Omega_ch with the degeneracy rule and E_ch; man(): the manifold value
struct Curv2Src {
    ModelView mv;
    int d0, d1, occ_sign;
    __device__ __forceinline__ Curv2 at(const PlaneArgs& P, const int (&ii)[3]) const {
        double kk[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int d = 0; d < 3; ++d)
            if (d < mv.dim_k) kk[d] = (double)ii[d] / (double)P.N[d];   // k_uniform_mesh's point, bit for bit
        return curv2_point(mv, kk, d0, d1);
    }
    __device__ __forceinline__ double band(const PlaneArgs& P, const int (&ii)[3], int64_t, const int ch, double& e) const {
        const Curv2 c = at(P, ii);
        e = ch ? c.e1 : c.e0;
        const double w = c.degenerate ? 0.0 : c.om;
        return ch ? -w : w;
    }
    __device__ __forceinline__ double man(const PlaneArgs& P, const int (&ii)[3], int64_t) const {
        const Curv2 c = at(P, ii);
        return occ_sign > 0 ? c.om : -c.om;
    }
};
struct ArraySrc {
    const double* om;   // [nch][npts]
    const double* ev;   // [n][npts] (Fermi scan only)
    __device__ __forceinline__ double band(const PlaneArgs& P, const int (&)[3], const int64_t idx, const int ch, double& e) const {
        e = ev ? ev[(int64_t)ch * P.npts + idx] : 0.0;
        return om[(int64_t)ch * P.npts + idx];
    }
    __device__ __forceinline__ double man(const PlaneArgs&, const int (&)[3], const int64_t idx) const { return om[idx]; }
};

// plane sums: row = s * nch + ch (blockIdx.y and every gridDim.y after it), blockIdx.x = g of gx; part[row][gx]
template <class Src>
__global__ __launch_bounds__(256) void k_curv_plane(const Src src, const PlaneArgs P, const int manifold, const int nch,
                                                    const int64_t nrows, double* __restrict__ part) {
    __shared__ double red[4];
    for (int64_t row = blockIdx.y; row < nrows; row += gridDim.y) {   // (rows beyond the grid's y limit: the next pass)
        const int s = (int)(row / nch), ch = (int)(row - (int64_t)s * nch);
        double acc = 0.0;
        for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < P.nplane; p += (int64_t)gridDim.x * 256) {
            int ii[3];
            const int64_t idx = plane_point(P, s, p, ii);
            double e;
            acc += manifold ? src.man(P, ii, idx) : src.band(P, ii, idx, ch, e);
        }
        const double t = block_sum(acc, red);
        if (threadIdx.x == 0) part[row * gridDim.x + blockIdx.x] = t;
        __syncthreads();                                              // (red is reused by the next row)
    }
}

// Fermi scan: every (point, band) item of slice s adds Omega_n to the bin of the first sorted level mu_j >= E_n.  A tile of 256 items
// is staged in LDS as (bin, Omega); each lane owns a fixed range of the window's bins and adds the tile's items in item order.
// blockIdx.x = g of gx (tiles g, g + gx, ...), blockIdx.y = slice (and every gridDim.y after it), blockIdx.z = window of kFermiWin
// levels.
// part[s][j][gx]
template <class Src>
__global__ __launch_bounds__(256) void k_curv_fermi(const Src src, const PlaneArgs P, const int nb, const double* __restrict__ mu,
                                                    const int nmu, double* __restrict__ part) {
    __shared__ double bins[kFermiWin];
    __shared__ double tw[256];
    __shared__ int tb[256];
    for (int s = blockIdx.y; s < P.nslice; s += gridDim.y) {   // (slices beyond the grid's y limit: the next pass)
        const int w0 = blockIdx.z * kFermiWin, wn = min(kFermiWin, nmu - w0);
        for (int j = threadIdx.x; j < kFermiWin; j += 256) bins[j] = 0.0;
        const int per = (wn + 255) / 256;
        const int lo = threadIdx.x * per, hi = min(wn, lo + per);
        const int64_t total = P.nplane * nb;
        for (int64_t t0 = (int64_t)blockIdx.x * 256; t0 < total; t0 += (int64_t)gridDim.x * 256) {
            const int64_t it = t0 + threadIdx.x;
            int bin = -1;
            double w = 0.0;
            if (it < total) {
                const int64_t p = it / nb;
                const int band = (int)(it - p * nb);
                int ii[3];
                const int64_t idx = plane_point(P, s, p, ii);
                double e;
                w = src.band(P, ii, idx, band, e);
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
            tw[threadIdx.x] = w;
            __syncthreads();
            for (int q = 0; q < 256; ++q) {
                const int b = tb[q];
                if (b >= lo && b < hi) bins[b] += tw[q];
            }
        }
        __syncthreads();
        for (int j = threadIdx.x; j < wn; j += 256)
            part[((int64_t)s * nmu + w0 + j) * gridDim.x + blockIdx.x] = bins[j];
        __syncthreads();                                           // (bins are reused by the next slice)
    }
}

// out[r] = sum_g part[r][g] in a fixed order (one workgroup per row)
__global__ __launch_bounds__(256) void k_curv_rows(const double* __restrict__ part, const int gx, double* __restrict__ out) {
    __shared__ double red[4];
    const double* p = part + (int64_t)blockIdx.x * gx;
    double acc = 0.0;
    for (int g = threadIdx.x; g < gx; g += 256) acc += p[g];
    const double t = block_sum(acc, red);
    if (threadIdx.x == 0) out[blockIdx.x] = t;
}

// ---------------------------------------------------------------- n != 2: contraction of the solver's eigenvectors
// Up to 32 states: ONE kernel, P = min(64, 4096 / (4 n^2)) points per workgroup, everything of a point in LDS (64 KiB):
// U (its eigenvectors, read once from HBM), D = d_{d0} H and X = d_{d1} H (built from the non-empty slots), T = D U^T, then
// D := V^{d0} = conj(U) T, T := X U^T, and one lane per (point, band) forms V^{d1} from T on the fly and sums (1) or (2).
// Nothing but Omega (and E for a Fermi scan) is written.
#define CURV_LDS_CD 4096
static inline int curv_lds_points(int n) { return std::max(1, std::min(64, CURV_LDS_CD / (4 * n * n))); }
__global__ __launch_bounds__(256) void k_curv_lds(const ModelView mv, const double* __restrict__ k, const cd* __restrict__ evec,
                                                  const double* __restrict__ eval, const int64_t nk, const int d0, const int d1,
                                                  const int P, const int* __restrict__ occ, const int64_t first, const int64_t nfull,
                                                  double* __restrict__ om, double* __restrict__ ev) {
    __shared__ cd L[CURV_LDS_CD];
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
        const int p = e / nn, r = e - p * nn, i = r / n, mm = r - i * n;
        const cd* dr = D + p * nn + i * n;
        const cd* um = U + p * nn + mm * n;
        cd acc{0.0, 0.0};
        for (int j = 0; j < n; ++j) cfma(acc, dr[j], um[j]);
        T[e] = acc;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < np * nn; e += 256) {            // D := V^{d0} = conj(U) T   (reads U, T only)
        const int p = e / nn, r = e - p * nn, b = r / n, mm = r - b * n;
        const cd* ub = U + p * nn + b * n;
        const cd* tc = T + p * nn + mm;
        cd acc{0.0, 0.0};
        for (int i = 0; i < n; ++i) cfmac(acc, ub[i], tc[i * n]);
        D[e] = acc;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < np * nn; e += 256) {            // T := X U^T
        const int p = e / nn, r = e - p * nn, i = r / n, mm = r - i * n;
        const cd* xr = X + p * nn + i * n;
        const cd* um = U + p * nn + mm * n;
        cd acc{0.0, 0.0};
        for (int j = 0; j < n; ++j) cfma(acc, xr[j], um[j]);
        T[e] = acc;
    }
    __syncthreads();
    double* share = (double*)X;                                    // (X is dead: the band shares of (2) go there)
    for (int e = threadIdx.x; e < np * n; e += 256) {
        const int p = e / n, b = e - p * n;
        const int64_t ik = ik0 + p;
        const double eb = eval[(int64_t)b * nk + ik];
        const cd* ub = U + p * nn + b * n;
        const cd* va = D + p * nn + b * n;
        const cd* tp = T + p * nn;
        double acc = 0.0;
        if (!occ || occ[b]) {
            for (int mm = 0; mm < n; ++mm) {
                if (mm == b) continue;
                const double em = eval[(int64_t)mm * nk + ik];
                const double de = eb - em;
                if (occ) {
                    if (occ[mm]) continue;
                } else if (!(fabs(de) > 1e-9 * fmax(1.0, fmax(fabs(eb), fabs(em))))) {
                    continue;
                }
                cd vb{0.0, 0.0};
                for (int i = 0; i < n; ++i) cfmac(vb, ub[i], tp[i * n + mm]);
                const cd a = va[mm];
                acc += (a.y * vb.x - a.x * vb.y) / (de * de);       // Im V^a_bm V^b_mb = Im V^a_bm conj(V^b_bm)
            }
        }
        const double o = -2.0 * acc;
        if (occ) {
            share[e] = o;
        } else {
            om[(int64_t)b * nfull + first + ik] = o;
            if (ev) ev[(int64_t)b * nfull + first + ik] = eb;
        }
    }
    if (occ) {
        __syncthreads();
        for (int p = threadIdx.x; p < np; p += 256) {
            double s = 0.0;
            for (int b = 0; b < n; ++b) s += share[p * n + b];
            om[first + ik0 + p] = s;
        }
    }
}

// 33..2048 states: W^d[ik][i][m] = sum_j d_d H_ij u_m[j] from the non-empty slots only (ModelView.nz; no dense d_d H).  Workgroup
// (point, block of 256 columns); lane m owns column m of both W^d -- every slot adds to two entries of each, and no other lane
// touches them: no atomics, a fixed order.  The slot values (both directions) are computed once per point and staged in LDS.
__global__ __launch_bounds__(256) void k_curv_wsp(const ModelView mv, const double* __restrict__ k, const cd* __restrict__ evec,
                                                  const int64_t nk, const int d0, const int d1, cd* __restrict__ wt) {
    __shared__ int sab[256];
    __shared__ cd sv0[256], sv1[256];
    const int n = mv.nsta;
    const int64_t ik = blockIdx.x, nn = (int64_t)n * n;
    const int m = blockIdx.y * 256 + threadIdx.x;
    const bool live = m < n;
    cd* w0 = wt + 2 * ik * nn;
    cd* w1 = w0 + nn;
    if (live)
        for (int i = 0; i < n; ++i) {
            w0[(int64_t)i * n + m] = cd{0.0, 0.0};
            w1[(int64_t)i * n + m] = cd{0.0, 0.0};
        }
    double kk[4];
    cd z[4];
    k_phases(mv, k, ik, kk, z);
    const cd* u = evec + ((int64_t)(live ? m : 0) * nk + ik) * n;
    for (int q0 = 0; q0 < mv.nnz; q0 += 256) {
        __syncthreads();
        if (q0 + (int)threadIdx.x < mv.nnz) {
            const int4 z4 = mv.nz[q0 + threadIdx.x];
            cd h;
            dham_terms(mv, z4.x & 0xffff, z4.x >> 16, z4.y, z4.z, kk, z, d0, d1, h, sv0[threadIdx.x], sv1[threadIdx.x]);
            sab[threadIdx.x] = z4.x;
        }
        __syncthreads();
        const int cnt = min(256, mv.nnz - q0);
        if (!live) continue;
        for (int q = 0; q < cnt; ++q) {
            const int a = sab[q] & 0xffff, b = sab[q] >> 16;
            const cd v0 = sv0[q], v1 = sv1[q], ub = u[b];
            cd* pa0 = w0 + (int64_t)a * n + m;
            cd* pa1 = w1 + (int64_t)a * n + m;
            cd t0 = *pa0, t1 = *pa1;
            cfma(t0, v0, ub);
            cfma(t1, v1, ub);
            *pa0 = t0;
            *pa1 = t1;
            if (a != b) {
                const cd ua = u[a];
                cd* pb0 = w0 + (int64_t)b * n + m;
                cd* pb1 = w1 + (int64_t)b * n + m;
                cd s0 = *pb0, s1 = *pb1;
                cfma(s0, cconj(v0), ua);
                cfma(s1, cconj(v1), ua);
                *pb0 = s0;
                *pb1 = s1;
            }
        }
    }
}

// 33..2048 states, one lane per (ik, band nb): V^d_{nb,m} = sum_i conj(u_nb[i]) W^d[i][m]; Omega as in (1) (occ == null) or band nb's share of (2)
// (occ[nb] set: sum over m outside occ; else 0).  Per band: om[nb][first + ik] (and ev[nb][first + ik] = E_nb when ev is set);
// manifold: tmp[ik][nb], summed per point by k_curv_occ_sum.
__global__ __launch_bounds__(256) void k_curv_contract(const cd* __restrict__ evec, const double* __restrict__ eval,
                                                       const cd* __restrict__ wt, const int64_t nk, const int n,
                                                       const int* __restrict__ occ, const int64_t first, const int64_t nfull,
                                                       double* __restrict__ om, double* __restrict__ ev, double* __restrict__ tmp) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nk * n) return;
    const int64_t ik = idx / n;
    const int b = (int)(idx - ik * n);
    const int64_t nn = (int64_t)n * n;
    const cd* u = evec + ((int64_t)b * nk + ik) * n;
    const cd* w0 = wt + (2 * ik) * nn;
    const cd* w1 = w0 + nn;
    const double eb = eval[(int64_t)b * nk + ik];
    const bool in_b = occ && occ[b];
    double acc = 0.0;
    if (!occ || in_b) {
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
            // Im V^a_bm V^b_mb = Im V^a_bm conj(V^b_bm)
            acc += (va.y * vb.x - va.x * vb.y) / (de * de);
        }
    }
    const double o = -2.0 * acc;
    if (occ) {
        tmp[ik * n + b] = o;
    } else {
        om[(int64_t)b * nfull + first + ik] = o;
        if (ev) ev[(int64_t)b * nfull + first + ik] = eb;
    }
}

__global__ __launch_bounds__(256) void k_curv_occ_sum(const double* __restrict__ tmp, const int64_t nk, const int n,
                                                      double* __restrict__ out) {
    const int64_t ik = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (ik >= nk) return;
    double s = 0.0;
    for (int b = 0; b < n; ++b) s += tmp[ik * n + b];
    out[ik] = s;
}

// ---------------------------------------------------------------- host side
static inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
static inline unsigned nblk(int64_t threads) { return (unsigned)((threads + 255) / 256); }

// common argument checks; *mask (n entries) = 1 for the bands of occ; *occ_sign for n = 2 manifolds of one band
static int curv_check(const char* fn, tbk_model* m, int dir0, int dir1, const int32_t* occ, int nocc, std::vector<int>& mask) {
    TBK_REQUIRE(m, TBK_EINVAL, "%s: null model", fn);
    TBK_REQUIRE(m->dim_k >= 2, TBK_EINVAL, "%s: the curvature needs dim_k >= 2 (the model has %d)", fn, m->dim_k);
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

extern "C" int tbk_gen_dham(tbk_model* m, const double* k, int64_t nk, int dir, double* out) {
    TBK_REQUIRE(m && out && nk >= 0, TBK_EINVAL, "tbk_gen_dham: bad argument");
    TBK_REQUIRE(m->dim_k >= 1 && dir >= 0 && dir < m->dim_k, TBK_EINVAL, "tbk_gen_dham: dir=%d outside [0, dim_k=%d)", dir,
                m->dim_k);
    TBK_REQUIRE(k || nk == 0, TBK_EINVAL, "tbk_gen_dham: null k");
    if (nk == 0) return TBK_OK;
    tbk_ctx* ctx = m->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    const int n = m->nsta;
    const size_t kb = (size_t)nk * m->dim_k * sizeof(double), hb = (size_t)nk * n * n * sizeof(cd);
    void* base = nullptr;
    int rc = tbk_ctx_scratch(ctx, 256 + al256(kb) + al256(hb), &base);
    if (rc) return rc;
    double* k_dev = (double*)((unsigned char*)base + 256);
    cd* h_dev = (cd*)((unsigned char*)k_dev + al256(kb));
    TBK_HIP(hipMemcpyAsync(k_dev, k, kb, hipMemcpyHostToDevice, ctx->stream));
    TBK_HIP(hipMemsetAsync(h_dev, 0, hb, ctx->stream));
    if (m->view.nnz > 0) {
        ProfScope ps(ctx, "gen_dham");
        hipLaunchKernelGGL(k_curv_dham, dim3(nblk(nk * m->view.nnz)), dim3(256), 0, ctx->stream, m->view, nk, (const double*)k_dev, dir, dir,
                           (int64_t)n * n, h_dev, (cd*)nullptr);
        TBK_HIP(hipGetLastError());
    }
    TBK_HIP(hipMemcpyAsync(out, h_dev, hb, hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    return TBK_OK;
}

// The n != 2 pipeline over points [0, nk): k from k_all (list) or generated from `mesh`, in chunks.  Per band: om_dev[n][nk]
// (+ ev_dev[n][nk] when set); manifold: om_dev[nk].  `work` is scratch behind the caller's buffers, `work_bytes` its size.
struct CurvWork {
    size_t bytes;
    int64_t chunk;
};
static CurvWork curv_work_size(int n, int dim_k, int64_t nk, bool manifold) {
    const size_t vb = (size_t)n * n * sizeof(cd);
    int64_t chunk = std::max<int64_t>(1, (int64_t)(kCurvChunkBytes / vb));
    chunk = std::min<int64_t>(chunk, std::max<int64_t>(nk, 1));
    const bool wide = n > 32;
    size_t b = al256((size_t)chunk * dim_k * sizeof(double)) + al256((size_t)chunk * n * sizeof(double)) + al256((size_t)chunk * vb) +
               (wide ? al256(2 * (size_t)chunk * vb) : 0) + al256((size_t)n * sizeof(int)) +
               (wide && manifold ? al256((size_t)chunk * n * sizeof(double)) : 0);
    return CurvWork{b, chunk};
}
static int curv_general(tbk_model* m, const double* k_all_dev, const int32_t* mesh, int64_t nk, int d0, int d1,
                        const std::vector<int>& mask, unsigned char* work, const CurvWork& cw, double* om_dev, double* ev_dev) {
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
            const int P = curv_lds_points(n);
            ProfScope ps(ctx, "curv_lds");
            hipLaunchKernelGGL(k_curv_lds, dim3((unsigned)((cnt + P - 1) / P)), dim3(256), 0, ctx->stream, m->view, kp, (const cd*)vc,
                               (const double*)ec, cnt, d0, d1, P, occ_arg, first, nk, om_dev, ev_dev);
            TBK_HIP(hipGetLastError());
            continue;
        }
        {
            ProfScope ps(ctx, "curv_wsp");
            hipLaunchKernelGGL(k_curv_wsp, dim3((unsigned)cnt, (unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, m->view, kp,
                               (const cd*)vc, cnt, d0, d1, wt);
            TBK_HIP(hipGetLastError());
        }
        {
            ProfScope ps(ctx, "curv_contract");
            hipLaunchKernelGGL(k_curv_contract, dim3(nblk(cnt * n)), dim3(256), 0, ctx->stream, (const cd*)vc, (const double*)ec,
                               (const cd*)wt, cnt, n, occ_arg, first, nk, om_dev, ev_dev, tmp);
            TBK_HIP(hipGetLastError());
        }
        if (manifold) {
            ProfScope ps(ctx, "curv_occ_sum");
            hipLaunchKernelGGL(k_curv_occ_sum, dim3(nblk(cnt)), dim3(256), 0, ctx->stream, (const double*)tmp, cnt, n, om_dev + first);
            TBK_HIP(hipGetLastError());
        }
    }
    return TBK_OK;
}

extern "C" int tbk_berry_curv_list(tbk_model* m, const double* k, int64_t nk, int dir0, int dir1, const int32_t* occ, int nocc,
                                   double* out) {
    std::vector<int> mask;
    int rc = curv_check("tbk_berry_curv_list", m, dir0, dir1, occ, nocc, mask);
    if (rc) return rc;
    TBK_REQUIRE(nk >= 0 && out && (k || nk == 0), TBK_EINVAL, "tbk_berry_curv_list: bad k list or output");
    const int n = m->nsta, dk = m->dim_k;
    const bool manifold = occ != nullptr;
    const int64_t nout = manifold ? nk : (int64_t)n * nk;
    if (nk == 0) return TBK_OK;
    if (manifold && nocc == n) {           // the complement is empty: nothing to sum
        std::fill(out, out + nout, 0.0);
        return TBK_OK;
    }
    tbk_ctx* ctx = m->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    const size_t kb = al256((size_t)nk * dk * sizeof(double)), ob = al256((size_t)nout * sizeof(double));
    const CurvWork cw = n == 2 ? CurvWork{0, 0} : curv_work_size(n, dk, nk, manifold);
    void* base = nullptr;
    rc = tbk_ctx_scratch(ctx, 256 + kb + ob + cw.bytes, &base);
    if (rc) return rc;
    unsigned char* p = (unsigned char*)base + 256;
    double* k_dev = (double*)p;
    double* o_dev = (double*)(p + kb);
    TBK_HIP(hipMemcpyAsync(k_dev, k, (size_t)nk * dk * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (n == 2) {
        ProfScope ps(ctx, "curv2_list");
        const int sign = manifold ? (mask[0] ? 1 : -1) : 0;
        hipLaunchKernelGGL(k_curv2_list, dim3(nblk(nk)), dim3(256), 0, ctx->stream, m->view, nk, (const double*)k_dev, dir0, dir1,
                           sign, o_dev);
        TBK_HIP(hipGetLastError());
    } else {
        rc = curv_general(m, k_dev, nullptr, nk, dir0, dir1, mask, p + kb + ob, cw, o_dev, nullptr);
        if (rc) return rc;
    }
    TBK_HIP(hipMemcpyAsync(out, o_dev, (size_t)nout * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    return TBK_OK;
}

extern "C" int tbk_berry_curv_mesh(tbk_model* m, const int32_t* mesh, int dir0, int dir1, const int32_t* occ, int nocc, int nmu,
                                   const double* mu, double* out) {
    std::vector<int> mask;
    int rc = curv_check("tbk_berry_curv_mesh", m, dir0, dir1, occ, nocc, mask);
    if (rc) return rc;
    TBK_REQUIRE(mesh && out, TBK_EINVAL, "tbk_berry_curv_mesh: null argument");
    TBK_REQUIRE(m->dim_k == 2 || m->dim_k == 3, TBK_EINVAL, "tbk_berry_curv_mesh: dim_k=%d (meshes of 2 or 3 dimensions)", m->dim_k);
    TBK_REQUIRE(nmu >= 0 && nmu <= 8192 && (nmu == 0 || mu), TBK_EINVAL, "tbk_berry_curv_mesh: nmu=%d (0..8192 levels)", nmu);
    TBK_REQUIRE(!(nmu > 0 && occ), TBK_EINVAL, "tbk_berry_curv_mesh: a band set and a Fermi scan are exclusive");
    for (int j = 0; j < nmu; ++j)
        TBK_REQUIRE(std::isfinite(mu[j]), TBK_EINVAL, "tbk_berry_curv_mesh: Fermi level %d is not finite", j);
    const int n = m->nsta, dk = m->dim_k;
    PlaneArgs P{};
    int64_t npts = 1;
    for (int d = 0; d < 3; ++d) {
        if (d < dk) TBK_REQUIRE(mesh[d] >= 1, TBK_EINVAL, "tbk_berry_curv_mesh: mesh[%d]=%d", d, mesh[d]);
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
    const bool manifold = occ != nullptr, fermi = nmu > 0;
    const int nch = fermi ? nmu : (manifold ? 1 : n);
    const int64_t nout = (int64_t)nch * nslice;
    if (manifold && nocc == n) {
        std::fill(out, out + nout, 0.0);
        return TBK_OK;
    }
    tbk_ctx* ctx = m->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    // levels sorted on the host (ties by index); results come back in input order
    std::vector<int> ord(nmu);
    std::iota(ord.begin(), ord.end(), 0);
    std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return mu[x] < mu[y]; });
    std::vector<double> mus(nmu);
    for (int j = 0; j < nmu; ++j) mus[j] = mu[ord[j]];
    // partial layout and counts: the grid-stride shapes depend on the mesh shape alone
    const int nplane_ch = (!fermi && !manifold && n == 2) ? 1 : nch;   // n = 2 per band: band 1 is -band 0, bit for bit
    int gx;
    if (fermi) {
        const int64_t tiles = (P.nplane * n + 255) / 256;
        const int64_t cap = std::max<int64_t>(1, ((int64_t)1 << 22) / ((int64_t)nslice * nmu));
        gx = (int)std::max<int64_t>(1, std::min<int64_t>({(tiles + 7) / 8, 512, cap}));
    } else {
        gx = (int)std::max<int64_t>(1, std::min<int64_t>((P.nplane + 2047) / 2048, 1024));
    }
    const int64_t nrows = (int64_t)nslice * nplane_ch;
    const size_t partb = al256((size_t)nrows * gx * sizeof(double)), rowb = al256((size_t)nrows * sizeof(double));
    const size_t mub = al256((size_t)std::max(nmu, 1) * sizeof(double));
    const bool general = n != 2;
    const size_t omb = general ? al256((size_t)(manifold ? 1 : n) * npts * sizeof(double)) : 0;
    const size_t evb = general && fermi ? al256((size_t)n * npts * sizeof(double)) : 0;
    const CurvWork cw = general ? curv_work_size(n, dk, npts, manifold) : CurvWork{0, 0};
    void* base = nullptr;
    rc = tbk_ctx_scratch(ctx, 256 + partb + rowb + mub + omb + evb + cw.bytes, &base);
    if (rc) return rc;
    unsigned char* p = (unsigned char*)base + 256;
    double* part = (double*)p;
    double* rows = (double*)(p + partb);
    double* mu_dev = (double*)(p + partb + rowb);
    double* om_dev = (double*)(p + partb + rowb + mub);
    double* ev_dev = evb ? (double*)(p + partb + rowb + mub + omb) : nullptr;
    unsigned char* work = p + partb + rowb + mub + omb + evb;
    if (fermi) TBK_HIP(hipMemcpyAsync(mu_dev, mus.data(), (size_t)nmu * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    auto reduce = [&](auto src) -> int {
        if (fermi) {
            ProfScope ps(ctx, n == 2 ? "curv2_fermi" : "curv_fermi");
            const unsigned nwin = (unsigned)((nmu + kFermiWin - 1) / kFermiWin);
            hipLaunchKernelGGL(k_curv_fermi<decltype(src)>, dim3(gx, (unsigned)std::min(nslice, 65535), nwin), dim3(256), 0, ctx->stream, src, P, n,
                               (const double*)mu_dev, nmu, part);
            TBK_HIP(hipGetLastError());
        } else {
            ProfScope ps(ctx, n == 2 ? "curv2_plane" : "curv_plane");
            hipLaunchKernelGGL(k_curv_plane<decltype(src)>, dim3(gx, (unsigned)std::min<int64_t>(nrows, 65535)), dim3(256), 0, ctx->stream, src,
                               P, manifold ? 1 : 0, nplane_ch, nrows, part);
            TBK_HIP(hipGetLastError());
        }
        ProfScope ps(ctx, "curv_rows");
        hipLaunchKernelGGL(k_curv_rows, dim3((unsigned)nrows), dim3(256), 0, ctx->stream, (const double*)part, gx, rows);
        TBK_HIP(hipGetLastError());
        return TBK_OK;
    };
    if (general) {
        rc = curv_general(m, nullptr, mesh, npts, dir0, dir1, mask, work, cw, om_dev, ev_dev);
        if (rc) return rc;
        rc = reduce(ArraySrc{om_dev, ev_dev});
    } else {
        rc = reduce(Curv2Src{m->view, dir0, dir1, manifold ? (mask[0] ? 1 : -1) : 0});
    }
    if (rc) return rc;
    std::vector<double> sums((size_t)nrows);
    TBK_HIP(hipMemcpyAsync(sums.data(), rows, (size_t)nrows * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    const double inv = 1.0 / (double)P.nplane;
    // out[ch][s]: the Python shapes (nch,) for a 2-D mesh, (nch, nslice) for a 3-D one
    for (int s = 0; s < nslice; ++s) {
        if (fermi) {
            double acc = 0.0;                       // I(mu_j) = sum of the bins up to j: a prefix sum over the sorted levels
            for (int j = 0; j < nmu; ++j) {
                acc += sums[(size_t)s * nmu + j];
                out[(size_t)ord[j] * nslice + s] = acc * inv;
            }
        } else if (nplane_ch == 1 && !manifold) {   // n = 2 per band
            const double v = sums[(size_t)s] * inv;
            out[s] = v;
            out[(size_t)nslice + s] = -v;
        } else {
            for (int c = 0; c < nch; ++c) out[(size_t)c * nslice + s] = sums[(size_t)s * nch + c] * inv;
        }
    }
    return TBK_OK;
}
