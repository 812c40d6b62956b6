// tbk_pairs.h -- what the two translation units that turn (point, pair) records into frequency sums share (tbk_optics.hip, DESIGN.md
// section 12; tbk_shift.hip, section 17): the index of a pair, the occupation weight, the dense product V^d = conj(U) W^d of the wide
// pair stage, the reciprocal of the frequency stage and the sum over k-groups.  Kernels are static: each unit holds its own copy.
#pragma once
#include "tbk_kubo.h"

// the pair (i, j), i < j, of index q in the row-major order of the strict upper triangle of n x n
__device__ __forceinline__ void opt_pair_of(const int n, const int64_t q, int& i, int& j) {
    const double t = 2.0 * n - 1.0;
    int r = (int)((t - sqrt(fmax(t * t - 8.0 * (double)q, 0.0))) * 0.5);
    r = max(0, min(r, n - 2));
    while (r > 0 && (int64_t)r * (2 * n - r - 1) / 2 > q) --r;
    while (r < n - 2 && (int64_t)(r + 1) * (2 * n - r - 2) / 2 <= q) ++r;
    i = r;
    j = (int)(q - (int64_t)r * (2 * n - r - 1) / 2) + r + 1;
}

// c = (f_m - f_n) / eps for E_m = E_n + eps, eps > 0.  kT > 0: with h = eps / 2kT and u = ((E_n + E_m) / 2 - mu) / kT,
// f_m - f_n = -sinh h / (cosh h + cosh u), evaluated as exp(h - M) expm1(-2h) / (e^{h-M} + e^{-h-M} + e^{|u|-M} + e^{-|u|-M}),
// M = max(h, |u|): no cancellation for close levels, no overflow far from mu.
__device__ __forceinline__ double opt_weight(const double en, const double em, const double eps, const double mu, const double kT) {
    if (kT == 0.0) return (en <= mu && !(em <= mu)) ? -1.0 / eps : 0.0;
    const double h = 0.5 * eps / kT, u = fabs((0.5 * (en + em) - mu) / kT), M = fmax(h, u);
    const double den = exp(h - M) + exp(-h - M) + exp(u - M) + exp(-u - M);
    return exp(h - M) * expm1(-2.0 * h) / den / eps;
}

// V^d = conj(U) W^d for every (point, direction) z = ik nd + d (blockIdx.z): 16 x 16 output tiles, the 16-wide slices of conj(U) and
// W^d staged in LDS.  vt[ik][d][n][n], V^d[b][m] = <b| d_d H |m>.
static __global__ __launch_bounds__(256) void k_opt_vprod(const cd* __restrict__ evec, const cd* __restrict__ wt, const int64_t nk, const int n,
                                                   const int nd, cd* __restrict__ vt) {
    __shared__ cd Ut[16][17], Wt[16][17];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int64_t zi = blockIdx.z, nn = (int64_t)n * n;
    const int64_t ik = zi / nd;
    const int row = blockIdx.y * 16 + ty, col = blockIdx.x * 16 + tx;
    const cd* w = wt + zi * nn;
    cd acc{0.0, 0.0};
    for (int k0 = 0; k0 < n; k0 += 16) {
        const int uc = k0 + tx, wr = k0 + ty;
        Ut[ty][tx] = (row < n && uc < n) ? evec[((int64_t)row * nk + ik) * n + uc] : cd{0.0, 0.0};
        Wt[ty][tx] = (wr < n && col < n) ? w[(int64_t)wr * n + col] : cd{0.0, 0.0};
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 16; ++q) cfmac(acc, Ut[ty][q], Wt[q][tx]);
        __syncthreads();
    }
    if (row < n && col < n) vt[zi * nn + (int64_t)row * n + col] = acc;
}

// 1 / x by v_rcp_f64 and two Newton steps (x > 0, normal)
__device__ __forceinline__ double opt_rcp(const double x) {
    double r = __builtin_amdgcn_rcp(x);
    double e = fma(-x, r, 1.0);
    r = fma(r, e, r);
    e = fma(-x, r, 1.0);
    return fma(r, e, r);
}

// rows[r] = inv sum_g part[g][r] in a fixed order (one workgroup per row)
static __global__ __launch_bounds__(256) void k_opt_rows(const double* __restrict__ part, const int G, const int64_t nrows, const double inv,
                                                  double* __restrict__ rows) {
    __shared__ double red[4];
    double acc = 0.0;
    for (int g = threadIdx.x; g < G; g += 256) acc += part[(int64_t)g * nrows + blockIdx.x];
    const double t = block_sum(acc, red);
    if (threadIdx.x == 0) rows[blockIdx.x] = t * inv;
}
