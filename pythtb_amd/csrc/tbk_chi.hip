// tbk_chi.hip -- the bare (Lindhard) susceptibility chi0(q, w) on uniform meshes.
//
// k and q in reduced coordinates, E_n(k) and u_n(k) the eigenpairs of the solver (the convention-II matrix of tbk_gen_ham: u is the
// cell-periodic part), f = [E <= mu] (kT = 0) or 1 / (1 + exp((E - mu) / kT)), M_nm(k, q) = sum_j conj(u_n(k)[j]) u_m(k+q)[j]:
//   dynamic   chi0(q, w) = -(1 / N_k) sum_k sum_{n,m} [f_n(k) - f_m(k+q)] |M_nm|^2 / (w + i eta + E_n(k) - E_m(k+q))
//   static    chi0(q)    =  (1 / N_k) sum_k sum_{n,m} L_nm |M_nm|^2,   L = -(f_n - f_m) / (E_n - E_m), -f'(E) where the levels meet
// over ALL n^2 ordered pairs (n = m included); without TBK_CHI_MATRIX_ELEMENTS |M|^2 = 1 and no eigenvector is formed anywhere.
//
// Pipeline, in chunks of a fixed number of mesh points (tbk_chi.h's plan; tbk_kubo.h's chunk loop kubo_for_chunks): the device k
// generator and the list solver at k ONCE per chunk, then for every q of the list
//   k_chi_kq       k + q
//   the list solver at k + q (eigenvalues only without matrix elements) into the chunk's first extra buffer
//   PAIR stage     n <= 32   k_chi_pairs: U(k) and U(k+q) of P points in LDS, one lane per (point, n, m) forms M_nm
//                  n > 32    k_chi_mprod (|conj(U(k)) U(k+q)^T|^2 in 16 x 16 LDS tiles), then k_chi_lanes, one lane per (point, n, m)
//                  no matrix elements: k_chi_lanes alone
//                  static: every lane forms L |M|^2 and the workgroup's sum goes to part[g]; dynamic: a record (d, c) =
//                  (E_n - E_m, (f_n - f_m) |M|^2) per ordered pair
//   FREQUENCY stage (dynamic) k_chi_omega: x = sum c (w + d) r and y = sum c r, r = 1 / ((w + d)^2 + eta^2), per k-group
//   k_group_rows   acc[q][row] (+)= sum_g part[g][row], the groups in a fixed order, chunk after chunk in stream order
// and chi0 = (-x + i eta y) / N_k on the host.  The chunk, the groups and the tiles do not depend on the q list and nothing uses
// atomics: two calls give the same bits, and a q gives the same bits alone and inside a longer list.
#include <math.h>
#include "tbk_chi.h"
#include "tbk_chi_dev.h"

// what a lane does with its ordered pair (n at k, m at k + q) of point ik: the record, or its term of the static sum
template <bool STATIC>
__device__ __forceinline__ double chi_pair(const double en, const double em, const double m2, const double mu, const double kT,
                                           double* __restrict__ rec) {
    if constexpr (STATIC) return chi_static_weight(en, em, mu, kT) * m2;
    rec[0] = en - em;
    rec[1] = chi_fdiff(en, em, mu, kT) * m2;
    return 0.0;
}

// ---------------------------------------------------------------- pair stage, 1 .. 32 states with matrix elements
// P points per workgroup, U(k) and U(k+q) in LDS; one lane per (point, n, m).  The lane of column m starts its dot product at
// component m (and wraps): the 16 lanes of a ds_read_b128 group then read 16 different 16-byte slots of 256 B for any n that is a
// multiple of 16, where rows n apart would all meet in one.  out: the records [ik][n][m][2], or part[workgroup].
template <bool STATIC>
__global__ __launch_bounds__(256) void k_chi_pairs(const cd* __restrict__ evec1, const cd* __restrict__ evec2, const double* __restrict__ e1,
                                                   const double* __restrict__ e2, const int64_t nk, const int n, const int P,
                                                   const double mu, const double kT, double* __restrict__ out) {
    __shared__ cd L[CHI_LDS_CD];
    __shared__ double red[4];
    const int nn = n * n;
    const int64_t ik0 = (int64_t)blockIdx.x * P;
    const int np = (int)std::min<int64_t>(P, nk - ik0);
    cd* U1 = L;
    cd* U2 = L + P * nn;
    kubo_lds_load(U1, evec1, nk, ik0, np, n, nn, [](int) {});
    kubo_lds_load(U2, evec2, nk, ik0, np, n, nn, [](int) {});
    __syncthreads();
    double acc = 0.0;
    for (int e = threadIdx.x; e < np * nn; e += 256) {
        const int p = e / nn, r = e - p * nn, a = r / n, b = r - a * n;
        const cd* ua = U1 + p * nn + a * n;
        const cd* ub = U2 + p * nn + b * n;
        cd mm{0.0, 0.0};
        int j = b;
        for (int t = 0; t < n; ++t) {
            cfmac(mm, ua[j], ub[j]);
            j = j + 1 == n ? 0 : j + 1;
        }
        const int64_t ik = ik0 + p;
        acc += chi_pair<STATIC>(e1[(int64_t)a * nk + ik], e2[(int64_t)b * nk + ik], cabs2(mm), mu, kT, out + (ik * nn + r) * 2);
    }
    if constexpr (STATIC) {
        const double t = block_sum(acc, red);
        if (threadIdx.x == 0) out[blockIdx.x] = t;
    }
}

// ---------------------------------------------------------------- pair stage, 33 .. 2048 states
// m2[ik][a][b] = |sum_j conj(u_a(k)[j]) u_b(k+q)[j]|^2: 16 x 16 output tiles (blockIdx.y, blockIdx.x) of point blockIdx.z.  Both
// operands come as evec[state][point][component], so both 16-wide slices are read along the components (lane tx) and the second one
// is used transposed from LDS (row stride 17: the 16 lanes of a group read 16 different slots).
__global__ __launch_bounds__(256) void k_chi_mprod(const cd* __restrict__ evec1, const cd* __restrict__ evec2, const int64_t nk, const int n,
                                                   double* __restrict__ m2) {
    __shared__ cd At[16][17], Bt[16][17];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int64_t ik = blockIdx.z, nn = (int64_t)n * n;
    const int row = blockIdx.y * 16 + ty, col = blockIdx.x * 16 + tx;
    const int brow = blockIdx.x * 16 + ty;                         // the state of evec2 this lane loads
    cd acc{0.0, 0.0};
    for (int k0 = 0; k0 < n; k0 += 16) {
        const int c = k0 + tx;
        At[ty][tx] = (row < n && c < n) ? evec1[((int64_t)row * nk + ik) * n + c] : cd{0.0, 0.0};
        Bt[ty][tx] = (brow < n && c < n) ? evec2[((int64_t)brow * nk + ik) * n + c] : cd{0.0, 0.0};
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 16; ++j) cfmac(acc, At[ty][j], Bt[tx][j]);
        __syncthreads();
    }
    if (row < n && col < n) m2[ik * nn + (int64_t)row * n + col] = cabs2(acc);
}

// One lane per (point, n, m) on |M|^2 from m2 (null: 1, no matrix elements): workgroup g takes the points [g nk / G, (g + 1) nk / G)
// of the chunk.  out: the records, or part[g].
template <bool STATIC>
__global__ __launch_bounds__(256) void k_chi_lanes(const double* __restrict__ e1, const double* __restrict__ e2, const double* __restrict__ m2,
                                                   const int64_t nk, const int n, const int G, const double mu, const double kT,
                                                   double* __restrict__ out) {
    __shared__ double red[4];
    const int64_t nn = (int64_t)n * n;
    const int64_t p0 = (int64_t)blockIdx.x * nk / G, p1 = (int64_t)(blockIdx.x + 1) * nk / G;
    double acc = 0.0;
    for (int64_t e = threadIdx.x; e < (p1 - p0) * nn; e += 256) {
        const int64_t ik = p0 + e / nn, r = e % nn;
        const int a = (int)(r / n), b = (int)(r - (int64_t)a * n);
        const int64_t i = ik * nn + r;
        acc += chi_pair<STATIC>(e1[(int64_t)a * nk + ik], e2[(int64_t)b * nk + ik], m2 ? m2[i] : 1.0, mu, kT, out + i * 2);
    }
    if constexpr (STATIC) {
        const double t = block_sum(acc, red);
        if (threadIdx.x == 0) out[blockIdx.x] = t;
    }
}

// ---------------------------------------------------------------- frequency stage
// Workgroup (tile of kPairTile frequencies, k-group g), the plan of tbk_pairs.h's k_pair_omega, kept as this unit's own text: as a
// policy of that kernel the same loop body compiled with its scalar adds in another order and measured slower (DESIGN.md section 14,
// last addendum).  Lane t takes w[tile + t] and w[tile + 256 + t] and walks the records of the points [g nk / G, (g + 1) nk / G) of
// the chunk in order (wave-uniform values; c = 0: skipped).
// part[g][0][w] = sum c (w + d) r, part[g][1][w] = sum c r with r = 1 / ((w + d)^2 + eta^2).  A tile whose second half holds no
// frequency (nw <= 256, or the last tile) walks with one frequency per lane: the same operations on that one, half the work.
template <int NS>
__device__ __forceinline__ void chi_walk(const double* __restrict__ p, const int64_t nrec, const double (&om)[2], const double eta2,
                                         double (&sx)[2], double (&sy)[2]) {
    for (int64_t r = 0; r < nrec; ++r, p += 2) {
        const double d = p[0], c = p[1];
        if (c == 0.0) continue;                                    // (uniform branch)
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const double t = om[s] + d;
            const double rr = opt_rcp(fma(t, t, eta2));
            sx[s] = fma(c * t, rr, sx[s]);
            sy[s] = fma(c, rr, sy[s]);
        }
    }
}
__global__ __launch_bounds__(256) void k_chi_omega(const double* __restrict__ rec, const int64_t nk, const int64_t nn, const int G,
                                                   const double* __restrict__ omega, const int nw, const double eta,
                                                   double* __restrict__ part) {
    const int base = blockIdx.x * kPairTile;
    if (base + (int)(threadIdx.x & ~63u) >= nw) return;            // a wavefront without a frequency (uniform)
    const int g = blockIdx.y;
    int wi[2];
    double om[2], sx[2] = {0.0, 0.0}, sy[2] = {0.0, 0.0};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        wi[s] = base + s * 256 + threadIdx.x;
        om[s] = wi[s] < nw ? omega[wi[s]] : 0.0;
    }
    const int64_t r0 = (int64_t)g * nk / G * nn, r1 = (int64_t)(g + 1) * nk / G * nn;
    if (base + 256 < nw) chi_walk<2>(rec + r0 * 2, r1 - r0, om, eta * eta, sx, sy);   // (uniform over the workgroup)
    else chi_walk<1>(rec + r0 * 2, r1 - r0, om, eta * eta, sx, sy);
    double* out = part + (int64_t)g * 2 * nw;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        if (wi[s] >= nw) continue;
        out[wi[s]] = sx[s];
        out[nw + wi[s]] = sy[s];
    }
}

// ---------------------------------------------------------------- host side
template <bool STATIC>
static int chi_pair_stage(tbk_model* m, const ChiPlan& pl, int64_t cnt, const double* e1, const cd* v1, const double* e2, const cd* v2,
                          double* m2, double mu, double kT, double* out, int& groups) {
    tbk_ctx* ctx = m->ctx;
    const int n = m->nsta;
    if (pl.lds) {
        ProfScope ps(ctx, "chi_pairs");
        groups = (int)((cnt + pl.P - 1) / pl.P);
        hipLaunchKernelGGL(k_chi_pairs<STATIC>, dim3((unsigned)groups), dim3(256), 0, ctx->stream, v1, v2, e1, e2, cnt, n, pl.P, mu, kT, out);
        TBK_HIP(hipGetLastError());
        return TBK_OK;
    }
    if (pl.wide) {
        // cnt <= kKuboChunkBytes / (33^2 16 B) < 65536 (the grid's z limit)
        ProfScope ps(ctx, "chi_mprod");
        const unsigned t = (unsigned)((n + 15) / 16);
        hipLaunchKernelGGL(k_chi_mprod, dim3(t, t, (unsigned)cnt), dim3(256), 0, ctx->stream, v1, v2, cnt, n, m2);
        TBK_HIP(hipGetLastError());
    }
    ProfScope ps(ctx, "chi_pairs");
    groups = pl.G;
    hipLaunchKernelGGL(k_chi_lanes<STATIC>, dim3((unsigned)pl.G), dim3(256), 0, ctx->stream, e1, e2, (const double*)(pl.wide ? m2 : nullptr),
                       cnt, n, pl.G, mu, kT, out);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

extern "C" int tbk_susceptibility_mesh(tbk_model* m, const int32_t* mesh, int nq, const double* q, int nomega, const double* omega,
                                       double eta, double mu, double kT, int flags, double* out) {
    const char* fn = "tbk_susceptibility_mesh";
    TBK_REQUIRE(m && mesh && q && out, TBK_EINVAL, "%s: null argument", fn);
    const int dk = m->dim_k, n = m->nsta;
    int64_t npts;
    int rc = chi_check(fn, dk, n, mesh, nq, q, nomega, omega, eta, mu, kT, flags, npts);
    if (rc) return rc;
    const ChiPlan pl = chi_plan(n, dk, npts, nq, nomega, flags);
    tbk_ctx* ctx = m->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    void* base = nullptr;
    rc = tbk_ctx_scratch(ctx, pl.total, &base);
    if (rc) return rc;
    unsigned char* b = (unsigned char*)base;
    double* om_dev = (double*)(b + pl.off_om);
    double* q_dev = (double*)(b + pl.off_q);
    double* acc = (double*)(b + pl.off_acc);
    double* part = (double*)(b + pl.off_part);
    KuboChunks cw = pl.cw;
    cw.base = b + pl.off_chunks;
    unsigned char* x0 = cw.extra<unsigned char>(0);
    double* kq = (double*)x0;
    double* e2 = (double*)(x0 + pl.off_e2);
    cd* v2 = pl.me ? (cd*)(x0 + pl.off_v2) : nullptr;
    double* rec = cw.extra<double>(1);
    double* m2 = cw.extra<double>(2);
    if (pl.dynamic) TBK_HIP(hipMemcpyAsync(om_dev, omega, (size_t)nomega * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    TBK_HIP(hipMemcpyAsync(q_dev, q, (size_t)nq * dk * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    const int64_t nn = (int64_t)n * n;
    // the solve at k once per chunk (eigenvalues only without matrix elements: v1 is null), then every q of the list
    rc = kubo_for_chunks(m, cw, nullptr, mesh, npts, [&](int64_t first, int64_t cnt, const double* kc, const double* e1, const cd* v1) -> int {
        for (int iq = 0; iq < nq; ++iq) {
            {
                ProfScope ps(ctx, "chi_kq");
                hipLaunchKernelGGL(k_chi_kq, dim3(nblk(cnt * dk)), dim3(256), 0, ctx->stream, kc, (const double*)(q_dev + (int64_t)iq * dk), cnt,
                                   dk, kq);
                TBK_HIP(hipGetLastError());
            }
            int r2 = tbk_solve_list_dev_checked(m, kq, cnt, e2, (double*)v2);
            if (r2) return r2;
            int groups = 0;
            if (pl.dynamic) {
                r2 = chi_pair_stage<false>(m, pl, cnt, e1, v1, e2, v2, m2, mu, kT, rec, groups);
                if (r2) return r2;
                ProfScope ps(ctx, "chi_omega");
                groups = pl.G;
                hipLaunchKernelGGL(k_chi_omega, dim3(pl.ntile, (unsigned)pl.G), dim3(256), 0, ctx->stream, (const double*)rec, cnt, nn, pl.G,
                                   (const double*)om_dev, nomega, eta, part);
                TBK_HIP(hipGetLastError());
            } else {
                r2 = chi_pair_stage<true>(m, pl, cnt, e1, v1, e2, v2, m2, mu, kT, part, groups);
            }
            if (r2) return r2;
            ProfScope ps(ctx, "chi_rows");
            hipLaunchKernelGGL(k_group_rows, dim3((unsigned)pl.nrows), dim3(256), 0, ctx->stream, (const double*)part, groups, pl.nrows, 1.0,
                               first > 0 ? 1 : 0, acc + (int64_t)iq * pl.nrows);
            TBK_HIP(hipGetLastError());
        }
        return TBK_OK;
    });
    if (rc) return rc;
    std::vector<double> sums((size_t)pl.acc_doubles);
    TBK_HIP(hipMemcpyAsync(sums.data(), acc, sums.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    const double nk = (double)npts;
    if (!pl.dynamic) {
        for (int iq = 0; iq < nq; ++iq) out[iq] = sums[iq] / nk;
        return TBK_OK;
    }
    for (int iq = 0; iq < nq; ++iq) {
        const double* s = sums.data() + (size_t)iq * pl.nrows;
        for (int w = 0; w < nomega; ++w) {
            double* o = out + 2 * ((size_t)iq * nomega + w);
            o[0] = (0.0 - s[w]) / nk;
            o[1] = eta * s[nomega + w] / nk;
        }
    }
    return TBK_OK;
}
