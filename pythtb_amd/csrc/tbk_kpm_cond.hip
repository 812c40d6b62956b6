// tbk_kpm_cond.hip -- kernel polynomial method: the double Chebyshev moments of the Kubo-Bastin conductivity.
//
//   mu^{ab}_mn(v) = <v| V^a T_m(H~) V^b T_n(H~) |v> / <v|v>,   m, n < M,   H~ = (H(k) - b) / a,   V^a = dH/dk_a (reduced coordinates)
//
// on the sparse operator of tbk_kpm.hip (Garcia, Covaci, Rappoport, Phys. Rev. Lett. 114, 116602).  dH/dk_a has the sparsity of H: the
// entry of H times 2 pi i (R + orb_col - orb_row)_a, the convention of tbk_gen_dham -- nothing new is uploaded.  No reference
// counterpart (PythTB 1.8 has no sparse operator).
//
// Per k: the values of H, V^a and V^b in one pass.  Per block of NV = 8 start vectors r:
//   Phi_n = T_n(H~) r for all n < M, kept in a workspace phi[n][row][NV];
//   chi_0 = V^a r, chi_m = T_m(H~) chi_0 (two buffers), psi_m = V^b chi_m in tiles psi[m - m0][row][NV] of KPMC_TM moments;
//   H~, V^a and V^b are Hermitian, so mu_mn = <psi_m|Phi_n>: every tile is contracted against all of Phi by k_kpm_contract, a
//   (TM x nsta).(nsta x M) complex product per vector, into per-workgroup partial sums that k_kpm_contract_reduce adds in ascending
//   order (no floating-point atomics: two calls give the same bits) and divides by <r|r>.
// 3 M sparse products and M^2 nsta complex multiply-adds per vector.  The contraction runs on the vector unit: on gfx950 the fp64
// matrix instruction has the vector unit's rate, and with the vector index fastest in memory a lane owns one (row, vector) pair and
// reads 16 contiguous bytes per operand -- the matrix instruction would want the row index across the lanes of one vector, a strided
// gather of this layout.  Each lane keeps a 4 x 4 tile of (m, n) sums in registers; the four wavefronts of a workgroup take the four
// quarters of the psi tile against the same four Phi_n, whose loads the later wavefronts find in the vector cache.
// Launches on the context's stream, one host synchronisation at the end of the call.
#include <math.h>
#include <algorithm>
#include <cmath>
#include "tbk_kpm.h"

#define KPMC_TM 16                           // moments of psi per tile: 4 per wavefront
#define KPMC_TN 4                            // moments of Phi per workgroup
#define KPMC_MAX_CHUNKS 256                  // row chunks of a contraction = partial sums per moment pair
#define KPMC_PART_BYTES ((size_t)64 << 20)   // ... and the workspace they may take

// ------------------------------------------------------------------ kernels
// part[chunk][m][n][NV] = sum over the rows of the chunk of conj(psi[m][row][v]) phi[n][row][v], m < KPMC_TM (zero from mt on),
// n < nmom.  grid (chunks, ceil(nmom / KPMC_TN)); chunk c takes the row tiles c, c + chunks, ... of 64 / NV rows.  A lane owns one
// (row, vector) pair and a 4 x 4 tile of sums: wavefront w the moments 4 w .. 4 w + 3 of psi, the workgroup the moments
// n0 .. n0 + 3 of Phi; the 64 / NV rows of a wavefront are added by shuffles in a fixed order at the end.
template <int NV>
__global__ __launch_bounds__(256) void k_kpm_contract(const int nsta, const int nmom, const int mt, const cd* __restrict__ psi,
                                                      const cd* __restrict__ phi, cd* __restrict__ part) {
    constexpr int RPW = 64 / NV;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, v = lane % NV, rw = lane / NV;
    const int m0 = wave * 4, n0 = blockIdx.y * KPMC_TN;
    const int64_t ntiles = ((int64_t)nsta + RPW - 1) / RPW;
    cd acc[4][KPMC_TN];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < KPMC_TN; ++j) acc[i][j] = cd{0.0, 0.0};
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row = tile * RPW + rw;
        if (row < nsta) {
            cd p[4], f[KPMC_TN];
#pragma unroll
            for (int i = 0; i < 4; ++i) p[i] = m0 + i < mt ? psi[((int64_t)(m0 + i) * nsta + row) * NV + v] : cd{0.0, 0.0};
#pragma unroll
            for (int j = 0; j < KPMC_TN; ++j) f[j] = n0 + j < nmom ? phi[((int64_t)(n0 + j) * nsta + row) * NV + v] : cd{0.0, 0.0};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < KPMC_TN; ++j) cfmac(acc[i][j], p[i], f[j]);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < KPMC_TN; ++j) {
#pragma unroll
            for (int o = NV; o < 64; o <<= 1) {
                acc[i][j].x += __shfl_xor(acc[i][j].x, o);
                acc[i][j].y += __shfl_xor(acc[i][j].y, o);
            }
            if (lane < NV && n0 + j < nmom) part[(((int64_t)blockIdx.x * KPMC_TM + m0 + i) * nmom + n0 + j) * NV + lane] = acc[i][j];
        }
}

// mu[v][m0 + m][n] = sum over the chunks, in ascending order, of part[chunk][m][n][v], divided by <r_v|r_v> = norm[v];
// m < mt, n < nmom, v < nv; a thread per element
template <int NV>
__global__ __launch_bounds__(256) void k_kpm_contract_reduce(const int nchunk, const int nmom, const int mt, const int nv, const int m0,
                                                             const cd* __restrict__ part, const double* __restrict__ norm,
                                                             cd* __restrict__ mu) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)mt * nmom * nv) return;
    const int v = (int)(idx % nv), n = (int)((idx / nv) % nmom), m = (int)(idx / ((int64_t)nv * nmom));
    cd s{0.0, 0.0};
    for (int c = 0; c < nchunk; ++c) s = cadd(s, part[(((int64_t)c * KPMC_TM + m) * nmom + n) * NV + v]);
    const double a0 = norm[v];
    mu[((int64_t)v * nmom + m0 + m) * nmom + n] = cd{s.x / a0, s.y / a0};
}

// ------------------------------------------------------------------ host entry point
extern "C" int tbk_kpm_double_moments(tbk_sparse* sp, const double* k, int64_t nk, int n_moments, double emin, double emax, int dir_a,
                                      int dir_b, int nvec, const double* vectors, const int32_t* states, uint64_t seed, double* mu) {
    constexpr int NV = KPM_NV, NC = 2 * NV;
    TBK_REQUIRE(sp && mu, TBK_EINVAL, "tbk_kpm_double_moments: null argument");
    const int dim_k = sp->dim_k, n = sp->nsta, M = n_moments;
    TBK_REQUIRE(dim_k >= 1, TBK_EINVAL, "tbk_kpm_double_moments: the velocity operator needs a periodic axis (dim_k = 0)");
    TBK_REQUIRE(dir_a >= 0 && dir_a < dim_k && dir_b >= 0 && dir_b < dim_k, TBK_EINVAL,
                "tbk_kpm_double_moments: directions (%d, %d) outside [0, %d)", dir_a, dir_b, dim_k);
    int rc = kpm_check_args("tbk_kpm_double_moments", sp, "n_moments", M, nvec, vectors, states, emin, emax, k, &nk);
    if (rc) return rc;
    if (nk == 0) return TBK_OK;
    tbk_ctx* ctx = sp->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    const double a = 0.5 * (emax - emin), b = 0.5 * (emax + emin), inv_a = 1.0 / a;
    const int nwg = kpm_plan(n, 0).nwg;
    const size_t vec_len = (size_t)n * NV;                        // one block of vectors
    const size_t chunk_len = (size_t)KPMC_TM * M * NV;            // the partial sums of one row chunk
    const int nchunk = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(((int64_t)n + 64 / NV - 1) / (64 / NV), KPMC_MAX_CHUNKS),
                                                                   (int64_t)(KPMC_PART_BYTES / (chunk_len * sizeof(cd)))));
    KpmStart start(sp, k, nk, nvec, vectors, states, seed);
    cd *val, *va, *vb, *chi0, *chi1, *phi, *psi, *part, *mu_dev;
    double *npart, *norm;
    size_t total;
    rc = kpm_workspace(ctx, [&](KpmCarve& c) {
        c.take(val, (size_t)sp->nnz);
        c.take(va, (size_t)sp->nnz);
        c.take(vb, (size_t)sp->nnz);
        c.take(chi0, vec_len);
        c.take(chi1, vec_len);
        c.take(phi, (size_t)M * vec_len);
        c.take(psi, (size_t)KPMC_TM * vec_len);
        c.take(part, (size_t)nchunk * chunk_len);
        c.take(npart, (size_t)nwg * NC);
        c.take(norm, (size_t)NC);
        c.take(mu_dev, (size_t)nk * nvec * M * M);
        start.carve(c);
    }, &total);
    if (rc == TBK_ENOMEM) {
        (void)hipGetLastError();
        tbk_set_error("tbk_kpm_double_moments: no device workspace of %zu bytes (%zu of them for the %d vectors T_n(H~) r of %d "
                      "states, 8 start vectors at a time): use fewer moments",
                      total, up256((size_t)M * vec_len * sizeof(cd)), M, n);
    }
    if (rc) return rc;
    rc = start.upload(ctx);
    if (rc) return rc;
    // out = 2 H~ in - prev, out possibly prev; first: out = H~ in, or with the values of a velocity operator and (shift, scale) =
    // (0, 1) the plain product
    auto apply = [&](const char* name, const cd* values, const cd* in, bool first, const cd* prev, cd* out, double shift,
                     double scale) -> int {
        auto kernel = first ? k_kpm_step<NV, true, KpmNoSums>
                            : (prev == out ? k_kpm_step<NV, false, KpmNoSums> : k_kpm_step<NV, false, KpmNoSums, false>);
        ProfScope ps(ctx, name);
        hipLaunchKernelGGL(kernel, dim3(nwg), dim3(256), 0, ctx->stream, n, sp->row_ptr, sp->col, values, in, prev, out, shift, scale,
                           KpmNoSums{});
        TBK_HIP(hipGetLastError());
        return TBK_OK;
    };
    for (int64_t q = 0; q < nk; ++q) {
        {
            ProfScope ps(ctx, "kpm_cond_values");
            hipLaunchKernelGGL(k_kpm_values<true>, dim3(kpm_stream_grid(sp->nnz)), dim3(256), 0, ctx->stream, sp->nnz, dim_k, dir_a, dir_b,
                               start.k_at(q), sp->col, sp->row_of, sp->amp, sp->R, sp->orb, val, va, vb);
            TBK_HIP(hipGetLastError());
        }
        for (int v0 = 0; v0 < nvec; v0 += NV) {
            const int nv = std::min(NV, nvec - v0);
            rc = start.launch(ctx, nwg, q, v0, nv, phi, npart);    // Phi_0 = r and the partial sums of <r|r>
            if (rc) return rc;
            rc = kpm_reduce(ctx, nwg, 1, npart, norm);
            if (rc) return rc;
            for (int j = 1; j < M; ++j) {   // Phi_j = T_j(H~) r
                cd* out = phi + (size_t)j * vec_len;
                rc = apply("kpm_apply", val, out - vec_len, j == 1, out - 2 * vec_len, out, b, inv_a);
                if (rc) return rc;
            }
            cd *x = chi0, *y = chi1;        // x = chi_m, y = chi_m-1
            for (int m0 = 0; m0 < M; m0 += KPMC_TM) {
                const int mt = std::min(KPMC_TM, M - m0);
                for (int m = m0; m < m0 + mt; ++m) {
                    if (m == 0) {
                        rc = apply("kpm_apply_v", va, phi, true, nullptr, x, 0.0, 1.0);              // chi_0 = V^a r
                    } else {
                        rc = apply("kpm_apply", val, x, m == 1, y, y, b, inv_a);    // chi_1 = H~ chi_0, chi_m+1 = 2 H~ chi_m - chi_m-1 over chi_m-1
                        std::swap(x, y);
                    }
                    if (rc) return rc;
                    rc = apply("kpm_apply_v", vb, x, true, nullptr, psi + (size_t)(m - m0) * vec_len, 0.0, 1.0);   // psi_m = V^b chi_m
                    if (rc) return rc;
                }
                {
                    ProfScope ps(ctx, "kpm_contract");
                    hipLaunchKernelGGL((k_kpm_contract<NV>), dim3(nchunk, (M + KPMC_TN - 1) / KPMC_TN), dim3(256), 0, ctx->stream, n, M, mt,
                                       psi, phi, part);
                    TBK_HIP(hipGetLastError());
                }
                {
                    ProfScope ps(ctx, "kpm_contract_reduce");
                    const int64_t items = (int64_t)mt * M * nv;
                    hipLaunchKernelGGL((k_kpm_contract_reduce<NV>), dim3((unsigned)((items + 255) / 256)), dim3(256), 0, ctx->stream, nchunk,
                                       M, mt, nv, m0, part, norm, mu_dev + ((size_t)q * nvec + v0) * M * M);
                    TBK_HIP(hipGetLastError());
                }
            }
        }
    }
    const size_t nmu = (size_t)nk * nvec * M * M;
    TBK_HIP(hipMemcpyAsync(mu, mu_dev, nmu * sizeof(cd), hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    // divergence guard: |T_m(x)| <= 1 only inside [-1, 1], so |mu_mn| <= ||V^a|| ||V^b|| there; outside, the recursion grows without limit
    const double cap = (1.0 + 1e-6) * sp->vbound[dir_a] * sp->vbound[dir_b];
    for (size_t i = 0; i < nmu; ++i) {
        const double re = mu[2 * i], im = mu[2 * i + 1];
        if (!(std::isfinite(re) && std::isfinite(im) && re * re + im * im <= cap * cap)) {
            const size_t mn = i % ((size_t)M * M);
            tbk_set_error("tbk_kpm_double_moments: moment (%lld, %lld) of sample %lld is (%g, %g), beyond ||V^a|| ||V^b|| <= %g: the bounds "
                          "(%.17g, %.17g) do not contain the spectrum (Gershgorin interval of this operator: (%.17g, %.17g))",
                          (long long)(mn / (size_t)M), (long long)(mn % (size_t)M), (long long)(i / ((size_t)M * M)), re, im,
                          sp->vbound[dir_a] * sp->vbound[dir_b], emin, emax, sp->gmin, sp->gmax);
            return TBK_EINVAL;
        }
    }
    return TBK_OK;
}
