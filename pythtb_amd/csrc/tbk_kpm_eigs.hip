// tbk_kpm_eigs.hip -- kernel polynomial method: the eigenpairs of the sparse H(k) inside an energy window, for any number of
// states.  Chebyshev-filtered subspace iteration (Pieper, Kreutzer, Alvermann, Galgon, Fehske, Hager,
// Lang, Wellein, J. Comput. Phys. 325, 226); the filter-norm test for spurious Ritz values follows FEAST's reduced-filter test.
//
//   X: n_search start vectors.  Per iteration: Y = p(H~) X, p the Jackson-damped Chebyshev series of the indicator of the widened
//   window (kpm_series_run, block by block); G = Y^H Y, A = Y^H H Y (k_kpm_gram); on the host eigh(G) -> Wh, B = Wh^H A Wh,
//   eigh(B) -> W, theta; X <- Y (Wh W) (k_kpm_rotate); r_j = |H x_j - theta_j x_j| (k_kpm_step with the KpmResid epilogue).
//   tau_j = sqrt(G_jj) of the NEXT iteration is the filter norm of Ritz vector j: an eigenvector inside the window has tau >= 1/2,
//   a mixture of states on both sides of it whose Rayleigh quotient falls inside has not.  Done when every pair with tau >= 1/2
//   and theta inside the window has r <= tol a and fewer pairs have tau >= 1/2 than the subspace has directions.
//
// No reference counterpart (PythTB 1.8 has no sparse operator).  One plain launch per stage on the context's stream, one host
// synchronisation per iteration besides those of the two dense solves; fixed-order sums, no floating-point atomics, no grid
// barrier, no persistent kernel: two calls give the same bits.
#include <math.h>
#include <algorithm>
#include <cmath>
#include <new>
#include <vector>
#include "tbk_kpm_eigs.h"

// ------------------------------------------------------------------ kernels
// cur[row][NV] = scale in[row][NV] and the partial sums of <cur|cur>: the start of a series from a block of X
template <int NV>
__global__ __launch_bounds__(256) void k_kpm_eigs_load(const int nsta, const double scale, const cd* __restrict__ in,
                                                       cd* __restrict__ cur, double* __restrict__ part) {
    double dA = 0.0;
    kpm_for_rows<NV>(nsta, [&](const int64_t row, const int v) {
        const cd x = cscale(in[row * NV + v], scale);
        cur[row * NV + v] = x;
        dA += cabs2(x);
    });
    kpm_block_sums<NV>(dA, 0.0, part);
}

// The epilogue of k_kpm_step (FIRST, (b, 1 / a) = (0, 1): nw = H cur) that leaves the row-local sums of |nw - theta_v cur|^2.
struct KpmResid {
    static constexpr bool SUMS = true;
    const double* theta;     // [NV], the Ritz values of this block
    double* part;
    template <int NV, bool FIRST>
    __device__ __forceinline__ void row(int, int64_t, const int v, const cd x0, const cd nw, double& dA, double&) const {
        const double t = theta[v];
        const double dx = fma(-t, x0.x, nw.x), dy = fma(-t, x0.y, nw.y);
        dA = fma(dx, dx, fma(dy, dy, dA));
    }
};

// The 8 x 8 sums over the rows of conj(Y_p[row][i]) Y_q[row][j] (G) and conj(Y_p[row][i]) Z_q[row][j] (A, Z = H Y) for the block
// pair number pair0 + blockIdx.y of the upper block triangle, pairs counted (0,0), (0,1) .. (0,nb-1), (1,1) ...  A lane per (i, j);
// a wavefront walks 16 rows of a tile of 64, the workgroups stride over the tiles; the four wavefronts are added through LDS in
// a fixed order.  part[(pair in launch) * 16 + c / 16][workgroup][c % 16], c = component * 64 + i * 8 + j with the components
// (Re G, Im G, Re A, Im A): the layout k_kpm_reduce adds up, 16 slots per pair.
template <int NV>
__global__ __launch_bounds__(256) void k_kpm_gram(const int nsta, const int nb, const int64_t pair0, const cd* __restrict__ Y,
                                                  const cd* __restrict__ Z, double* __restrict__ part) {
    static_assert(NV == 8, "k_kpm_gram: a wavefront holds the 8 x 8 pairs of two blocks");
    constexpr int TR = 64, RW = TR / 4;
    int64_t idx = pair0 + blockIdx.y;
    int p = 0;
    while (idx >= nb - p) {
        idx -= nb - p;
        ++p;
    }
    const int q = p + (int)idx;
    const cd* yp = Y + (int64_t)p * nsta * NV;
    const cd* yq = Y + (int64_t)q * nsta * NV;
    const cd* zq = Z + (int64_t)q * nsta * NV;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane / NV, j = lane % NV;
    cd g{0.0, 0.0}, h{0.0, 0.0};
    const int64_t ntiles = ((int64_t)nsta + TR - 1) / TR;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t r0 = tile * TR + wave * RW, r1 = r0 + RW < nsta ? r0 + RW : (int64_t)nsta;
        for (int64_t row = r0; row < r1; ++row) {
            const cd a = yp[row * NV + i];
            cfmac_x(g, yq[row * NV + j], a);      // += conj(a) y
            cfmac_x(h, zq[row * NV + j], a);
        }
    }
    __shared__ double red[4][4][64];
    red[wave][0][lane] = g.x;
    red[wave][1][lane] = g.y;
    red[wave][2][lane] = h.x;
    red[wave][3][lane] = h.y;
    __syncthreads();
    const int c = threadIdx.x, comp = c >> 6, ij = c & 63;
    const double s = ((red[0][comp][ij] + red[1][comp][ij]) + red[2][comp][ij]) + red[3][comp][ij];
    part[(((int64_t)blockIdx.y * 16 + c / 16) * gridDim.x + blockIdx.x) * 16 + c % 16] = s;
}

// X_q[row][NV] = sum_p sum_i Y_p[row][i] M[p NV + i][q NV + v] for every output block q < nb: M (ns x ns, row-major) is staged in
// LDS in panels of KPME_PANEL rows x NV columns; a workgroup takes 32 rows, a lane one (row, v); the rows of Y come from memory
// once and from the caches for the blocks q after the first.  X is not Y.
template <int NV>
__global__ __launch_bounds__(256) void k_kpm_rotate(const int nsta, const int nb, const cd* __restrict__ Y, const cd* __restrict__ M,
                                                    cd* __restrict__ X) {
    constexpr int RPB = 256 / NV;
    __shared__ cd panel[KPME_PANEL][NV];
    const int ns = nb * NV, v = threadIdx.x % NV, rl = threadIdx.x / NV;
    const int64_t ntiles = ((int64_t)nsta + RPB - 1) / RPB;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row = tile * RPB + rl;
        const bool live = row < nsta;
        for (int q = 0; q < nb; ++q) {
            cd acc{0.0, 0.0};
            for (int p0 = 0; p0 < ns; p0 += KPME_PANEL) {
                const int cnt = ns - p0 < KPME_PANEL ? ns - p0 : KPME_PANEL;
                __syncthreads();
                for (int r = rl; r < cnt; r += RPB) panel[r][v] = M[(int64_t)(p0 + r) * ns + q * NV + v];
                __syncthreads();
                if (live)
                    for (int r = 0; r < cnt; ++r) {
                        const int col = p0 + r;
                        cfma_x(acc, Y[((int64_t)(col / NV) * nsta + row) * NV + col % NV], panel[r][v]);
                    }
            }
            if (live) X[((int64_t)q * nsta + row) * NV + v] = acc;
        }
    }
}

// ------------------------------------------------------------------ host
namespace {
struct HostBuffers {
    std::vector<double> coef, gram, lam, theta, resid, tau, res_raw;
    std::vector<cd> G, A, U, wh, tmp, B, W, rot, coef_c;
    std::vector<int> sel;
};

int eigs_iterate(tbk_sparse* sp, const double* k, double e_lo, double e_hi, double emin, double emax, int ns, int degree, double tol,
                 int max_iter, uint64_t seed, int* n_found, double* eval, double* evec, double* resid_out, int32_t* info,
                 HostBuffers& hb) {
    constexpr int NV = KPM_NV, NC = 2 * NV;
    tbk_ctx* ctx = sp->ctx;
    const int n = sp->nsta, ncoef = degree + 1;
    const double a = 0.5 * (emax - emin), b = 0.5 * (emax + emin);
    KpmEigsWork w(sp, ns, degree);
    const int nb = w.nb, nwg = w.P.nwg;
    int rc = kpm_series_workspace("tbk_kpm_eigs", ctx, [&](KpmCarve& c) { w.carve(c); });
    if (rc) return rc;

    hb.coef.resize((size_t)ncoef);
    hb.coef_c.resize((size_t)ncoef);
    kpm_eigs_coefficients(e_lo, e_hi, emin, emax, degree, hb.coef.data());
    for (int m = 0; m < ncoef; ++m) hb.coef_c[(size_t)m] = cd{hb.coef[(size_t)m], 0.0};
    hb.gram.resize((size_t)w.npairs * 4 * NV * NV);
    hb.G.resize((size_t)ns * ns);
    hb.A.resize((size_t)ns * ns);
    hb.U.resize((size_t)ns * ns);
    hb.wh.resize((size_t)ns * ns);
    hb.tmp.resize((size_t)ns * ns);
    hb.B.resize((size_t)ns * ns);
    hb.W.resize((size_t)ns * ns);
    hb.rot.resize((size_t)ns * ns);
    hb.lam.resize((size_t)ns);
    hb.theta.assign((size_t)ns, 0.0);
    hb.resid.assign((size_t)ns, 0.0);
    hb.tau.resize((size_t)ns);
    hb.res_raw.resize((size_t)nb * NC);
    hb.sel.resize((size_t)ns);

    TBK_HIP(hipMemsetAsync(w.rec, 0, KPMS_GUARD * sizeof(double), ctx->stream));
    TBK_HIP(hipMemcpyAsync(w.coef, hb.coef_c.data(), (size_t)ncoef * sizeof(cd), hipMemcpyHostToDevice, ctx->stream));
    const cd* val = sp->amp;
    if (sp->dim_k > 0) {
        TBK_HIP(hipMemcpyAsync(w.k_dev, k, (size_t)sp->dim_k * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        rc = kpm_values_at(sp, w.k_dev, w.val);
        if (rc) return rc;
        val = w.val;
    }
    // the start vectors: random phases number 0 .. ns - 1 of the seed; the first load scales them by 1 / sqrt(nsta)
    const KpmStart start(sp, nullptr, 1, ns, nullptr, nullptr, seed);
    for (int blk = 0; blk < nb; ++blk) {
        rc = start.launch(ctx, nwg, 0, blk * NV, NV, w.X + (size_t)blk * w.block_len(), w.part);
        if (rc) return rc;
    }
    const KpmSeries S{ctx, sp, w.P, 1, ncoef, b, 1.0 / a, w.coef, w.cur, w.prev, w.part, w.dots, w.rec};
    const int64_t gtiles = ((int64_t)n + 256 / NV - 1) / (256 / NV);
    const unsigned rows_grid = (unsigned)std::min<int64_t>(gtiles, KPM_MAX_WG);
    double scale = 1.0 / sqrt((double)n);
    int rank = 0;
    for (int it = 1; it <= max_iter; ++it) {
        for (int blk = 0; blk < nb; ++blk) {        // Y = p(H~) X
            {
                ProfScope ps(ctx, "kpm_eigs_load");
                hipLaunchKernelGGL((k_kpm_eigs_load<NV>), dim3(nwg), dim3(256), 0, ctx->stream, n, scale,
                                   w.X + (size_t)blk * w.block_len(), w.cur, w.part);
                TBK_HIP(hipGetLastError());
            }
            rc = kpm_series_run(S, val, w.Y + (size_t)blk * w.block_len(), (double)((it - 1) * nb + blk));
            if (rc) return rc;
        }
        scale = 1.0;
        for (int blk = 0; blk < nb; ++blk) {        // H Y: the plain product, (b, 1 / a) = (0, 1)
            ProfScope ps(ctx, "kpm_eigs_hy");
            hipLaunchKernelGGL((k_kpm_step<NV, true, KpmNoSums>), dim3(nwg), dim3(256), 0, ctx->stream, n, sp->row_ptr, sp->col, val,
                               w.Y + (size_t)blk * w.block_len(), nullptr, w.HY + (size_t)blk * w.block_len(), 0.0, 1.0, KpmNoSums{});
            TBK_HIP(hipGetLastError());
        }
        for (int64_t pair0 = 0; pair0 < w.npairs; pair0 += w.pair_chunk) {       // G = Y^H Y, A = Y^H H Y
            const int cnt = (int)std::min<int64_t>(w.pair_chunk, w.npairs - pair0);
            {
                ProfScope ps(ctx, "kpm_eigs_gram");
                hipLaunchKernelGGL((k_kpm_gram<NV>), dim3(w.gram_wg, cnt), dim3(256), 0, ctx->stream, n, nb, pair0, w.Y, w.HY, w.gpart);
                TBK_HIP(hipGetLastError());
            }
            rc = kpm_reduce(ctx, w.gram_wg, cnt * 16, w.gpart, w.gram + (size_t)pair0 * 4 * NV * NV);
            if (rc) return rc;
        }
        double rec_host[KPMS_GUARD];
        TBK_HIP(hipMemcpyAsync(hb.gram.data(), w.gram, hb.gram.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        TBK_HIP(hipMemcpyAsync(rec_host, w.rec, sizeof(rec_host), hipMemcpyDeviceToHost, ctx->stream));
        if (it > 1)
            TBK_HIP(hipMemcpyAsync(hb.res_raw.data(), w.res, hb.res_raw.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        TBK_HIP(hipStreamSynchronize(ctx->stream));
        rc = kpm_series_verdict("tbk_kpm_eigs", rec_host, sp, emin, emax);
        if (rc) return rc;
        kpm_eigs_assemble(nb, hb.gram.data(), hb.G.data(), hb.A.data());
        info[0] = it;
        if (it > 1) {       // the stop test on the Ritz pairs of the previous iteration
            for (int j = 0; j < ns; ++j) {
                hb.tau[(size_t)j] = sqrt(hb.G[(size_t)j * ns + j].x);
                hb.resid[(size_t)j] = sqrt(hb.res_raw[(size_t)(j / NV) * NC + j % NV]);
            }
            const KpmEigsVerdict v = kpm_eigs_verdict(rank, hb.theta.data(), hb.resid.data(), hb.tau.data(), e_lo, e_hi, tol * a,
                                                      hb.sel.data());
            info[1] = rank;
            info[2] = v.nstrong;
            info[3] = v.nsel;
            if ((v.converged || it == max_iter) && !v.room) {
                tbk_set_error("tbk_kpm_eigs: the subspace is saturated: %d Ritz pairs have a filter norm tau >= 1/2, as many as it has "
                              "directions (%d) -- states of the window (%g, %g) may be missing: raise n_search (now %d)",
                              v.nstrong, rank, e_lo, e_hi, ns);
                return TBK_ENOCONV;
            }
            if (!v.converged && it == max_iter) {
                tbk_set_error("tbk_kpm_eigs: not converged after %d filter applications of degree %d: the worst residual of the %d "
                              "pairs in the window (%g, %g) is %.3e, above tol a = %.3e",
                              it, degree, v.nsel, e_lo, e_hi, v.worst, tol * a);
                return TBK_ENOCONV;
            }
            if (v.converged) {
                // the selected columns of X -> out[m][nsta]; Y is free now and holds the vector-major copy of X
                for (int blk = 0; blk < nb; ++blk) {
                    ProfScope ps(ctx, "kpm_series_gather");
                    hipLaunchKernelGGL((k_kpm_series_gather<NV>), dim3(rows_grid, 1), dim3(256), 0, ctx->stream, n, NV, (int64_t)0,
                                       w.X + (size_t)blk * w.block_len(), w.Y + (size_t)blk * w.block_len());
                    TBK_HIP(hipGetLastError());
                }
                for (int m = 0; m < v.nsel; ++m) {
                    const int j = hb.sel[(size_t)m];
                    eval[m] = hb.theta[(size_t)j];
                    if (resid_out) resid_out[m] = hb.resid[(size_t)j];
                    TBK_HIP(hipMemcpyAsync(evec + (size_t)m * n * 2, w.Y + (size_t)j * n, (size_t)n * sizeof(cd), hipMemcpyDeviceToHost,
                                           ctx->stream));
                }
                TBK_HIP(hipStreamSynchronize(ctx->stream));
                *n_found = v.nsel;
                return TBK_OK;
            }
        }
        // orthonormalise: eigh(G) on the device solver, the kept directions scaled by lam^-1/2
        TBK_HIP(hipMemcpyAsync(w.eig_h, hb.G.data(), (size_t)ns * ns * sizeof(cd), hipMemcpyHostToDevice, ctx->stream));
        rc = tbk_eigh_dev_checked(ctx, ns, w.eig_h, 1, w.eig_e, w.eig_v, "kpm_eigs_gram_eigh");
        if (rc) return rc;
        TBK_HIP(hipMemcpyAsync(hb.lam.data(), w.eig_e, (size_t)ns * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        TBK_HIP(hipMemcpyAsync(hb.U.data(), w.eig_v, (size_t)ns * ns * sizeof(cd), hipMemcpyDeviceToHost, ctx->stream));
        TBK_HIP(hipStreamSynchronize(ctx->stream));
        rank = kpm_eigs_whiten(ns, hb.lam.data(), hb.U.data(), hb.wh.data());
        if (rank == 0) {        // the filter leaves nothing of the start vectors: no state anywhere near the window
            info[1] = info[2] = info[3] = 0;
            *n_found = 0;
            return TBK_OK;
        }
        // Rayleigh-Ritz in the kept directions
        kpm_eigs_project(ns, rank, hb.A.data(), hb.wh.data(), hb.tmp.data(), hb.B.data());
        TBK_HIP(hipMemcpyAsync(w.eig_h, hb.B.data(), (size_t)rank * rank * sizeof(cd), hipMemcpyHostToDevice, ctx->stream));
        rc = tbk_eigh_dev_checked(ctx, rank, w.eig_h, 1, w.eig_e, w.eig_v, "kpm_eigs_ritz_eigh");
        if (rc) return rc;
        std::fill(hb.theta.begin(), hb.theta.end(), 0.0);
        TBK_HIP(hipMemcpyAsync(hb.theta.data(), w.eig_e, (size_t)rank * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        TBK_HIP(hipMemcpyAsync(hb.W.data(), w.eig_v, (size_t)rank * rank * sizeof(cd), hipMemcpyDeviceToHost, ctx->stream));
        TBK_HIP(hipStreamSynchronize(ctx->stream));
        kpm_eigs_rotation(ns, rank, hb.wh.data(), hb.W.data(), hb.rot.data());
        TBK_HIP(hipMemcpyAsync(w.rot, hb.rot.data(), (size_t)ns * ns * sizeof(cd), hipMemcpyHostToDevice, ctx->stream));
        TBK_HIP(hipMemcpyAsync(w.theta, hb.theta.data(), (size_t)ns * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        {       // X = Y (Wh W)
            ProfScope ps(ctx, "kpm_eigs_rotate");
            hipLaunchKernelGGL((k_kpm_rotate<NV>), dim3(rows_grid), dim3(256), 0, ctx->stream, n, nb, w.Y, w.rot, w.X);
            TBK_HIP(hipGetLastError());
        }
        for (int blk = 0; blk < nb; ++blk) {        // r_j^2 = |H x_j - theta_j x_j|^2; H X goes over H Y, which is spent
            {
                ProfScope ps(ctx, "kpm_eigs_resid");
                hipLaunchKernelGGL((k_kpm_step<NV, true, KpmResid>), dim3(nwg), dim3(256), 0, ctx->stream, n, sp->row_ptr, sp->col, val,
                                   w.X + (size_t)blk * w.block_len(), nullptr, w.HY + (size_t)blk * w.block_len(), 0.0, 1.0,
                                   KpmResid{w.theta + (size_t)blk * NV, w.part});
                TBK_HIP(hipGetLastError());
            }
            rc = kpm_reduce(ctx, nwg, 1, w.part, w.res + (size_t)blk * NC);
            if (rc) return rc;
        }
        // the host buffers of the two uploads are rewritten only after the next synchronisation
    }
    tbk_set_error("tbk_kpm_eigs: max_iter=%d", max_iter);      // not reached: the last iteration returns
    return TBK_EINVAL;
}
}  // namespace

extern "C" int tbk_kpm_eigs(tbk_sparse* sp, const double* k, double e_lo, double e_hi, double emin, double emax, int n_search, int degree,
                            double tol, int max_iter, uint64_t seed, int* n_found, double* eval, double* evec, double* resid,
                            int32_t* info) {
    int rc = kpm_eigs_check_args(sp, k, e_lo, e_hi, emin, emax, n_search, degree, tol, max_iter, n_found, eval, evec, info);
    if (rc) return rc;
    *n_found = 0;
    info[0] = info[1] = info[2] = info[3] = 0;
    tbk_ctx* ctx = sp->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    try {
        HostBuffers hb;
        rc = eigs_iterate(sp, k, e_lo, e_hi, emin, emax, n_search, degree, tol, max_iter, seed, n_found, eval, evec, resid, info, hb);
        if (rc) hipStreamSynchronize(ctx->stream);       // nothing of this call is in flight when its host buffers go
        return rc;
    } catch (const std::bad_alloc&) {
        hipStreamSynchronize(ctx->stream);
        tbk_set_error("tbk_kpm_eigs: out of host memory");
        return TBK_ENOMEM;
    }
}
