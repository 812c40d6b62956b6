// tbk_mf_dev.h -- what the self-consistency drivers share on the device side (DESIGN.md sections 33 and 36): the kernels of tbk_mf.hip
// that write H[x] into a private model's tables, gather x_out and mix, and the iteration loop with its check cadence.  The kernels are
// defined once, in tbk_mf.hip; tbk_bdg.hip launches the same code.
#pragma once
#include <cmath>
#include "tbk_mf.h"

// term_amp[t] = base[t] + sum_p c_{t,p} x_p for every term that carries a field, one lane per term (the CSR map of tbk_mf.h)
__global__ __launch_bounds__(256) void k_mf_apply(const int nft, const int32_t* __restrict__ tptr, const int32_t* __restrict__ tterm,
                                                  const int64_t* __restrict__ trblk, const double* __restrict__ tbase,
                                                  const double* __restrict__ ccoef, const int32_t* __restrict__ cpar,
                                                  const int32_t* __restrict__ cpart, const double* __restrict__ x, cd* __restrict__ amp,
                                                  cd* __restrict__ rblock);
// x_out[p] = acc[gidx[p]] / N_k
__global__ __launch_bounds__(256) void k_mf_gather(const int64_t np, const int64_t* __restrict__ gidx, const double* __restrict__ acc,
                                                   const double nk, double* __restrict__ xout);
__global__ __launch_bounds__(256) void k_mf_copy(const int64_t np, const double* __restrict__ src, double* __restrict__ dst);
// ONE workgroup: the residual into the ring, max |r| and the Gram row by fixed-order sums, the Anderson solve, the next x_in; the
// occupation row of the iteration from acc[n][n] (n = 0: none is written)
__global__ __launch_bounds__(256) void k_mf_mix(const int64_t np, const int it, const int m, const double alpha, const int n, const double nk,
                                                const double* __restrict__ acc, double* __restrict__ xin, const double* __restrict__ xout,
                                                double* __restrict__ xprev, double* __restrict__ ringx, double* __restrict__ ringr,
                                                double* __restrict__ gram, double* __restrict__ res_hist, double* __restrict__ occ_hist);

// The loop: pass() takes x_in to x_out, mix(it) mixes and leaves the residual of iteration `it` in resh_dev[it]; both only launch.  At a
// convergence check (every check_every iterations, and at the last) the host reads that residual by a plain 8-byte copy behind a
// stream synchronisation, and the solver's status words with it.
template <class Pass, class Mix>
static int mf_iterate(tbk_ctx* ctx, const char* fn, int nsta, int max_iter, int check_every, double tol, const double* resh_dev, Pass&& pass,
                      Mix&& mix, int* iterations, int* converged) {
    *iterations = 0;
    *converged = 0;
    int rc;
    for (int it = 0; it < max_iter; ++it) {
        if ((rc = pass())) return rc;
        if ((rc = mix(it))) return rc;
        *iterations = it + 1;
        if ((it + 1) % check_every != 0 && it + 1 != max_iter) continue;
        double res = 0.0;                                           // the check: one 8-byte copy behind a synchronisation
        TBK_HIP(hipMemcpyAsync(&res, resh_dev + it, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        TBK_HIP(hipStreamSynchronize(ctx->stream));
        if ((rc = tbk_eigh_check(ctx, nsta))) return rc;
        TBK_REQUIRE(std::isfinite(res), TBK_ENOCONV, "%s: the residual of iteration %d is not finite", fn, it + 1);
        if (tol > 0.0 && res <= tol) {
            *converged = 1;
            break;
        }
    }
    return TBK_OK;
}
