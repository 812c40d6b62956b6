// tbk_mf_dev.h -- what the self-consistency drivers share on the device side (DESIGN.md sections 33, 36 and 38): the kernels of
// tbk_mf.hip that write H[x] into a private model's tables, gather x_out and mix, the iteration loop with its check cadence, and the
// frame of a driver around its own passes: the private model and workspace, the launches of k_mf_apply and k_mf_mix, the closing scan
// with the downloads, and the double-counting sum.  The kernels are defined once, in tbk_mf.hip; tbk_bdg.hip launches the same code.
#pragma once
#include <cmath>
#include "tbk_mf.h"
#include "tbk_occ_dev.h"

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
// occupation row of the iteration from acc[n][n]
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

// ---------------------------------------------------------------- the driver frame
// What a driver owns for the length of one call: the private model (every field entry pinned; never the caller's cached handle) and
// the private workspace, released behind a synchronisation of the stream.
struct MfFrame {
    tbk_ctx* ctx = nullptr;
    tbk_model* m = nullptr;
    unsigned char* base = nullptr;
    size_t total = 0, k_all = 0;         // from the plan callback, with L: the block's size and where its k points sit
    MfLoopBufs L;
    MfMap map;                           // the term -> parameter map on the host, from mf_frame_open until mf_frame_start releases it
    int nft = 0;
    int64_t np = 0;
    cd *amp = nullptr, *rblock = nullptr;
    template <class T>
    T* lp(int i) const { return (T*)(base + L.off[i]); }
    MfFrame() = default;
    MfFrame(const MfFrame&) = delete;
    ~MfFrame() {
        if (base) {
            hipStreamSynchronize(ctx->stream);
            hipFree(base);
        }
        if (m) tbk_model_free(m);
    }
};

// Setup, in three steps between which a driver uploads into its own buffers (the order of the copies on the stream is each
// driver's own and stays as it was).  First: the private model of the given tables with the pins of P, the term -> parameter map of
// P.field over it, the driver's plan (plan(F, nft, nnz) lays the workspace out and sets F.L, F.total, F.k_all) and the block.
template <class Plan>
static int mf_frame_open(MfFrame& F, tbk_ctx* ctx, const char* fn, int dim_k, int norb, int nspin, const double* orb, const double* onsite,
                         int64_t nhop, const int32_t* hop_i, const int32_t* hop_j, const int32_t* hop_R, const double* hop_amp,
                         const MfProblem& P, int64_t np, Plan&& plan) {
    F.ctx = ctx, F.np = np;
    TbkFlatTerms T;
    int rc = tbk_model_upload_pinned(ctx, dim_k, norb, nspin, orb, onsite, nhop, hop_i, hop_j, hop_R, hop_amp, (int64_t)P.pin.size() / 6,
                                     P.pin.data(), &F.m, &T);
    if (rc) return rc;
    std::vector<double> amp2((size_t)T.nterm * 2);
    for (int64_t t = 0; t < T.nterm; ++t) amp2[2 * t] = T.amp[t].x, amp2[2 * t + 1] = T.amp[t].y;
    rc = mf_map(fn, P, T.nslot, T.slot_ptr, T.R4, amp2, T.nR, T.rvec, F.map);
    if (rc) return rc;
    F.nft = (int)F.map.term.size();
    plan(F, (int64_t)F.map.term.size(), (int64_t)F.map.coef.size());
    void* blk = nullptr;
    hipError_t e = hipMalloc(&blk, F.total);
    if (e != hipSuccess) {
        tbk_set_error("%s: hipMalloc(%zu) for the workspace: %s", fn, F.total, hipGetErrorString(e));
        return TBK_ENOMEM;
    }
    F.base = (unsigned char*)blk;
    F.amp = (cd*)((unsigned char*)F.m->blob + T.o_amp);
    F.rblock = (cd*)((unsigned char*)F.m->blob + T.o_rblk);
    return TBK_OK;
}
// Second: the uploads of gidx, the map and (where given) the start vector.
static int mf_frame_upload(const MfFrame& F, const std::vector<int64_t>& gidx, const double* x_start) {
    const MfMap& map = F.map;
    int rc;
    auto up = [&](int i, const void* src, size_t bytes) -> int {
        if (bytes) TBK_HIP(hipMemcpyAsync(F.base + F.L.off[i], src, bytes, hipMemcpyHostToDevice, F.ctx->stream));
        return TBK_OK;
    };
    if ((rc = up(MfLoopBufs::GIDX, gidx.data(), gidx.size() * sizeof(int64_t)))) return rc;
    if ((rc = up(MfLoopBufs::TBASE, map.base.data(), map.base.size() * sizeof(double)))) return rc;
    if ((rc = up(MfLoopBufs::TPTR, map.ptr.data(), map.ptr.size() * sizeof(int32_t)))) return rc;
    if ((rc = up(MfLoopBufs::TTERM, map.term.data(), map.term.size() * sizeof(int32_t)))) return rc;
    if ((rc = up(MfLoopBufs::TRBLK, map.rblk.data(), map.rblk.size() * sizeof(int64_t)))) return rc;
    if ((rc = up(MfLoopBufs::CCOEF, map.coef.data(), map.coef.size() * sizeof(double)))) return rc;
    if ((rc = up(MfLoopBufs::CPAR, map.par.data(), map.par.size() * sizeof(int32_t)))) return rc;
    if ((rc = up(MfLoopBufs::CPART, map.part.data(), map.part.size() * sizeof(int32_t)))) return rc;
    if (x_start && (rc = up(MfLoopBufs::XIN, x_start, (size_t)F.np * sizeof(double)))) return rc;
    return TBK_OK;
}
// Third: the zeroed Gram matrix (and `zero_bytes` at `zero`, where a driver wants a region of its own zeroed), the synchronisation
// behind which the host vectors go out of use (the map is released), and the k points.
static int mf_frame_start(MfFrame& F, int dim_k, const int32_t* mesh, void* zero = nullptr, size_t zero_bytes = 0) {
    hipStream_t st = F.ctx->stream;
    TBK_HIP(hipMemsetAsync(F.lp<double>(MfLoopBufs::SMALL), 0, 1024, st));
    if (zero) TBK_HIP(hipMemsetAsync(zero, 0, zero_bytes, st));
    TBK_HIP(hipStreamSynchronize(st));
    F.map = MfMap();
    return tbk_k_uniform_mesh_dev(F.ctx, dim_k, mesh, (double*)(F.base + F.k_all));
}

// H[x_in] into the tables of the private model, under the driver's profiling bracket
static int mf_launch_apply(const MfFrame& F, const char* scope) {
    if (F.nft <= 0) return TBK_OK;
    ProfScope ps(F.ctx, scope);
    hipLaunchKernelGGL(k_mf_apply, dim3(nblk(F.nft)), dim3(256), 0, F.ctx->stream, F.nft, (const int32_t*)F.lp<int32_t>(MfLoopBufs::TPTR),
                       (const int32_t*)F.lp<int32_t>(MfLoopBufs::TTERM), (const int64_t*)F.lp<int64_t>(MfLoopBufs::TRBLK),
                       (const double*)F.lp<double>(MfLoopBufs::TBASE), (const double*)F.lp<double>(MfLoopBufs::CCOEF),
                       (const int32_t*)F.lp<int32_t>(MfLoopBufs::CPAR), (const int32_t*)F.lp<int32_t>(MfLoopBufs::CPART),
                       (const double*)F.lp<double>(MfLoopBufs::XIN), F.amp, F.rblock);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}
// The mixing step of iteration `it`.  n: the states whose occupations k_mf_mix writes into the iteration's history row, read from the
// diagonal of acc[n][n]; n = 0: it writes none (a driver whose acc is no such matrix writes the row itself: k_bdg_mu).
static int mf_launch_mix(const MfFrame& F, const char* scope, int it, int history, double mixing, int n, double nk, const cd* acc) {
    ProfScope ps(F.ctx, scope);
    hipLaunchKernelGGL(k_mf_mix, dim3(1), dim3(256), 0, F.ctx->stream, F.np, it, history, mixing, n, nk, (const double*)acc,
                       F.lp<double>(MfLoopBufs::XIN), (const double*)F.lp<double>(MfLoopBufs::XOUT), F.lp<double>(MfLoopBufs::XPREV),
                       F.lp<double>(MfLoopBufs::RINGX), F.lp<double>(MfLoopBufs::RINGR), F.lp<double>(MfLoopBufs::SMALL),
                       F.lp<double>(MfLoopBufs::RESH), F.lp<double>(MfLoopBufs::OCCH));
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

// Closing.  Once, from the last iteration's own levels: N, sum f E and S by the thermal scan of section 27 at the level in
// level_dev[0], into spart[3 G] and the three sums behind it (returned in *srows; on the device: the driver copies them).
static int mf_frame_scan(const MfFrame& F, const char* scope, const double* lev, int64_t nlev, int G, const double* level_dev, double kT,
                         double* spart, double** srows) {
    *srows = spart + (size_t)3 * G;
    {
        ProfScope ps(F.ctx, scope);
        hipLaunchKernelGGL(k_occ_scan, dim3(1, (unsigned)G), dim3(256), 0, F.ctx->stream, lev, nlev, G, level_dev, 1, kT, spart);
        TBK_HIP(hipGetLastError());
    }
    return kubo_rows_launch(F.ctx, spart, G, 3, *srows);
}
// The copies to the host of x_in (the vector the last iteration solved in) and x_out, and of the two histories (occ_cols occupations
// per iteration): two calls, since mean field copies its density between them.  Nothing is synchronised: the driver does that
// behind its own copies.
static int mf_frame_download_x(const MfFrame& F, double* x_in, double* x_out) {
    hipStream_t st = F.ctx->stream;
    TBK_HIP(hipMemcpyAsync(x_in, F.lp<double>(MfLoopBufs::XPREV), (size_t)F.np * sizeof(double), hipMemcpyDeviceToHost, st));
    TBK_HIP(hipMemcpyAsync(x_out, F.lp<double>(MfLoopBufs::XOUT), (size_t)F.np * sizeof(double), hipMemcpyDeviceToHost, st));
    return TBK_OK;
}
static int mf_frame_download_hist(const MfFrame& F, int iterations, int occ_cols, double* res_hist, double* occ_hist) {
    hipStream_t st = F.ctx->stream;
    TBK_HIP(hipMemcpyAsync(res_hist, F.lp<double>(MfLoopBufs::RESH), (size_t)iterations * sizeof(double), hipMemcpyDeviceToHost, st));
    TBK_HIP(hipMemcpyAsync(occ_hist, F.lp<double>(MfLoopBufs::OCCH), (size_t)iterations * occ_cols * sizeof(double), hipMemcpyDeviceToHost, st));
    return TBK_OK;
}

// The double counting of the state of the last iteration (density x_out in the field of x_in), every bracket with its channel:
//   E_dc = sum_e V [n_a^in n_b^out + n_b^in n_a^out - n_a^out n_b^out                  (hartree)
//                   - 2 Re(conj(D^in) D^out) + |D^out|^2                                (par_d >= 0: the first parameter of the D block)
//                   + 2 Re(conj(F^in) F^out) - |F^out|^2]                               (par_f >= 0: that of the F block)
static double mf_edc(int nint, const int32_t* ab, const double* V, const std::vector<int>& occ_par, bool hartree, int par_d, int par_f,
                     const double* x_in, const double* x_out) {
    double edc = 0.0;
    for (int e = 0; e < nint; ++e) {
        const int pa = occ_par[ab[2 * e]], pb = occ_par[ab[2 * e + 1]];
        double t = 0.0;
        if (hartree) t += x_in[pa] * x_out[pb] + x_in[pb] * x_out[pa] - x_out[pa] * x_out[pb];
        if (par_d >= 0) {
            const int pr = par_d + 2 * e, pi = pr + 1;
            t += -2.0 * (x_in[pr] * x_out[pr] + x_in[pi] * x_out[pi]) + x_out[pr] * x_out[pr] + x_out[pi] * x_out[pi];
        }
        if (par_f >= 0) {
            const int pr = par_f + 2 * e, pi = pr + 1;
            t += 2.0 * (x_in[pr] * x_out[pr] + x_in[pi] * x_out[pi]) - x_out[pr] * x_out[pr] - x_out[pi] * x_out[pi];
        }
        edc += V[e] * t;
    }
    return edc;
}
