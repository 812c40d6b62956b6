// tbk_unfold.hip -- band unfolding: the eigenstates of a supercell projected on the Bloch sums of the primitive cell, per band and as
// the spectral function in the primitive zone.
//
// The call is made on the supercell model (n states).  The caller solves it at K = S k -- the same Cartesian vector as the primitive
// k, passed as given, not reduced modulo 1 -- and gives every state j its group g = group[j] (the primitive orbital, times spin, it is
// an image of; -1: none) and every orbital its displacement delta from the nearest lattice image of its ideal site, in primitive
// reduced coordinates.  With (E_b, u_b) the solver's eigenpairs at K and N_c the primitive cells per supercell:
//   W[b][g](k) = (1 / N_c) | sum_{j in g} e^{2 pi i k.delta_j} u_b[j] |^2
//   A[g](k, w) = sum_b W[b][g](k) (eta / pi) / ((w - E_b)^2 + eta^2) = -(1 / pi) Im <k,g| (w + i eta - H_sc)^-1 |k,g>
// and the totals over g.  delta = null: every displacement is 0 and no phase is formed.
//
// The k list goes through tbk_kubo.h's chunks (solve with eigenvectors); per chunk
//   k_unfold_phase    (delta only) ph[p][j] = e^{2 pi i k_p.delta_j}, a lane per (point, state): once per point, for all its bands
//   k_unfold_weights  workgroup (point p, tile of BT bands): the tile's components come into LDS through kubo_lds_load, coalesced, times
//                     ph on the way in (<true>; <false> is the copy without phases).  Lanes are BB bands x NGP group slots x L shares:
//                     share l of group g adds the members l, l + L, ... of the host's index list (ascending states) in that order, one
//                     lane adds the L shares in index order and squares; the total over g is added by one lane in group order.  States
//                     of group -1 are in no list: never read into a sum.
//   k_unfold_spectral<GT>  workgroup (point p, block of UNF_FB frequencies): a lane owns a frequency and GT accumulators; the bands go
//                     through LDS in strips of UNF_SB (E_b and W[b][0 .. GT), zero beyond ngo); the Lorentzian -- one division -- is
//                     formed once per (band, frequency) and feeds every group; bands in index order.  A lane beyond the last
//                     frequency works on a copy of the last one and stores nothing.
// No floating-point atomics; no partition depends on the values of k or omega, and no number of a point or a frequency on what stands
// beside it: two calls give the same bits, a frequency the same bits alone and inside a longer list, and a k-point too wherever the
// solver takes the same route for both list lengths (its method is a function of n and the points of a launch).
#include <math.h>
#include "tbk_unfold.h"

// ph[p][j] = e^{2 pi i k_p.delta_{orbital of j}}; pk is the chunk's part of the primitive k list
__global__ __launch_bounds__(256) void k_unfold_phase(const double* __restrict__ pk, const double* __restrict__ delta, const int64_t cnt,
                                                      const int n, const int nspin, const int dk, cd* __restrict__ ph) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= cnt * n) return;
    const int64_t p = e / n;
    const int o = (int)(e - p * n) / nspin;
    double x = 0.0;
    for (int d = 0; d < dk; ++d) x = fma(pk[p * dk + d], delta[o * dk + d], x);
    ph[e] = expi2pi(x);
}

template <bool PH>
__global__ __launch_bounds__(256) void k_unfold_weights(const cd* __restrict__ evec, const double* __restrict__ ev, const int64_t nk, const int n,
                                                        const int BT, const int ng, const int NGP, const int L,
                                                        const int32_t* __restrict__ goff, const int32_t* __restrict__ idx,
                                                        const cd* __restrict__ ph, const double inv_nc, const int per_state,
                                                        double* __restrict__ W, const int64_t sb, const int64_t sp,
                                                        double* __restrict__ ev_out, const int64_t ev_stride) {
    __shared__ cd U[kUnfLdsCd];
    __shared__ cd Pt[256];
    __shared__ double Wl[256];
    __shared__ int sidx[kUnfStatesMax];
    __shared__ int soff[kUnfGroupsMax + 1];
    const int t = threadIdx.x;
    const int64_t p = blockIdx.x;
    const int b0 = blockIdx.y * BT, nb = min(BT, n - b0);
    if (t <= ng) soff[t] = goff[t];
    const int nidx = goff[ng];
    for (int e = t; e < nidx; e += 256) sidx[e] = idx[e];
    kubo_lds_load(U, evec + (int64_t)b0 * nk * n, nk, p, 1, n, nb * n, [&](const int e) {
        if (PH) U[e] = cmul_x(U[e], ph[p * n + e % n]);
    });
    if (ev_out && t < nb) ev_out[(int64_t)(b0 + t) * ev_stride + p] = ev[(int64_t)(b0 + t) * nk + p];
    __syncthreads();
    const int per = NGP * L, BB = 256 / per;
    const int bb = t / per, r = t - bb * per, g = r / L, l = r - g * L;
    const int bb2 = t / NGP, g2 = t - bb2 * NGP;                  // (the lane that finishes band bb2, group g2)
    for (int b1 = 0; b1 < nb; b1 += BB) {
        cd s{0.0, 0.0};
        if (b1 + bb < nb && g < ng) {
            const cd* u = U + (b1 + bb) * n;
            for (int e = soff[g] + l; e < soff[g + 1]; e += L) s = cadd(s, u[sidx[e]]);
        }
        Pt[t] = s;
        __syncthreads();
        if (t < BB * NGP && b1 + bb2 < nb && g2 < ng) {
            const cd* q = Pt + t * L;                              // ((bb2 NGP + g2) L)
            cd a = q[0];
            for (int j = 1; j < L; ++j) a = cadd(a, q[j]);
            const double w = fma(a.x, a.x, a.y * a.y) * inv_nc;
            if (per_state)
                W[(int64_t)(b0 + b1 + bb2) * sb + p * sp + g2] = w;
            else
                Wl[t] = w;
        }
        if (!per_state) {                                          // (uniform over the launch)
            __syncthreads();
            if (t < BB && b1 + t < nb) {
                double tot = Wl[t * NGP];
                for (int j = 1; j < ng; ++j) tot += Wl[t * NGP + j];
                W[(int64_t)(b0 + b1 + t) * sb + p * sp] = tot;
            }
        }
        __syncthreads();                                           // (Pt and Wl are read)
    }
}

// A[p][w][g] = sum_b W[p][b][g] (eta / pi) / ((w - E_b[p])^2 + eta^2); Wc[cnt][n][ngo], ev[n][cnt], A[cnt][nw][ngo]
template <int GT>
__global__ __launch_bounds__(256) void k_unfold_spectral(const double* __restrict__ ev, const int64_t cnt, const int n, const int ngo,
                                                         const double* __restrict__ Wc, const double* __restrict__ omega, const int nw,
                                                         const double eta, double* __restrict__ A) {
    __shared__ double Es[UNF_SB];
    __shared__ double Ws[UNF_SB * GT];
    const int t = threadIdx.x;
    const int64_t p = blockIdx.x;
    const int w = blockIdx.y * UNF_FB + t;
    const double om = omega[min(w, nw - 1)];
    const double c = eta * 0.31830988618379067154, e2 = eta * eta;
    const double* Wp = Wc + p * n * ngo;
    double acc[GT];
#pragma unroll
    for (int g = 0; g < GT; ++g) acc[g] = 0.0;
    for (int b0 = 0; b0 < n; b0 += UNF_SB) {
        const int nb = min(UNF_SB, n - b0);
        __syncthreads();                                           // (the previous strip is consumed)
        if (t < nb) Es[t] = ev[(int64_t)(b0 + t) * cnt + p];
        for (int e = t; e < nb * GT; e += 256) {
            const int bb = e / GT, g = e - bb * GT;
            Ws[e] = g < ngo ? Wp[(int64_t)(b0 + bb) * ngo + g] : 0.0;
        }
        __syncthreads();
        for (int bb = 0; bb < nb; ++bb) {
            const double d = om - Es[bb];
            const double lor = c / fma(d, d, e2);                  // once per (band, frequency), for every group
#pragma unroll
            for (int g = 0; g < GT; ++g) acc[g] = fma(Ws[bb * GT + g], lor, acc[g]);
        }
    }
    if (w < nw) {
        double* a = A + (p * nw + w) * ngo;
#pragma unroll
        for (int g = 0; g < GT; ++g)
            if (g < ngo) a[g] = acc[g];
    }
}

// ---------------------------------------------------------------- host side
// nw = 0: the bands call (eval_out[n][nk], out[n][nk][ngo]); else the spectral call (out[nk][nw][ngo])
static int unf_run(const char* fn, tbk_model* m, const double* k_sc, int64_t nk, int ng, const int32_t* group, const double* phase_k,
                   const double* delta, double inv_nc, int per_state, int nw, const double* omega, double eta, double* eval_out, double* out) {
    TBK_REQUIRE(m && out && (nw || eval_out), TBK_EINVAL, "%s: null argument", fn);
    const int dk = m->dim_k, n = m->nsta;
    int rc = unf_check(fn, dk, n, m->norb, nk, k_sc, ng, group, phase_k, delta, inv_nc, per_state, nw, omega, eta);
    if (rc) return rc;
    const UnfGroups gt = unf_groups(n, ng, group);
    const bool phases = delta != nullptr;
    const UnfPlan pl = unf_plan(n, dk, m->norb, nk, ng, per_state, nw, phases, (int)gt.idx.size());
    tbk_ctx* ctx = m->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    void* base = nullptr;
    rc = tbk_ctx_scratch(ctx, pl.total, &base);
    if (rc) return rc;
    unsigned char* b = (unsigned char*)base;
    double* k_dev = (double*)(b + pl.off_k);
    double* pk_dev = (double*)(b + pl.off_pk);
    double* delta_dev = (double*)(b + pl.off_delta);
    double* om_dev = (double*)(b + pl.off_om);
    int32_t* goff_dev = (int32_t*)(b + pl.off_goff);
    int32_t* idx_dev = (int32_t*)(b + pl.off_idx);
    double* ev_dev = (double*)(b + pl.off_ev);
    double* out_dev = (double*)(b + pl.off_out);
    KuboChunks cw = pl.cw;
    cw.base = b + pl.off_chunks;
    const size_t D = sizeof(double);
    TBK_HIP(hipMemcpyAsync(k_dev, k_sc, (size_t)nk * dk * D, hipMemcpyHostToDevice, ctx->stream));
    if (phases) {
        TBK_HIP(hipMemcpyAsync(pk_dev, phase_k, (size_t)nk * dk * D, hipMemcpyHostToDevice, ctx->stream));
        TBK_HIP(hipMemcpyAsync(delta_dev, delta, (size_t)m->norb * dk * D, hipMemcpyHostToDevice, ctx->stream));
    }
    if (nw) TBK_HIP(hipMemcpyAsync(om_dev, omega, (size_t)nw * D, hipMemcpyHostToDevice, ctx->stream));
    TBK_HIP(hipMemcpyAsync(goff_dev, gt.off.data(), gt.off.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    TBK_HIP(hipMemcpyAsync(idx_dev, gt.idx.data(), gt.idx.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));                     // (the host arrays may be the caller's temporaries)
    const int ngo = pl.ngo;
    rc = kubo_for_chunks(m, cw, k_dev, nullptr, nk, [&](int64_t first, int64_t cnt, const double*, const double* ec, const cd* vc) -> int {
        cd* ph = cw.extra<cd>(0);
        if (phases) {
            ProfScope ps(ctx, "unfold_phase");
            hipLaunchKernelGGL(k_unfold_phase, dim3(nblk(cnt * n)), dim3(256), 0, ctx->stream, (const double*)(pk_dev + first * dk),
                               (const double*)delta_dev, cnt, n, m->nspin, dk, ph);
            TBK_HIP(hipGetLastError());
        }
        double* W = nw ? cw.extra<double>(1) : out_dev + first * ngo;
        const int64_t sb = nw ? (int64_t)ngo : nk * ngo, sp = nw ? (int64_t)n * ngo : (int64_t)ngo;
        double* evo = nw ? nullptr : ev_dev + first;
        {
            ProfScope ps(ctx, "unfold_weights");
            const dim3 grid((unsigned)cnt, (unsigned)pl.ntile);
            if (phases)
                hipLaunchKernelGGL(k_unfold_weights<true>, grid, dim3(256), 0, ctx->stream, vc, ec, cnt, n, pl.BT, ng, pl.NGP, pl.L,
                                   (const int32_t*)goff_dev, (const int32_t*)idx_dev, (const cd*)ph, inv_nc, per_state, W, sb, sp, evo, nk);
            else
                hipLaunchKernelGGL(k_unfold_weights<false>, grid, dim3(256), 0, ctx->stream, vc, ec, cnt, n, pl.BT, ng, pl.NGP, pl.L,
                                   (const int32_t*)goff_dev, (const int32_t*)idx_dev, (const cd*)nullptr, inv_nc, per_state, W, sb, sp, evo, nk);
            TBK_HIP(hipGetLastError());
        }
        if (!nw) return TBK_OK;
        ProfScope ps(ctx, "unfold_spectral");
        const dim3 grid((unsigned)cnt, (unsigned)pl.nwb);
        double* A = out_dev + first * nw * ngo;
        switch (pl.GT) {
            case 1:
                hipLaunchKernelGGL(k_unfold_spectral<1>, grid, dim3(256), 0, ctx->stream, ec, cnt, n, ngo, (const double*)W, (const double*)om_dev, nw, eta, A);
                break;
            case 4:
                hipLaunchKernelGGL(k_unfold_spectral<4>, grid, dim3(256), 0, ctx->stream, ec, cnt, n, ngo, (const double*)W, (const double*)om_dev, nw, eta, A);
                break;
            case 16:
                hipLaunchKernelGGL(k_unfold_spectral<16>, grid, dim3(256), 0, ctx->stream, ec, cnt, n, ngo, (const double*)W, (const double*)om_dev, nw, eta, A);
                break;
            default:
                hipLaunchKernelGGL(k_unfold_spectral<64>, grid, dim3(256), 0, ctx->stream, ec, cnt, n, ngo, (const double*)W, (const double*)om_dev, nw, eta, A);
        }
        TBK_HIP(hipGetLastError());
        return TBK_OK;
    });
    if (rc) return rc;
    if (!nw) TBK_HIP(hipMemcpyAsync(eval_out, ev_dev, (size_t)n * nk * D, hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipMemcpyAsync(out, out_dev, (size_t)pl.out_d * D, hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    return TBK_OK;
}

extern "C" int tbk_unfold_bands_list(tbk_model* m, const double* k_sc, int64_t nk, int ng, const int32_t* group, const double* phase_k,
                                     const double* delta, double inv_nc, int per_state, double* eval_out, double* w_out) {
    return unf_run("tbk_unfold_bands_list", m, k_sc, nk, ng, group, phase_k, delta, inv_nc, per_state, 0, nullptr, 0.0, eval_out, w_out);
}

extern "C" int tbk_unfold_spectral_list(tbk_model* m, const double* k_sc, int64_t nk, int ng, const int32_t* group, const double* phase_k,
                                        const double* delta, double inv_nc, int nomega, const double* omega, double eta, int per_state,
                                        double* out) {
    TBK_REQUIRE(nomega >= 1, TBK_EINVAL, "tbk_unfold_spectral_list: nomega=%d (1..%d frequencies)", nomega, kKuboOmegaMax);
    return unf_run("tbk_unfold_spectral_list", m, k_sc, nk, ng, group, phase_k, delta, inv_nc, per_state, nomega, omega, eta, nullptr, out);
}
