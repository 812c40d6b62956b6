// tbk_kpm_series.hip -- kernel polynomial method: a function of the sparse H(k) applied to vectors, and the local Chern marker
// (DESIGN.md section 23).
//
//   f(H) v = sum_{m < ncoef} c_m T_m(H~) v,   H~ = (H(k) - b) / a,
//
// on the sparse operator of tbk_kpm.hip.  tbk_kpm_moments and tbk_kpm_double_moments return traces; here the vector itself comes
// back: with the Chebyshev coefficients of a step f(H) is the Fermi projector, with (2 - delta_m0) (-i)^m J_m(a t) e^{-i b t} the
// time evolution e^{-i H t}.  No reference counterpart (PythTB 1.8 has no sparse operator); Weisse, Wellein, Alvermann, Fehske,
// Rev. Mod. Phys. 78, 275; the marker: Bianco, Resta, Phys. Rev. B 84, 241106.
//
// Per block of NV = 8 start vectors: the recursion of k_kpm_step, nw = 2 H~ cur - prev over prev, and in the same pass, for every
// coefficient set s in ascending order, acc[s][row][NV] += c[s][j] nw.  The launch of j = 1 writes acc = c[s][0] v + c[s][1] H~ v:
// nothing is zeroed first.  Every step also leaves the row-local sums of <nw|nw> (kpm_block_sums, k_kpm_reduce): inside the bounds
// ||T_j(H~) v|| <= ||v||, so a norm beyond that -- or not finite -- says that the bounds do not contain the spectrum.  One plain
// launch per step on the context's stream, one host synchronisation per call; no floating-point atomics, no grid barrier, no
// persistent kernel: two calls give the same bits.  The series itself (its epilogue, guard and gather kernels, kpm_series_run)
// lives in tbk_kpm.h: tbk_kpm_eigs.hip filters with it.
#include <math.h>
#include <algorithm>
#include <cmath>
#include <new>
#include <vector>
#include "tbk_kpm.h"

// ------------------------------------------------------------------ kernels
// cur[row][NV] = d[row] in[row][NV] (a real diagonal operator) and the partial sums of <cur|cur>: the start of a series from a
// device buffer.
template <int NV>
__global__ __launch_bounds__(256) void k_kpm_series_scale(const int nsta, const double* __restrict__ d, const cd* __restrict__ in,
                                                          cd* __restrict__ cur, double* __restrict__ part) {
    double dA = 0.0;
    kpm_for_rows<NV>(nsta, [&](const int64_t row, const int v) {
        const cd x = cscale(in[row * NV + v], d[row]);
        cur[row * NV + v] = x;
        dA += cabs2(x);
    });
    kpm_block_sums<NV>(dA, 0.0, part);
}

// part[workgroup][2][NV] = the row-local sums of (Re, Im) conj(x[row][v]) d[row] y[row][v]
template <int NV>
__global__ __launch_bounds__(256) void k_kpm_series_dot(const int nsta, const double* __restrict__ d, const cd* __restrict__ x,
                                                        const cd* __restrict__ y, double* __restrict__ part) {
    double dA = 0.0, dB = 0.0;
    kpm_for_rows<NV>(nsta, [&](const int64_t row, const int v) {
        const cd z = cscale(cmulc(x[row * NV + v], y[row * NV + v]), d[row]);
        dA += z.x;
        dB += z.y;
    });
    kpm_block_sums<NV>(dA, dB, part);
}

// ------------------------------------------------------------------ host
extern "C" int tbk_kpm_apply_series(tbk_sparse* sp, const double* k, int64_t nk, int ncoef, int nset, const double* coeffs, double emin,
                                    double emax, int nvec, const double* vectors, const int32_t* states, uint64_t seed, double* out) {
    constexpr int NV = KPM_NV, NC = 2 * NV;
    TBK_REQUIRE(sp && coeffs && out, TBK_EINVAL, "tbk_kpm_apply_series: null argument");
    TBK_REQUIRE(nset >= 1, TBK_EINVAL, "tbk_kpm_apply_series: nset=%d", nset);
    int rc = kpm_check_args("tbk_kpm_apply_series", sp, "ncoef", ncoef, nvec, vectors, states, emin, emax, k, &nk);
    if (rc) return rc;
    if (nk == 0) return TBK_OK;
    const int dim_k = sp->dim_k, n = sp->nsta;
    tbk_ctx* ctx = sp->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    const double a = 0.5 * (emax - emin), b = 0.5 * (emax + emin);
    const KpmPlan P = kpm_plan(n, ncoef - 1);
    const size_t nout = (size_t)nk * nset * nvec * n;
    KpmStart start(sp, k, nk, nvec, vectors, states, seed);
    cd *val_dev, *cur, *prev, *acc, *out_dev, *coef_dev;
    double *part, *dots, *rec;
    rc = kpm_series_workspace("tbk_kpm_apply_series", ctx, [&](KpmCarve& c) {
        c.take(val_dev, dim_k > 0 ? (size_t)sp->nnz : 0);
        c.take(cur, (size_t)n * NV);
        c.take(prev, (size_t)n * NV);
        c.take(acc, (size_t)nset * n * NV);
        c.take(part, P.part_len());
        c.take(dots, (size_t)ncoef * NC);
        c.take(rec, (size_t)KPMS_GUARD);
        c.take(out_dev, nout);
        c.take(coef_dev, (size_t)nset * ncoef);
        start.carve(c);
    });
    if (rc) return rc;
    TBK_HIP(hipMemsetAsync(rec, 0, KPMS_GUARD * sizeof(double), ctx->stream));
    TBK_HIP(hipMemcpyAsync(coef_dev, coeffs, (size_t)nset * ncoef * sizeof(cd), hipMemcpyHostToDevice, ctx->stream));
    rc = start.upload(ctx);
    if (rc) return rc;
    const KpmSeries S{ctx, sp, P, nset, ncoef, b, 1.0 / a, coef_dev, cur, prev, part, dots, rec};
    const int64_t gtiles = ((int64_t)n + 256 / NV - 1) / (256 / NV);
    for (int64_t q = 0; q < nk; ++q) {
        const cd* val = sp->amp;
        if (dim_k > 0) {
            rc = kpm_values_at(sp, start.k_at(q), val_dev);
            if (rc) return rc;
            val = val_dev;
        }
        for (int v0 = 0; v0 < nvec; v0 += NV) {
            const int nv = std::min(NV, nvec - v0);
            rc = start.launch(ctx, P.nwg, q, v0, nv, cur, part);
            if (rc) return rc;
            rc = kpm_series_run(S, val, acc, (double)q);
            if (rc) return rc;
            ProfScope ps(ctx, "kpm_series_gather");
            hipLaunchKernelGGL((k_kpm_series_gather<NV>), dim3((unsigned)std::min<int64_t>(gtiles, KPM_MAX_WG), nset), dim3(256), 0,
                               ctx->stream, n, nv, (int64_t)nvec * n, acc, out_dev + ((size_t)q * nset * nvec + v0) * n);
            TBK_HIP(hipGetLastError());
        }
    }
    double rec_host[KPMS_GUARD];
    TBK_HIP(hipMemcpyAsync(out, out_dev, nout * sizeof(cd), hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipMemcpyAsync(rec_host, rec, sizeof(rec_host), hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    // divergence guard: |T_m(x)| <= 1 only inside [-1, 1]; outside, the recursion grows without limit (a floating-point outcome)
    return kpm_series_verdict("tbk_kpm_apply_series", rec_host, sp, emin, emax);
}

extern "C" int tbk_kpm_marker(tbk_sparse* sp, int ncoef, const double* coeffs, double emin, double emax, const double* da,
                              const double* db, int nvec, const int32_t* states, double* out) {
    constexpr int NV = KPM_NV, NC = 2 * NV;
    TBK_REQUIRE(sp && coeffs && da && db && states && out, TBK_EINVAL, "tbk_kpm_marker: null argument");
    TBK_REQUIRE(sp->dim_k == 0, TBK_EINVAL, "tbk_kpm_marker: the position operator needs an open sample (dim_k = %d, not 0)", sp->dim_k);
    int64_t nk = 1;
    int rc = kpm_check_args("tbk_kpm_marker", sp, "ncoef", ncoef, nvec, nullptr, states, emin, emax, nullptr, &nk);
    if (rc) return rc;
    const int n = sp->nsta;
    std::vector<cd> coef_host;
    try {
        coef_host.resize((size_t)ncoef);
    } catch (const std::bad_alloc&) {
        tbk_set_error("tbk_kpm_marker: out of host memory");
        return TBK_ENOMEM;
    }
    for (int m = 0; m < ncoef; ++m) coef_host[(size_t)m] = cd{coeffs[m], 0.0};
    tbk_ctx* ctx = sp->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    const double a = 0.5 * (emax - emin), b = 0.5 * (emax + emin);
    const KpmPlan P = kpm_plan(n, ncoef - 1);
    const int nwg = P.nwg, nblk = (nvec + NV - 1) / NV;
    KpmStart start(sp, nullptr, 0, nvec, nullptr, states, 0);     // the unit vectors s
    cd *cur, *prev, *w1, *w3, *coef_dev;
    double *part, *dots, *rec, *res, *da_dev, *db_dev;
    rc = kpm_series_workspace("tbk_kpm_marker", ctx, [&](KpmCarve& c) {
        c.take(cur, (size_t)n * NV);
        c.take(prev, (size_t)n * NV);
        c.take(w1, (size_t)n * NV);
        c.take(w3, (size_t)n * NV);
        c.take(part, P.part_len());
        c.take(dots, (size_t)ncoef * NC);
        c.take(rec, (size_t)KPMS_GUARD);
        c.take(res, (size_t)nblk * NC);
        c.take(coef_dev, (size_t)ncoef);
        c.take(da_dev, (size_t)n);
        c.take(db_dev, (size_t)n);
        start.carve(c);
    });
    if (rc) return rc;
    TBK_HIP(hipMemsetAsync(rec, 0, KPMS_GUARD * sizeof(double), ctx->stream));
    TBK_HIP(hipMemcpyAsync(coef_dev, coef_host.data(), (size_t)ncoef * sizeof(cd), hipMemcpyHostToDevice, ctx->stream));
    TBK_HIP(hipMemcpyAsync(da_dev, da, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    TBK_HIP(hipMemcpyAsync(db_dev, db, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    rc = start.upload(ctx);
    if (rc) return rc;
    const KpmSeries S{ctx, sp, P, 1, ncoef, b, 1.0 / a, coef_dev, cur, prev, part, dots, rec};
    for (int blk = 0; blk < nblk; ++blk) {
        const int v0 = blk * NV, nv = std::min(NV, nvec - v0);
        rc = start.launch(ctx, nwg, 0, v0, nv, cur, part);
        if (rc) return rc;
        rc = kpm_series_run(S, sp->amp, w1, (double)blk);      // w1 = F s
        if (rc) return rc;
        {   // u = B w1
            ProfScope ps(ctx, "kpm_series_scale");
            hipLaunchKernelGGL((k_kpm_series_scale<NV>), dim3(nwg), dim3(256), 0, ctx->stream, n, db_dev, w1, cur, part);
            TBK_HIP(hipGetLastError());
        }
        rc = kpm_series_run(S, sp->amp, w3, (double)blk);      // w3 = F u
        if (rc) return rc;
        {   // <w1| A |w3>
            ProfScope ps(ctx, "kpm_series_dot");
            hipLaunchKernelGGL((k_kpm_series_dot<NV>), dim3(nwg), dim3(256), 0, ctx->stream, n, da_dev, w1, w3, part);
            TBK_HIP(hipGetLastError());
        }
        rc = kpm_reduce(ctx, nwg, 1, part, res + (size_t)blk * NC);
        if (rc) return rc;
    }
    std::vector<double> res_host;
    try {
        res_host.resize((size_t)nblk * NC);
    } catch (const std::bad_alloc&) {
        hipStreamSynchronize(ctx->stream);
        tbk_set_error("tbk_kpm_marker: out of host memory");
        return TBK_ENOMEM;
    }
    double rec_host[KPMS_GUARD];
    TBK_HIP(hipMemcpyAsync(res_host.data(), res, res_host.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipMemcpyAsync(rec_host, rec, sizeof(rec_host), hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    rc = kpm_series_verdict("tbk_kpm_marker", rec_host, sp, emin, emax);
    if (rc) return rc;
    for (int v = 0; v < nvec; ++v) {
        out[2 * v] = res_host[(size_t)(v / NV) * NC + v % NV];
        out[2 * v + 1] = res_host[(size_t)(v / NV) * NC + NV + v % NV];
    }
    return TBK_OK;
}
