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
// persistent kernel: two calls give the same bits.
#include <math.h>
#include <algorithm>
#include <cmath>
#include <new>
#include <vector>
#include "tbk_kpm.h"

#define KPMS_GUARD 5                         // doubles of the guard record: flag, <T_j v|T_j v>, <v|v>, sample, vector

// ------------------------------------------------------------------ kernels
// The epilogue of k_kpm_step that adds the term of step j to every series: acc[s][row][NV] += coef[s][j] nw, s ascending; FIRST
// (j = 1) writes acc[s] = coef[s][0] cur + coef[s][1] nw instead.  part: the row-local sums of <nw|nw> (the second slot stays zero).
struct KpmSeriesTerm {
    static constexpr bool SUMS = true;
    int nset, ncoef, j;
    const cd* coef;
    cd* acc;
    double* part;
    template <int NV, bool FIRST>
    __device__ __forceinline__ void row(const int nsta, const int64_t row, const int v, const cd x0, const cd nw, double& dA, double&) const {
        add<NV, FIRST>(nset, ncoef, j, coef, acc, nsta, row, v, x0, nw);
        dA += cabs2(nw);
    }
    // a function of its own for the __restrict__ of its arguments, which a member cannot carry: with it the coefficients come
    // through scalar loads
    template <int NV, bool FIRST>
    static __device__ __forceinline__ void add(const int nset, const int ncoef, const int j, const cd* __restrict__ coef,
                                               cd* __restrict__ acc, const int nsta, const int64_t row, const int v, const cd x0,
                                               const cd nw) {
        for (int s = 0; s < nset; ++s) {
            cd* dst = acc + ((int64_t)s * nsta + row) * NV + v;
            cd t = FIRST ? cmul_x(coef[(int64_t)s * ncoef], x0) : *dst;
            cfma_x(t, coef[(int64_t)s * ncoef + j], nw);
            *dst = t;
        }
    }
};

// ncoef = 1: acc[s][row][NV] = coef[s][0] cur, no sparse product; a lane per element
__global__ __launch_bounds__(256) void k_kpm_series_const(const int64_t len, const int nset, const int ncoef, const cd* __restrict__ coef,
                                                          const cd* __restrict__ cur, cd* __restrict__ acc) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < len; i += (int64_t)gridDim.x * 256) {
        const cd x = cur[i];
        for (int s = 0; s < nset; ++s) acc[(int64_t)s * len + i] = cmul_x(coef[(int64_t)s * ncoef], x);
    }
}

// The guard of one series: dots[step][2][NV] holds A_step = <T_step v|T_step v> per vector, A_0 = <v|v>.  The largest A per vector
// (a NaN counts as infinite) against (1 + 1e-6) A_0; the first violation of a call is recorded in rec = (1, A, A_0, sample, vector).
// One workgroup; the launches of a call are ordered on the stream, so "first" is the same in every run.
template <int NV>
__global__ __launch_bounds__(256) void k_kpm_series_guard(const int nstep, const double* __restrict__ dots, const double sample,
                                                          double* __restrict__ rec) {
    constexpr int NC = 2 * NV, G = 256 / NV;
    const int v = threadIdx.x % NV, g = threadIdx.x / NV;
    double mx = 0.0;
    for (int s = g; s < nstep; s += G) {
        const double A = dots[(int64_t)s * NC + v];
        mx = fmax(mx, A == A ? A : INFINITY);
    }
    __shared__ double red[G][NV];
    red[g][v] = mx;
    __syncthreads();
    if (threadIdx.x == 0 && rec[0] == 0.0)
        for (int u = 0; u < NV; ++u) {
            double t = red[0][u];
            for (int i = 1; i < G; ++i) t = fmax(t, red[i][u]);
            const double a0 = dots[u];
            if (!(t <= (1.0 + 1e-6) * a0)) {
                rec[0] = 1.0;
                rec[1] = t;
                rec[2] = a0;
                rec[3] = sample;
                rec[4] = (double)u;
                break;
            }
        }
}

// out[s][v][nsta] = acc[s][row][v], v < nv: a tile of 32 rows x NV vectors through LDS, so that both sides move whole segments.
// grid (row tiles, sets); out is the slice of this block of vectors, set_stride elements between two sets.
template <int NV>
__global__ __launch_bounds__(256) void k_kpm_series_gather(const int nsta, const int nv, const int64_t set_stride,
                                                           const cd* __restrict__ acc, cd* __restrict__ out) {
    constexpr int RPB = 256 / NV;
    __shared__ cd t[NV][RPB + 1];
    const int64_t ntiles = ((int64_t)nsta + RPB - 1) / RPB;
    const int s = blockIdx.y;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row0 = tile * RPB;
        {
            const int r = threadIdx.x / NV, v = threadIdx.x % NV;
            if (row0 + r < nsta) t[v][r] = acc[((int64_t)s * nsta + row0 + r) * NV + v];
        }
        __syncthreads();
        {
            const int v = threadIdx.x / RPB, r = threadIdx.x % RPB;
            if (v < nv && row0 + r < nsta) out[(int64_t)s * set_stride + (int64_t)v * nsta + row0 + r] = t[v][r];
        }
        __syncthreads();
    }
}

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
namespace {
// One series for a block of NV vectors.  On entry `cur` holds the start vectors and slot 0 of `part` the partial sums of their
// norms; on return (of the launches) acc[s][row][NV] holds sum_m coef[s][m] T_m(H~) cur and the guard has seen every norm.
struct Series {
    tbk_ctx* ctx;
    const tbk_sparse* sp;
    KpmPlan plan;
    int nset, ncoef;
    double b, inv_a;
    const cd* coef;      // device, [nset][ncoef]
    cd *cur, *prev;
    double *part, *dots, *rec;
};

int series_run(const Series& S, const cd* val, cd* acc, double sample) {
    constexpr int NV = KPM_NV;
    tbk_ctx* ctx = S.ctx;
    const int n = S.sp->nsta, nsteps = S.ncoef - 1, nwg = S.plan.nwg;
    if (nsteps == 0) {
        ProfScope ps(ctx, "kpm_series_const");
        hipLaunchKernelGGL(k_kpm_series_const, dim3(kpm_stream_grid((int64_t)n * NV)), dim3(256), 0, ctx->stream, (int64_t)n * NV, S.nset,
                           S.ncoef, S.coef, S.cur, acc);
        TBK_HIP(hipGetLastError());
    }
    int rc = kpm_run_steps(ctx, S.plan, nsteps, S.cur, S.prev, S.part, S.dots, [&](int j, const cd* x, cd* y, double* pj) {
        const KpmSeriesTerm term{S.nset, S.ncoef, j, S.coef, acc, pj};
        ProfScope ps(ctx, "kpm_series_step");
        if (j == 1)
            hipLaunchKernelGGL((k_kpm_step<NV, true, KpmSeriesTerm>), dim3(nwg), dim3(256), 0, ctx->stream, n, S.sp->row_ptr, S.sp->col, val,
                               x, nullptr, y, S.b, S.inv_a, term);
        else
            hipLaunchKernelGGL((k_kpm_step<NV, false, KpmSeriesTerm>), dim3(nwg), dim3(256), 0, ctx->stream, n, S.sp->row_ptr, S.sp->col, val,
                               x, nullptr, y, S.b, S.inv_a, term);
        TBK_HIP(hipGetLastError());
        return TBK_OK;
    });
    if (rc) return rc;
    ProfScope ps(ctx, "kpm_series_guard");
    hipLaunchKernelGGL((k_kpm_series_guard<NV>), dim3(1), dim3(256), 0, ctx->stream, nsteps + 1, S.dots, sample, S.rec);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

// the verdict of the guard record after the call's synchronisation
int series_verdict(const char* who, const double* rec, const tbk_sparse* sp, double emin, double emax) {
    if (rec[0] == 0.0) return TBK_OK;
    tbk_set_error("%s: <T_j v|T_j v> reaches %g for vector %lld of sample %lld, beyond <v|v> = %g: the bounds (%.17g, %.17g) do not "
                  "contain the spectrum (Gershgorin interval of this operator: (%.17g, %.17g))",
                  who, rec[1], (long long)rec[4], (long long)rec[3], rec[2], emin, emax, sp->gmin, sp->gmax);
    return TBK_EINVAL;
}

template <class Layout>
int series_workspace(const char* who, tbk_ctx* ctx, Layout&& layout) {
    size_t total;
    int rc = kpm_workspace(ctx, layout, &total);
    if (rc == TBK_ENOMEM) {
        (void)hipGetLastError();
        tbk_set_error("%s: no device workspace of %zu bytes", who, total);
    }
    return rc;
}
}  // namespace

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
    rc = series_workspace("tbk_kpm_apply_series", ctx, [&](KpmCarve& c) {
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
    const Series S{ctx, sp, P, nset, ncoef, b, 1.0 / a, coef_dev, cur, prev, part, dots, rec};
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
            rc = series_run(S, val, acc, (double)q);
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
    return series_verdict("tbk_kpm_apply_series", rec_host, sp, emin, emax);
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
    rc = series_workspace("tbk_kpm_marker", ctx, [&](KpmCarve& c) {
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
    const Series S{ctx, sp, P, 1, ncoef, b, 1.0 / a, coef_dev, cur, prev, part, dots, rec};
    for (int blk = 0; blk < nblk; ++blk) {
        const int v0 = blk * NV, nv = std::min(NV, nvec - v0);
        rc = start.launch(ctx, nwg, 0, v0, nv, cur, part);
        if (rc) return rc;
        rc = series_run(S, sp->amp, w1, (double)blk);      // w1 = F s
        if (rc) return rc;
        {   // u = B w1
            ProfScope ps(ctx, "kpm_series_scale");
            hipLaunchKernelGGL((k_kpm_series_scale<NV>), dim3(nwg), dim3(256), 0, ctx->stream, n, db_dev, w1, cur, part);
            TBK_HIP(hipGetLastError());
        }
        rc = series_run(S, sp->amp, w3, (double)blk);      // w3 = F u
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
    rc = series_verdict("tbk_kpm_marker", rec_host, sp, emin, emax);
    if (rc) return rc;
    for (int v = 0; v < nvec; ++v) {
        out[2 * v] = res_host[(size_t)(v / NV) * NC + v % NV];
        out[2 * v + 1] = res_host[(size_t)(v / NV) * NC + NV + v % NV];
    }
    return TBK_OK;
}
