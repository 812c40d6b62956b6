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

#define KPMS_MAX_SLOTS 128                   // steps between two reductions of the partial sums
#define KPMS_PART_BYTES ((size_t)32 << 20)   // ... and the workspace they may take
#define KPMS_GUARD 5                         // doubles of the guard record: flag, <T_j v|T_j v>, <v|v>, sample, vector

// ------------------------------------------------------------------ kernels
// One Chebyshev step of k_kpm_step for a block of NV vectors -- nw = 2 H~ cur - prev (FIRST: nw = H~ cur), stored over prev -- that
// also adds the term of this step to every series: acc[s][row][NV] += coef[s][j] nw, s ascending; FIRST (j = 1) writes
// acc[s] = coef[s][0] cur + coef[s][1] nw instead.  part: the row-local sums of <nw|nw> (the second slot stays zero).  The thread
// layout of k_kpm_step: 8 rows x 8 vectors per wavefront, 32 rows per workgroup, grid-stride over the row tiles.
template <int NV, bool FIRST>
__global__ __launch_bounds__(256) void k_kpm_series_step(const int nsta, const int64_t* __restrict__ row_ptr,
                                                         const int32_t* __restrict__ col, const cd* __restrict__ val,
                                                         const cd* __restrict__ cur, cd* __restrict__ prev, const double b,
                                                         const double inv_a, const int nset, const int ncoef, const int j,
                                                         const cd* __restrict__ coef, cd* __restrict__ acc, double* __restrict__ part) {
    constexpr int RPW = 64 / NV, RPB = 4 * RPW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, v = lane % NV, rw = lane / NV;
    const int64_t ntiles = ((int64_t)nsta + RPB - 1) / RPB;
    double dA = 0.0;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row = tile * RPB + wave * RPW + rw;
        if (row < nsta) {
            const int64_t e0 = row_ptr[row], e1 = row_ptr[row + 1];
            cd sum{0.0, 0.0};
            for (int64_t e = e0; e < e1; ++e) cfma(sum, val[e], cur[(int64_t)col[e] * NV + v]);
            const cd x0 = cur[row * NV + v];
            const cd h{(sum.x - b * x0.x) * inv_a, (sum.y - b * x0.y) * inv_a};
            cd nw = h;
            if (!FIRST) {
                const cd p = prev[row * NV + v];
                nw = cd{2.0 * h.x - p.x, 2.0 * h.y - p.y};
            }
            prev[row * NV + v] = nw;
            for (int s = 0; s < nset; ++s) {
                cd* dst = acc + ((int64_t)s * nsta + row) * NV + v;
                cd t = FIRST ? cmul_x(coef[(int64_t)s * ncoef], x0) : *dst;
                cfma_x(t, coef[(int64_t)s * ncoef + j], nw);
                *dst = t;
            }
            dA += cabs2(nw);
        }
    }
    kpm_block_sums<NV>(dA, 0.0, part);
}

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
// device buffer.  The thread layout of k_kpm_init.
template <int NV>
__global__ __launch_bounds__(256) void k_kpm_series_scale(const int nsta, const double* __restrict__ d, const cd* __restrict__ in,
                                                          cd* __restrict__ cur, double* __restrict__ part) {
    constexpr int RPW = 64 / NV, RPB = 4 * RPW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, v = lane % NV, rw = lane / NV;
    const int64_t ntiles = ((int64_t)nsta + RPB - 1) / RPB;
    double dA = 0.0;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row = tile * RPB + wave * RPW + rw;
        if (row < nsta) {
            const cd x = cscale(in[row * NV + v], d[row]);
            cur[row * NV + v] = x;
            dA += cabs2(x);
        }
    }
    kpm_block_sums<NV>(dA, 0.0, part);
}

// part[workgroup][2][NV] = the row-local sums of (Re, Im) conj(x[row][v]) d[row] y[row][v]
template <int NV>
__global__ __launch_bounds__(256) void k_kpm_series_dot(const int nsta, const double* __restrict__ d, const cd* __restrict__ x,
                                                        const cd* __restrict__ y, double* __restrict__ part) {
    constexpr int RPW = 64 / NV, RPB = 4 * RPW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, v = lane % NV, rw = lane / NV;
    const int64_t ntiles = ((int64_t)nsta + RPB - 1) / RPB;
    double dA = 0.0, dB = 0.0;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row = tile * RPB + wave * RPW + rw;
        if (row < nsta) {
            const cd z = cscale(cmulc(x[row * NV + v], y[row * NV + v]), d[row]);
            dA += z.x;
            dB += z.y;
        }
    }
    kpm_block_sums<NV>(dA, dB, part);
}

// ------------------------------------------------------------------ host
namespace {
// One series for a block of NV vectors.  On entry `cur` holds the start vectors and slot 0 of `part` the partial sums of their
// norms; on return (of the launches) acc[s][row][NV] holds sum_m coef[s][m] T_m(H~) cur and the guard has seen every norm.
struct Series {
    tbk_ctx* ctx;
    const tbk_sparse* sp;
    int nwg, nslots, nset, ncoef;
    double b, inv_a;
    const cd* coef;      // device, [nset][ncoef]
    cd *cur, *prev;
    double *part, *dots, *rec;
};

int series_run(const Series& S, const cd* val, cd* acc, double sample) {
    constexpr int NV = KPM_NV, NC = 2 * NV;
    tbk_ctx* ctx = S.ctx;
    const int n = S.sp->nsta, nsteps = S.ncoef - 1;
    const size_t part_slot = (size_t)S.nwg * NC;
    cd *x = S.cur, *y = S.prev;
    if (nsteps == 0) {
        ProfScope ps(ctx, "kpm_series_const");
        hipLaunchKernelGGL(k_kpm_series_const, dim3(kpm_stream_grid((int64_t)n * NV)), dim3(256), 0, ctx->stream, (int64_t)n * NV, S.nset,
                           S.ncoef, S.coef, x, acc);
        TBK_HIP(hipGetLastError());
    }
    int chunk0 = 0;    // first step of the partial sums not yet reduced; step j sits in slot j - chunk0
    for (int j = 1; j <= nsteps; ++j) {
        if (j - chunk0 == S.nslots) {
            ProfScope ps(ctx, "kpm_reduce");
            hipLaunchKernelGGL((k_kpm_reduce<NV>), dim3(S.nslots), dim3(256), 0, ctx->stream, S.nwg, S.part, S.dots + (size_t)chunk0 * NC);
            TBK_HIP(hipGetLastError());
            chunk0 = j;
        }
        double* pj = S.part + (size_t)(j - chunk0) * part_slot;
        ProfScope ps(ctx, "kpm_series_step");
        if (j == 1)
            hipLaunchKernelGGL((k_kpm_series_step<NV, true>), dim3(S.nwg), dim3(256), 0, ctx->stream, n, S.sp->row_ptr, S.sp->col, val, x, y,
                               S.b, S.inv_a, S.nset, S.ncoef, j, S.coef, acc, pj);
        else
            hipLaunchKernelGGL((k_kpm_series_step<NV, false>), dim3(S.nwg), dim3(256), 0, ctx->stream, n, S.sp->row_ptr, S.sp->col, val, x, y,
                               S.b, S.inv_a, S.nset, S.ncoef, j, S.coef, acc, pj);
        TBK_HIP(hipGetLastError());
        std::swap(x, y);
    }
    {
        ProfScope ps(ctx, "kpm_reduce");
        hipLaunchKernelGGL((k_kpm_reduce<NV>), dim3(nsteps + 1 - chunk0), dim3(256), 0, ctx->stream, S.nwg, S.part,
                           S.dots + (size_t)chunk0 * NC);
        TBK_HIP(hipGetLastError());
    }
    {
        ProfScope ps(ctx, "kpm_series_guard");
        hipLaunchKernelGGL((k_kpm_series_guard<NV>), dim3(1), dim3(256), 0, ctx->stream, nsteps + 1, S.dots, sample, S.rec);
        TBK_HIP(hipGetLastError());
    }
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

int series_scratch(const char* who, tbk_ctx* ctx, size_t total, void** ws) {
    int rc = tbk_ctx_scratch(ctx, total, ws);
    if (rc == TBK_ENOMEM) {
        (void)hipGetLastError();
        tbk_set_error("%s: no device workspace of %zu bytes", who, total);
    }
    return rc;
}

int series_slots(int nwg, int ncoef) {
    return (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(KPMS_MAX_SLOTS, (size_t)ncoef),
                                                     KPMS_PART_BYTES / ((size_t)nwg * 2 * KPM_NV * sizeof(double))));
}
}  // namespace

extern "C" int tbk_kpm_apply_series(tbk_sparse* sp, const double* k, int64_t nk, int ncoef, int nset, const double* coeffs, double emin,
                                    double emax, int nvec, const double* vectors, const int32_t* states, uint64_t seed, double* out) {
    constexpr int NV = KPM_NV, NC = 2 * NV;
    TBK_REQUIRE(sp && coeffs && out, TBK_EINVAL, "tbk_kpm_apply_series: null argument");
    TBK_REQUIRE(ncoef >= 1, TBK_EINVAL, "tbk_kpm_apply_series: ncoef=%d", ncoef);
    TBK_REQUIRE(nset >= 1, TBK_EINVAL, "tbk_kpm_apply_series: nset=%d", nset);
    TBK_REQUIRE(nvec >= 1, TBK_EINVAL, "tbk_kpm_apply_series: nvec=%d", nvec);
    TBK_REQUIRE(!(vectors && states), TBK_EINVAL, "tbk_kpm_apply_series: both vectors and states given");
    TBK_REQUIRE(std::isfinite(emin) && std::isfinite(emax) && emax > emin, TBK_EINVAL, "tbk_kpm_apply_series: bounds (%g, %g)", emin, emax);
    const int dim_k = sp->dim_k, n = sp->nsta;
    if (dim_k == 0) nk = 1;
    TBK_REQUIRE(nk >= 0 && (dim_k == 0 || k || nk == 0), TBK_EINVAL, "tbk_kpm_apply_series: null k list");
    if (states)
        for (int v = 0; v < nvec; ++v)
            TBK_REQUIRE(states[v] >= 0 && states[v] < n, TBK_EINVAL, "tbk_kpm_apply_series: state %d out of range [0, %d)", states[v], n);
    if (nk == 0) return TBK_OK;
    tbk_ctx* ctx = sp->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    const double a = 0.5 * (emax - emin), b = 0.5 * (emax + emin);
    const int64_t ntiles = ((int64_t)n + 4 * (64 / NV) - 1) / (4 * (64 / NV));
    const int nwg = (int)std::min<int64_t>(ntiles, KPM_MAX_WG);
    const int nslots = series_slots(nwg, ncoef);
    const int mode = vectors ? 2 : (states ? 1 : 0);
    const size_t nout = (size_t)nk * nset * nvec * n;
    const size_t b_val = dim_k > 0 ? up256((size_t)sp->nnz * sizeof(cd)) : 0, b_vec = up256((size_t)n * NV * sizeof(cd)),
                 b_acc = up256((size_t)nset * n * NV * sizeof(cd)), b_part = up256((size_t)nslots * nwg * NC * sizeof(double)),
                 b_dots = up256((size_t)ncoef * NC * sizeof(double)), b_rec = up256(KPMS_GUARD * sizeof(double)),
                 b_out = up256(nout * sizeof(cd)), b_coef = up256((size_t)nset * ncoef * sizeof(cd)),
                 b_k = up256((size_t)nk * std::max(dim_k, 1) * sizeof(double)),
                 b_src = mode == 2 ? up256((size_t)nvec * n * sizeof(cd)) : (mode == 1 ? up256((size_t)nvec * sizeof(int32_t)) : 0);
    void* ws = nullptr;
    {
        int rc = series_scratch("tbk_kpm_apply_series", ctx, b_val + 2 * b_vec + b_acc + b_part + b_dots + b_rec + b_out + b_coef + b_k + b_src,
                                &ws);
        if (rc) return rc;
    }
    unsigned char* p = (unsigned char*)ws;
    auto take = [&p](size_t bytes) {
        unsigned char* q = p;
        p += bytes;
        return q;
    };
    cd* val_dev = (cd*)take(b_val);
    cd* cur = (cd*)take(b_vec);
    cd* prev = (cd*)take(b_vec);
    cd* acc = (cd*)take(b_acc);
    double* part = (double*)take(b_part);
    double* dots = (double*)take(b_dots);
    double* rec = (double*)take(b_rec);
    cd* out_dev = (cd*)take(b_out);
    cd* coef_dev = (cd*)take(b_coef);
    double* k_dev = (double*)take(b_k);
    void* src_dev = take(b_src);
    TBK_HIP(hipMemsetAsync(rec, 0, KPMS_GUARD * sizeof(double), ctx->stream));
    TBK_HIP(hipMemcpyAsync(coef_dev, coeffs, (size_t)nset * ncoef * sizeof(cd), hipMemcpyHostToDevice, ctx->stream));
    if (dim_k > 0) TBK_HIP(hipMemcpyAsync(k_dev, k, (size_t)nk * dim_k * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (mode == 2) TBK_HIP(hipMemcpyAsync(src_dev, vectors, (size_t)nvec * n * sizeof(cd), hipMemcpyHostToDevice, ctx->stream));
    if (mode == 1) TBK_HIP(hipMemcpyAsync(src_dev, states, (size_t)nvec * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    const Series S{ctx, sp, nwg, nslots, nset, ncoef, b, 1.0 / a, coef_dev, cur, prev, part, dots, rec};
    const int64_t gtiles = ((int64_t)n + 256 / NV - 1) / (256 / NV);
    for (int64_t q = 0; q < nk; ++q) {
        const cd* val = sp->amp;
        if (dim_k > 0) {
            int rc = kpm_values_at(sp, k_dev + q * dim_k, val_dev);
            if (rc) return rc;
            val = val_dev;
        }
        for (int v0 = 0; v0 < nvec; v0 += NV) {
            const int nv = std::min(NV, nvec - v0);
            {
                ProfScope ps(ctx, "kpm_init");
                hipLaunchKernelGGL((k_kpm_init<NV>), dim3(nwg), dim3(256), 0, ctx->stream, n, nv, mode, seed, (uint64_t)(q * nvec + v0),
                                   mode == 1 ? (const int32_t*)src_dev + v0 : nullptr,
                                   mode == 2 ? (const cd*)src_dev + (size_t)v0 * n : nullptr, cur, part);
                TBK_HIP(hipGetLastError());
            }
            int rc = series_run(S, val, acc, (double)q);
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
    TBK_REQUIRE(ncoef >= 1, TBK_EINVAL, "tbk_kpm_marker: ncoef=%d", ncoef);
    TBK_REQUIRE(nvec >= 1, TBK_EINVAL, "tbk_kpm_marker: nvec=%d", nvec);
    TBK_REQUIRE(std::isfinite(emin) && std::isfinite(emax) && emax > emin, TBK_EINVAL, "tbk_kpm_marker: bounds (%g, %g)", emin, emax);
    const int n = sp->nsta;
    for (int v = 0; v < nvec; ++v)
        TBK_REQUIRE(states[v] >= 0 && states[v] < n, TBK_EINVAL, "tbk_kpm_marker: state %d out of range [0, %d)", states[v], n);
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
    const int64_t ntiles = ((int64_t)n + 4 * (64 / NV) - 1) / (4 * (64 / NV));
    const int nwg = (int)std::min<int64_t>(ntiles, KPM_MAX_WG);
    const int nslots = series_slots(nwg, ncoef);
    const int nblk = (nvec + NV - 1) / NV;
    const size_t b_vec = up256((size_t)n * NV * sizeof(cd)), b_part = up256((size_t)nslots * nwg * NC * sizeof(double)),
                 b_dots = up256((size_t)ncoef * NC * sizeof(double)), b_rec = up256(KPMS_GUARD * sizeof(double)),
                 b_res = up256((size_t)nblk * NC * sizeof(double)), b_coef = up256((size_t)ncoef * sizeof(cd)),
                 b_diag = up256((size_t)n * sizeof(double)), b_sta = up256((size_t)nvec * sizeof(int32_t));
    void* ws = nullptr;
    {
        int rc = series_scratch("tbk_kpm_marker", ctx, 4 * b_vec + b_part + b_dots + b_rec + b_res + b_coef + 2 * b_diag + b_sta, &ws);
        if (rc) return rc;
    }
    unsigned char* p = (unsigned char*)ws;
    auto take = [&p](size_t bytes) {
        unsigned char* q = p;
        p += bytes;
        return q;
    };
    cd* cur = (cd*)take(b_vec);
    cd* prev = (cd*)take(b_vec);
    cd* w1 = (cd*)take(b_vec);
    cd* w3 = (cd*)take(b_vec);
    double* part = (double*)take(b_part);
    double* dots = (double*)take(b_dots);
    double* rec = (double*)take(b_rec);
    double* res = (double*)take(b_res);
    cd* coef_dev = (cd*)take(b_coef);
    double* da_dev = (double*)take(b_diag);
    double* db_dev = (double*)take(b_diag);
    int32_t* sta_dev = (int32_t*)take(b_sta);
    TBK_HIP(hipMemsetAsync(rec, 0, KPMS_GUARD * sizeof(double), ctx->stream));
    TBK_HIP(hipMemcpyAsync(coef_dev, coef_host.data(), (size_t)ncoef * sizeof(cd), hipMemcpyHostToDevice, ctx->stream));
    TBK_HIP(hipMemcpyAsync(da_dev, da, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    TBK_HIP(hipMemcpyAsync(db_dev, db, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    TBK_HIP(hipMemcpyAsync(sta_dev, states, (size_t)nvec * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    const Series S{ctx, sp, nwg, nslots, 1, ncoef, b, 1.0 / a, coef_dev, cur, prev, part, dots, rec};
    for (int blk = 0; blk < nblk; ++blk) {
        const int v0 = blk * NV, nv = std::min(NV, nvec - v0);
        int rc;
        {   // the unit vectors s
            ProfScope ps(ctx, "kpm_init");
            hipLaunchKernelGGL((k_kpm_init<NV>), dim3(nwg), dim3(256), 0, ctx->stream, n, nv, 1, (uint64_t)0, (uint64_t)0, sta_dev + v0,
                               (const cd*)nullptr, cur, part);
            TBK_HIP(hipGetLastError());
        }
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
        ProfScope ps(ctx, "kpm_reduce");
        hipLaunchKernelGGL((k_kpm_reduce<NV>), dim3(1), dim3(256), 0, ctx->stream, nwg, part, res + (size_t)blk * NC);
        TBK_HIP(hipGetLastError());
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
    int rc = series_verdict("tbk_kpm_marker", rec_host, sp, emin, emax);
    if (rc) return rc;
    for (int v = 0; v < nvec; ++v) {
        out[2 * v] = res_host[(size_t)(v / NV) * NC + v % NV];
        out[2 * v + 1] = res_host[(size_t)(v / NV) * NC + NV + v % NV];
    }
    return TBK_OK;
}
