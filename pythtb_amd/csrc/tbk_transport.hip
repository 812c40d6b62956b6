// tbk_transport.hip -- Fermi-surface transport on k lists and uniform meshes: band velocities, the thermal
// anomalous Hall and Nernst integrals, the Berry curvature dipole and the Drude weight.
//
// k reduced, H the convention-II matrix of tbk_gen_ham, V^c = d_c H (tbk_gen_dham), E_n and |n> the eigenpairs of the solver.
// A group G at a k point is a maximal run of consecutive sorted levels, each degenerate with its predecessor by kubo_degenerate.
// For band n in group G:
//   v^c_n     = Re <n|d_c H|n>                                  (raw; inside a group only the group's trace is defined)
//   vbar^c_n  = mean over m in G of <m|d_c H|m>                 (a group of one: v^c_n)
//   w^{cd}_n  = sum_{m in G} Re <n|d_c H|m> <m|d_d H|n>         (a group of one: v^c_n v^d_n), c <= d, stored row by row
// vbar and the sum of w over a group do not change when the solver's eigenvectors are rotated inside G.
// With x = (E - mu) / kT and t = e^{-|x|}:  f = 1 / (1 + e^x),  -df/dE = t / (1 + t)^2 / kT,  s = log1p(t) + |x| t / (1 + t), and
//   hall(mu)      = mean_k sum_n f_n Omega_n            nernst(mu) = mean_k sum_n s_n Omega_n
//   dipole_c(mu)  = mean_k sum_n (-df/dE)_n Omega_n vbar^c_n       (means over the (dir0, dir1) planes, Omega_n of tbk_curv.hip)
//   D_cd(mu)      = mean_k sum_n (-df/dE)_n w^{cd}_n               (mean over the whole mesh)
//
// Pipeline: the chunk loop of tbk_kubo.h (k generator, solver with vectors); per chunk the contraction with CurvQ (E_n, Omega_n; every
// n, two states included) and the velocity kernel below -- a sparse bilinear form over the non-empty slots, O(nnz) per matrix element,
// no dense d H and no matrix product; then one thermal scan over the per-band records of the whole mesh (k_kubo_thermal of
// tbk_kubo.h with the policies TrThermal and DrudeThermal below) and k_kubo_rows.  Every partition depends on the mesh, n and
// the number of levels alone, and nothing uses atomics on floating-point data: two calls give the same bits.
#include <math.h>
#include <string.h>
#include "tbk_kubo.h"

#define TR_LDS_U 1024                                    // k_tr_vel_lds: eigenvectors of a workgroup's points, P n^2 <= 1024 cd
#define TR_LDS_SV 2048                                   // and their slot values, 3 P nnz <= 3 P n (n + 1) / 2 <= 1920 cd

// where the velocity kernels write: index (row b, point first + ik) of arrays with nfull points per row; null = not wanted
struct VelOut {
    double* ev;     // [n][nfull]        E_b
    double* v;      // [dk][n][nfull]    raw v^c_b (the wide form needs it: it holds the diagonal between its passes)
    double* vbar;   // [dk][n][nfull]
    double* w;      // [dk (dk + 1) / 2][n][nfull]
    int64_t first, nfull;
};

// d_c H_ab, c = 0 .. dim_k - 1, of one non-empty slot (dham_terms serves two directions per walk of the slot's terms)
__device__ __forceinline__ void slot_velocities(const ModelView& mv, const int4 z4, const double (&kk)[4], const cd (&z)[4],
                                                cd (&v)[3]) {
    const int a = z4.x & 0xffff, b = z4.x >> 16;
    cd h, x;
    dham_terms(mv, a, b, z4.y, z4.z, kk, z, 0, mv.dim_k > 1 ? 1 : 0, h, v[0], v[1]);
    v[2] = cd{0.0, 0.0};
    if (mv.dim_k > 2) dham_terms(mv, a, b, z4.y, z4.z, kk, z, 2, 2, h, v[2], x);
}

// one slot's share of <x|d_c H|y>, every c: v_c conj(x_a) y_b, and v_c^* conj(x_b) y_a for the lower half of an off-diagonal slot
__device__ __forceinline__ void slot_add(cd (&e)[3], const int dk, const int a, const int b, const cd v0, const cd v1, const cd v2,
                                         const cd* __restrict__ ux, const cd* __restrict__ uy) {
    const cd t = cmulc(ux[a], uy[b]);
    cfma(e[0], v0, t);
    if (dk > 1) cfma(e[1], v1, t);
    if (dk > 2) cfma(e[2], v2, t);
    if (a != b) {
        const cd s = cmulc(ux[b], uy[a]);
        cfmac(e[0], v0, s);
        if (dk > 1) cfmac(e[1], v1, s);
        if (dk > 2) cfmac(e[2], v2, s);
    }
}

// w6 += Re x_c conj(x_d) for c <= d, in the row-by-row order of three directions (00 01 02 11 12 22; a direction the model
// does not have contributes zeros); w_pick: entry q of the dk-direction order (dk = 2: 00 01 11)
__device__ __forceinline__ void w_add(double (&w)[6], const cd (&x)[3]) {
    int q = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int d = c; d < 3; ++d) w[q++] += x[c].x * x[d].x + x[c].y * x[d].y;
}
#define W_PICK(w, dk, q) ((dk) == 2 && (q) == 2 ? (w)[3] : (w)[q])

// ---------------------------------------------------------------- velocities, 1 .. 32 states
// P = kubo_lds_points(n) points per workgroup.  U (read once from HBM, coalesced) and the slot values of every point for all dim_k
// directions are staged in LDS; then one lane per (point, band) walks its group: the diagonal elements of the group's members for
// vbar, and the elements <b|d_c H|m> for w.  Every lane of a group sums the same terms in the same order, so vbar has the same bits
// for every member.
__global__ __launch_bounds__(256) void k_tr_vel_lds(const ModelView mv, const double* __restrict__ k, const cd* __restrict__ evec,
                                                    const double* __restrict__ eval, const int64_t nk, const int P, const VelOut o) {
    __shared__ cd U[TR_LDS_U];
    __shared__ cd SV[TR_LDS_SV];
    const int n = mv.nsta, nn = n * n, dk = mv.dim_k, nnz = mv.nnz;
    const int64_t ik0 = (int64_t)blockIdx.x * P;
    const int np = (int)std::min<int64_t>(P, nk - ik0);
    for (int e = threadIdx.x; e < np * nn; e += 256) {
        const int p = e / nn, r = e - p * nn, b = r / n, i = r - b * n;
        U[e] = evec[((int64_t)b * nk + ik0 + p) * n + i];
    }
    for (int e = threadIdx.x; e < np * nnz; e += 256) {
        const int p = e / nnz;
        double kk[4];
        cd z[4], v[3];
        k_phases(mv, k, ik0 + p, kk, z);
        slot_velocities(mv, mv.nz[e - p * nnz], kk, z, v);
        SV[3 * e] = v[0];
        SV[3 * e + 1] = v[1];
        SV[3 * e + 2] = v[2];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < np * n; e += 256) {
        const int p = e / n, b = e - p * n;
        const int64_t ik = ik0 + p, at = o.first + ik;
        const cd* up = U + p * nn;
        const cd* sv = SV + 3 * p * nnz;
        int g0, g1;
        band_group(eval, nk, ik, n, b, g0, g1);
        double vs[3] = {0.0, 0.0, 0.0}, vb[3] = {0.0, 0.0, 0.0}, w[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int m = g0; m < g1; ++m) {
            cd dm[3] = {cd{0.0, 0.0}, cd{0.0, 0.0}, cd{0.0, 0.0}}, x[3] = {cd{0.0, 0.0}, cd{0.0, 0.0}, cd{0.0, 0.0}};
            for (int q = 0; q < nnz; ++q) {
                const int ab = mv.nz[q].x;
                slot_add(dm, dk, ab & 0xffff, ab >> 16, sv[3 * q], sv[3 * q + 1], sv[3 * q + 2], up + m * n, up + m * n);
                if (m != b && o.w) slot_add(x, dk, ab & 0xffff, ab >> 16, sv[3 * q], sv[3 * q + 1], sv[3 * q + 2], up + b * n, up + m * n);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                vs[c] += dm[c].x;
                if (m == b) {
                    vb[c] = dm[c].x;
                    x[c] = dm[c];
                }
            }
            w_add(w, x);
        }
        const double inv = 1.0 / (double)(g1 - g0);
        if (o.ev) o.ev[(int64_t)b * o.nfull + at] = eval[(int64_t)b * nk + ik];
#pragma unroll
        for (int c = 0; c < 3; ++c)
            if (c < dk) {
                const int64_t i = ((int64_t)c * n + b) * o.nfull + at;
                if (o.v) o.v[i] = vb[c];
                if (o.vbar) o.vbar[i] = g1 - g0 == 1 ? vs[c] : vs[c] * inv;
            }
        if (o.w)
#pragma unroll
            for (int q = 0; q < 6; ++q)
                if (q < dk * (dk + 1) / 2) o.w[((int64_t)q * n + b) * o.nfull + at] = W_PICK(w, dk, q);
    }
}

// ---------------------------------------------------------------- velocities, 33 .. 2048 states
// One workgroup per point.  Pass d = 0, 1, ... (as many as the point's largest group has members; one for a point without degenerate
// levels) forms <b|d_c H|b + d> for every b whose group holds b + d: the slot values of a tile of 256 slots are computed once per pass
// for all directions and staged in LDS, then a wavefront per band walks the tile with the slots across its lanes -- u_b[a] and
// u_m[b'] are read along the contiguous index of evec[b][ik][.] -- and adds its shuffle-tree sum to the band's LDS accumulator (one
// owner per band, the tiles in order: no atomics).  After a pass the band's thread adds the pair's products to w (its own entry of the
// output, pass after pass) and, for d = 0, stores the raw velocity; vbar is the group's mean of those.
// Dynamic LDS: acc[3][n] cd, grp[n] int (g0 | g1 << 16): 52 n bytes.
__global__ __launch_bounds__(256) void k_tr_vel_wide(const ModelView mv, const double* __restrict__ k, const cd* __restrict__ evec,
                                                     const double* __restrict__ eval, const int64_t nk, const VelOut o) {
    extern __shared__ __align__(16) unsigned char tr_lds[];
    __shared__ int sab[256];
    __shared__ cd sval[3][256];
    __shared__ int gmax;
    const int n = mv.nsta, dk = mv.dim_k, nnz = mv.nnz, nw = dk * (dk + 1) / 2;
    cd* acc = (cd*)tr_lds;
    int* grp = (int*)(acc + 3 * n);
    const int64_t ik = blockIdx.x, at = o.first + ik;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (threadIdx.x == 0) gmax = 1;
    __syncthreads();
    for (int b = threadIdx.x; b < n; b += 256) {
        int g0, g1;
        band_group(eval, nk, ik, n, b, g0, g1);
        grp[b] = g0 | (g1 << 16);
        if (g1 - g0 > 1) atomicMax(&gmax, g1 - g0);
        if (o.ev) o.ev[(int64_t)b * o.nfull + at] = eval[(int64_t)b * nk + ik];
        if (o.w)
            for (int q = 0; q < nw; ++q) o.w[((int64_t)q * n + b) * o.nfull + at] = 0.0;
    }
    double kk[4];
    cd z[4];
    k_phases(mv, k, ik, kk, z);
    __syncthreads();
    const int passes = gmax;
    for (int d = 0; d < passes; ++d) {
        for (int i = threadIdx.x; i < 3 * n; i += 256) acc[i] = cd{0.0, 0.0};
        for (int q0 = 0; q0 < nnz; q0 += 256) {
            __syncthreads();                                       // (acc is zeroed; the previous tile is consumed)
            if (q0 + (int)threadIdx.x < nnz) {
                const int4 z4 = mv.nz[q0 + threadIdx.x];
                cd v[3];
                slot_velocities(mv, z4, kk, z, v);
                sab[threadIdx.x] = z4.x;
                sval[0][threadIdx.x] = v[0];
                sval[1][threadIdx.x] = v[1];
                sval[2][threadIdx.x] = v[2];
            }
            __syncthreads();
            const int cnt = min(256, nnz - q0);
            for (int b = wave; b + d < n; b += 4) {
                const int m = b + d;
                if (m >= (grp[b] >> 16)) continue;                 // (uniform: a wavefront per band)
                const cd* ux = evec + ((int64_t)b * nk + ik) * n;
                const cd* uy = evec + ((int64_t)m * nk + ik) * n;
                cd e[3] = {cd{0.0, 0.0}, cd{0.0, 0.0}, cd{0.0, 0.0}};
                for (int q = lane; q < cnt; q += 64) slot_add(e, dk, sab[q] & 0xffff, sab[q] >> 16, sval[0][q], sval[1][q], sval[2][q], ux, uy);
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    if (c < dk) {
#pragma unroll
                        for (int s = 32; s > 0; s >>= 1) {
                            e[c].x += __shfl_xor(e[c].x, s);
                            e[c].y += __shfl_xor(e[c].y, s);
                        }
                        if (lane == 0) acc[c * n + b] = cadd(acc[c * n + b], e[c]);
                    }
            }
        }
        __syncthreads();
        for (int b = threadIdx.x; b < n; b += 256) {
            const int g0 = grp[b] & 0xffff, g1 = grp[b] >> 16;
            if (d == 0)
                for (int c = 0; c < dk; ++c) o.v[((int64_t)c * n + b) * o.nfull + at] = acc[c * n + b].x;
            if (o.w) {
                double w[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                if (b + d < g1) {                                  // the pair (b, b + d) ...
                    const cd x[3] = {acc[b], acc[n + b], acc[2 * n + b]};
                    w_add(w, x);
                }
                if (d > 0 && b - d >= g0) {                        // ... and (b - d, b), whose products are the same by hermiticity
                    const cd x[3] = {acc[b - d], acc[n + b - d], acc[2 * n + b - d]};
                    w_add(w, x);
                }
#pragma unroll
                for (int q = 0; q < 6; ++q)
                    if (q < nw) o.w[((int64_t)q * n + b) * o.nfull + at] += W_PICK(w, dk, q);
            }
        }
        __syncthreads();                                           // (acc is zeroed again by the next pass; o.v is complete)
    }
    if (o.vbar)
        for (int b = threadIdx.x; b < n; b += 256) {
            const int g0 = grp[b] & 0xffff, g1 = grp[b] >> 16;
            const double inv = 1.0 / (double)(g1 - g0);
            for (int c = 0; c < dk; ++c) {
                double s = 0.0;
                for (int m = g0; m < g1; ++m) s += o.v[((int64_t)c * n + m) * o.nfull + at];
                o.vbar[((int64_t)c * n + b) * o.nfull + at] = g1 - g0 == 1 ? s : s * inv;
            }
        }
}

// ---------------------------------------------------------------- thermal scan
// The policies of k_kubo_thermal (tbk_kubo.h): the records beside E are Omega and vbar^c (transport: hall, nernst, dipole_c) or the
// w^{cd} (Drude; the whole mesh).  Per (record, level) one exp, one division and (transport) one log1p (tbk_kubo.h's fermi_terms).
template <int DK>
struct TrThermal {
    static constexpr int NR = 1 + DK, NQ = 2 + DK;
    static constexpr bool kWhole = false;
    static __device__ __forceinline__ void add(const double e, const double (&r)[NR], const double u, double, const double ikT,
                                               double (&acc)[NQ]) {
        const FermiTerms ft = fermi_terms((e - u) * ikT);
        const double df = ft.mdf() * ikT;                           // -df/dE
        acc[0] = fma(ft.f(), r[0], acc[0]);
        acc[1] = fma(ft.entropy(), r[0], acc[1]);                   // -f ln f - (1 - f) ln(1 - f)
        const double dw = df * r[0];
#pragma unroll
        for (int c = 0; c < DK; ++c) acc[2 + c] = fma(dw, r[1 + c], acc[2 + c]);
    }
};
template <int DK>
struct DrudeThermal {
    static constexpr int NR = DK * (DK + 1) / 2, NQ = NR;
    static constexpr bool kWhole = true;
    static __device__ __forceinline__ void add(const double e, const double (&r)[NR], const double u, double, const double ikT,
                                               double (&acc)[NQ]) {
        const double df = fermi_terms((e - u) * ikT).mdf() * ikT;   // -df/dE
#pragma unroll
        for (int c = 0; c < NQ; ++c) acc[c] = fma(df, r[c], acc[c]);
    }
};

// ---------------------------------------------------------------- host side
static int tr_levels_check(const char* fn, int nmu, const double* mu, double kT) {
    int rc = kubo_levels_check(fn, nmu, mu, 1);
    if (!rc) rc = kubo_kt_check(fn, kT, true);
    return rc ? rc : kubo_levels_finite(fn, nmu, mu);
}
// the velocity kernel of one chunk (eigenpairs ec[n][cnt], vc[n][cnt][n] of the points kp)
static int tr_velocity(tbk_model* m, const double* kp, const double* ec, const cd* vc, int64_t cnt, const VelOut& o) {
    tbk_ctx* ctx = m->ctx;
    const int n = m->nsta;
    if (n <= 32) {
        const int P = kubo_lds_points(n);
        TBK_REQUIRE(P * n * n <= TR_LDS_U && 3 * P * m->view.nnz <= TR_LDS_SV, TBK_EINVAL, "tr_velocity: %d slots of %d states", m->view.nnz, n);
        ProfScope ps(ctx, "tr_vel_lds");
        hipLaunchKernelGGL(k_tr_vel_lds, dim3((unsigned)((cnt + P - 1) / P)), dim3(256), 0, ctx->stream, m->view, kp, vc, ec, cnt, P, o);
        TBK_HIP(hipGetLastError());
        return TBK_OK;
    }
    TBK_REQUIRE(n <= 2048 && o.v, TBK_EINVAL, "tr_velocity: %d states", n);
    const size_t lds = (size_t)n * (3 * sizeof(cd) + sizeof(int));
    if (lds > 48 * 1024)
        TBK_HIP(hipFuncSetAttribute((const void*)k_tr_vel_wide, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    ProfScope ps(ctx, "tr_vel_wide");
    hipLaunchKernelGGL(k_tr_vel_wide, dim3((unsigned)cnt), dim3(256), lds, ctx->stream, m->view, kp, vc, ec, cnt, o);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

// the thermal scan of rec over the planes P and the row sums: sums[s][j][NQ] on the host
template <class Pol>
static int tr_scan(tbk_ctx* ctx, const PlaneArgs& P, int n, const double* rec, const double* mu_dev, int nmu, double kT, int G,
                   double* part, double* rows, std::vector<double>& sums) {
    {
        ProfScope ps(ctx, Pol::kWhole ? "drude_scan" : "tr_scan");
        int rc = kubo_thermal_launch<Pol>(ctx, P, n, rec, mu_dev, nmu, kT, G, part);
        if (rc) return rc;
    }
    return kubo_rows_to_host(ctx, "tr_rows", part, G, (int64_t)P.nslice * nmu * Pol::NQ, rows, sums);
}

extern "C" int tbk_band_velocity_list(tbk_model* m, const double* k, int64_t nk, int dir, double* out) {
    TBK_REQUIRE(m, TBK_EINVAL, "tbk_band_velocity_list: null model");
    TBK_REQUIRE(m->dim_k >= 1 && m->dim_k <= 3, TBK_EINVAL, "tbk_band_velocity_list: the band velocity needs dim_k 1, 2 or 3 (the model has %d)",
                m->dim_k);
    TBK_REQUIRE(dir >= -1 && dir < m->dim_k, TBK_EINVAL, "tbk_band_velocity_list: dir=%d must be -1 (every axis) or an axis in [0, %d)", dir,
                m->dim_k);
    TBK_REQUIRE(nk >= 0 && out && (k || nk == 0), TBK_EINVAL, "tbk_band_velocity_list: bad k list or output");
    if (nk == 0) return TBK_OK;
    const int n = m->nsta, dk = m->dim_k;
    tbk_ctx* ctx = m->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    KuboChunks cw(n, dk, kubo_chunk_len(n, nk), 0, 0, 0);
    double *k_dev, *v_dev;
    KuboCarve ws;
    ws.add(k_dev, (size_t)nk * dk * sizeof(double)), ws.add(v_dev, (size_t)dk * n * nk * sizeof(double)), ws.add(cw.base, cw.bytes());
    int rc = kubo_carve(ctx, ws);
    if (rc) return rc;
    TBK_HIP(hipMemcpyAsync(k_dev, k, (size_t)nk * dk * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    rc = kubo_for_chunks(m, cw, k_dev, nullptr, nk, [&](int64_t first, int64_t cnt, const double* kp, const double* ec, const cd* vc) -> int {
        return tr_velocity(m, kp, ec, vc, cnt, VelOut{nullptr, v_dev, nullptr, nullptr, first, nk});
    });
    if (rc) return rc;
    const size_t row = (size_t)n * nk;
    TBK_HIP(hipMemcpyAsync(out, dir < 0 ? v_dev : v_dev + (size_t)dir * row, (dir < 0 ? dk : 1) * row * sizeof(double), hipMemcpyDeviceToHost,
                           ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    return TBK_OK;
}

extern "C" int tbk_anom_transport_mesh(tbk_model* m, const int32_t* mesh, int dir0, int dir1, int nmu, const double* mu, double kT,
                                       double* out) {
    std::vector<int> mask;
    int rc = kubo_check("tbk_anom_transport_mesh", "anomalous transport", m, dir0, dir1, nullptr, 0, mask);
    if (rc) return rc;
    TBK_REQUIRE(mesh && out, TBK_EINVAL, "tbk_anom_transport_mesh: null argument");
    TBK_REQUIRE(m->dim_k == 2 || m->dim_k == 3, TBK_EINVAL, "tbk_anom_transport_mesh: dim_k=%d (meshes of 2 or 3 dimensions)", m->dim_k);
    rc = tr_levels_check("tbk_anom_transport_mesh", nmu, mu, kT);
    if (rc) return rc;
    const int n = m->nsta, dk = m->dim_k, nq = 2 + dk;
    PlaneArgs P;
    rc = kubo_planes("tbk_anom_transport_mesh", mesh, dir0, dir1, dk, P);
    if (rc) return rc;
    const int64_t npts = P.npts;
    const int nslice = P.nslice;
    if (n < 2) {                              // no pair to sum: Omega = 0
        std::fill(out, out + (size_t)nq * nmu * nslice, 0.0);
        return TBK_OK;
    }
    tbk_ctx* ctx = m->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    const int G = kubo_thermal_groups(P, n, nmu, nq);
    KuboChunks cw = kubo_contract_chunks(n, dk, npts, false, CurvQ::NSET);
    const int64_t nrows = (int64_t)nslice * nmu * nq;
    const size_t recb = (size_t)n * npts * sizeof(double);                       // rec[2 + dk][n][npts]: E, Omega, vbar^c
    double *part, *rows, *mu_dev, *rec, *v_dev;
    KuboCarve ws;
    ws.add(part, (size_t)nrows * G * sizeof(double)), ws.add(rows, (size_t)nrows * sizeof(double)), ws.add(mu_dev, (size_t)nmu * sizeof(double));
    ws.add(rec, (2 + dk) * recb), ws.add(v_dev, n > 32 ? dk * recb : 0), ws.add(cw.base, cw.bytes());   // v: the wide form's diagonal
    rc = kubo_carve(ctx, ws);
    if (rc) return rc;
    double* ev_dev = rec;
    double* om_dev = rec + (size_t)n * npts;
    double* vbar_dev = rec + 2 * (size_t)n * npts;
    TBK_HIP(hipMemcpyAsync(mu_dev, mu, (size_t)nmu * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    rc = kubo_contract<CurvQ>(m, nullptr, mesh, npts, dir0, dir1, mask, cw, CurvQ::Out{om_dev, ev_dev},
                              [&](int64_t first, int64_t cnt, const double* kp, const double* ec, const cd* vc) -> int {
                                  return tr_velocity(m, kp, ec, vc, cnt, VelOut{nullptr, v_dev, vbar_dev, nullptr, first, npts});
                              });
    if (rc) return rc;
    std::vector<double> sums;
    rc = dk == 2 ? tr_scan<TrThermal<2>>(ctx, P, n, rec, mu_dev, nmu, kT, G, part, rows, sums)
                 : tr_scan<TrThermal<3>>(ctx, P, n, rec, mu_dev, nmu, kT, G, part, rows, sums);
    if (rc) return rc;
    const double inv = 1.0 / (double)P.nplane;
    // out[q][j][s], q = hall, nernst, dipole_0 .. dipole_{dk - 1}
    for (int s = 0; s < nslice; ++s)
        for (int j = 0; j < nmu; ++j)
            for (int q = 0; q < nq; ++q) out[((size_t)q * nmu + j) * nslice + s] = sums[((size_t)s * nmu + j) * nq + q] * inv;
    return TBK_OK;
}

extern "C" int tbk_drude_mesh(tbk_model* m, const int32_t* mesh, int nmu, const double* mu, double kT, double* out) {
    TBK_REQUIRE(m && mesh && out, TBK_EINVAL, "tbk_drude_mesh: null argument");
    TBK_REQUIRE(m->dim_k >= 1 && m->dim_k <= 3, TBK_EINVAL, "tbk_drude_mesh: dim_k=%d (meshes of 1, 2 or 3 dimensions)", m->dim_k);
    int rc = tr_levels_check("tbk_drude_mesh", nmu, mu, kT);
    if (rc) return rc;
    const int n = m->nsta, dk = m->dim_k, nq = dk * (dk + 1) / 2;
    PlaneArgs P;                               // one "plane": the whole mesh in k_uniform_mesh order
    rc = kubo_whole_mesh("tbk_drude_mesh", mesh, dk, P);
    if (rc) return rc;
    const int64_t npts = P.npts;
    tbk_ctx* ctx = m->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    const int G = kubo_thermal_groups(P, n, nmu, nq);
    const int64_t nrows = (int64_t)nmu * nq;
    KuboChunks cw(n, dk, kubo_chunk_len(n, npts), 0, 0, 0);
    const size_t recb = (size_t)n * npts * sizeof(double);                       // rec[1 + nq][n][npts]: E, w^{cd}
    double *part, *rows, *mu_dev, *rec, *v_dev;
    KuboCarve ws;
    ws.add(part, (size_t)nrows * G * sizeof(double)), ws.add(rows, (size_t)nrows * sizeof(double)), ws.add(mu_dev, (size_t)nmu * sizeof(double));
    ws.add(rec, (1 + nq) * recb), ws.add(v_dev, n > 32 ? dk * recb : 0), ws.add(cw.base, cw.bytes());
    rc = kubo_carve(ctx, ws);
    if (rc) return rc;
    TBK_HIP(hipMemcpyAsync(mu_dev, mu, (size_t)nmu * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    rc = kubo_for_chunks(m, cw, nullptr, mesh, npts, [&](int64_t first, int64_t cnt, const double* kp, const double* ec, const cd* vc) -> int {
        return tr_velocity(m, kp, ec, vc, cnt, VelOut{rec, v_dev, nullptr, rec + (size_t)n * npts, first, npts});
    });
    if (rc) return rc;
    std::vector<double> sums;
    rc = dk == 1   ? tr_scan<DrudeThermal<1>>(ctx, P, n, rec, mu_dev, nmu, kT, G, part, rows, sums)
         : dk == 2 ? tr_scan<DrudeThermal<2>>(ctx, P, n, rec, mu_dev, nmu, kT, G, part, rows, sums)
                   : tr_scan<DrudeThermal<3>>(ctx, P, n, rec, mu_dev, nmu, kT, G, part, rows, sums);
    if (rc) return rc;
    const double inv = 1.0 / (double)npts;
    for (size_t i = 0; i < (size_t)nrows; ++i) out[i] = sums[i] * inv;           // out[j][q], q over c <= d row by row
    return TBK_OK;
}
