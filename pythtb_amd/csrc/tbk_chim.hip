// tbk_chim.hip -- the orbital-resolved bare susceptibility chi0_ab(q, w) on uniform meshes and the RPA on top of it (DESIGN.md
// section 28).
//
// Conventions of tbk_chi.hip (section 26): k and q reduced, E_n(k), u_n(k) the solver's eigenpairs, f = [E <= mu] or the Fermi function,
// all n^2 ordered pairs, the mean over k_uniform_mesh(mesh).  a, b run over the na <= 16 selected STATE indices (components of u):
//   A^{nm}_a(k, q) = conj(u_n(k)[a]) u_m(k+q)[a]
//   dynamic   chi0_ab(q, w) = -(1 / N_k) sum_k sum_{n,m} [f_n(k) - f_m(k+q)] A_a conj(A_b) / (w + i eta + E_n(k) - E_m(k+q))
//   static    chi0_ab(q)    =  (1 / N_k) sum_k sum_{n,m} L_nm A_a conj(A_b)            (L: chi_static_weight)
//   RPA       chi = (1 - chi0 V)^-1 chi0,   det = det(1 - chi0 V)
// Nothing of size n^2 na^2 is stored: sum_{n,m} w_nm A_a conj(A_b) = sum_n X^n_ab sum_m w_nm Y^m_ab with
//   X^n_ab = conj(u_n(k)[a]) u_n(k)[b],   Y^m_ab = u_m(k+q)[a] conj(u_m(k+q)[b]).
//
// Pipeline: the chunk loop of tbk_susceptibility_mesh (the solve at k once per chunk, then per q: k_chi_kq, the solve at k + q), then
//   static, n <= 32   k_chim_static: the selected components of U(k), U(k+q) and the n^2 weights of a batch of points in LDS, a lane per
//                     entry (a, b), spare lanes on further points; part[g][ab]
//   otherwise         k_chim_weights (the records (d, c) = (E_n - E_m, f_n - f_m), or L_nm) and k_chim_tables (X, Y of the selection),
//                     both from global memory, then
//                       dynamic   k_chim_omega: workgroup (frequency tile, k-group, block of entries), a lane per frequency;
//                                 part[g][ab][re, im][w]
//                       static    k_chim_contract (n > 32): a lane per entry; part[g][ab]
//   k_group_rows / k_group_rows_lanes   acc[q][row] (+)= sum_g part[g][row], the groups in index order
// and after the last chunk k_chim_finish (chi0 = acc / N_k in the layout of the result) and, with an interaction, k_chim_rpa.
// The chunk, groups, tiles and blocks do not depend on the q list and nothing uses atomics: two calls give the same bits, and a q
// gives the same bits alone and inside a longer list.
#include <math.h>
#include "tbk_chim.h"
#include "tbk_chi_dev.h"
#include "tbk_small_solve.h"

// ---------------------------------------------------------------- static, 1 .. 32 states
// Workgroup g takes the points [g nk / G, (g + 1) nk / G) of the chunk in batches of P.  Per point the LDS holds u1[s][a] =
// u_s(k)[sel a], u2[s][a] = u_s(k+q)[sel a] (na complex per state) and the weights L[s][m]; lane t = share nab + (a na + b) takes the
// points share, share + Q, ... of the batch (Q = 256 / nab shares, added in index order through LDS at the end).  All lanes of a
// wavefront that work on one point read the same state row at the same time: u[s][a] is one address for every na consecutive lanes
// (a broadcast), u[s][b] are consecutive 16-byte slots, L[s][m] one address: no bank conflict for any n.
__global__ __launch_bounds__(256) void k_chim_static(const cd* __restrict__ evec1, const cd* __restrict__ evec2, const double* __restrict__ e1,
                                                     const double* __restrict__ e2, const int64_t nk, const int n, const int32_t* __restrict__ sel,
                                                     const int na, const int P, const int G, const double mu, const double kT,
                                                     cd* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) double S[CHIM_LDS_D];
    const int t = threadIdx.x, nab = na * na, nn = n * n, ns = n * na;
    const int g = blockIdx.x;
    const int64_t p0 = (int64_t)g * nk / G, p1 = (int64_t)(g + 1) * nk / G;
    const int Q = 256 / nab, share = t / nab, el = t - share * nab;
    const int ia = el / na, ib = el - ia * na;
    cd* U1 = (cd*)S;
    cd* U2 = U1 + P * ns;
    double* W = S + 4 * P * ns;
    cd acc{0.0, 0.0};
    for (int64_t b0 = p0; b0 < p1; b0 += P) {
        const int np = (int)std::min<int64_t>(P, p1 - b0);
        for (int i = t; i < np * ns; i += 256) {
            const int p = i / ns, r = i - p * ns, s = r / na, a = r - s * na;
            const int64_t at = ((int64_t)s * nk + b0 + p) * n + sel[a];
            U1[i] = evec1[at];
            U2[i] = evec2[at];
        }
        for (int i = t; i < np * nn; i += 256) {
            const int p = i / nn, r = i - p * nn, s = r / n, m = r - s * n;
            W[i] = chi_static_weight(e1[(int64_t)s * nk + b0 + p], e2[(int64_t)m * nk + b0 + p], mu, kT);
        }
        __syncthreads();
        if (share < Q)
            for (int p = share; p < np; p += Q) {
                const cd* u1 = U1 + p * ns;
                const cd* u2 = U2 + p * ns;
                const double* w = W + p * nn;
                for (int s = 0; s < n; ++s) {
                    cd T{0.0, 0.0};
                    bool any = false;
                    for (int m = 0; m < n; ++m) {
                        const double l = w[s * n + m];
                        if (l == 0.0) continue;                    // (kT = 0: both levels on one side of mu)
                        any = true;
                        const cd y = cmulc(u2[m * na + ib], u2[m * na + ia]);   // u[a] conj(u[b])
                        T.x = fma(l, y.x, T.x);
                        T.y = fma(l, y.y, T.y);
                    }
                    if (any) cfma_x(acc, cmulc(u1[s * na + ia], u1[s * na + ib]), T);
                }
            }
        __syncthreads();                                           // (the batch is consumed)
    }
    cd* buf = (cd*)S;
    buf[t] = acc;
    __syncthreads();
    if (t < nab) {
        cd s = buf[t];
        for (int qq = 1; qq < Q; ++qq) s = cadd(s, buf[qq * nab + t]);
        part[(int64_t)g * nab + t] = s;
    }
}

// ---------------------------------------------------------------- the plain form: weights and tables from global memory
// one lane per (point, n, m): the record (d, c) = (E_n(k) - E_m(k+q), f_n - f_m), or the static weight L_nm
template <bool STATIC>
__global__ __launch_bounds__(256) void k_chim_weights(const double* __restrict__ e1, const double* __restrict__ e2, const int64_t nk, const int n,
                                                      const double mu, const double kT, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, nn = (int64_t)n * n;
    if (i >= nk * nn) return;
    const int64_t ik = i / nn, r = i - ik * nn;
    const int a = (int)(r / n), b = (int)(r - (int64_t)a * n);
    const double en = e1[(int64_t)a * nk + ik], em = e2[(int64_t)b * nk + ik];
    if constexpr (STATIC) {
        out[i] = chi_static_weight(en, em, mu, kT);
    } else {
        out[2 * i] = en - em;
        out[2 * i + 1] = chi_fdiff(en, em, mu, kT);
    }
}
// one lane per (point, state s, entry ab): X[ik][s][ab] = conj(u_s(k)[a]) u_s(k)[b], Y[ik][s][ab] = u_s(k+q)[a] conj(u_s(k+q)[b])
__global__ __launch_bounds__(256) void k_chim_tables(const cd* __restrict__ evec1, const cd* __restrict__ evec2, const int64_t nk, const int n,
                                                     const int32_t* __restrict__ sel, const int na, cd* __restrict__ X, cd* __restrict__ Y) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int nab = na * na;
    if (i >= nk * n * nab) return;
    const int64_t is = i / nab, ik = is / n;
    const int el = (int)(i - is * nab), s = (int)(is - ik * n), ia = el / na, ib = el - ia * na;
    const int64_t row = ((int64_t)s * nk + ik) * n;
    X[i] = cmulc(evec1[row + sel[ia]], evec1[row + sel[ib]]);
    Y[i] = cmulc(evec2[row + sel[ib]], evec2[row + sel[ia]]);
}

// static, from 33 states: workgroup g takes the points [g nk / G, (g + 1) nk / G) of the chunk, lane t = share nab + ab the points
// share, share + Q, ... of them; the shares are added in index order through LDS.  No speed is claimed for it.
__global__ __launch_bounds__(256) void k_chim_contract(const double* __restrict__ L, const cd* __restrict__ X, const cd* __restrict__ Y,
                                                       const int64_t nk, const int n, const int nab, const int G, cd* __restrict__ part) {
    __shared__ cd buf[256];
    const int t = threadIdx.x, g = blockIdx.x;
    const int64_t p0 = (int64_t)g * nk / G, p1 = (int64_t)(g + 1) * nk / G, nn = (int64_t)n * n;
    const int Q = 256 / nab, share = t / nab, el = t - share * nab;
    cd acc{0.0, 0.0};
    if (share < Q)
        for (int64_t ik = p0 + share; ik < p1; ik += Q) {
            const double* w = L + ik * nn;
            const cd* x = X + ik * n * nab + el;
            const cd* y = Y + ik * n * nab + el;
            for (int s = 0; s < n; ++s) {
                cd T{0.0, 0.0};
                bool any = false;
                for (int m = 0; m < n; ++m) {
                    const double l = w[(int64_t)s * n + m];
                    if (l == 0.0) continue;
                    any = true;
                    const cd ym = y[(int64_t)m * nab];
                    T.x = fma(l, ym.x, T.x);
                    T.y = fma(l, ym.y, T.y);
                }
                if (any) cfma_x(acc, x[(int64_t)s * nab], T);
            }
        }
    buf[t] = acc;
    __syncthreads();
    if (t < nab) {
        cd s = buf[t];
        for (int qq = 1; qq < Q; ++qq) s = cadd(s, buf[qq * nab + t]);
        part[(int64_t)g * nab + t] = s;
    }
}

// ---------------------------------------------------------------- frequency stage
// Workgroup (tile of kPairTile frequencies, k-group g, block of EB entries), the plan of k_chi_omega: lane t takes w[tile + t] and
// w[tile + 256 + t] and walks the points [g nk / G, (g + 1) nk / G) of the chunk in order; records and tables are wave-uniform values.
// Per (n, m) with c != 0 the resolvent g = -c (t - i eta) r, t = w + d, r = 1 / (t^2 + eta^2), is formed once and feeds
// T_ab += g Y^m_ab for the block's entries; after the m loop acc_ab += X^n_ab T_ab.  An entry beyond the last reads the last one
// and is not written.  part[g][ab][re, im][w]
template <int EB, int NS>
__device__ __forceinline__ void chim_walk(const double* __restrict__ rec, const cd* __restrict__ X, const cd* __restrict__ Y, const int64_t i0,
                                          const int64_t i1, const int n, const int nab, const int (&el)[EB], const double (&om)[2],
                                          const double eta, cd (&acc)[EB][2]) {
    const double eta2 = eta * eta;
    for (int64_t ik = i0; ik < i1; ++ik) {
        const double* p = rec + ik * n * n * 2;
        const cd* x = X + ik * n * nab;
        const cd* y = Y + ik * n * nab;
        for (int s = 0; s < n; ++s, x += nab) {
            cd T[EB][2];
#pragma unroll
            for (int j = 0; j < EB; ++j) T[j][0] = T[j][1] = cd{0.0, 0.0};
            bool any = false;
            for (int m = 0; m < n; ++m, p += 2) {
                const double d = p[0], c = p[1];
                if (c == 0.0) continue;                            // (uniform branch)
                any = true;
                cd ym[EB];
#pragma unroll
                for (int j = 0; j < EB; ++j) ym[j] = y[m * nab + el[j]];
#pragma unroll
                for (int q = 0; q < NS; ++q) {
                    const double tt = om[q] + d;
                    const double cr = c * opt_rcp(fma(tt, tt, eta2));
                    const cd gg{-(cr * tt), cr * eta};
#pragma unroll
                    for (int j = 0; j < EB; ++j) cfma_x(T[j][q], gg, ym[j]);
                }
            }
            if (!any) continue;
#pragma unroll
            for (int j = 0; j < EB; ++j) {
                const cd xs = x[el[j]];
#pragma unroll
                for (int q = 0; q < NS; ++q) cfma_x(acc[j][q], xs, T[j][q]);
            }
        }
    }
}
template <int EB>
__global__ __launch_bounds__(256) void k_chim_omega(const double* __restrict__ rec, const cd* __restrict__ X, const cd* __restrict__ Y,
                                                    const int64_t nk, const int n, const int nab, const int G,
                                                    const double* __restrict__ omega, const int nw, const double eta,
                                                    double* __restrict__ part) {
    const int base = blockIdx.x * kPairTile;
    if (base + (int)(threadIdx.x & ~63u) >= nw) return;            // a wavefront without a frequency (uniform)
    const int g = blockIdx.y, e0 = blockIdx.z * EB;
    int wi[2], el[EB];
    double om[2];
    cd acc[EB][2];
#pragma unroll
    for (int j = 0; j < EB; ++j) {
        el[j] = min(e0 + j, nab - 1);
        acc[j][0] = acc[j][1] = cd{0.0, 0.0};
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        wi[s] = base + s * 256 + threadIdx.x;
        om[s] = wi[s] < nw ? omega[wi[s]] : 0.0;
    }
    const int64_t i0 = (int64_t)g * nk / G, i1 = (int64_t)(g + 1) * nk / G;
    if (base + 256 < nw) chim_walk<EB, 2>(rec, X, Y, i0, i1, n, nab, el, om, eta, acc);   // (uniform over the workgroup)
    else chim_walk<EB, 1>(rec, X, Y, i0, i1, n, nab, el, om, eta, acc);
    double* out = part + (int64_t)g * 2 * nab * nw;
#pragma unroll
    for (int j = 0; j < EB; ++j) {
        if (e0 + j >= nab) continue;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (wi[s] >= nw) continue;
            out[((int64_t)(e0 + j) * 2) * nw + wi[s]] = acc[j][s].x;
            out[((int64_t)(e0 + j) * 2 + 1) * nw + wi[s]] = acc[j][s].y;
        }
    }
}

// ---------------------------------------------------------------- the result
// chi0[q][w][ab] = acc[q][..] / N_k: one lane per complex number; acc[q] is [ab][re, im][w] (dynamic) or [ab][re, im] (static)
__global__ __launch_bounds__(256) void k_chim_finish(const double* __restrict__ acc, const int64_t nmat, const int nab, const int nwz,
                                                     const double nk, cd* __restrict__ chi0) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nmat * nab) return;
    const int64_t im = i / nab, iq = im / nwz;
    const int el = (int)(i - im * nab), w = (int)(im - iq * nwz);
    const double* a = acc + iq * 2 * nab * nwz + (int64_t)el * 2 * nwz + w;
    chi0[i] = cd{a[0] / nk, a[nwz] / nk};
}

// RPA, one matrix per workgroup of ONE wavefront: M = [1 - chi0 V | chi0] (na rows of 2 na) in LDS through tbk_small_solve.h's
// small_solve (Gaussian elimination with partial pivoting, back substitution, det = the signed product of the pivots).  A pivot of
// squared modulus exactly 0: det = 0 and the matrix of chi is NaN.  V is V[0] or V[q].
__global__ __launch_bounds__(64) void k_chim_rpa(const cd* __restrict__ chi0, const cd* __restrict__ V, const int vq, const int nwz,
                                                 const int na, cd* __restrict__ chi, cd* __restrict__ det) {
    __shared__ cd M[kChimSelMax][2 * kChimSelMax + 1];
    __shared__ cd C0[kChimSelMax * kChimSelMax], Vs[kChimSelMax * kChimSelMax];
    const int t = threadIdx.x, nab = na * na;
    const int64_t im = blockIdx.x;
    const cd* c0 = chi0 + im * nab;
    const cd* v = V + (vq ? im / nwz : 0) * nab;
    for (int e = t; e < nab; e += 64) {
        C0[e] = c0[e];
        Vs[e] = v[e];
    }
    __syncthreads();
    for (int e = t; e < nab; e += 64) {
        const int a = e / na, b = e - a * na;
        cd s{a == b ? 1.0 : 0.0, 0.0};
        for (int c = 0; c < na; ++c) {
            const cd x = C0[a * na + c], y = Vs[c * na + b];
            s.x = fma(x.y, y.y, fma(-x.x, y.x, s.x));
            s.y = fma(-x.y, y.x, fma(-x.x, y.y, s.y));
        }
        M[a][b] = s;
        M[a][na + b] = C0[e];
    }
    __syncthreads();
    cd d;
    if (!small_solve<kChimSelMax>(M, na, t, d)) {                  // (uniform over the workgroup)
        const double nan = __builtin_nan("");
        for (int e = t; e < nab; e += 64) chi[im * nab + e] = cd{nan, nan};
        if (t == 0) det[im] = cd{0.0, 0.0};
        return;
    }
    for (int e = t; e < nab; e += 64) chi[im * nab + e] = M[e / na][na + e % na];
    if (t == 0) det[im] = d;
}

// ---------------------------------------------------------------- host side
static int chim_group_sum(tbk_ctx* ctx, const ChimPlan& pl, const double* part, int accumulate, double* acc) {
    ProfScope ps(ctx, "chim_rows");
    if (pl.lane_rows)
        hipLaunchKernelGGL(k_group_rows_lanes, dim3(nblk(pl.nrows)), dim3(256), 0, ctx->stream, part, pl.G, pl.nrows, pl.nrows, pl.nrows,
                           accumulate, acc);
    else
        hipLaunchKernelGGL(k_group_rows, dim3((unsigned)pl.nrows), dim3(256), 0, ctx->stream, part, pl.G, pl.nrows, 1.0, accumulate, acc);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

extern "C" int tbk_susceptibility_matrix_mesh(tbk_model* m, const int32_t* mesh, int nq, const double* q, int nomega, const double* omega,
                                              double eta, double mu, double kT, int nsel, const int32_t* sel, const double* v, int nvq,
                                              double* chi0, double* chi_rpa, double* det) {
    const char* fn = "tbk_susceptibility_matrix_mesh";
    TBK_REQUIRE(m && mesh && q && sel && chi0, TBK_EINVAL, "%s: null argument", fn);
    const int dk = m->dim_k, n = m->nsta;
    int64_t npts;
    int rc = chim_check(fn, dk, n, mesh, nq, q, nomega, omega, eta, mu, kT, nsel, sel, v, nvq, chi_rpa != nullptr, det != nullptr, npts);
    if (rc) return rc;
    const ChimPlan pl = chim_plan(n, dk, npts, nq, nomega, nsel, nvq);
    tbk_ctx* ctx = m->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    void* base = nullptr;
    rc = tbk_ctx_scratch(ctx, pl.total, &base);
    if (rc) return rc;
    unsigned char* b = (unsigned char*)base;
    double* om_dev = (double*)(b + pl.off_om);
    double* q_dev = (double*)(b + pl.off_q);
    int32_t* sel_dev = (int32_t*)(b + pl.off_sel);
    cd* v_dev = (cd*)(b + pl.off_v);
    double* acc = (double*)(b + pl.off_acc);
    double* part = (double*)(b + pl.off_part);
    cd* out_dev = (cd*)(b + pl.off_out);
    KuboChunks cw = pl.cw;
    cw.base = b + pl.off_chunks;
    unsigned char* x0 = cw.extra<unsigned char>(0);
    double* kq = (double*)x0;
    double* e2 = (double*)(x0 + pl.off_e2);
    cd* v2 = (cd*)(x0 + pl.off_v2);
    double* rec = cw.extra<double>(1);
    cd* X = cw.extra<cd>(2);
    cd* Y = (cd*)(cw.extra<unsigned char>(2) + pl.off_y);
    const int na = pl.na, nab = pl.nab;
    if (pl.dynamic) TBK_HIP(hipMemcpyAsync(om_dev, omega, (size_t)nomega * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    TBK_HIP(hipMemcpyAsync(q_dev, q, (size_t)nq * dk * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    TBK_HIP(hipMemcpyAsync(sel_dev, sel, (size_t)na * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    if (pl.rpa) TBK_HIP(hipMemcpyAsync(v_dev, v, (size_t)nvq * nab * sizeof(cd), hipMemcpyHostToDevice, ctx->stream));
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
            if (pl.lds) {
                ProfScope ps(ctx, "chim_static");
                hipLaunchKernelGGL(k_chim_static, dim3((unsigned)pl.G), dim3(256), 0, ctx->stream, v1, (const cd*)v2, e1, (const double*)e2, cnt, n,
                                   (const int32_t*)sel_dev, na, pl.P, pl.G, mu, kT, (cd*)part);
                TBK_HIP(hipGetLastError());
            } else {
                {
                    ProfScope ps(ctx, "chim_pairs");
                    if (pl.dynamic)
                        hipLaunchKernelGGL(k_chim_weights<false>, dim3(nblk(cnt * n * n)), dim3(256), 0, ctx->stream, e1, (const double*)e2, cnt, n,
                                           mu, kT, rec);
                    else
                        hipLaunchKernelGGL(k_chim_weights<true>, dim3(nblk(cnt * n * n)), dim3(256), 0, ctx->stream, e1, (const double*)e2, cnt, n,
                                           mu, kT, rec);
                    TBK_HIP(hipGetLastError());
                    hipLaunchKernelGGL(k_chim_tables, dim3(nblk(cnt * n * nab)), dim3(256), 0, ctx->stream, v1, (const cd*)v2, cnt, n,
                                       (const int32_t*)sel_dev, na, X, Y);
                    TBK_HIP(hipGetLastError());
                }
                if (pl.dynamic) {
                    ProfScope ps(ctx, "chim_omega");
                    const dim3 grid(pl.ntile, (unsigned)pl.G, pl.neb);
                    if (pl.EB == 1)
                        hipLaunchKernelGGL(k_chim_omega<1>, grid, dim3(256), 0, ctx->stream, (const double*)rec, (const cd*)X, (const cd*)Y, cnt, n,
                                           nab, pl.G, (const double*)om_dev, nomega, eta, part);
                    else
                        hipLaunchKernelGGL(k_chim_omega<kChimBlock>, grid, dim3(256), 0, ctx->stream, (const double*)rec, (const cd*)X,
                                           (const cd*)Y, cnt, n, nab, pl.G, (const double*)om_dev, nomega, eta, part);
                } else {
                    ProfScope ps(ctx, "chim_contract");
                    hipLaunchKernelGGL(k_chim_contract, dim3((unsigned)pl.G), dim3(256), 0, ctx->stream, (const double*)rec, (const cd*)X,
                                       (const cd*)Y, cnt, n, nab, pl.G, (cd*)part);
                }
                TBK_HIP(hipGetLastError());
            }
            r2 = chim_group_sum(ctx, pl, part, first > 0 ? 1 : 0, acc + (int64_t)iq * pl.nrows);
            if (r2) return r2;
        }
        return TBK_OK;
    });
    if (rc) return rc;
    const int nwz = std::max(nomega, 1);
    const size_t nc0 = (size_t)pl.nmat * nab;
    {
        ProfScope ps(ctx, "chim_finish");
        hipLaunchKernelGGL(k_chim_finish, dim3(nblk((int64_t)nc0)), dim3(256), 0, ctx->stream, (const double*)acc, pl.nmat, nab, nwz, (double)npts,
                           out_dev);
        TBK_HIP(hipGetLastError());
    }
    if (!pl.rpa) {
        TBK_HIP(hipMemcpyAsync(chi0, out_dev, nc0 * sizeof(cd), hipMemcpyDeviceToHost, ctx->stream));
        TBK_HIP(hipStreamSynchronize(ctx->stream));
        return TBK_OK;
    }
    {
        ProfScope ps(ctx, "chim_rpa");
        hipLaunchKernelGGL(k_chim_rpa, dim3((unsigned)pl.nmat), dim3(64), 0, ctx->stream, (const cd*)out_dev, (const cd*)v_dev, nvq > 1 ? 1 : 0,
                           nwz, na, out_dev + nc0, out_dev + 2 * nc0);
        TBK_HIP(hipGetLastError());
    }
    // chi0, chi and det in one download
    std::vector<cd> host((size_t)pl.out_cd);
    TBK_HIP(hipMemcpyAsync(host.data(), out_dev, host.size() * sizeof(cd), hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    memcpy(chi0, host.data(), nc0 * sizeof(cd));
    memcpy(chi_rpa, host.data() + nc0, nc0 * sizeof(cd));
    if (det) memcpy(det, host.data() + 2 * nc0, (size_t)pl.nmat * sizeof(cd));
    return TBK_OK;
}
