// tbk_wan.hip -- projected and maximally localised Wannier functions on uniform k meshes.
//
// The mesh goes through the solver once, in tbk_kubo.h's chunks with eigenvectors; per chunk
//   k_wan_project   one wavefront per point: A = V_bands+ g~ (a lane per entry, the trial terms in list order), S = A+ A, its eigen-
//                   decomposition by small_eig_jacobi (tbk_small_eig.h), U = A S^-1/2, the smallest singular value of the point
//   k_wan_rotate    u~ = V_bands U for P points per workgroup, their U in LDS; u~[N_k][nw][nsta] stays resident
// then, with nothing left of the solver's output,
//   k_wan_overlap   M(k, b) = u~(k)+ D_G u~(k + b) for Q (point, b) items per workgroup, both sides staged through LDS in tiles of 32
//                   components, the neighbour multiplied by e^{-2 pi i G.tau_j} on the way in; a lane owns an entry (m, n)
//   k_wan_sum<1>, k_wan_fin1   sum_k Im ln M_nn(k, b) by k-groups, then b.r_n for every (function, b-vector)
//   k_wan_sum<2>, k_wan_fin2   the three parts of the spread and the per-function spreads, Omega into the history
// and per iteration of the Marzari-Vanderbilt descent (step alpha = 1), all in stream order:
//   k_wan_grad      one wavefront per point: dW(k) from M(k, b) and M(k - b, b)+, e^{dW} = Q e^{-i lam} Q+ from the eigen-decomposition
//                   of the Hermitian i dW (exactly unitary), U_acc(k) <- U_acc(k) e^{dW}
//   k_wan_mupdate   M(k, b) <- e^{-dW(k)} M(k, b) e^{dW(k + b)}
//   the two spread passes again
// At a convergence check the host reads the change of Omega of that iteration (8 bytes).  At the end
//   k_wan_hw        U_tot = U U_acc, H^W(k) = U_tot+ E U_tot
//   k_wan_fourier   t(R) = (1 / N_k) sum_k e^{-2 pi i k.R} H^W(k), a lane per (R, m, n) and k-group, phases from per-axis tables of exact
//                   integers; few lattice vectors: more k-groups, added in group order by k_wan_fourier_sum
//   k_wan_final, k_wan_functions   (on request) u~ U_acc e^{2 pi i k.tau_j} and its Fourier sum w_n(R, j)
// No atomics; every sum in a fixed order over a partition that depends on (mesh, nsta, nb, nw) alone: two calls give the same bits, and
// a run of max_iter = m gives the first m + 1 entries of the history of a longer run.
#include <math.h>
#include "tbk_wan.h"

namespace {
__device__ __forceinline__ cd wan_expi2pi(const double x) {
    double s, c;
    sincospi(2.0 * x, &s, &c);
    return cd{c, s};
}
__device__ __forceinline__ void wan_decode(const WanMesh& M, int64_t idx, int* i) {
    i[0] = i[1] = i[2] = 0;
    for (int d = M.dk - 1; d >= 0; --d) {
        i[d] = (int)(idx % M.N[d]);
        idx /= M.N[d];
    }
}
struct WanSteps {
    int s[WAN_BV_MAX][3];
    double w[WAN_BV_MAX];
    int nbv;
};
}  // namespace

// ---------------------------------------------------------------- projection and Loewdin factor: one wavefront per point
__global__ __launch_bounds__(64) void k_wan_project(const ModelView mv, const WanMesh Mh, const int64_t first, const int64_t cnt,
                                                    const cd* __restrict__ evec, const double* __restrict__ eval,
                                                    const int32_t* __restrict__ bands, const int nb, const int nw,
                                                    const int32_t* __restrict__ tptr, const int32_t* __restrict__ tstate,
                                                    const int32_t* __restrict__ trv, const cd* __restrict__ tamp, cd* __restrict__ U0,
                                                    double* __restrict__ EB, double* __restrict__ svk) {
    __shared__ cd Am[WAN_NB_MAX * SE_LD], S[SE_NMAX * SE_LD], Qm[SE_NMAX * SE_LD], X[SE_NMAX * SE_LD];
    const int t = threadIdx.x, n = mv.nsta;
    const int64_t kl = blockIdx.x, kk = first + kl;
    int ii[3];
    wan_decode(Mh, kk, ii);
    double kd[3] = {0.0, 0.0, 0.0};
    for (int d = 0; d < Mh.dk; ++d) kd[d] = (double)ii[d] / (double)Mh.N[d];   // k_uniform_mesh's point, bit for bit
    for (int e = t; e < nb * nw; e += 64) {
        const int b = e / nw, w = e % nw;
        const cd* v = evec + ((int64_t)bands[b] * cnt + kl) * n;
        cd acc{0.0, 0.0};
        for (int q = tptr[w]; q < tptr[w + 1]; ++q) {
            const int j = tstate[q];
            const double4 o = mv.orb[j];
            const double x = kd[0] * ((double)trv[3 * q] + o.x) + kd[1] * ((double)trv[3 * q + 1] + o.y) + kd[2] * ((double)trv[3 * q + 2] + o.z);
            cfmac_x(acc, cmul_x(tamp[q], wan_expi2pi(-x)), v[j]);           // g conj(v)
        }
        Am[b * SE_LD + w] = acc;
    }
    for (int b = t; b < nb; b += 64) EB[kk * nb + b] = eval[(int64_t)bands[b] * cnt + kl];
    __syncthreads();
    for (int e = t; e < nw * nw; e += 64) {
        const int r = e / nw, c = e % nw;
        cd acc{0.0, 0.0};
        if (r <= c) {
            for (int b = 0; b < nb; ++b) cfmac_x(acc, Am[b * SE_LD + c], Am[b * SE_LD + r]);
            if (r == c) acc.y = 0.0;
            S[r * SE_LD + c] = acc;
            if (r != c) S[c * SE_LD + r] = cconj(acc);
        }
    }
    __syncthreads();
    small_eig_jacobi(S, Qm, nw, t, 64);
    double lmin = S[0].x;
    for (int j = 1; j < nw; ++j) lmin = fmin(lmin, S[j * SE_LD + j].x);
    if (t == 0) svk[kk] = sqrt(fmax(lmin, 0.0));
    for (int e = t; e < nw * nw; e += 64) {
        const int r = e / nw, c = e % nw;
        cd acc{0.0, 0.0};
        for (int j = 0; j < nw; ++j) {
            const double lam = S[j * SE_LD + j].x;
            const double li = lam > 1e-300 ? 1.0 / sqrt(lam) : 0.0;
            cfma_x(acc, cscale(Qm[r * SE_LD + j], li), cconj(Qm[c * SE_LD + j]));
        }
        X[r * SE_LD + c] = acc;
    }
    __syncthreads();
    for (int e = t; e < nb * nw; e += 64) {
        const int b = e / nw, w = e % nw;
        cd acc{0.0, 0.0};
        for (int m = 0; m < nw; ++m) cfma_x(acc, Am[b * SE_LD + m], X[m * SE_LD + w]);
        U0[(kk * nb + b) * nw + w] = acc;
    }
}

// ---------------------------------------------------------------- u~ = V_bands U, P points per workgroup
__global__ __launch_bounds__(256) void k_wan_rotate(const int n, const int64_t first, const int64_t cnt, const int P,
                                                    const cd* __restrict__ evec, const int32_t* __restrict__ bands, const int nb, const int nw,
                                                    const cd* __restrict__ U0, cd* __restrict__ ut) {
    __shared__ cd Ul[WAN_ROT_LDS];
    const int t = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * P;
    const int np = (int)min((int64_t)P, cnt - p0);
    const int bw = nb * nw;
    for (int e = t; e < np * bw; e += 256) Ul[e] = U0[(first + p0) * bw + e];
    __syncthreads();
    const int64_t total = (int64_t)np * nw * n;
    for (int64_t e = t; e < total; e += 256) {
        const int j = (int)(e % n), w = (int)((e / n) % nw), pp = (int)(e / ((int64_t)n * nw));
        const int64_t kl = p0 + pp;
        cd acc{0.0, 0.0};
        for (int b = 0; b < nb; ++b) cfma_x(acc, evec[((int64_t)bands[b] * cnt + kl) * n + j], Ul[(pp * nb + b) * nw + w]);
        ut[((first + kl) * nw + w) * n + j] = acc;
    }
}

// ---------------------------------------------------------------- overlaps: Q (point, b) items per workgroup, nw^2 lanes each
__global__ __launch_bounds__(256) void k_wan_overlap(const WanMesh Mh, const WanSteps St, const int n, const int nw, const int Q,
                                                     const int64_t nitems, const cd* __restrict__ ut, const cd* __restrict__ phase,
                                                     cd* __restrict__ Mov) {
    __shared__ cd tile[WAN_OV_ROWS][WAN_OV_TJ + 1];
    const int t = threadIdx.x, nw2 = nw * nw, rows = 2 * nw;
    const int q = t / nw2, mn = t % nw2, m = mn / nw, c = mn % nw;
    const int64_t item = (int64_t)blockIdx.x * Q + q;
    const bool live = q < Q && item < nitems;
    cd acc{0.0, 0.0};
    for (int j0 = 0; j0 < n; j0 += WAN_OV_TJ) {
        for (int e = t; e < Q * rows * WAN_OV_TJ; e += 256) {
            const int jj = e % WAN_OV_TJ, row = e / WAN_OV_TJ, qq = row / rows, r = row % rows, j = j0 + jj;
            const int64_t it2 = (int64_t)blockIdx.x * Q + qq;
            cd v{0.0, 0.0};
            if (it2 < nitems && j < n) {
                const int64_t k = it2 / St.nbv;
                const int ib = (int)(it2 % St.nbv);
                if (r < nw) {
                    v = ut[(k * nw + r) * n + j];
                } else {
                    int G[3] = {0, 0, 0};
                    const int64_t k2 = wan_neighbour(Mh, k, St.s[ib], G);
                    v = ut[(k2 * nw + (r - nw)) * n + j];
                    for (int d = 0; d < Mh.dk; ++d)
                        if (G[d]) v = cmul_x(v, G[d] > 0 ? phase[d * n + j] : cconj(phase[d * n + j]));
                }
            }
            tile[row][jj] = v;
        }
        __syncthreads();
        if (live) {
            const cd* a = tile[q * rows + m];
            const cd* b = tile[q * rows + nw + c];
#pragma unroll 8
            for (int jj = 0; jj < WAN_OV_TJ; ++jj) cfmac_x(acc, b[jj], a[jj]);   // conj(u~_m(k)) u~_n(k + b)
        }
        __syncthreads();
    }
    if (live) Mov[item * nw2 + mn] = acc;
}

// ---------------------------------------------------------------- the spread sums: k-group g, lane (slice sl, function n, b-vector ib)
// The 128 lanes of a workgroup hold 128 / nq slices of the nq = nw nbv (function, b-vector) pairs: slice sl walks the points
// k0 + sl, k0 + sl + nsl, ... of the group, and lane (0, q) adds the slices' sums in slice order.
// PASS 1: sum_k phi_n;  PASS 2: sum_k of (1 - sum_m |M_mn|^2), (1 - |M_nn|^2), q_n^2, phi_n^2 with q_n = phi_n + b.r_n
template <int PASS>
__global__ __launch_bounds__(128) void k_wan_sum(const int64_t npts, const int nbv, const int nw, const int G, const cd* __restrict__ Mov,
                                                 const double* __restrict__ cb, double* __restrict__ part) {
    __shared__ double red[128][PASS == 1 ? 1 : 4];
    const int t = threadIdx.x, nq = nw * nbv, g = blockIdx.x, nsl = 128 / nq;
    const int q = t % nq, sl = t / nq;
    const int w = q / nbv, ib = q % nbv, nw2 = nw * nw;
    const int64_t k0 = (int64_t)g * npts / G, k1 = (int64_t)(g + 1) * npts / G;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (sl < nsl) {
        const double c = PASS == 2 ? cb[q] : 0.0;
        for (int64_t k = k0 + sl; k < k1; k += nsl) {
            const cd* M = Mov + (k * nbv + ib) * nw2;
            const cd d = M[w * nw + w];
            const double phi = atan2(d.y, d.x);
            if (PASS == 1) {
                s0 += phi;
            } else {
                double col = 0.0;
                for (int m = 0; m < nw; ++m) col += cabs2(M[m * nw + w]);
                s0 += 1.0 - col;
                s1 += 1.0 - cabs2(d);
                s2 += (phi + c) * (phi + c);
                s3 += phi * phi;
            }
        }
    }
    red[t][0] = s0;
    if (PASS == 2) red[t][PASS == 2 ? 1 : 0] = s1, red[t][PASS == 2 ? 2 : 0] = s2, red[t][PASS == 2 ? 3 : 0] = s3;
    __syncthreads();
    if (t >= nq) return;
    if (PASS == 1) {
        double a = 0.0;
        for (int j = 0; j < nsl; ++j) a += red[j * nq + q][0];
        part[(int64_t)g * nq + q] = a;
    } else {
        double a[4] = {0.0, 0.0, 0.0, 0.0};
        for (int j = 0; j < nsl; ++j)
            for (int i = 0; i < 4; ++i) a[i] += red[j * nq + q][PASS == 2 ? i : 0];
        double* p = part + ((int64_t)g * nq + q) * 4;
        p[0] = a[0], p[1] = a[1], p[2] = a[2], p[3] = a[3];
    }
}
// S1[n][ib] = sum_g, then cb[n][ib] = b_ib . r_n = -(2 / N_k) sum_ib' w_ib' (b_ib . b_ib') S1[n][ib']
__global__ __launch_bounds__(128) void k_wan_fin1(const int64_t npts, const int nbv, const int nw, const int G, const double* __restrict__ part,
                                                  const double* __restrict__ bw, const double* __restrict__ gram, double* __restrict__ S1,
                                                  double* __restrict__ cb) {
    __shared__ double s[WAN_NW_MAX * WAN_BV_MAX];
    const int q = threadIdx.x, nq = nw * nbv;
    if (q < nq) {
        double a = 0.0;
        for (int g = 0; g < G; ++g) a += part[(int64_t)g * nq + q];
        s[q] = a;
        S1[q] = a;
    }
    __syncthreads();
    if (q < nq) {
        const int w = q / nbv, ib = q % nbv;
        double a = 0.0;
        for (int j = 0; j < nbv; ++j) a += bw[j] * gram[ib * nbv + j] * s[w * nbv + j];
        cb[q] = -2.0 * a / (double)npts;
    }
}
// fin[0..3] = Omega_I, Omega_OD, Omega_D, Omega; fin[4 + n] = the spread of function n; hist[it] = Omega, dhist[it] = its change
__global__ __launch_bounds__(128) void k_wan_fin2(const int64_t npts, const int nbv, const int nw, const int G, const double* __restrict__ part,
                                                  const double* __restrict__ bw, const double* __restrict__ S1, const double* __restrict__ cb,
                                                  const int it, double* __restrict__ fin, double* __restrict__ hist, double* __restrict__ dhist) {
    __shared__ double s[WAN_NW_MAX * WAN_BV_MAX][4];
    const int q = threadIdx.x, nq = nw * nbv;
    if (q < nq) {
        double a[4] = {0.0, 0.0, 0.0, 0.0};
        for (int g = 0; g < G; ++g) {
            const double* p = part + ((int64_t)g * nq + q) * 4;
            a[0] += p[0], a[1] += p[1], a[2] += p[2], a[3] += p[3];
        }
        for (int i = 0; i < 4; ++i) s[q][i] = a[i];
    }
    __syncthreads();
    if (q == 0) {
        const double f = 2.0 / (double)npts;
        double oi = 0.0, ood = 0.0, od = 0.0;
        for (int ib = 0; ib < nbv; ++ib) {
            double a0 = 0.0, a1 = 0.0, a2 = 0.0;
            for (int w = 0; w < nw; ++w) a0 += s[w * nbv + ib][0], a1 += s[w * nbv + ib][1], a2 += s[w * nbv + ib][2];
            oi += bw[ib] * a0;
            ood += bw[ib] * (a1 - a0);
            od += bw[ib] * a2;
        }
        oi *= f, ood *= f, od *= f;
        const double om = oi + ood + od;
        fin[0] = oi, fin[1] = ood, fin[2] = od, fin[3] = om;
        hist[it] = om;
        dhist[it] = it > 0 ? om - hist[it - 1] : 0.0;
    }
    if (q < nw) {                                                  // <r^2>_n - |r_n|^2, |r_n|^2 = -(2 / N_k) sum_b w_b S1[n][b] (b . r_n)
        double r2 = 0.0, rr = 0.0;
        for (int ib = 0; ib < nbv; ++ib) {
            r2 += bw[ib] * (s[q * nbv + ib][1] + s[q * nbv + ib][3]);
            rr += bw[ib] * S1[q * nbv + ib] * cb[q * nbv + ib];
        }
        fin[4 + q] = 2.0 / (double)npts * (r2 + rr);
    }
}

// ---------------------------------------------------------------- one descent step: one wavefront per point
__global__ __launch_bounds__(64) void k_wan_grad(const WanMesh Mh, const WanSteps St, const int nw, const cd* __restrict__ Mov,
                                                 const double* __restrict__ cb, cd* __restrict__ expw, cd* __restrict__ uacc) {
    __shared__ cd MA[SE_NMAX * SE_LD], MB[SE_NMAX * SE_LD], H[SE_NMAX * SE_LD], Qm[SE_NMAX * SE_LD];
    __shared__ double qa[SE_NMAX], qb[SE_NMAX];
    const int t = threadIdx.x, nw2 = nw * nw, nbv = St.nbv;
    const int64_t k = blockIdx.x;
    cd acc[4] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
    double wsum = 0.0;
    for (int ib = 0; ib < nbv; ++ib) {
        int G[3], sm[3] = {-St.s[ib][0], -St.s[ib][1], -St.s[ib][2]};
        const int64_t kb = wan_neighbour(Mh, k, sm, G);
        const cd* pa = Mov + (k * nbv + ib) * nw2;
        const cd* pb = Mov + (kb * nbv + ib) * nw2;
        __syncthreads();
        for (int e = t; e < nw2; e += 64) {
            const int r = e / nw, c = e % nw;
            MA[r * SE_LD + c] = pa[e];
            MB[c * SE_LD + r] = cconj(pb[e]);                        // M(k, -b) = M(k - b, b)+
        }
        __syncthreads();
        if (t < nw) {
            const cd a = MA[t * SE_LD + t], b = MB[t * SE_LD + t];
            qa[t] = atan2(a.y, a.x) + cb[t * nbv + ib];
            qb[t] = atan2(b.y, b.x) - cb[t * nbv + ib];
        }
        __syncthreads();
        const double w = St.w[ib];
        wsum += 2.0 * w;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = t + 64 * i;
            if (e >= nw2) continue;
            const int r = e / nw, c = e % nw;
#pragma unroll
            for (int side = 0; side < 2; ++side) {
                const cd* M = side ? MB : MA;
                const double* qq = side ? qb : qa;
                const cd mrc = M[r * SE_LD + c], mcr = M[c * SE_LD + r], mcc = M[c * SE_LD + c], mrr = M[r * SE_LD + r];
                const cd Rrc = cmul_x(mrc, cconj(mcc)), Rcr = cmul_x(mcr, cconj(mrr));
                const double icc = 1.0 / cabs2(mcc), irr = 1.0 / cabs2(mrr);
                const cd Trc = cscale(cmul_x(mrc, cconj(mcc)), icc * qq[c]), Tcr = cscale(cmul_x(mcr, cconj(mrr)), irr * qq[r]);
                // A[R] = (R - R+) / 2,  S[T] = (T + T+) / 2i
                const cd Ar{0.5 * (Rrc.x - Rcr.x), 0.5 * (Rrc.y + Rcr.y)};
                const cd Tp{Trc.x + Tcr.x, Trc.y - Tcr.y};
                const cd Sr{0.5 * Tp.y, -0.5 * Tp.x};
                acc[i].x += w * (Ar.x - Sr.x);
                acc[i].y += w * (Ar.y - Sr.y);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {                                    // H = i dW, dW = acc / sum_{+-b} w_b
        const int e = t + 64 * i;
        if (e >= nw2) continue;
        const int r = e / nw, c = e % nw;
        const cd d{acc[i].x / wsum, acc[i].y / wsum};
        H[r * SE_LD + c] = cd{-d.y, r == c ? 0.0 : d.x};
    }
    __syncthreads();
    small_eig_jacobi(H, Qm, nw, t, 64);
    // e^{dW} = Q e^{-i lam} Q+ into MA, U_acc(k) into MB
    cd* ua = uacc + k * nw2;
    for (int e = t; e < nw2; e += 64) {
        const int r = e / nw, c = e % nw;
        cd a{0.0, 0.0};
        for (int j = 0; j < nw; ++j) {
            double sn, cs;
            sincos(-H[j * SE_LD + j].x, &sn, &cs);
            cfma_x(a, cmul_x(Qm[r * SE_LD + j], cd{cs, sn}), cconj(Qm[c * SE_LD + j]));
        }
        MA[r * SE_LD + c] = a;
        MB[r * SE_LD + c] = ua[e];
        expw[k * nw2 + e] = a;
    }
    __syncthreads();
    for (int e = t; e < nw2; e += 64) {
        const int r = e / nw, c = e % nw;
        cd a{0.0, 0.0};
        for (int j = 0; j < nw; ++j) cfma_x(a, MB[r * SE_LD + j], MA[j * SE_LD + c]);
        ua[e] = a;
    }
}

// M(k, b) <- E(k)+ M(k, b) E(k + b): one wavefront per (point, b)
__global__ __launch_bounds__(64) void k_wan_mupdate(const WanMesh Mh, const WanSteps St, const int nw, const cd* __restrict__ expw,
                                                    cd* __restrict__ Mov) {
    __shared__ cd E1[SE_NMAX * SE_LD], E2[SE_NMAX * SE_LD], Mm[SE_NMAX * SE_LD], Tm[SE_NMAX * SE_LD];
    const int t = threadIdx.x, nw2 = nw * nw;
    const int64_t item = blockIdx.x, k = item / St.nbv;
    const int ib = (int)(item % St.nbv);
    int G[3];
    const int64_t k2 = wan_neighbour(Mh, k, St.s[ib], G);
    cd* M = Mov + item * nw2;
    for (int e = t; e < nw2; e += 64) {
        const int r = e / nw, c = e % nw;
        E1[r * SE_LD + c] = expw[k * nw2 + e];
        E2[r * SE_LD + c] = expw[k2 * nw2 + e];
        Mm[r * SE_LD + c] = M[e];
    }
    __syncthreads();
    for (int e = t; e < nw2; e += 64) {
        const int r = e / nw, c = e % nw;
        cd a{0.0, 0.0};
        for (int j = 0; j < nw; ++j) cfma_x(a, Mm[r * SE_LD + j], E2[j * SE_LD + c]);
        Tm[r * SE_LD + c] = a;
    }
    __syncthreads();
    for (int e = t; e < nw2; e += 64) {
        const int r = e / nw, c = e % nw;
        cd a{0.0, 0.0};
        for (int j = 0; j < nw; ++j) cfmac_x(a, Tm[j * SE_LD + c], E1[j * SE_LD + r]);
        M[e] = a;
    }
}

// ---------------------------------------------------------------- the Wannier Hamiltonian
// U_tot = U U_acc (written back over U), H^W(k) = U_tot+ E U_tot: one wavefront per point
__global__ __launch_bounds__(64) void k_wan_hw(const int nb, const int nw, const double* __restrict__ EB, cd* __restrict__ U0,
                                               const cd* __restrict__ uacc, cd* __restrict__ HW) {
    __shared__ cd Ul[WAN_NB_MAX * SE_LD], Ua[SE_NMAX * SE_LD], Ut[WAN_NB_MAX * SE_LD];
    __shared__ double el[WAN_NB_MAX];
    const int t = threadIdx.x, nw2 = nw * nw;
    const int64_t k = blockIdx.x;
    cd* u = U0 + k * nb * nw;
    for (int e = t; e < nb * nw; e += 64) Ul[(e / nw) * SE_LD + e % nw] = u[e];
    for (int e = t; e < nw2; e += 64) Ua[(e / nw) * SE_LD + e % nw] = uacc[k * nw2 + e];
    if (t < nb) el[t] = EB[k * nb + t];
    __syncthreads();
    for (int e = t; e < nb * nw; e += 64) {
        const int b = e / nw, c = e % nw;
        cd a{0.0, 0.0};
        for (int m = 0; m < nw; ++m) cfma_x(a, Ul[b * SE_LD + m], Ua[m * SE_LD + c]);
        Ut[b * SE_LD + c] = a;
        u[e] = a;
    }
    __syncthreads();
    for (int e = t; e < nw2; e += 64) {
        const int r = e / nw, c = e % nw;
        cd a{0.0, 0.0};
        for (int b = 0; b < nb; ++b) cfmac_x(a, cscale(Ut[b * SE_LD + c], el[b]), Ut[b * SE_LD + r]);
        HW[k * nw2 + e] = a;
    }
}

// out[r][e] = (1 / N_k) sum_k tw(sign k.R_r) src(k, e), e < ne; tw: per-axis tables e^{-2 pi i p / N_a}; sign +1 takes their
// conjugates.  src(k, e) = src[k kstride + perm(e)]: the caller's layout through (sa, sb, nbm): e = a nbm + b -> a sa + b sb.  A lane per
// (r, e) and k-group (blockIdx.y, G of them): it walks its group's points in ascending order.  G = 1: the sum goes out scaled; else
// into part[g][r][e], which k_wan_fourier_sum adds in group order.
__global__ __launch_bounds__(256) void k_wan_fourier(const WanMesh Mh, const int64_t npts, const int nR, const int32_t* __restrict__ R,
                                                     const cd* __restrict__ tw, const int sign, const int ne, const int nbm, const int64_t sa,
                                                     const int64_t sb, const int64_t kstride, const cd* __restrict__ src, const int G,
                                                     cd* __restrict__ part, cd* __restrict__ out) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x, tot = (int64_t)nR * ne;
    if (id >= tot) return;
    const int g = blockIdx.y;
    const int r = (int)(id / ne), e = (int)(id % ne);
    const cd* s = src + (e / nbm) * sa + (e % nbm) * sb;
    const int64_t k0 = (int64_t)g * npts / G, k1 = (int64_t)(g + 1) * npts / G;
    int ra[3] = {0, 0, 0}, p[3] = {0, 0, 0}, i[3] = {0, 0, 0}, o[3] = {0, 0, 0};
    wan_decode(Mh, k0, i);
    for (int d = 0, off = 0; d < Mh.dk; ++d) {
        ra[d] = ((R[r * 3 + d] % Mh.N[d]) + Mh.N[d]) % Mh.N[d];
        p[d] = (int)(((int64_t)i[d] * ra[d]) % Mh.N[d]);
        o[d] = off;
        off += Mh.N[d];
    }
    cd acc{0.0, 0.0};
    for (int64_t k = k0; k < k1; ++k) {
        cd ph = tw[o[0] + p[0]];
        if (Mh.dk > 1) ph = cmul_x(ph, tw[o[1] + p[1]]);
        if (Mh.dk > 2) ph = cmul_x(ph, tw[o[2] + p[2]]);
        if (sign > 0) ph.y = -ph.y;
        cfma_x(acc, ph, s[k * kstride]);
        for (int d = Mh.dk - 1; d >= 0; --d) {                     // the next point: the last axis runs fastest
            if (++i[d] < Mh.N[d]) {
                p[d] += ra[d];
                if (p[d] >= Mh.N[d]) p[d] -= Mh.N[d];
                break;
            }
            i[d] = 0, p[d] = 0;
        }
    }
    if (G == 1) {
        const double inv = 1.0 / (double)npts;
        out[id] = cd{acc.x * inv, acc.y * inv};
    } else {
        part[(int64_t)g * tot + id] = acc;
    }
}
__global__ __launch_bounds__(256) void k_wan_fourier_sum(const int64_t npts, const int64_t tot, const int G, const cd* __restrict__ part,
                                                         cd* __restrict__ out) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= tot) return;
    cd acc{0.0, 0.0};
    for (int g = 0; g < G; ++g) acc = cadd(acc, part[(int64_t)g * tot + id]);
    const double inv = 1.0 / (double)npts;
    out[id] = cd{acc.x * inv, acc.y * inv};
}

// u~(k) <- u~(k) U_acc(k), component j times e^{2 pi i k.tau_j}: one workgroup per point, a lane per component
__global__ __launch_bounds__(256) void k_wan_final(const ModelView mv, const WanMesh Mh, const int nw, const cd* __restrict__ uacc,
                                                   cd* __restrict__ ut) {
    __shared__ cd Ua[SE_NMAX * SE_LD];
    const int t = threadIdx.x, n = mv.nsta, nw2 = nw * nw;
    const int64_t k = blockIdx.x;
    int ii[3];
    wan_decode(Mh, k, ii);
    double kd[3] = {0.0, 0.0, 0.0};
    for (int d = 0; d < Mh.dk; ++d) kd[d] = (double)ii[d] / (double)Mh.N[d];
    for (int e = t; e < nw2; e += 256) Ua[(e / nw) * SE_LD + e % nw] = uacc[k * nw2 + e];
    __syncthreads();
    for (int j = t; j < n; j += 256) {
        cd v[WAN_NW_MAX];
#pragma unroll
        for (int m = 0; m < WAN_NW_MAX; ++m) v[m] = m < nw ? ut[(k * nw + m) * n + j] : cd{0.0, 0.0};
        const double4 o = mv.orb[j];
        const cd ph = wan_expi2pi(kd[0] * o.x + kd[1] * o.y + kd[2] * o.z);
        for (int c = 0; c < nw; ++c) {
            cd a{0.0, 0.0};
#pragma unroll
            for (int m = 0; m < WAN_NW_MAX; ++m)
                if (m < nw) cfma_x(a, v[m], Ua[m * SE_LD + c]);
            ut[(k * nw + c) * n + j] = cmul_x(a, ph);
        }
    }
}

__global__ __launch_bounds__(256) void k_wan_identity(const int64_t npts, const int nw, cd* __restrict__ uacc) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= npts * nw * nw) return;
    const int e = (int)(id % (nw * nw));
    uacc[id] = cd{e / nw == e % nw ? 1.0 : 0.0, 0.0};
}

// ---------------------------------------------------------------- host side
namespace {
struct WanRun {
    tbk_ctx* ctx;
    WanPlan pl;
    WanMesh M;
    WanSteps St;
    unsigned char* base;
    template <class T>
    T* buf(int i) const { return (T*)(base + pl.off[i]); }
};

// the two spread passes of the state in M; Omega lands in hist[it]
int wan_spread(const WanRun& S, int it) {
    const WanPlan& p = S.pl;
    hipStream_t st = S.ctx->stream;
    ProfScope ps(S.ctx, "wan_spread");
    hipLaunchKernelGGL(k_wan_sum<1>, dim3(p.G), dim3(128), 0, st, p.npts, p.nbv, p.nw, p.G, (const cd*)S.buf<cd>(WanPlan::MOV),
                       (const double*)nullptr, S.buf<double>(WanPlan::PART));
    hipLaunchKernelGGL(k_wan_fin1, dim3(1), dim3(128), 0, st, p.npts, p.nbv, p.nw, p.G, (const double*)S.buf<double>(WanPlan::PART),
                       (const double*)S.buf<double>(WanPlan::BW), (const double*)S.buf<double>(WanPlan::BGRAM), S.buf<double>(WanPlan::S1),
                       S.buf<double>(WanPlan::CB));
    hipLaunchKernelGGL(k_wan_sum<2>, dim3(p.G), dim3(128), 0, st, p.npts, p.nbv, p.nw, p.G, (const cd*)S.buf<cd>(WanPlan::MOV),
                       (const double*)S.buf<double>(WanPlan::CB), S.buf<double>(WanPlan::PART));
    hipLaunchKernelGGL(k_wan_fin2, dim3(1), dim3(128), 0, st, p.npts, p.nbv, p.nw, p.G, (const double*)S.buf<double>(WanPlan::PART),
                       (const double*)S.buf<double>(WanPlan::BW), (const double*)S.buf<double>(WanPlan::S1),
                       (const double*)S.buf<double>(WanPlan::CB), it, S.buf<double>(WanPlan::FIN), S.buf<double>(WanPlan::HIST),
                       S.buf<double>(WanPlan::DHIST));
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}
// the Fourier sum of src over the mesh for the nR lattice vectors, ne entries each, in wan_fourier_groups k-groups
int wan_fourier(const WanRun& S, int sign, int nR, int ne, int nbm, int64_t sa, int64_t sb, int64_t kstride, const cd* src, cd* out) {
    const WanPlan& p = S.pl;
    hipStream_t st = S.ctx->stream;
    const int64_t tot = (int64_t)nR * ne;
    const int G = wan_fourier_groups(p.npts, tot);
    hipLaunchKernelGGL(k_wan_fourier, dim3(nblk(tot), (unsigned)G), dim3(256), 0, st, S.M, p.npts, nR, (const int32_t*)S.buf<int32_t>(WanPlan::RDEV),
                       (const cd*)S.buf<cd>(WanPlan::TW), sign, ne, nbm, sa, sb, kstride, src, G, S.buf<cd>(WanPlan::FPART), out);
    if (G > 1)
        hipLaunchKernelGGL(k_wan_fourier_sum, dim3(nblk(tot)), dim3(256), 0, st, p.npts, tot, G, (const cd*)S.buf<cd>(WanPlan::FPART), out);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}
int wan_step(const WanRun& S) {
    const WanPlan& p = S.pl;
    hipStream_t st = S.ctx->stream;
    ProfScope ps(S.ctx, "wan_step");
    hipLaunchKernelGGL(k_wan_grad, dim3((unsigned)p.npts), dim3(64), 0, st, S.M, S.St, p.nw, (const cd*)S.buf<cd>(WanPlan::MOV),
                       (const double*)S.buf<double>(WanPlan::CB), S.buf<cd>(WanPlan::EXPW), S.buf<cd>(WanPlan::UACC));
    hipLaunchKernelGGL(k_wan_mupdate, dim3((unsigned)(p.npts * p.nbv)), dim3(64), 0, st, S.M, S.St, p.nw, (const cd*)S.buf<cd>(WanPlan::EXPW),
                       S.buf<cd>(WanPlan::MOV));
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}
// the workspace block: freed behind a synchronisation when the call returns, whichever way
struct WanBlock {
    hipStream_t st;
    void* blk = nullptr;
    ~WanBlock() {
        if (blk) {
            hipStreamSynchronize(st);
            hipFree(blk);
        }
    }
    int alloc(const char* fn, size_t bytes) {
        hipError_t e = hipMalloc(&blk, bytes);
        if (e != hipSuccess) {
            blk = nullptr;
            tbk_set_error("%s: hipMalloc(%zu) for the workspace: %s", fn, bytes, hipGetErrorString(e));
            return TBK_ENOMEM;
        }
        return TBK_OK;
    }
};
WanRun wan_run(tbk_model* m, const int32_t* mesh, const WanPlan& pl, const WanArgs& A) {
    WanRun S{};
    const int dk = m->dim_k;
    S.ctx = m->ctx;
    S.pl = pl;
    S.M = WanMesh{{1, 1, 1}, dk};
    for (int d = 0; d < dk; ++d) S.M.N[d] = mesh[d];
    S.St.nbv = A.nbv;
    for (int i = 0; i < WAN_BV_MAX; ++i) {
        S.St.w[i] = i < A.nbv ? A.bw[i] : 0.0;
        for (int d = 0; d < 3; ++d) S.St.s[i][d] = i < A.nbv && d < dk ? A.bstep[i * dk + d] : 0;
    }
    return S;
}
// the small tables of a call, uploaded
int wan_tables(const WanRun& S, tbk_model* m, const int32_t* mesh, const WanArgs& A) {
    const WanPlan& p = S.pl;
    hipStream_t st = S.ctx->stream;
    const int dk = m->dim_k, n = m->nsta, nb = A.nb, nw = A.nw, nbv = A.nbv, nR = A.nR;
    const int64_t nterm = A.nterm;
    int rc;
    std::vector<int32_t> trv((size_t)nterm * 3, 0), rdev((size_t)nR * 3, 0);
    for (int64_t t = 0; t < nterm; ++t)
        for (int d = 0; d < dk; ++d) trv[3 * t + d] = A.term_R[t * dk + d];
    for (int64_t r = 0; r < nR; ++r)
        for (int d = 0; d < dk; ++d) rdev[3 * r + d] = A.R[r * dk + d];
    std::vector<double4> orb((size_t)n);
    TBK_HIP(hipMemcpyAsync(orb.data(), m->view.orb, (size_t)n * sizeof(double4), hipMemcpyDeviceToHost, st));
    TBK_HIP(hipStreamSynchronize(st));
    const double twopi = 6.283185307179586476925286766559;
    std::vector<cd> phase((size_t)3 * n, cd{1.0, 0.0}), tw;
    for (int j = 0; j < n; ++j) {
        const double o[3] = {orb[j].x, orb[j].y, orb[j].z};
        for (int d = 0; d < dk; ++d) phase[(size_t)d * n + j] = cd{cos(twopi * o[d]), -sin(twopi * o[d])};   // e^{-2 pi i tau_j[d]}
    }
    for (int d = 0; d < dk; ++d)
        for (int q = 0; q < mesh[d]; ++q) tw.push_back(cd{cos(twopi * q / mesh[d]), -sin(twopi * q / mesh[d])});
    auto up = [&](int i, const void* src, size_t bytes) -> int {
        if (bytes) TBK_HIP(hipMemcpyAsync(S.base + p.off[i], src, bytes, hipMemcpyHostToDevice, st));
        return TBK_OK;
    };
    if ((rc = up(WanPlan::BANDS, A.bands, (size_t)nb * sizeof(int32_t)))) return rc;
    if ((rc = up(WanPlan::TPTR, A.term_ptr, (size_t)(nw + 1) * sizeof(int32_t)))) return rc;
    if ((rc = up(WanPlan::TSTATE, A.term_state, (size_t)nterm * sizeof(int32_t)))) return rc;
    if ((rc = up(WanPlan::TRV, trv.data(), trv.size() * sizeof(int32_t)))) return rc;
    if ((rc = up(WanPlan::TAMP, A.term_amp, (size_t)nterm * sizeof(cd)))) return rc;
    if ((rc = up(WanPlan::PHASE, phase.data(), phase.size() * sizeof(cd)))) return rc;
    if ((rc = up(WanPlan::BW, A.bw, (size_t)nbv * sizeof(double)))) return rc;
    if ((rc = up(WanPlan::BGRAM, A.bgram, (size_t)nbv * nbv * sizeof(double)))) return rc;
    if ((rc = up(WanPlan::TW, tw.data(), tw.size() * sizeof(cd)))) return rc;
    if ((rc = up(WanPlan::RDEV, rdev.data(), rdev.size() * sizeof(int32_t)))) return rc;
    TBK_HIP(hipStreamSynchronize(st));                              // (the host vectors above go out of use)
    return TBK_OK;
}
// the smallest singular value of the projection over the mesh, into sums[4 + WAN_NW_MAX]; below kWanSvMin the call ends here
int wan_sv_check(const char* fn, const WanRun& S, int dk, const int32_t* mesh, double* sums) {
    const int64_t npts = S.pl.npts;
    hipStream_t st = S.ctx->stream;
    std::vector<double> sv((size_t)npts);
    TBK_HIP(hipMemcpyAsync(sv.data(), S.buf<double>(WanPlan::SVK), (size_t)npts * sizeof(double), hipMemcpyDeviceToHost, st));
    TBK_HIP(hipStreamSynchronize(st));
    int64_t at = 0;
    for (int64_t k = 0; k < npts; ++k) {
        TBK_REQUIRE(std::isfinite(sv[k]), TBK_ENOCONV, "%s: the projection at mesh point %lld is not finite", fn, (long long)k);
        if (sv[k] < sv[at]) at = k;
    }
    sums[4 + WAN_NW_MAX] = sv[at];
    if (sv[at] < kWanSvMin) {
        int i[3] = {0, 0, 0};
        int64_t idx = at;
        for (int d = dk - 1; d >= 0; --d) i[d] = (int)(idx % mesh[d]), idx /= mesh[d];
        char where[96];
        int len = 0;
        for (int d = 0; d < dk; ++d) len += snprintf(where + len, sizeof where - len, d ? ", %d/%d" : "%d/%d", i[d], mesh[d]);
        tbk_set_error("%s: trial functions are singular on the bands at k = (%s): smallest singular value %.3g", fn, where, sv[at]);
        return TBK_EINVAL;
    }
    return TBK_OK;
}
// the descent from the overlaps in MOV (U_acc the identity): the spread of the start, then up to max_iter steps
int wan_descend(const char* fn, const WanRun& S, int max_iter, double tol, int check_every, int& iterations, int& converged) {
    hipStream_t st = S.ctx->stream;
    int rc;
    if ((rc = wan_spread(S, 0))) return rc;
    iterations = 0, converged = 0;
    for (int it = 1; it <= max_iter; ++it) {
        if ((rc = wan_step(S))) return rc;
        if ((rc = wan_spread(S, it))) return rc;
        iterations = it;
        if (it % check_every != 0 && it != max_iter) continue;
        double d = 0.0;                                             // the check: one 8-byte copy behind a synchronisation
        TBK_HIP(hipMemcpyAsync(&d, S.buf<double>(WanPlan::DHIST) + it, sizeof(double), hipMemcpyDeviceToHost, st));
        TBK_HIP(hipStreamSynchronize(st));
        TBK_REQUIRE(std::isfinite(d), TBK_ENOCONV, "%s: the spread of iteration %d is not finite", fn, it);
        if (tol > 0.0 && fabs(d) < tol) {
            converged = 1;
            break;
        }
    }
    return TBK_OK;
}
// the Wannier Hamiltonian, on request the functions, and the downloads
int wan_finish(const WanRun& S, tbk_model* m, int nR, int iterations, double* hop, double* sums, double* hist, double* functions_or_null,
               double* gauge_or_null) {
    const WanPlan& p = S.pl;
    tbk_ctx* ctx = S.ctx;
    hipStream_t st = ctx->stream;
    const int n = p.n, nb = p.nb, nw = p.nw, nbv = p.nbv;
    const int64_t npts = p.npts;
    int rc;
    {
        ProfScope ps(ctx, "wan_model");
        hipLaunchKernelGGL(k_wan_hw, dim3((unsigned)npts), dim3(64), 0, st, nb, nw, (const double*)S.buf<double>(WanPlan::EB), S.buf<cd>(WanPlan::U0),
                           (const cd*)S.buf<cd>(WanPlan::UACC), S.buf<cd>(WanPlan::HW));
        const int nw2 = nw * nw;
        if ((rc = wan_fourier(S, -1, nR, nw2, nw2, 0, 1, nw2, S.buf<cd>(WanPlan::HW), S.buf<cd>(WanPlan::HOP)))) return rc;
        if (functions_or_null) {
            hipLaunchKernelGGL(k_wan_final, dim3((unsigned)npts), dim3(256), 0, st, m->view, S.M, nw, (const cd*)S.buf<cd>(WanPlan::UACC),
                               S.buf<cd>(WanPlan::UT));
            TBK_HIP(hipGetLastError());
            // out (nR, nsta, nw): e = j nw + c reads u~[k][c][j]
            if ((rc = wan_fourier(S, 1, nR, n * nw, nw, 1, n, (int64_t)nw * n, S.buf<cd>(WanPlan::UT), S.buf<cd>(WanPlan::FN)))) return rc;
        }
    }
    TBK_HIP(hipMemcpyAsync(hop, S.buf<cd>(WanPlan::HOP), (size_t)nR * nw * nw * sizeof(cd), hipMemcpyDeviceToHost, st));
    TBK_HIP(hipMemcpyAsync(sums, S.buf<double>(WanPlan::FIN), (size_t)(4 + nw) * sizeof(double), hipMemcpyDeviceToHost, st));
    TBK_HIP(hipMemcpyAsync(sums + 5 + WAN_NW_MAX, S.buf<double>(WanPlan::S1), (size_t)nw * nbv * sizeof(double), hipMemcpyDeviceToHost, st));
    TBK_HIP(hipMemcpyAsync(hist, S.buf<double>(WanPlan::HIST), (size_t)(iterations + 1) * sizeof(double), hipMemcpyDeviceToHost, st));
    if (functions_or_null)
        TBK_HIP(hipMemcpyAsync(functions_or_null, S.buf<cd>(WanPlan::FN), (size_t)nR * n * nw * sizeof(cd), hipMemcpyDeviceToHost, st));
    if (gauge_or_null)
        TBK_HIP(hipMemcpyAsync(gauge_or_null, S.buf<cd>(WanPlan::U0), (size_t)npts * nb * nw * sizeof(cd), hipMemcpyDeviceToHost, st));
    TBK_HIP(hipStreamSynchronize(st));
    return TBK_OK;
}
}  // namespace

extern "C" int tbk_wannier_mesh(tbk_model* m, const int32_t* mesh, int nb, const int32_t* bands, int nw, int64_t nterm,
                                const int32_t* term_ptr, const int32_t* term_state, const int32_t* term_R, const double* term_amp, int nbv,
                                const int32_t* bstep, const double* bw, const double* bgram, int max_iter, double tol, int check_every,
                                int nR, int r_user, const int32_t* R, double* hop, double* sums, double* hist, double* functions_or_null,
                                double* gauge_or_null, int32_t* info) {
    const char* fn = "tbk_wannier_mesh";
    TBK_REQUIRE(m && hop && sums && hist && info, TBK_EINVAL, "%s: null argument", fn);
    const int dk = m->dim_k, n = m->nsta;
    WanArgs A;
    A.nb = nb, A.nw = nw, A.bands = bands, A.nterm = nterm, A.term_ptr = term_ptr, A.term_state = term_state, A.term_R = term_R;
    A.term_amp = term_amp, A.nbv = nbv, A.bstep = bstep, A.bw = bw, A.bgram = bgram, A.max_iter = max_iter, A.tol = tol;
    A.check_every = check_every, A.nR = nR, A.r_user = r_user, A.R = R, A.want_fn = functions_or_null ? 1 : 0;
    int64_t npts;
    int rc = wan_check(fn, dk, n, mesh, A, npts);
    if (rc) return rc;
    tbk_ctx* ctx = m->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;

    WanRun S = wan_run(m, mesh, wan_plan(n, dk, npts, mesh, nb, nw, nbv, nterm, max_iter, nR, A.want_fn), A);
    const WanPlan& p = S.pl;
    WanBlock guard{st};
    if ((rc = guard.alloc(fn, p.total))) return rc;
    S.base = (unsigned char*)guard.blk;
    if ((rc = wan_tables(S, m, mesh, A))) return rc;

    // the solve, the projection and the rotation, chunk by chunk
    KuboChunks cw = p.cw;
    cw.base = S.base + p.off[WanPlan::CHUNKS];
    rc = kubo_for_chunks(m, cw, nullptr, mesh, npts, [&](int64_t first, int64_t cnt, const double*, const double* ec, const cd* vc) -> int {
        ProfScope ps(ctx, "wan_project");
        hipLaunchKernelGGL(k_wan_project, dim3((unsigned)cnt), dim3(64), 0, st, m->view, S.M, first, cnt, vc, ec,
                           (const int32_t*)S.buf<int32_t>(WanPlan::BANDS), nb, nw, (const int32_t*)S.buf<int32_t>(WanPlan::TPTR),
                           (const int32_t*)S.buf<int32_t>(WanPlan::TSTATE), (const int32_t*)S.buf<int32_t>(WanPlan::TRV),
                           (const cd*)S.buf<cd>(WanPlan::TAMP), S.buf<cd>(WanPlan::U0), S.buf<double>(WanPlan::EB), S.buf<double>(WanPlan::SVK));
        hipLaunchKernelGGL(k_wan_rotate, dim3((unsigned)((cnt + p.P - 1) / p.P)), dim3(256), 0, st, n, first, cnt, p.P, vc,
                           (const int32_t*)S.buf<int32_t>(WanPlan::BANDS), nb, nw, (const cd*)S.buf<cd>(WanPlan::U0), S.buf<cd>(WanPlan::UT));
        TBK_HIP(hipGetLastError());
        return TBK_OK;
    });
    if (rc) return rc;
    if ((rc = wan_sv_check(fn, S, dk, mesh, sums))) return rc;

    // the overlaps, the spread of the projection and the descent
    {
        ProfScope ps(ctx, "wan_overlap");
        const int64_t nitems = npts * nbv;
        hipLaunchKernelGGL(k_wan_overlap, dim3((unsigned)((nitems + p.Q - 1) / p.Q)), dim3(256), 0, st, S.M, S.St, n, nw, p.Q, nitems,
                           (const cd*)S.buf<cd>(WanPlan::UT), (const cd*)S.buf<cd>(WanPlan::PHASE), S.buf<cd>(WanPlan::MOV));
        hipLaunchKernelGGL(k_wan_identity, dim3(nblk(npts * nw * nw)), dim3(256), 0, st, npts, nw, S.buf<cd>(WanPlan::UACC));
        TBK_HIP(hipGetLastError());
    }
    int iterations = 0, converged = 0;
    if ((rc = wan_descend(fn, S, max_iter, tol, check_every, iterations, converged))) return rc;
    if ((rc = wan_finish(S, m, nR, iterations, hop, sums, hist, functions_or_null, gauge_or_null))) return rc;
    info[0] = iterations;
    info[1] = converged;
    info[2] = p.P;
    info[3] = p.Q;
    info[4] = p.G;
    return TBK_OK;
}

// the disentanglement entry shares this translation unit: it runs the spread, descent, model and Fourier kernels above unchanged
#include "tbk_wdis.hip"
