// tbk_wdis.hip -- disentangled Wannier functions with energy windows on uniform k meshes (Souza, Marzari and Vanderbilt, PRB 65,
// 035109).  Included at the end of tbk_wan.hip: the two entries are one translation unit, and this one runs the
// spread, descent, model and Fourier kernels of section 34 unchanged.
//
// The mesh goes through the solver once, in tbk_kubo.h's chunks with eigenvectors; per chunk
//   k_wdis_project  one wavefront per point: A = V_bands+ g~ over all nb candidate bands (k_wan_project's arithmetic), the eigenvalues
//   k_wdis_gather   the nb candidate eigenvectors of every point into V_bands[N_k][nb][nsta], which stays resident
// then, with nothing left of the solver's output,
//   k_wdis_mask     a lane per point: the window and frozen masks (a bit per band) and their counts; the host reads the counts once
//   k_wdis_overlap  M0(k, b) = V_bands(k)+ D_G V_bands(k + b), one (point, b) item per workgroup, both sides staged through LDS in
//                   tiles of 32 components (rows of 33), the neighbour multiplied by e^{-2 pi i G.tau_j} on the way in
//   k_wdis_select<1>  one wavefront per point: U = A (A+ A)^-1/2 with the rows outside the window zero, P = U U+, the selection below
// per iteration of the disentanglement, all in stream order:
//   k_wdis_select<0>  one wavefront per point: Z = sum_{+-b} w_b T T+, T = M0(k, +-b) U_dis(k +- b) from the previous iteration's
//                   buffer (M0(k, -b) = M0(k - b, b)+), the b-vectors in list order, + before -; Z_in = alpha Z + (1 - alpha) Z_in
//                   when alpha < 1; Z compacted to the free indices (in the window, not frozen), small_eig_jacobi32, the
//                   nw - n_frozen largest eigenvalues (ties to the lower index) behind the frozen unit vectors into the other buffer
//   k_wdis_reduce   one wavefront per (point, b): U_dis(k)+ M0(k, b) U_dis(k + b) into section 34's M
//   k_wdis_osum, k_wdis_ofin   Omega_I by k_wan_sum's groups and slices, as 1 - sum_m |M_mn|^2 per column, into dis_history[it]
// At a check the host reads the change of Omega_I of that iteration (8 bytes).  At the end
//   k_wdis_gauge    one wavefront per point: A' = U_dis+ A, its smallest singular value, U0 = U_dis A' (A'+ A')^-1/2
//   k_wdis_reduce   M(k, b) = U0(k)+ M0(k, b) U0(k + b): no second pass over the states
//   k_wdis_rotate   (with the functions) u~ = V_bands U0
// and section 34 takes over.  No atomics; every sum in a fixed order over a partition that depends on (mesh, nsta, nb, nw, nbv) alone.
#include "tbk_wdis.h"

// ---------------------------------------------------------------- per chunk
__global__ __launch_bounds__(64) void k_wdis_project(const ModelView mv, const WanMesh Mh, const int64_t first, const int64_t cnt,
                                                     const cd* __restrict__ evec, const double* __restrict__ eval,
                                                     const int32_t* __restrict__ bands, const int nb, const int nw,
                                                     const int32_t* __restrict__ tptr, const int32_t* __restrict__ tstate,
                                                     const int32_t* __restrict__ trv, const cd* __restrict__ tamp, cd* __restrict__ AM,
                                                     double* __restrict__ EB) {
    const int t = threadIdx.x, n = mv.nsta;
    const int64_t kl = blockIdx.x, kk = first + kl;
    int ii[3];
    wan_decode(Mh, kk, ii);
    double kd[3] = {0.0, 0.0, 0.0};
    for (int d = 0; d < Mh.dk; ++d) kd[d] = (double)ii[d] / (double)Mh.N[d];
    for (int e = t; e < nb * nw; e += 64) {
        const int b = e / nw, w = e % nw;
        const cd* v = evec + ((int64_t)bands[b] * cnt + kl) * n;
        cd acc{0.0, 0.0};
        for (int q = tptr[w]; q < tptr[w + 1]; ++q) {
            const int j = tstate[q];
            const double4 o = mv.orb[j];
            const double x = kd[0] * ((double)trv[3 * q] + o.x) + kd[1] * ((double)trv[3 * q + 1] + o.y) + kd[2] * ((double)trv[3 * q + 2] + o.z);
            cfmac_x(acc, cmul_x(tamp[q], wan_expi2pi(-x)), v[j]);
        }
        AM[kk * nb * nw + e] = acc;
    }
    for (int b = t; b < nb; b += 64) EB[kk * nb + b] = eval[(int64_t)bands[b] * cnt + kl];
}

__global__ __launch_bounds__(256) void k_wdis_gather(const int n, const int64_t first, const int64_t cnt, const cd* __restrict__ evec,
                                                     const int32_t* __restrict__ bands, const int nb, cd* __restrict__ VB) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= cnt * nb * n) return;
    const int j = (int)(id % n), b = (int)((id / n) % nb);
    const int64_t kl = id / ((int64_t)n * nb);
    VB[((first + kl) * nb + b) * n + j] = evec[((int64_t)bands[b] * cnt + kl) * n + j];
}

// ---------------------------------------------------------------- the masks
__global__ __launch_bounds__(256) void k_wdis_mask(const int64_t npts, const int nb, const double* __restrict__ EB, const int have_window,
                                                   const double wlo, const double whi, const int have_frozen, const double flo,
                                                   const double fhi, uint32_t* __restrict__ win, uint32_t* __restrict__ frz,
                                                   int32_t* __restrict__ nwin, int32_t* __restrict__ nfrz) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= npts) return;
    uint32_t mw = 0, mf = 0;
    for (int b = 0; b < nb; ++b) {
        const double e = EB[k * nb + b];
        const bool in = !have_window || (e >= wlo && e <= whi);
        if (in) mw |= 1u << b;
        if (in && have_frozen && e >= flo && e <= fhi) mf |= 1u << b;
    }
    win[k] = mw, frz[k] = mf;
    nwin[k] = __popc(mw), nfrz[k] = __popc(mf);
}

// ---------------------------------------------------------------- M0: one (point, b) item per workgroup, lane t owns entries t + 256 i
__global__ __launch_bounds__(256) void k_wdis_overlap(const WanMesh Mh, const WanSteps St, const int n, const int nb,
                                                      const cd* __restrict__ VB, const cd* __restrict__ phase, cd* __restrict__ M0) {
    __shared__ cd tile[WDIS_OV_ROWS][WDIS_OV_TJ + 1];
    const int t = threadIdx.x, nb2 = nb * nb;
    const int64_t item = blockIdx.x, k = item / St.nbv;
    const int ib = (int)(item % St.nbv);
    int G[3] = {0, 0, 0};
    const int64_t k2 = wan_neighbour(Mh, k, St.s[ib], G);
    cd acc[WDIS_OV_EPL];
#pragma unroll
    for (int i = 0; i < WDIS_OV_EPL; ++i) acc[i] = cd{0.0, 0.0};
    for (int j0 = 0; j0 < n; j0 += WDIS_OV_TJ) {
        for (int e = t; e < 2 * nb * WDIS_OV_TJ; e += 256) {
            const int jj = e % WDIS_OV_TJ, row = e / WDIS_OV_TJ, j = j0 + jj;
            cd v{0.0, 0.0};
            if (j < n) {
                if (row < nb) {
                    v = VB[(k * nb + row) * n + j];
                } else {
                    v = VB[(k2 * nb + (row - nb)) * n + j];
                    for (int d = 0; d < Mh.dk; ++d)
                        if (G[d]) v = cmul_x(v, G[d] > 0 ? phase[d * n + j] : cconj(phase[d * n + j]));
                }
            }
            tile[row][jj] = v;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < WDIS_OV_EPL; ++i) {
            const int e = t + 256 * i;
            if (e >= nb2) continue;
            const cd* a = tile[e / nb];
            const cd* b = tile[nb + e % nb];
#pragma unroll 8
            for (int jj = 0; jj < WDIS_OV_TJ; ++jj) cfmac_x(acc[i], b[jj], a[jj]);   // conj(u_m(k)) u_n(k + b)
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < WDIS_OV_EPL; ++i) {
        const int e = t + 256 * i;
        if (e < nb2) M0[item * nb2 + e] = acc[i];
    }
}

// ---------------------------------------------------------------- the selection: one wavefront
// Z (Hermitian, nb x nb in rows of SE32_LD, written, a barrier passed) -> U_dis(k) (nb x nw): the frozen unit vectors in band order,
// then the eigenvectors of Z on the free indices with the nsel = nw - n_frozen largest eigenvalues, the largest first, ties to the
// lower index of the solver's output.  Nothing rejected (nsel = n_free): the free unit vectors, no eigen-solve.  gap: the last
// selected eigenvalue minus the first rejected one, infinity where nothing is selected or nothing rejected.
__device__ __forceinline__ void wdis_select(const cd* Z, cd* Qm, cd* Zc, double* W, double* lam, int* ix, const uint32_t win,
                                            const uint32_t frz, const int nb, const int nw, const int t, cd* __restrict__ ud,
                                            double* __restrict__ gap) {
    int* fidx = ix;                       // free position -> band
    int* pos = ix + SE32_NMAX;            // band -> free position, -1
    int* fz = ix + 2 * SE32_NMAX;         // frozen position -> band
    int* sel = ix + 3 * SE32_NMAX;        // rank -> column of Q
    const uint32_t fr = win & ~frz;
    const int nf = __popc(frz), nfree = __popc(fr), nsel = nw - nf;
    const bool solve = nsel > 0 && nsel < nfree;
    if (t == 0) {
        int a = 0, c = 0;
        for (int b = 0; b < nb; ++b) {
            pos[b] = -1;
            if ((fr >> b) & 1u) fidx[a] = b, pos[b] = a++;
            if ((frz >> b) & 1u) fz[c++] = b;
        }
    }
    __syncthreads();
    double g = INFINITY;
    if (solve) {
        for (int e = t; e < nfree * nfree; e += 64) Zc[(e / nfree) * SE32_LD + e % nfree] = Z[fidx[e / nfree] * SE32_LD + fidx[e % nfree]];
        __syncthreads();
        small_eig_jacobi32(Zc, Qm, W, nfree, t, 64);
        if (t < nfree) lam[t] = Zc[t * SE32_LD + t].x;
        __syncthreads();
        if (t < nfree) {
            int r = 0;
            for (int j = 0; j < nfree; ++j) r += (lam[j] > lam[t] || (lam[j] == lam[t] && j < t)) ? 1 : 0;
            sel[r] = t;
        }
        __syncthreads();
        g = lam[sel[nsel - 1]] - lam[sel[nsel]];
    }
    if (t == 0) *gap = g;
    for (int e = t; e < nb * nw; e += 64) {
        const int b = e / nw, c = e % nw;
        cd v{0.0, 0.0};
        if (c < nf) {
            if (fz[c] == b) v.x = 1.0;
        } else if (pos[b] >= 0) {
            if (solve) v = Qm[pos[b] * SE32_LD + sel[c - nf]];
            else if (pos[b] == c - nf) v.x = 1.0;
        }
        ud[e] = v;
    }
}

// START: the subspace of the projection; else one iteration.  ud_in | ud_out: the two U_dis buffers; zin: Z_in or null (alpha = 1)
template <int START>
__global__ __launch_bounds__(64) void k_wdis_select(const WanMesh Mh, const WanSteps St, const int nb, const int nw, const cd* __restrict__ AM,
                                                    const cd* __restrict__ M0, const cd* __restrict__ ud_in, cd* __restrict__ ud_out,
                                                    cd* __restrict__ zin, const int first_iter, const double alpha,
                                                    const uint32_t* __restrict__ win, const uint32_t* __restrict__ frz,
                                                    double* __restrict__ gap, double* __restrict__ svp) {
    __shared__ cd bA[WDIS_LDS_A], bB[WDIS_LDS_A], bC[WDIS_LDS_C];
    __shared__ double W[SE32_W], lam[SE32_NMAX];
    __shared__ int ix[4 * SE32_NMAX];
    const int t = threadIdx.x, nb2 = nb * nb, bw = nb * nw;
    const int64_t k = blockIdx.x;
    const uint32_t mw = win[k], mf = frz[k];
    cd* P0 = bC;                                                   // two nb x nw panels in rows of SE_LD
    cd* P1 = bC + WAN_NB_MAX * SE_LD;
    if (START) {
        cd *S = bB, *Qs = bB + SE_NMAX * SE_LD, *X = bB + 2 * SE_NMAX * SE_LD;
        for (int e = t; e < bw; e += 64) {
            const int b = e / nw, w = e % nw;
            P0[b * SE_LD + w] = (mw >> b) & 1u ? AM[k * bw + e] : cd{0.0, 0.0};
        }
        __syncthreads();
        for (int e = t; e < nw * nw; e += 64) {
            const int r = e / nw, c = e % nw;
            cd acc{0.0, 0.0};
            if (r <= c) {
                for (int b = 0; b < nb; ++b) cfmac_x(acc, P0[b * SE_LD + c], P0[b * SE_LD + r]);
                if (r == c) acc.y = 0.0;
                S[r * SE_LD + c] = acc;
                if (r != c) S[c * SE_LD + r] = cconj(acc);
            }
        }
        __syncthreads();
        small_eig_jacobi(S, Qs, nw, t, 64);
        double lmin = S[0].x;
        for (int j = 1; j < nw; ++j) lmin = fmin(lmin, S[j * SE_LD + j].x);
        if (t == 0) svp[k] = sqrt(fmax(lmin, 0.0));
        for (int e = t; e < nw * nw; e += 64) {
            const int r = e / nw, c = e % nw;
            cd acc{0.0, 0.0};
            for (int j = 0; j < nw; ++j) {
                const double l = S[j * SE_LD + j].x;
                const double li = l > 1e-300 ? 1.0 / sqrt(l) : 0.0;
                cfma_x(acc, cscale(Qs[r * SE_LD + j], li), cconj(Qs[c * SE_LD + j]));
            }
            X[r * SE_LD + c] = acc;
        }
        __syncthreads();
        for (int e = t; e < bw; e += 64) {
            const int b = e / nw, w = e % nw;
            cd acc{0.0, 0.0};
            for (int m = 0; m < nw; ++m) cfma_x(acc, P0[b * SE_LD + m], X[m * SE_LD + w]);
            P1[b * SE_LD + w] = acc;
        }
        __syncthreads();
        for (int e = t; e < nb2; e += 64) {                         // P = U U+, (m, n) and (n, m) from the same instructions
            const int r = e / nb, c = e % nb;
            if (r > c) continue;
            cd acc{0.0, 0.0};
            for (int w = 0; w < nw; ++w) cfmac_x(acc, P1[r * SE_LD + w], P1[c * SE_LD + w]);   // conj(U_cw) U_rw
            if (r == c) acc.y = 0.0;
            bA[r * SE32_LD + c] = acc;
            if (r != c) bA[c * SE32_LD + r] = cconj(acc);
        }
        __syncthreads();
    } else {
        for (int e = t; e < nb2; e += 64) bA[(e / nb) * SE32_LD + e % nb] = cd{0.0, 0.0};
        for (int ib = 0; ib < St.nbv; ++ib) {
            for (int side = 0; side < 2; ++side) {
                int G[3], s[3] = {St.s[ib][0], St.s[ib][1], St.s[ib][2]};
                if (side) s[0] = -s[0], s[1] = -s[1], s[2] = -s[2];
                const int64_t kn = wan_neighbour(Mh, k, s, G);
                const cd* pm = M0 + ((side ? kn : k) * St.nbv + ib) * nb2;
                __syncthreads();                                   // (the previous side's reads of bB and bC are done)
                for (int e = t; e < nb2; e += 64) {
                    const int r = e / nb, c = e % nb;
                    if (side) bB[c * SE32_LD + r] = cconj(pm[e]);   // M0(k, -b) = M0(k - b, b)+
                    else bB[r * SE32_LD + c] = pm[e];
                }
                for (int e = t; e < bw; e += 64) P0[(e / nw) * SE_LD + e % nw] = ud_in[kn * bw + e];
                __syncthreads();
                for (int e = t; e < bw; e += 64) {
                    const int m = e / nw, j = e % nw;
                    cd acc{0.0, 0.0};
                    for (int q = 0; q < nb; ++q) cfma_x(acc, bB[m * SE32_LD + q], P0[q * SE_LD + j]);
                    P1[m * SE_LD + j] = acc;
                }
                __syncthreads();
                const double w = St.w[ib];
                for (int e = t; e < nb2; e += 64) {
                    const int r = e / nb, c = e % nb;
                    if (r > c) continue;
                    cd acc{0.0, 0.0};
                    for (int j = 0; j < nw; ++j) cfmac_x(acc, P1[r * SE_LD + j], P1[c * SE_LD + j]);   // T_rj conj(T_cj)
                    if (r == c) acc.y = 0.0;
                    cd z = bA[r * SE32_LD + c];
                    z.x = fma(w, acc.x, z.x), z.y = fma(w, acc.y, z.y);
                    bA[r * SE32_LD + c] = z;
                    if (r != c) bA[c * SE32_LD + r] = cconj(z);
                }
            }
        }
        __syncthreads();
        if (zin) {
            cd* zk = zin + k * nb2;
            for (int e = t; e < nb2; e += 64) {
                cd z = bA[(e / nb) * SE32_LD + e % nb];
                if (!first_iter) {
                    const cd o = zk[e];
                    z = cd{alpha * z.x + (1.0 - alpha) * o.x, alpha * z.y + (1.0 - alpha) * o.y};
                }
                zk[e] = z;
                bA[(e / nb) * SE32_LD + e % nb] = z;
            }
            __syncthreads();
        }
    }
    wdis_select(bA, bB, bC, W, lam, ix, mw, mf, nb, nw, t, ud_out + k * bw, gap + k);
}

// ---------------------------------------------------------------- M(k, b) = Ua(k)+ M0(k, b) Ua(k + b): one wavefront per item
__global__ __launch_bounds__(64) void k_wdis_reduce(const WanMesh Mh, const WanSteps St, const int nb, const int nw, const cd* __restrict__ M0,
                                                    const cd* __restrict__ ua, cd* __restrict__ Mov) {
    __shared__ cd Mm[WDIS_LDS_A], U1[WAN_NB_MAX * SE_LD], U2[WAN_NB_MAX * SE_LD], T[WAN_NB_MAX * SE_LD];
    const int t = threadIdx.x, nb2 = nb * nb, bw = nb * nw, nw2 = nw * nw;
    const int64_t item = blockIdx.x, k = item / St.nbv;
    const int ib = (int)(item % St.nbv);
    int G[3];
    const int64_t k2 = wan_neighbour(Mh, k, St.s[ib], G);
    for (int e = t; e < nb2; e += 64) Mm[(e / nb) * SE32_LD + e % nb] = M0[item * nb2 + e];
    for (int e = t; e < bw; e += 64) {
        U1[(e / nw) * SE_LD + e % nw] = ua[k * bw + e];
        U2[(e / nw) * SE_LD + e % nw] = ua[k2 * bw + e];
    }
    __syncthreads();
    for (int e = t; e < bw; e += 64) {
        const int m = e / nw, j = e % nw;
        cd acc{0.0, 0.0};
        for (int q = 0; q < nb; ++q) cfma_x(acc, Mm[m * SE32_LD + q], U2[q * SE_LD + j]);
        T[m * SE_LD + j] = acc;
    }
    __syncthreads();
    for (int e = t; e < nw2; e += 64) {
        const int i = e / nw, j = e % nw;
        cd acc{0.0, 0.0};
        for (int m = 0; m < nb; ++m) cfmac_x(acc, T[m * SE_LD + j], U1[m * SE_LD + i]);   // conj(U1_mi) T_mj
        Mov[item * nw2 + e] = acc;
    }
}

// ---------------------------------------------------------------- Omega_I: k_wan_sum's groups and slices, k_wan_fin2's order
__global__ __launch_bounds__(128) void k_wdis_osum(const int64_t npts, const int nbv, const int nw, const int G, const cd* __restrict__ Mov,
                                                   double* __restrict__ part) {
    __shared__ double red[128];
    const int t = threadIdx.x, nq = nw * nbv, g = blockIdx.x, nsl = 128 / nq;
    const int q = t % nq, sl = t / nq;
    const int w = q / nbv, ib = q % nbv, nw2 = nw * nw;
    const int64_t k0 = (int64_t)g * npts / G, k1 = (int64_t)(g + 1) * npts / G;
    double s0 = 0.0;
    if (sl < nsl)
        for (int64_t k = k0 + sl; k < k1; k += nsl) {
            const cd* M = Mov + (k * nbv + ib) * nw2;
            double col = 0.0;
            for (int m = 0; m < nw; ++m) col += cabs2(M[m * nw + w]);
            s0 += 1.0 - col;
        }
    red[t] = s0;
    __syncthreads();
    if (t >= nq) return;
    double a = 0.0;
    for (int j = 0; j < nsl; ++j) a += red[j * nq + q];
    part[(int64_t)g * nq + q] = a;
}
__global__ __launch_bounds__(128) void k_wdis_ofin(const int64_t npts, const int nbv, const int nw, const int G, const double* __restrict__ part,
                                                   const double* __restrict__ bw, const int it, double* __restrict__ hist,
                                                   double* __restrict__ dhist) {
    __shared__ double s[WAN_NW_MAX * WAN_BV_MAX];
    const int q = threadIdx.x, nq = nw * nbv;
    if (q < nq) {
        double a = 0.0;
        for (int g = 0; g < G; ++g) a += part[(int64_t)g * nq + q];
        s[q] = a;
    }
    __syncthreads();
    if (q == 0) {
        double oi = 0.0;
        for (int ib = 0; ib < nbv; ++ib) {
            double a0 = 0.0;
            for (int w = 0; w < nw; ++w) a0 += s[w * nbv + ib];
            oi += bw[ib] * a0;
        }
        oi *= 2.0 / (double)npts;
        hist[it] = oi;
        dhist[it] = it > 0 ? oi - hist[it - 1] : 0.0;
    }
}

// ---------------------------------------------------------------- the gauge inside the subspace: one wavefront per point
__global__ __launch_bounds__(64) void k_wdis_gauge(const int nb, const int nw, const cd* __restrict__ AM, const cd* __restrict__ ud,
                                                   const uint32_t* __restrict__ win, cd* __restrict__ U0, double* __restrict__ svk) {
    __shared__ cd Ud[WAN_NB_MAX * SE_LD], Am[WAN_NB_MAX * SE_LD], Ap[SE_NMAX * SE_LD], S[SE_NMAX * SE_LD], Qs[SE_NMAX * SE_LD],
        X[SE_NMAX * SE_LD], Y[SE_NMAX * SE_LD];
    const int t = threadIdx.x, bw = nb * nw, nw2 = nw * nw;
    const int64_t k = blockIdx.x;
    const uint32_t mw = win[k];
    for (int e = t; e < bw; e += 64) {
        const int b = e / nw, w = e % nw;
        Ud[b * SE_LD + w] = ud[k * bw + e];
        Am[b * SE_LD + w] = (mw >> b) & 1u ? AM[k * bw + e] : cd{0.0, 0.0};
    }
    __syncthreads();
    for (int e = t; e < nw2; e += 64) {                             // A' = U_dis+ A
        const int i = e / nw, j = e % nw;
        cd acc{0.0, 0.0};
        for (int b = 0; b < nb; ++b) cfmac_x(acc, Am[b * SE_LD + j], Ud[b * SE_LD + i]);
        Ap[i * SE_LD + j] = acc;
    }
    __syncthreads();
    for (int e = t; e < nw2; e += 64) {
        const int r = e / nw, c = e % nw;
        cd acc{0.0, 0.0};
        if (r <= c) {
            for (int b = 0; b < nw; ++b) cfmac_x(acc, Ap[b * SE_LD + c], Ap[b * SE_LD + r]);
            if (r == c) acc.y = 0.0;
            S[r * SE_LD + c] = acc;
            if (r != c) S[c * SE_LD + r] = cconj(acc);
        }
    }
    __syncthreads();
    small_eig_jacobi(S, Qs, nw, t, 64);
    double lmin = S[0].x;
    for (int j = 1; j < nw; ++j) lmin = fmin(lmin, S[j * SE_LD + j].x);
    if (t == 0) svk[k] = sqrt(fmax(lmin, 0.0));
    for (int e = t; e < nw2; e += 64) {
        const int r = e / nw, c = e % nw;
        cd acc{0.0, 0.0};
        for (int j = 0; j < nw; ++j) {
            const double l = S[j * SE_LD + j].x;
            const double li = l > 1e-300 ? 1.0 / sqrt(l) : 0.0;
            cfma_x(acc, cscale(Qs[r * SE_LD + j], li), cconj(Qs[c * SE_LD + j]));
        }
        X[r * SE_LD + c] = acc;
    }
    __syncthreads();
    for (int e = t; e < nw2; e += 64) {                             // Y = A' (A'+ A')^-1/2
        const int r = e / nw, c = e % nw;
        cd acc{0.0, 0.0};
        for (int m = 0; m < nw; ++m) cfma_x(acc, Ap[r * SE_LD + m], X[m * SE_LD + c]);
        Y[r * SE_LD + c] = acc;
    }
    __syncthreads();
    for (int e = t; e < bw; e += 64) {
        const int b = e / nw, w = e % nw;
        cd acc{0.0, 0.0};
        for (int m = 0; m < nw; ++m) cfma_x(acc, Ud[b * SE_LD + m], Y[m * SE_LD + w]);
        U0[k * bw + e] = acc;
    }
}

// u~ = V_bands U0 from the resident candidate states: one workgroup per point
__global__ __launch_bounds__(256) void k_wdis_rotate(const int n, const int nb, const int nw, const cd* __restrict__ VB, const cd* __restrict__ U0,
                                                     cd* __restrict__ ut) {
    __shared__ cd Ul[WAN_NB_MAX * WAN_NW_MAX];
    const int t = threadIdx.x, bw = nb * nw;
    const int64_t k = blockIdx.x;
    for (int e = t; e < bw; e += 256) Ul[e] = U0[k * bw + e];
    __syncthreads();
    for (int e = t; e < nw * n; e += 256) {
        const int j = e % n, w = e / n;
        cd acc{0.0, 0.0};
        for (int b = 0; b < nb; ++b) cfma_x(acc, VB[(k * nb + b) * n + j], Ul[b * nw + w]);
        ut[(k * nw + w) * n + j] = acc;
    }
}

// ---------------------------------------------------------------- host side
namespace {
struct WdisRun {
    WanRun S;
    WdisPlan pl;
    template <class T>
    T* buf(int i) const { return (T*)(S.base + pl.off[i]); }
};
// Omega_I of the subspace in ud into dis_history[it]
int wdis_omega(const WdisRun& R, const cd* ud, int it) {
    const WanRun& S = R.S;
    const WanPlan& p = S.pl;
    hipStream_t st = S.ctx->stream;
    hipLaunchKernelGGL(k_wdis_reduce, dim3((unsigned)(p.npts * p.nbv)), dim3(64), 0, st, S.M, S.St, p.nb, p.nw, (const cd*)R.buf<cd>(WdisPlan::M0),
                       ud, S.buf<cd>(WanPlan::MOV));
    hipLaunchKernelGGL(k_wdis_osum, dim3(p.G), dim3(128), 0, st, p.npts, p.nbv, p.nw, p.G, (const cd*)S.buf<cd>(WanPlan::MOV),
                       R.buf<double>(WdisPlan::OPART));
    hipLaunchKernelGGL(k_wdis_ofin, dim3(1), dim3(128), 0, st, p.npts, p.nbv, p.nw, p.G, (const double*)R.buf<double>(WdisPlan::OPART),
                       (const double*)S.buf<double>(WanPlan::BW), it, R.buf<double>(WdisPlan::DISH), R.buf<double>(WdisPlan::DISD));
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}
void wdis_where(char* where, size_t len, int dk, const int32_t* mesh, int64_t idx) {
    int i[3] = {0, 0, 0};
    for (int d = dk - 1; d >= 0; --d) i[d] = (int)(idx % mesh[d]), idx /= mesh[d];
    int at = 0;
    for (int d = 0; d < dk; ++d) at += snprintf(where + at, len - at, d ? ", %d/%d" : "%d/%d", i[d], mesh[d]);
}
}  // namespace

extern "C" int tbk_wannier_dis_mesh(tbk_model* m, const int32_t* mesh, int nb, const int32_t* bands, int nw, int64_t nterm,
                                    const int32_t* term_ptr, const int32_t* term_state, const int32_t* term_R, const double* term_amp,
                                    int nbv, const int32_t* bstep, const double* bw, const double* bgram, const double* window_or_null,
                                    const double* frozen_or_null, int dis_iter, double dis_mixing, double dis_tol, int max_iter, double tol,
                                    int check_every, int nR, int r_user, const int32_t* R, double* hop, double* sums, double* hist,
                                    double* dis_sums, double* dis_hist, int32_t* n_window, int32_t* n_frozen, double* functions_or_null,
                                    double* gauge_or_null, int32_t* info) {
    const char* fn = "tbk_wannier_dis_mesh";
    TBK_REQUIRE(m && hop && sums && hist && dis_sums && dis_hist && n_window && n_frozen && info, TBK_EINVAL, "%s: null argument", fn);
    const int dk = m->dim_k, n = m->nsta;
    WanArgs A;
    A.nb = nb, A.nw = nw, A.bands = bands, A.nterm = nterm, A.term_ptr = term_ptr, A.term_state = term_state, A.term_R = term_R;
    A.term_amp = term_amp, A.nbv = nbv, A.bstep = bstep, A.bw = bw, A.bgram = bgram, A.max_iter = max_iter, A.tol = tol;
    A.check_every = check_every, A.nR = nR, A.r_user = r_user, A.R = R, A.want_fn = functions_or_null ? 1 : 0;
    WdisArgs D;
    D.dis_iter = dis_iter, D.dis_mixing = dis_mixing, D.dis_tol = dis_tol, D.check_every = check_every;
    if (window_or_null) D.have_window = 1, D.window[0] = window_or_null[0], D.window[1] = window_or_null[1];
    if (frozen_or_null) D.have_frozen = 1, D.frozen[0] = frozen_or_null[0], D.frozen[1] = frozen_or_null[1];
    int64_t npts;
    int rc = wan_check(fn, dk, n, mesh, A, npts);
    if (rc) return rc;
    if ((rc = wdis_check(fn, n, npts, nb, nbv, D))) return rc;
    tbk_ctx* ctx = m->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;

    WdisRun Rn{};
    Rn.pl = wdis_plan(n, dk, npts, mesh, nb, nw, nbv, nterm, max_iter, nR, A.want_fn, dis_iter, dis_mixing);
    Rn.S = wan_run(m, mesh, Rn.pl.wan, A);
    WanRun& S = Rn.S;
    const WanPlan& p = S.pl;
    WanBlock guard{st};
    if ((rc = guard.alloc(fn, Rn.pl.total))) return rc;
    S.base = (unsigned char*)guard.blk;
    if ((rc = wan_tables(S, m, mesh, A))) return rc;

    // the solve, the projection on every candidate band and the candidate states, chunk by chunk
    KuboChunks cw = p.cw;
    cw.base = S.base + p.off[WanPlan::CHUNKS];
    rc = kubo_for_chunks(m, cw, nullptr, mesh, npts, [&](int64_t first, int64_t cnt, const double*, const double* ec, const cd* vc) -> int {
        ProfScope ps(ctx, "wdis_project");
        hipLaunchKernelGGL(k_wdis_project, dim3((unsigned)cnt), dim3(64), 0, st, m->view, S.M, first, cnt, vc, ec,
                           (const int32_t*)S.buf<int32_t>(WanPlan::BANDS), nb, nw, (const int32_t*)S.buf<int32_t>(WanPlan::TPTR),
                           (const int32_t*)S.buf<int32_t>(WanPlan::TSTATE), (const int32_t*)S.buf<int32_t>(WanPlan::TRV),
                           (const cd*)S.buf<cd>(WanPlan::TAMP), Rn.buf<cd>(WdisPlan::AM), S.buf<double>(WanPlan::EB));
        hipLaunchKernelGGL(k_wdis_gather, dim3(nblk(cnt * nb * n)), dim3(256), 0, st, n, first, cnt, vc,
                           (const int32_t*)S.buf<int32_t>(WanPlan::BANDS), nb, Rn.buf<cd>(WdisPlan::VB));
        TBK_HIP(hipGetLastError());
        return TBK_OK;
    });
    if (rc) return rc;

    // the masks; their counts are read once
    hipLaunchKernelGGL(k_wdis_mask, dim3(nblk(npts)), dim3(256), 0, st, npts, nb, (const double*)S.buf<double>(WanPlan::EB), D.have_window,
                       D.window[0], D.window[1], D.have_frozen, D.frozen[0], D.frozen[1], Rn.buf<uint32_t>(WdisPlan::WIN),
                       Rn.buf<uint32_t>(WdisPlan::FRZ), Rn.buf<int32_t>(WdisPlan::NWIN), Rn.buf<int32_t>(WdisPlan::NFRZ));
    TBK_HIP(hipGetLastError());
    TBK_HIP(hipMemcpyAsync(n_window, Rn.buf<int32_t>(WdisPlan::NWIN), (size_t)npts * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TBK_HIP(hipMemcpyAsync(n_frozen, Rn.buf<int32_t>(WdisPlan::NFRZ), (size_t)npts * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TBK_HIP(hipStreamSynchronize(st));
    for (int64_t k = 0; k < npts; ++k) {
        char where[96];
        if (n_window[k] < nw) {
            wdis_where(where, sizeof where, dk, mesh, k);
            tbk_set_error("%s: only %d of the bands lie in the window at k = (%s): fewer than the %d functions", fn, n_window[k], where, nw);
            return TBK_EINVAL;
        }
        if (n_frozen[k] > nw) {
            wdis_where(where, sizeof where, dk, mesh, k);
            tbk_set_error("%s: %d bands lie in the frozen window at k = (%s): more than the %d functions", fn, n_frozen[k], where, nw);
            return TBK_EINVAL;
        }
    }

    const uint32_t* win = Rn.buf<uint32_t>(WdisPlan::WIN);
    const uint32_t* frz = Rn.buf<uint32_t>(WdisPlan::FRZ);
    cd* ud[2] = {Rn.buf<cd>(WdisPlan::UD0), Rn.buf<cd>(WdisPlan::UD1)};
    cd* zin = Rn.pl.keep_zin ? Rn.buf<cd>(WdisPlan::ZIN) : nullptr;
    int cur = 0;
    {
        ProfScope ps(ctx, "wdis_overlap");
        hipLaunchKernelGGL(k_wdis_overlap, dim3((unsigned)(npts * nbv)), dim3(256), 0, st, S.M, S.St, n, nb, (const cd*)Rn.buf<cd>(WdisPlan::VB),
                           (const cd*)S.buf<cd>(WanPlan::PHASE), Rn.buf<cd>(WdisPlan::M0));
        hipLaunchKernelGGL(k_wdis_select<1>, dim3((unsigned)npts), dim3(64), 0, st, S.M, S.St, nb, nw, (const cd*)Rn.buf<cd>(WdisPlan::AM),
                           (const cd*)nullptr, (const cd*)nullptr, ud[0], (cd*)nullptr, 0, 1.0, win, frz, Rn.buf<double>(WdisPlan::GAP),
                           Rn.buf<double>(WdisPlan::SVP));
        TBK_HIP(hipGetLastError());
    }
    if ((rc = wdis_omega(Rn, ud[0], 0))) return rc;
    int dis_iterations = 0, dis_converged = 0;
    for (int it = 1; it <= dis_iter; ++it) {
        ProfScope ps(ctx, "wdis_step");
        hipLaunchKernelGGL(k_wdis_select<0>, dim3((unsigned)npts), dim3(64), 0, st, S.M, S.St, nb, nw, (const cd*)nullptr,
                           (const cd*)Rn.buf<cd>(WdisPlan::M0), (const cd*)ud[cur], ud[1 - cur], zin, it == 1 ? 1 : 0, dis_mixing, win, frz,
                           Rn.buf<double>(WdisPlan::GAP), (double*)nullptr);
        cur = 1 - cur;
        if ((rc = wdis_omega(Rn, ud[cur], it))) return rc;
        dis_iterations = it;
        if (it % check_every != 0 && it != dis_iter) continue;
        double d = 0.0;                                             // the check: one 8-byte copy behind a synchronisation
        TBK_HIP(hipMemcpyAsync(&d, Rn.buf<double>(WdisPlan::DISD) + it, sizeof(double), hipMemcpyDeviceToHost, st));
        TBK_HIP(hipStreamSynchronize(st));
        TBK_REQUIRE(std::isfinite(d), TBK_ENOCONV, "%s: Omega_I of disentanglement iteration %d is not finite", fn, it);
        if (dis_tol > 0.0 && fabs(d) < dis_tol) {
            dis_converged = 1;
            break;
        }
    }

    // the gauge inside the subspace, its singular values, the overlaps of section 34 from M0
    hipLaunchKernelGGL(k_wdis_gauge, dim3((unsigned)npts), dim3(64), 0, st, nb, nw, (const cd*)Rn.buf<cd>(WdisPlan::AM), (const cd*)ud[cur], win,
                       S.buf<cd>(WanPlan::U0), S.buf<double>(WanPlan::SVK));
    TBK_HIP(hipGetLastError());
    {
        std::vector<double> v((size_t)2 * npts);
        TBK_HIP(hipMemcpyAsync(v.data(), Rn.buf<double>(WdisPlan::SVP), (size_t)npts * sizeof(double), hipMemcpyDeviceToHost, st));
        TBK_HIP(hipMemcpyAsync(v.data() + npts, Rn.buf<double>(WdisPlan::GAP), (size_t)npts * sizeof(double), hipMemcpyDeviceToHost, st));
        TBK_HIP(hipStreamSynchronize(st));
        double svp = v[0], gap = v[(size_t)npts];
        for (int64_t k = 0; k < npts; ++k) {
            TBK_REQUIRE(std::isfinite(v[(size_t)k]), TBK_ENOCONV, "%s: the projection at mesh point %lld is not finite", fn, (long long)k);
            svp = std::min(svp, v[(size_t)k]);
            gap = std::min(gap, v[(size_t)(npts + k)]);
        }
        dis_sums[0] = svp, dis_sums[1] = gap;
    }
    if ((rc = wan_sv_check(fn, S, dk, mesh, sums))) return rc;
    {
        ProfScope ps(ctx, "wan_overlap");
        hipLaunchKernelGGL(k_wdis_reduce, dim3((unsigned)(npts * nbv)), dim3(64), 0, st, S.M, S.St, nb, nw, (const cd*)Rn.buf<cd>(WdisPlan::M0),
                           (const cd*)S.buf<cd>(WanPlan::U0), S.buf<cd>(WanPlan::MOV));
        hipLaunchKernelGGL(k_wan_identity, dim3(nblk(npts * nw * nw)), dim3(256), 0, st, npts, nw, S.buf<cd>(WanPlan::UACC));
        TBK_HIP(hipGetLastError());
    }
    int iterations = 0, converged = 0;
    if ((rc = wan_descend(fn, S, max_iter, tol, check_every, iterations, converged))) return rc;
    if (functions_or_null) {
        hipLaunchKernelGGL(k_wdis_rotate, dim3((unsigned)npts), dim3(256), 0, st, n, nb, nw, (const cd*)Rn.buf<cd>(WdisPlan::VB),
                           (const cd*)S.buf<cd>(WanPlan::U0), S.buf<cd>(WanPlan::UT));
        TBK_HIP(hipGetLastError());
    }
    TBK_HIP(hipMemcpyAsync(dis_hist, Rn.buf<double>(WdisPlan::DISH), (size_t)(dis_iterations + 1) * sizeof(double), hipMemcpyDeviceToHost, st));
    if ((rc = wan_finish(S, m, nR, iterations, hop, sums, hist, functions_or_null, gauge_or_null))) return rc;
    info[0] = iterations;
    info[1] = converged;
    info[2] = dis_iterations;
    info[3] = dis_converged;
    info[4] = p.G;
    return TBK_OK;
}
