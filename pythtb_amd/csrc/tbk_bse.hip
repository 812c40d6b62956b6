// tbk_bse.hip -- excitons on uniform k meshes: the Tamm-Dancoff Bethe-Salpeter operator of a density-density interaction, applied
// without forming its matrix, its dense eigenstates and its Haydock (Lanczos) spectrum.
//
// Transitions t = (k, v, c); X[k][v][c].  With T(k) = sum_vc X_vc(k) u_ck u_vk^+ and the set E of tbk_bse.h:
//   F_e   = (1/N) sum_k e^{-2 pi i k.d_e} T_ab(k),   rho_b = (1/N) sum_k T_bb(k),   h_a = sum_{e: a_e = a} V_e rho_{b_e}
//   (H X)_vc(k) = Delta X_vc(k) + sum_a h_a conj(u_c[a]) u_v[a] - sum_e V_e F_e e^{2 pi i k.d_e} conj(u_c[a]) u_v[b]
//
// Setup, once per call (bse_setup): the mesh solve with eigenvectors in the chunks of tbk_kubo.h; per chunk
//   k_bse_gather   counts the levels at or below the Fermi level of every point and copies the selected bands into the compact
//                  block U[k][band][n] (valence bands first), their levels into EV[k][band] and Delta into GAPS[k][v][c]
//   k_bse_scan     ONE workgroup: the smallest and the largest Delta, the largest |E|, the first point whose count differs
//   k_bse_dipole   (states, spectrum) D^a_t = <u_c| dH/dk_a |u_v> / Delta from dham_terms over the model's non-empty slots
// One application (bse_apply), two sweeps over U:
//   k_bse_pair     workgroup (k-group g, vector, BSE_EC sums): lane (q, v, c) of tbk_bse.h's map takes point q of a tile and adds
//                  u_c[a] X_vc conj(u_v[b]) e^{-2 pi i k.d} into its accumulator over the group's tiles; the phases of a tile are
//                  staged in LDS (exact integer k.R of tbk_lat_dev.h); the lanes are added in a fixed order: part[g][vector][p]
//   k_pairs_rows   (tbk_pairs_dm.hip) the groups in a fixed order: FSUM[vector][p]
//   k_bse_fields   FS_e = V_e F_e / N and h_a / N through the CSR map, a lane per value
//   k_bse_project  workgroup (k-group, vector), the same lanes: Y_vc = Delta X_vc + sum_a h_a conj(u_c[a]) u_v[a]
//                  - sum_e FS_e e^{2 pi i k.d_e} conj(u_c[a]) u_v[b], and the group's partial of Re <X|Y>
// The Lanczos driver (bse_lanczos) keeps alpha, beta, the three-term update and the breakdown flag on the device:
//   k_bse_lz_alpha   alpha_j = sum of the partials, groups in a fixed order
//   k_bse_lz_update  W = Y - alpha_j Q_j - beta_{j-1} Q_{j-1} over Q_{j-1}, and the partials of |W|^2
//   k_bse_lz_beta    beta_j = |W|; a run whose beta_j < 1e-10 max(largest |alpha| so far, largest Delta) ends: done, n_used = j + 1
//   k_bse_lz_scale   Q_{j+1} = W / beta_j
// beta is the norm of the updated vector, not sqrt(<Y|Y> - alpha^2 - beta^2): that difference cancels to 1e-8 |alpha| and could not
// carry the 1e-10 breakdown rule.  No floating-point atomics, and no partition depends on the block width or on the interaction
// list: two calls give the same bits, and a vector gives the same bits alone and inside any block.
#include <math.h>
#include "tbk_bse.h"
#include "tbk_occ_dev.h"

namespace {
struct BseDev {                 // what the kernels of an application read (device pointers)
    OccMesh M;
    int n, dk, nv, nc, ns, P, G, ned, nst, np;
    int64_t npts, nt;
    const double* k;            // [npts][dk]
    const double2* U;           // [npts][ns][n]
    const double* gaps;         // [nt]
    const double4* orb;
    const int32_t *pa, *pb, *pR, *st;
};

// e^{-2 pi i k.(R + tau_b - tau_a)} of sum p at mesh point ik
__device__ __forceinline__ cd bse_phase(const BseDev& D, const int64_t ik, const int p) {
    if (p >= D.ned) return cd{1.0, 0.0};
    double kk[4] = {0.0, 0.0, 0.0, 0.0};
    for (int d = 0; d < D.dk; ++d) kk[d] = D.k[ik * D.dk + d];
    const double4 ta = D.orb[D.pa[p]], tb = D.orb[D.pb[p]];
    const cd ph = expi2pi(kdot(kk, double4{ta.x - tb.x, ta.y - tb.y, ta.z - tb.z, 0.0}));
    return cmul_x(ph, dm_phase(D.M, ik, D.pR + 3 * p));
}

// the 256 lanes' values added in a fixed order (shuffle tree in each wavefront, then the four in index order); thread 0 has the sum
__device__ __forceinline__ cd bse_block_csum(cd v, cd* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        v.x += __shfl_xor(v.x, o);
        v.y += __shfl_xor(v.y, o);
    }
    __syncthreads();                                               // (red is free again)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return cadd(cadd(red[0], red[1]), cadd(red[2], red[3]));
}
__device__ __forceinline__ double bse_block_dsum(double v, double* red) {
    __syncthreads();
    return block_sum(v, red);
}

// ---------------------------------------------------------------- setup
// One workgroup per point of the chunk (ec[n][cnt], vc[n][cnt][n]).
__global__ __launch_bounds__(256) void k_bse_gather(const double* __restrict__ ec, const double2* __restrict__ vc, const int64_t cnt,
                                                    const int64_t first, const int n, const double mu, const int32_t* __restrict__ bands,
                                                    const int nv, const int nc, int32_t* __restrict__ count, double2* __restrict__ U,
                                                    double* __restrict__ EV, double* __restrict__ gaps) {
    __shared__ double red[4];
    const int64_t p = blockIdx.x, ik = first + p;
    const int t = threadIdx.x, ns = nv + nc;
    double c = 0.0;
    for (int b = t; b < n; b += 256) c += ec[(int64_t)b * cnt + p] <= mu ? 1.0 : 0.0;
    c = block_sum(c, red);
    if (t == 0) count[ik] = (int32_t)c;
    for (int e = t; e < ns * n; e += 256) {
        const int s = e / n, i = e - s * n;
        U[(ik * ns + s) * n + i] = vc[((int64_t)bands[s] * cnt + p) * n + i];
    }
    if (t < ns) EV[ik * ns + t] = ec[(int64_t)bands[t] * cnt + p];
    if (t < nv * nc) {
        const int v = t / nc, cc = t - v * nc;
        gaps[ik * nv * nc + t] = ec[(int64_t)bands[nv + cc] * cnt + p] - ec[(int64_t)bands[v] * cnt + p];
    }
}

// ONE workgroup of 1024: out = {min Delta, max Delta, max |E|, first point whose count is not nocc (-1: none), its count}
__global__ __launch_bounds__(1024) void k_bse_scan(const double* __restrict__ gaps, const int64_t nt, const double* __restrict__ EV,
                                                   const int64_t nlev, const int32_t* __restrict__ count, const int64_t npts, const int nocc,
                                                   double* __restrict__ out) {
    __shared__ double r0[16], r1[16], r2[16], r3[16];
    const int t = threadIdx.x;
    double gmin = INFINITY, gmax = -INFINITY, emax = 0.0, bad = 9.0e18;
    for (int64_t i = t; i < nt; i += 1024) {
        const double g = gaps[i];
        gmin = fmin(gmin, g);
        gmax = fmax(gmax, g);
    }
    for (int64_t i = t; i < nlev; i += 1024) emax = fmax(emax, fabs(EV[i]));
    for (int64_t i = t; i < npts; i += 1024)
        if (count[i] != nocc) {
            bad = (double)i;
            break;
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        gmin = fmin(gmin, __shfl_xor(gmin, o));
        gmax = fmax(gmax, __shfl_xor(gmax, o));
        emax = fmax(emax, __shfl_xor(emax, o));
        bad = fmin(bad, __shfl_xor(bad, o));
    }
    if ((t & 63) == 0) r0[t >> 6] = gmin, r1[t >> 6] = gmax, r2[t >> 6] = emax, r3[t >> 6] = bad;
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < 16; ++w) {
            gmin = fmin(gmin, r0[w]);
            gmax = fmax(gmax, r1[w]);
            emax = fmax(emax, r2[w]);
            bad = fmin(bad, r3[w]);
        }
        out[0] = gmin, out[1] = gmax, out[2] = emax;
        out[3] = bad < 9.0e18 ? bad : -1.0;
        out[4] = bad < 9.0e18 ? (double)count[(int64_t)bad] : 0.0;
    }
}

// One workgroup per point: D^a_vc = <u_c| dH/dk_a |u_v> / Delta, dip[a][nt].  The slots of the model go through LDS 64 at a time,
// a lane per slot forming dH_ab in every direction; then lane r = (v, c) adds the slots in order, both halves of an off-diagonal one.
#define BSE_DSL 64
__global__ __launch_bounds__(256) void k_bse_dipole(const ModelView mv, const BseDev D, cd* __restrict__ dip) {
    __shared__ cd dh[BSE_DSL][3];
    __shared__ int sab[BSE_DSL];
    const int64_t ik = blockIdx.x;
    const int t = threadIdx.x, nvc = D.nv * D.nc;
    const int v = t / D.nc, c = t - v * D.nc;
    const bool live = t < nvc;
    const double2* uv = D.U + (ik * D.ns + (live ? v : 0)) * D.n;
    const double2* uc = D.U + (ik * D.ns + D.nv + (live ? c : 0)) * D.n;
    double kk[4];
    cd z[4];
    k_phases(mv, D.k, ik, kk, z);
    cd acc[3] = {cd{0.0, 0.0}, cd{0.0, 0.0}, cd{0.0, 0.0}};
    for (int s0 = 0; s0 < mv.nnz; s0 += BSE_DSL) {
        const int sn = min(BSE_DSL, mv.nnz - s0);
        __syncthreads();
        if (t < sn) {
            const int4 e = mv.nz[s0 + t];
            const int a = e.x & 0xffff, b = e.x >> 16;
            cd h, v0, v1;
            dham_terms(mv, a, b, e.y, e.z, kk, z, 0, D.dk > 1 ? 1 : 0, h, v0, v1);
            dh[t][0] = v0, dh[t][1] = v1;
            if (D.dk > 2) {
                dham_terms(mv, a, b, e.y, e.z, kk, z, 2, 2, h, v0, v1);
                dh[t][2] = v0;
            }
            sab[t] = e.x;
        }
        __syncthreads();
        if (!live) continue;
        for (int s = 0; s < sn; ++s) {
            const int a = sab[s] & 0xffff, b = sab[s] >> 16;
            const double2 ca = uc[a], vb = uv[b];
            const cd w1 = cmulc(cd{ca.x, ca.y}, cd{vb.x, vb.y});           // conj(u_c[a]) u_v[b]
            cd w2{0.0, 0.0};
            if (a != b) {
                const double2 cb = uc[b], va = uv[a];
                w2 = cmulc(cd{cb.x, cb.y}, cd{va.x, va.y});               // conj(u_c[b]) u_v[a], with conj(dH_ab)
            }
            for (int d = 0; d < D.dk; ++d) {
                cfma_x(acc[d], w1, dh[s][d]);
                cfma_x(acc[d], w2, cconj(dh[s][d]));
            }
        }
    }
    if (!live) return;
    const int64_t it = ik * nvc + t;
    const double g = D.gaps[it];
    for (int d = 0; d < D.dk; ++d) dip[(int64_t)d * D.nt + it] = cd{acc[d].x / g, acc[d].y / g};
}

// ---------------------------------------------------------------- one application
// grid (G, nb, ceil(np / BSE_EC)); X[nb][nt]; part[g][nb][np]
__global__ __launch_bounds__(256) void k_bse_pair(const BseDev D, const cd* __restrict__ X, const int nb, cd* __restrict__ part) {
    __shared__ cd phs[256 * BSE_EC];
    __shared__ cd red[4];
    const int t = threadIdx.x, g = blockIdx.x, ib = blockIdx.y, e0 = blockIdx.z * BSE_EC;
    const int ecn = min(BSE_EC, D.np - e0), nvc = D.nv * D.nc;
    int q, r, v, c;
    bse_lane(t, nvc, D.nc, q, r, v, c);
    const bool live = q < D.P;
    const int64_t ntiles = (D.npts + D.P - 1) / D.P;
    const int64_t t0 = (int64_t)g * ntiles / D.G, t1 = (int64_t)(g + 1) * ntiles / D.G;
    int ea[BSE_EC], eb[BSE_EC];
#pragma unroll
    for (int j = 0; j < BSE_EC; ++j) {
        ea[j] = D.pa[e0 + (j < ecn ? j : 0)];
        eb[j] = D.pb[e0 + (j < ecn ? j : 0)];
    }
    cd acc[BSE_EC];
#pragma unroll
    for (int j = 0; j < BSE_EC; ++j) acc[j] = cd{0.0, 0.0};
    for (int64_t tile = t0; tile < t1; ++tile) {
        const int64_t k0 = tile * D.P, ik = k0 + q;
        __syncthreads();                                           // (the previous tile's phases are consumed)
        for (int e = t; e < D.P * ecn; e += 256) {
            const int qq = e / ecn, j = e - qq * ecn;
            if (k0 + qq < D.npts) phs[qq * BSE_EC + j] = bse_phase(D, k0 + qq, e0 + j);
        }
        __syncthreads();
        if (!live || ik >= D.npts) continue;
        const cd x = X[(int64_t)ib * D.nt + ik * nvc + r];
        const double2* uv = D.U + (ik * D.ns + v) * D.n;
        const double2* uc = D.U + (ik * D.ns + D.nv + c) * D.n;
#pragma unroll
        for (int j = 0; j < BSE_EC; ++j) {
            if (j >= ecn) break;
            const double2 a = uc[ea[j]], b = uv[eb[j]];
            const cd w = cmul_x(cd{a.x, a.y}, x);                   // u_c[a] X_vc
            cd tab{0.0, 0.0};
            cfmac_x(tab, w, cd{b.x, b.y});                          // ... conj(u_v[b])
            cfma_x(acc[j], tab, phs[q * BSE_EC + j]);
        }
    }
#pragma unroll
    for (int j = 0; j < BSE_EC; ++j) {
        if (j >= ecn) break;                                       // (uniform over the workgroup)
        const cd s = bse_block_csum(acc[j], red);
        if (t == 0) part[((int64_t)g * nb + ib) * D.np + e0 + j] = s;
    }
}

// fsum[nb][np] -> fs[nb][ned] = V_e F_e / N and hf[nb][nst] = h_a / N; a lane per value, the CSR row of a state in order
__global__ __launch_bounds__(256) void k_bse_fields(const int nb, const int ned, const int nst, const int np, const double nk,
                                                    const double* __restrict__ eV, const int32_t* __restrict__ hptr,
                                                    const int32_t* __restrict__ hent, const int32_t* __restrict__ hslot,
                                                    const cd* __restrict__ fsum, cd* __restrict__ fs, cd* __restrict__ hf) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nb * np) return;
    const int ib = i / np, p = i - ib * np;
    const cd* f = fsum + (int64_t)ib * np;
    if (p < ned) {
        const double s = eV[p] / nk;
        fs[(int64_t)ib * ned + p] = cd{f[p].x * s, f[p].y * s};
        return;
    }
    const int a = p - ned;
    cd h{0.0, 0.0};
    for (int q = hptr[a]; q < hptr[a + 1]; ++q) {
        const double s = eV[hent[q]] / nk;
        const cd rho = f[ned + hslot[q]];
        h.x = fma(s, rho.x, h.x);
        h.y = fma(s, rho.y, h.y);
    }
    hf[(int64_t)ib * nst + a] = h;
}

// grid (G, nb); Y[nb][nt]; dpart[nb][G] the group's partial of Re <X|Y> (where wanted)
__global__ __launch_bounds__(256) void k_bse_project(const BseDev D, const cd* __restrict__ X, const cd* __restrict__ fs,
                                                     const cd* __restrict__ hf, cd* __restrict__ Y, double* __restrict__ dpart) {
    __shared__ cd phs[256 * BSE_EC];
    __shared__ double red[4];
    const int t = threadIdx.x, g = blockIdx.x, ib = blockIdx.y, nvc = D.nv * D.nc;
    int q, r, v, c;
    bse_lane(t, nvc, D.nc, q, r, v, c);
    const bool live = q < D.P;
    const int64_t ntiles = (D.npts + D.P - 1) / D.P;
    const int64_t t0 = (int64_t)g * ntiles / D.G, t1 = (int64_t)(g + 1) * ntiles / D.G;
    const cd* fsb = fs + (int64_t)ib * D.ned;
    const cd* hfb = hf + (int64_t)ib * D.nst;
    double dot = 0.0;
    for (int64_t tile = t0; tile < t1; ++tile) {
        const int64_t k0 = tile * D.P, ik = k0 + q;
        const bool on = live && ik < D.npts;
        const int64_t it = (on ? ik : 0) * nvc + r;
        const double2* uv = D.U + ((on ? ik : 0) * D.ns + v) * D.n;
        const double2* uc = D.U + ((on ? ik : 0) * D.ns + D.nv + c) * D.n;
        cd x{0.0, 0.0}, y{0.0, 0.0};
        if (on) {
            x = X[(int64_t)ib * D.nt + it];
            const double dl = D.gaps[it];
            y = cd{dl * x.x, dl * x.y};
            for (int i = 0; i < D.nst; ++i) {
                const int a = D.st[i];
                const double2 ca = uc[a], va = uv[a];
                cfma_x(y, hfb[i], cmulc(cd{ca.x, ca.y}, cd{va.x, va.y}));
            }
        }
        for (int e0 = 0; e0 < D.ned; e0 += BSE_EC) {
            const int ecn = min(BSE_EC, D.ned - e0);
            __syncthreads();
            for (int e = t; e < D.P * ecn; e += 256) {
                const int qq = e / ecn, j = e - qq * ecn;
                if (k0 + qq < D.npts) phs[qq * BSE_EC + j] = bse_phase(D, k0 + qq, e0 + j);
            }
            __syncthreads();
            if (!on) continue;
            for (int j = 0; j < ecn; ++j) {
                const double2 ca = uc[D.pa[e0 + j]], vb = uv[D.pb[e0 + j]];
                cd f{0.0, 0.0};
                cfmac_x(f, fsb[e0 + j], phs[q * BSE_EC + j]);       // FS_e e^{+2 pi i k.d_e}
                const cd w = cmulc(cd{ca.x, ca.y}, cd{vb.x, vb.y});
                cfma_x(y, cd{-f.x, -f.y}, w);
            }
        }
        if (on) {
            Y[(int64_t)ib * D.nt + it] = y;
            dot = fma(x.x, y.x, fma(x.y, y.y, dot));
        }
    }
    if (!dpart) return;
    dot = bse_block_dsum(dot, red);
    if (t == 0) dpart[(int64_t)ib * D.G + g] = dot;
}

// ---------------------------------------------------------------- the Lanczos driver
// lz[run][8] doubles: 0 alpha of the step, 1 beta of the step, 2 |start|, 3 largest |alpha| so far (from the largest Delta), 4 done,
// 5 n_used
__global__ __launch_bounds__(256) void k_bse_lz_init(const int nb, const int nsteps, const double* __restrict__ scal, double* __restrict__ lz) {
    const int r = threadIdx.x;
    if (r >= nb) return;
    double* l = lz + 8 * r;
    l[0] = l[1] = l[2] = 0.0;
    l[3] = scal[1];
    l[4] = 0.0;
    l[5] = (double)nsteps;
}
// W[run] = D^a, D^a + D^b or D^a + i D^b, and the partials of its norm; grid (GN, runs)
__global__ __launch_bounds__(256) void k_bse_lz_start(const int64_t nt, const int GN, const int32_t* __restrict__ runs, const cd* __restrict__ dip,
                                                      cd* __restrict__ W, double* __restrict__ npart) {
    __shared__ double red[4];
    const int g = blockIdx.x, ib = blockIdx.y;
    const int a = runs[3 * ib], b = runs[3 * ib + 1], kind = runs[3 * ib + 2];
    double s = 0.0;
    for (int64_t i = (int64_t)g * 256 + threadIdx.x; i < nt; i += (int64_t)GN * 256) {
        cd w = dip[(int64_t)a * nt + i];
        if (kind) {
            const cd o = dip[(int64_t)b * nt + i];
            w = kind == 1 ? cadd(w, o) : cd{w.x - o.y, w.y + o.x};
        }
        W[(int64_t)ib * nt + i] = w;
        s = fma(w.x, w.x, fma(w.y, w.y, s));
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) npart[(int64_t)ib * GN + g] = s;
}
__global__ __launch_bounds__(256) void k_bse_lz_alpha(const int G, const int j, const int nsteps, const double* __restrict__ dpart,
                                                      double* __restrict__ lz, double* __restrict__ alpha) {
    __shared__ double red[4];
    const int ib = blockIdx.x;
    double* l = lz + 8 * ib;
    if (l[4] != 0.0) return;                                       // (uniform: the run has ended)
    double s = 0.0;
    for (int g = threadIdx.x; g < G; g += 256) s += dpart[(int64_t)ib * G + g];
    s = block_sum(s, red);
    if (threadIdx.x == 0) {
        l[0] = s;
        alpha[(int64_t)ib * nsteps + j] = s;
    }
}
// Z <- Y - alpha X - beta_prev Z (first: no Z term) and the partials of its norm; grid (GN, runs)
__global__ __launch_bounds__(256) void k_bse_lz_update(const int64_t nt, const int GN, const int first, const double* __restrict__ lz,
                                                       const cd* __restrict__ X, const cd* __restrict__ Y, cd* __restrict__ Z,
                                                       double* __restrict__ npart) {
    __shared__ double red[4];
    const int g = blockIdx.x, ib = blockIdx.y;
    const double* l = lz + 8 * ib;
    if (l[4] != 0.0) return;
    const double al = l[0], be = l[1];
    double s = 0.0;
    for (int64_t i = (int64_t)g * 256 + threadIdx.x; i < nt; i += (int64_t)GN * 256) {
        const int64_t e = (int64_t)ib * nt + i;
        const cd x = X[e], y = Y[e];
        cd w{fma(-al, x.x, y.x), fma(-al, x.y, y.y)};
        if (!first) {
            const cd z = Z[e];
            w.x = fma(-be, z.x, w.x);
            w.y = fma(-be, z.y, w.y);
        }
        Z[e] = w;
        s = fma(w.x, w.x, fma(w.y, w.y, s));
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) npart[(int64_t)ib * GN + g] = s;
}
// j < 0: the norm of the start vector (a zero start ends the run with n_used = 0)
__global__ __launch_bounds__(256) void k_bse_lz_beta(const int GN, const int j, const int nsteps, const double* __restrict__ npart,
                                                     double* __restrict__ lz, double* __restrict__ beta) {
    __shared__ double red[4];
    const int ib = blockIdx.x;
    double* l = lz + 8 * ib;
    if (l[4] != 0.0) return;
    double s = 0.0;
    for (int g = threadIdx.x; g < GN; g += 256) s += npart[(int64_t)ib * GN + g];
    s = block_sum(s, red);
    if (threadIdx.x != 0) return;
    const double b = sqrt(s);
    l[1] = b;
    if (j < 0) {
        l[2] = b;
        if (!(b > 0.0)) l[4] = 1.0, l[5] = 0.0;
        return;
    }
    beta[(int64_t)ib * nsteps + j] = b;
    l[3] = fmax(l[3], fabs(l[0]));
    if (!(b >= kBseBreakdown * l[3])) l[4] = 1.0, l[5] = (double)(j + 1);
}
__global__ __launch_bounds__(256) void k_bse_lz_scale(const int64_t nt, const double* __restrict__ lz, cd* __restrict__ Z) {
    const int ib = blockIdx.y;
    const double* l = lz + 8 * ib;
    if (l[4] != 0.0) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nt) return;
    const double b = l[1];
    cd* z = Z + (int64_t)ib * nt + i;
    *z = cd{z->x / b, z->y / b};
}

// ---------------------------------------------------------------- the dense path
// X[ib] = the unit vector of transition t0 + ib
__global__ __launch_bounds__(256) void k_bse_unit(const int64_t nt, const int64_t t0, cd* __restrict__ X) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nt) return;
    X[(int64_t)blockIdx.y * nt + i] = cd{i == t0 + blockIdx.y ? 1.0 : 0.0, 0.0};
}
// row t0 + ib of H is the conjugate of column t0 + ib = Y[ib]
__global__ __launch_bounds__(256) void k_bse_hrow(const int64_t nt, const int64_t t0, const cd* __restrict__ Y, cd* __restrict__ H) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nt) return;
    H[(t0 + blockIdx.y) * nt + i] = cconj(Y[(int64_t)blockIdx.y * nt + i]);
}
// out[row][col] = sum_t conj(A[row][t]) B[col][t]: one workgroup per entry, strided lanes, fixed order
__global__ __launch_bounds__(256) void k_bse_cdots(const int64_t nt, const cd* __restrict__ A, const cd* __restrict__ B, const int ncol,
                                                   cd* __restrict__ out) {
    __shared__ cd red[4];
    const int64_t row = blockIdx.x;
    const int col = blockIdx.y;
    cd s{0.0, 0.0};
    for (int64_t i = threadIdx.x; i < nt; i += 256) cfmac_x(s, B[(int64_t)col * nt + i], A[row * nt + i]);
    s = bse_block_csum(s, red);
    if (threadIdx.x == 0) out[row * ncol + col] = s;
}

// ---------------------------------------------------------------- host side
struct BseRunState {
    tbk_ctx* ctx;
    tbk_model* m;
    BsePlan pl;
    BseProblem Q;
    BseDev D;
    unsigned char* base;
    int nocc = 0;
    double scal[5];
    template <class T>
    T* buf(int i) const { return (T*)(base + pl.off[i]); }
};

// the number of levels at or below mu at the first mesh point (k = 0): what the band selection and the plan need before the solve
int bse_count_first(tbk_model* m, double mu, int& nocc) {
    tbk_ctx* ctx = m->ctx;
    const int n = m->nsta;
    void* base = nullptr;
    int rc = tbk_ctx_scratch(ctx, 512 + al256((size_t)n * sizeof(double)), &base);
    if (rc) return rc;
    double* kd = (double*)((unsigned char*)base + 256);
    double* ed = (double*)((unsigned char*)base + 512);
    TBK_HIP(hipMemsetAsync(kd, 0, 256, ctx->stream));
    rc = tbk_solve_list_dev_checked(m, kd, 1, ed, nullptr);
    if (rc) return rc;
    std::vector<double> e((size_t)n);
    TBK_HIP(hipMemcpyAsync(e.data(), ed, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    nocc = 0;
    for (double x : e) nocc += x <= mu ? 1 : 0;
    return TBK_OK;
}

// checks, selection, plan, workspace, the mesh solve and the gathered bands; info = {nocc, nv, nc}
int bse_setup(const char* fn, int mode, tbk_model* m, const int32_t* mesh, const BseArgs& A, int nb, int nsteps, int xnv, int xnc,
              BseRunState& S, int32_t* info) {
    const int dk = m->dim_k, n = m->nsta;
    int64_t npts;
    int rc = bse_check(fn, dk, n, mesh, A, npts);
    if (rc) return rc;
    rc = bse_problem(fn, dk, n, A, S.Q);
    if (rc) return rc;
    tbk_ctx* ctx = m->ctx;
    S.ctx = ctx, S.m = m;
    TBK_HIP(hipSetDevice(ctx->device));
    rc = bse_count_first(m, A.mu, S.nocc);
    if (rc) return rc;
    int32_t bands[2 * kBseBandMax] = {};
    int nv, nc;
    rc = bse_select(fn, n, S.nocc, A, bands, nv, nc);
    if (rc) return rc;
    info[0] = S.nocc, info[1] = nv, info[2] = nc;
    if (mode == 0)
        TBK_REQUIRE(xnv == nv && xnc == nc, TBK_EINVAL, "%s: vectors of %d x %d bands per point, the selection has %d x %d", fn, xnv, xnc, nv, nc);
    rc = bse_caps(fn, mode, n, npts, nv, nc);
    if (rc) return rc;
    S.pl = bse_plan(mode, n, dk, npts, nv, nc, nb, S.Q, nsteps);
    const BsePlan& pl = S.pl;
    void* base = nullptr;
    rc = tbk_ctx_scratch(ctx, pl.total, &base);
    if (rc) return rc;
    S.base = (unsigned char*)base;
    hipStream_t st = ctx->stream;
    auto up = [&](int i, const void* src, size_t bytes) -> int {
        if (bytes) TBK_HIP(hipMemcpyAsync(S.base + pl.off[i], src, bytes, hipMemcpyHostToDevice, st));
        return TBK_OK;
    };
    const BseProblem& Q = S.Q;
    if ((rc = up(BsePlan::BANDS, bands, sizeof bands))) return rc;
    if ((rc = up(BsePlan::PA, Q.pa.data(), Q.pa.size() * sizeof(int32_t)))) return rc;
    if ((rc = up(BsePlan::PB, Q.pb.data(), Q.pb.size() * sizeof(int32_t)))) return rc;
    if ((rc = up(BsePlan::PR, Q.pR.data(), Q.pR.size() * sizeof(int32_t)))) return rc;
    if ((rc = up(BsePlan::EVV, Q.eV.data(), Q.eV.size() * sizeof(double)))) return rc;
    if ((rc = up(BsePlan::ST, Q.st.data(), Q.st.size() * sizeof(int32_t)))) return rc;
    if ((rc = up(BsePlan::HPTR, Q.hptr.data(), Q.hptr.size() * sizeof(int32_t)))) return rc;
    if ((rc = up(BsePlan::HENT, Q.hent.data(), Q.hent.size() * sizeof(int32_t)))) return rc;
    if ((rc = up(BsePlan::HSLOT, Q.hslot.data(), Q.hslot.size() * sizeof(int32_t)))) return rc;
    TBK_HIP(hipStreamSynchronize(st));                              // (bands[] goes out of use)

    BseDev& D = S.D;
    D.M = OccMesh{{1, 1, 1}, dk};
    for (int d = 0; d < dk; ++d) D.M.N[d] = mesh[d];
    D.n = n, D.dk = dk, D.nv = nv, D.nc = nc, D.ns = nv + nc, D.P = pl.P, D.G = pl.G, D.ned = Q.ned, D.nst = Q.nst, D.np = Q.np;
    D.npts = npts, D.nt = pl.nt;
    D.k = S.buf<double>(BsePlan::K_ALL);
    D.U = S.buf<double2>(BsePlan::U);
    D.gaps = S.buf<double>(BsePlan::GAPS);
    D.orb = m->view.orb;
    D.pa = S.buf<int32_t>(BsePlan::PA), D.pb = S.buf<int32_t>(BsePlan::PB), D.pR = S.buf<int32_t>(BsePlan::PR);
    D.st = S.buf<int32_t>(BsePlan::ST);

    KuboChunks cw = pl.cw;
    cw.base = S.base + pl.off_chunks;
    rc = kubo_for_chunks(m, cw, nullptr, mesh, npts, [&](int64_t first, int64_t cnt, const double* kp, const double* ec, const cd* vc) -> int {
        TBK_HIP(hipMemcpyAsync(S.buf<double>(BsePlan::K_ALL) + first * dk, kp, (size_t)cnt * dk * sizeof(double), hipMemcpyDeviceToDevice, st));
        ProfScope ps(ctx, "bse_gather");
        hipLaunchKernelGGL(k_bse_gather, dim3((unsigned)cnt), dim3(256), 0, st, ec, (const double2*)vc, cnt, first, n, A.mu,
                           (const int32_t*)S.buf<int32_t>(BsePlan::BANDS), nv, nc, S.buf<int32_t>(BsePlan::CNT), S.buf<double2>(BsePlan::U),
                           S.buf<double>(BsePlan::EV), S.buf<double>(BsePlan::GAPS));
        TBK_HIP(hipGetLastError());
        return TBK_OK;
    });
    if (rc) return rc;
    {
        ProfScope ps(ctx, "bse_scan");
        hipLaunchKernelGGL(k_bse_scan, dim3(1), dim3(1024), 0, st, (const double*)S.buf<double>(BsePlan::GAPS), pl.nt,
                           (const double*)S.buf<double>(BsePlan::EV), npts * (nv + nc), (const int32_t*)S.buf<int32_t>(BsePlan::CNT), npts,
                           S.nocc, S.buf<double>(BsePlan::SCAL));
        TBK_HIP(hipGetLastError());
    }
    rc = tbk_small_d2h(ctx, S.scal, S.buf<double>(BsePlan::SCAL), sizeof S.scal);
    if (rc) return rc;
    if (S.scal[3] >= 0.0) {
        const int64_t bad = (int64_t)S.scal[3];
        int ii[3] = {0, 0, 0};
        int64_t rem = bad;
        for (int d = dk - 1; d >= 0; --d) ii[d] = (int)(rem % mesh[d]), rem /= mesh[d];
        tbk_set_error("%s: not an insulator: %d levels at or below the Fermi level at mesh point (%d, %d, %d), %d at the first point", fn,
                      (int)S.scal[4], ii[0], ii[1], ii[2], S.nocc);
        return TBK_EINVAL;
    }
    TBK_REQUIRE(S.scal[0] > 1e-9 * std::max(1.0, S.scal[2]), TBK_EINVAL, "%s: a metal: the smallest transition energy is %.3g", fn, S.scal[0]);
    if (mode) {
        ProfScope ps(ctx, "bse_dipole");
        hipLaunchKernelGGL(k_bse_dipole, dim3((unsigned)npts), dim3(256), 0, st, m->view, D, S.buf<cd>(BsePlan::DIP));
        TBK_HIP(hipGetLastError());
    }
    return TBK_OK;
}

// Y = H X for the nb vectors of X; dpart: the partials of Re <X|Y>, or null
int bse_apply(const BseRunState& S, int nb, const cd* X, cd* Y, double* dpart) {
    tbk_ctx* ctx = S.ctx;
    const BsePlan& pl = S.pl;
    const BseDev& D = S.D;
    hipStream_t st = ctx->stream;
    if (D.np > 0) {
        {
            ProfScope ps(ctx, "bse_pair");
            hipLaunchKernelGGL(k_bse_pair, dim3((unsigned)pl.G, (unsigned)nb, (unsigned)((D.np + BSE_EC - 1) / BSE_EC)), dim3(256), 0, st, D, X, nb,
                               S.buf<cd>(BsePlan::PART));
            TBK_HIP(hipGetLastError());
        }
        const int64_t nrows = 2 * (int64_t)nb * D.np;
        {
            ProfScope ps(ctx, "bse_rows");
            hipLaunchKernelGGL(k_pairs_rows, dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, st, (const double*)S.buf<cd>(BsePlan::PART), pl.G,
                               nrows, 0, (double*)S.buf<cd>(BsePlan::FSUM));
            TBK_HIP(hipGetLastError());
        }
        ProfScope ps(ctx, "bse_fields");
        hipLaunchKernelGGL(k_bse_fields, dim3(nblk((int64_t)nb * D.np)), dim3(256), 0, st, nb, D.ned, D.nst, D.np, (double)D.npts,
                           (const double*)S.buf<double>(BsePlan::EVV), (const int32_t*)S.buf<int32_t>(BsePlan::HPTR),
                           (const int32_t*)S.buf<int32_t>(BsePlan::HENT), (const int32_t*)S.buf<int32_t>(BsePlan::HSLOT),
                           (const cd*)S.buf<cd>(BsePlan::FSUM), S.buf<cd>(BsePlan::FS), S.buf<cd>(BsePlan::HF));
        TBK_HIP(hipGetLastError());
    }
    ProfScope ps(ctx, "bse_project");
    hipLaunchKernelGGL(k_bse_project, dim3((unsigned)pl.G, (unsigned)nb), dim3(256), 0, st, D, X, (const cd*)S.buf<cd>(BsePlan::FS),
                       (const cd*)S.buf<cd>(BsePlan::HF), Y, dpart);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

// S_ab = <D^a|D^b> (not yet divided by N) into the SAB buffer
int bse_dipole_norm(const BseRunState& S) {
    ProfScope ps(S.ctx, "bse_sab");
    hipLaunchKernelGGL(k_bse_cdots, dim3((unsigned)S.D.dk, (unsigned)S.D.dk), dim3(256), 0, S.ctx->stream, S.pl.nt,
                       (const cd*)S.buf<cd>(BsePlan::DIP), (const cd*)S.buf<cd>(BsePlan::DIP), S.D.dk, S.buf<cd>(BsePlan::SAB));
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}
BseArgs bse_args(int nint, const int32_t* ab, const int32_t* R, const double* V, double mu, int nv, const int32_t* vsel, int nc,
                 const int32_t* csel, int direct, int exchange) {
    BseArgs A;
    A.nint = nint, A.ab = ab, A.R = R, A.V = V, A.mu = mu, A.nv = nv, A.vsel = vsel, A.nc = nc, A.csel = csel;
    A.direct = direct ? 1 : 0, A.exchange = exchange ? 1 : 0;
    return A;
}
}  // namespace

extern "C" int tbk_exciton_apply_mesh(tbk_model* m, const int32_t* mesh, int nint, const int32_t* int_ab, const int32_t* int_R,
                                      const double* int_V, double mu, int nv, const int32_t* vsel, int nc, const int32_t* csel, int direct,
                                      int exchange, int nb, int xnv, int xnc, const double* vectors, double* out, double* gaps, int32_t* info) {
    const char* fn = "tbk_exciton_apply_mesh";
    TBK_REQUIRE(m && mesh && vectors && out && gaps && info, TBK_EINVAL, "%s: null argument", fn);
    TBK_REQUIRE(nb >= 1 && nb <= kBseBlockMax, TBK_EINVAL, "%s: %d vectors (1..%d)", fn, nb, kBseBlockMax);
    TBK_REQUIRE(xnv >= 1 && xnv <= kBseBandMax && xnc >= 1 && xnc <= kBseBandMax, TBK_EINVAL, "%s: vectors of %d x %d bands per point", fn, xnv, xnc);
    int64_t xpts;
    int rc = occ_mesh_check(fn, m->dim_k, m->nsta, mesh, xpts);
    if (rc) return rc;
    for (int64_t i = 0; i < 2 * xpts * xnv * xnc * nb; ++i)          // (before the mesh solve: the sizes follow from the arguments)
        TBK_REQUIRE(std::isfinite(vectors[i]), TBK_EINVAL, "%s: the vectors are not finite", fn);
    BseRunState S;
    rc = bse_setup(fn, 0, m, mesh, bse_args(nint, int_ab, int_R, int_V, mu, nv, vsel, nc, csel, direct, exchange), nb, 0, xnv, xnc, S, info);
    if (rc) return rc;
    const int64_t nt = S.pl.nt;
    hipStream_t st = S.ctx->stream;
    TBK_HIP(hipMemcpyAsync(S.buf<cd>(BsePlan::X), vectors, (size_t)nb * nt * sizeof(cd), hipMemcpyHostToDevice, st));
    rc = bse_apply(S, nb, S.buf<cd>(BsePlan::X), S.buf<cd>(BsePlan::Y), nullptr);
    if (rc) return rc;
    TBK_HIP(hipMemcpyAsync(out, S.buf<cd>(BsePlan::Y), (size_t)nb * nt * sizeof(cd), hipMemcpyDeviceToHost, st));
    TBK_HIP(hipMemcpyAsync(gaps, S.buf<double>(BsePlan::GAPS), (size_t)nt * sizeof(double), hipMemcpyDeviceToHost, st));
    TBK_HIP(hipStreamSynchronize(st));
    return TBK_OK;
}

// energies[cap], dipoles[cap][dk] c128, sab[dk][dk] c128 (already divided by N), vectors[nt][nt] c128 or null; cap: the room of the
// caller's arrays in transitions; info = {nocc, nv, nc}; scal = {gap, largest Delta}
extern "C" int tbk_exciton_states_mesh(tbk_model* m, const int32_t* mesh, int nint, const int32_t* int_ab, const int32_t* int_R,
                                       const double* int_V, double mu, int nv, const int32_t* vsel, int nc, const int32_t* csel, int direct,
                                       int exchange, int64_t cap, double* energies, double* dipoles, double* sab, double* vectors,
                                       double* scal, int32_t* info) {
    const char* fn = "tbk_exciton_states_mesh";
    TBK_REQUIRE(m && mesh && energies && dipoles && sab && scal && info, TBK_EINVAL, "%s: null argument", fn);
    BseRunState S;
    int rc = bse_setup(fn, 1, m, mesh, bse_args(nint, int_ab, int_R, int_V, mu, nv, vsel, nc, csel, direct, exchange), kBseBlockMax, 0, 0, 0, S,
                       info);
    if (rc) return rc;
    tbk_ctx* ctx = S.ctx;
    const int64_t nt = S.pl.nt;
    const int dk = S.D.dk;
    TBK_REQUIRE(nt <= cap, TBK_EINVAL, "%s: %lld transitions, room for %lld", fn, (long long)nt, (long long)cap);
    hipStream_t st = ctx->stream;
    cd *X = S.buf<cd>(BsePlan::X), *Y = S.buf<cd>(BsePlan::Y), *H = S.buf<cd>(BsePlan::HMAT);
    for (int64_t t0 = 0; t0 < nt; t0 += kBseBlockMax) {
        const int nb = (int)std::min<int64_t>(kBseBlockMax, nt - t0);
        hipLaunchKernelGGL(k_bse_unit, dim3(nblk(nt), (unsigned)nb), dim3(256), 0, st, nt, t0, X);
        TBK_HIP(hipGetLastError());
        rc = bse_apply(S, nb, X, Y, nullptr);
        if (rc) return rc;
        hipLaunchKernelGGL(k_bse_hrow, dim3(nblk(nt), (unsigned)nb), dim3(256), 0, st, nt, t0, (const cd*)Y, H);
        TBK_HIP(hipGetLastError());
    }
    rc = tbk_eigh_dev_checked(ctx, (int)nt, H, 1, S.buf<double>(BsePlan::EVAL), S.buf<cd>(BsePlan::EVEC), "bse_states");
    if (rc) return rc;
    {
        ProfScope ps(ctx, "bse_dl");                                // d^a_lambda = <A^lambda|D^a>
        hipLaunchKernelGGL(k_bse_cdots, dim3((unsigned)nt, (unsigned)dk), dim3(256), 0, st, nt, (const cd*)S.buf<cd>(BsePlan::EVEC),
                           (const cd*)S.buf<cd>(BsePlan::DIP), dk, S.buf<cd>(BsePlan::DL));
        TBK_HIP(hipGetLastError());
    }
    rc = bse_dipole_norm(S);
    if (rc) return rc;
    TBK_HIP(hipMemcpyAsync(energies, S.buf<double>(BsePlan::EVAL), (size_t)nt * sizeof(double), hipMemcpyDeviceToHost, st));
    TBK_HIP(hipMemcpyAsync(dipoles, S.buf<cd>(BsePlan::DL), (size_t)nt * dk * sizeof(cd), hipMemcpyDeviceToHost, st));
    TBK_HIP(hipMemcpyAsync(sab, S.buf<cd>(BsePlan::SAB), (size_t)dk * dk * sizeof(cd), hipMemcpyDeviceToHost, st));
    if (vectors) TBK_HIP(hipMemcpyAsync(vectors, S.buf<cd>(BsePlan::EVEC), (size_t)nt * nt * sizeof(cd), hipMemcpyDeviceToHost, st));
    TBK_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < 2 * dk * dk; ++i) sab[i] /= (double)S.D.npts;
    scal[0] = S.scal[0], scal[1] = S.scal[1];
    return TBK_OK;
}

// The runs of bse_runs(dim_k, da, db) (da < 0: the full tensor), all carried as one block: alpha[nrun][nsteps], beta[nrun][nsteps],
// norm2[nrun] = |start|^2, n_used[nrun]; sab[dk][dk] c128 divided by N; scal = {gap, largest Delta}
extern "C" int tbk_exciton_spectrum_mesh(tbk_model* m, const int32_t* mesh, int nint, const int32_t* int_ab, const int32_t* int_R,
                                         const double* int_V, double mu, int nv, const int32_t* vsel, int nc, const int32_t* csel, int direct,
                                         int exchange, int da, int db, int nsteps, double* alpha, double* beta, double* norm2,
                                         int32_t* n_used, double* sab, double* scal, int32_t* info) {
    const char* fn = "tbk_exciton_spectrum_mesh";
    TBK_REQUIRE(m && mesh && alpha && beta && norm2 && n_used && sab && scal && info, TBK_EINVAL, "%s: null argument", fn);
    const int dk = m->dim_k;
    TBK_REQUIRE((da < 0 && db < 0) || (da >= 0 && da < dk && db >= 0 && db < dk), TBK_EINVAL, "%s: directions (%d, %d) of %d", fn, da, db, dk);
    TBK_REQUIRE(nsteps >= 1 && nsteps <= kBseStepsMax, TBK_EINVAL, "%s: n_steps=%d (1..%d)", fn, nsteps, kBseStepsMax);
    TBK_REQUIRE(dk >= 1 && dk <= 3, TBK_EINVAL, "%s: dim_k=%d (1..3)", fn, dk);
    const std::vector<BseRun> runs = bse_runs(dk, da, db);
    const int nb = (int)runs.size();
    BseRunState S;
    int rc = bse_setup(fn, 2, m, mesh, bse_args(nint, int_ab, int_R, int_V, mu, nv, vsel, nc, csel, direct, exchange), nb, nsteps, 0, 0, S, info);
    if (rc) return rc;
    tbk_ctx* ctx = S.ctx;
    const BsePlan& pl = S.pl;
    const int64_t nt = pl.nt;
    hipStream_t st = ctx->stream;
    std::vector<int32_t> rt;
    for (const BseRun& r : runs) rt.push_back(r.a), rt.push_back(r.b), rt.push_back(r.kind);
    TBK_HIP(hipMemcpyAsync(S.buf<int32_t>(BsePlan::RUNS), rt.data(), rt.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    double *lz = S.buf<double>(BsePlan::LZ), *npart = S.buf<double>(BsePlan::NPART), *dpart = S.buf<double>(BsePlan::DPART);
    double *al = S.buf<double>(BsePlan::ALPHA), *be = S.buf<double>(BsePlan::BETA);
    TBK_HIP(hipMemsetAsync(al, 0, (size_t)nb * nsteps * sizeof(double), st));
    TBK_HIP(hipMemsetAsync(be, 0, (size_t)nb * nsteps * sizeof(double), st));
    cd *X = S.buf<cd>(BsePlan::X), *Y = S.buf<cd>(BsePlan::Y), *Z = S.buf<cd>(BsePlan::Z);
    hipLaunchKernelGGL(k_bse_lz_init, dim3(1), dim3(256), 0, st, nb, nsteps, (const double*)S.buf<double>(BsePlan::SCAL), lz);
    TBK_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_bse_lz_start, dim3((unsigned)pl.GN, (unsigned)nb), dim3(256), 0, st, nt, pl.GN,
                       (const int32_t*)S.buf<int32_t>(BsePlan::RUNS), (const cd*)S.buf<cd>(BsePlan::DIP), X, npart);
    TBK_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_bse_lz_beta, dim3((unsigned)nb), dim3(256), 0, st, pl.GN, -1, nsteps, (const double*)npart, lz, be);
    TBK_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_bse_lz_scale, dim3(nblk(nt), (unsigned)nb), dim3(256), 0, st, nt, (const double*)lz, X);
    TBK_HIP(hipGetLastError());
    for (int j = 0; j < nsteps; ++j) {
        rc = bse_apply(S, nb, X, Y, dpart);
        if (rc) return rc;
        ProfScope ps(ctx, "bse_lanczos");
        hipLaunchKernelGGL(k_bse_lz_alpha, dim3((unsigned)nb), dim3(256), 0, st, pl.G, j, nsteps, (const double*)dpart, lz, al);
        TBK_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_bse_lz_update, dim3((unsigned)pl.GN, (unsigned)nb), dim3(256), 0, st, nt, pl.GN, j == 0 ? 1 : 0, (const double*)lz,
                           (const cd*)X, (const cd*)Y, Z, npart);
        TBK_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_bse_lz_beta, dim3((unsigned)nb), dim3(256), 0, st, pl.GN, j, nsteps, (const double*)npart, lz, be);
        TBK_HIP(hipGetLastError());
        if (j + 1 == nsteps) break;
        hipLaunchKernelGGL(k_bse_lz_scale, dim3(nblk(nt), (unsigned)nb), dim3(256), 0, st, nt, (const double*)lz, Z);
        TBK_HIP(hipGetLastError());
        std::swap(X, Z);                                            // Q_{j+1} becomes X, Q_j becomes Z
    }
    rc = bse_dipole_norm(S);
    if (rc) return rc;
    std::vector<double> lzh((size_t)nb * 8);
    TBK_HIP(hipMemcpyAsync(alpha, al, (size_t)nb * nsteps * sizeof(double), hipMemcpyDeviceToHost, st));
    TBK_HIP(hipMemcpyAsync(beta, be, (size_t)nb * nsteps * sizeof(double), hipMemcpyDeviceToHost, st));
    TBK_HIP(hipMemcpyAsync(lzh.data(), lz, lzh.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    TBK_HIP(hipMemcpyAsync(sab, S.buf<cd>(BsePlan::SAB), (size_t)dk * dk * sizeof(cd), hipMemcpyDeviceToHost, st));
    TBK_HIP(hipStreamSynchronize(st));
    for (int r = 0; r < nb; ++r) {
        norm2[r] = lzh[8 * (size_t)r + 2] * lzh[8 * (size_t)r + 2];
        n_used[r] = (int32_t)lzh[8 * (size_t)r + 5];
    }
    for (int i = 0; i < 2 * dk * dk; ++i) sab[i] /= (double)S.D.npts;
    scal[0] = S.scal[0], scal[1] = S.scal[1];
    return TBK_OK;
}

// The continued fractions of the runs and the polarisation algebra, on the host: out[nw][dk][dk] c128 (da < 0) or out[nw]
extern "C" int tbk_exciton_reconstruct(int dim_k, int da, int db, int nsteps, const double* alpha, const double* beta, const double* norm2,
                                       const int32_t* n_used, int64_t npts, int nw, const double* omega, double eta, double* out) {
    const char* fn = "tbk_exciton_reconstruct";
    TBK_REQUIRE(alpha && beta && norm2 && n_used && out && npts >= 1, TBK_EINVAL, "%s: null argument", fn);
    int rc = bse_reconstruct_check(fn, dim_k, da, db, nsteps, nw, omega, eta);
    if (rc) return rc;
    const std::vector<BseRun> runs = bse_runs(dim_k, da, db);
    const int nr = (int)runs.size(), no = da < 0 ? dim_k * dim_k : 1;
    for (int r = 0; r < nr; ++r)
        TBK_REQUIRE(n_used[r] >= 0 && n_used[r] <= nsteps, TBK_EINVAL, "%s: run %d used %d of %d steps", fn, r, n_used[r], nsteps);
    std::vector<bse_c> g((size_t)nr), o((size_t)no);
    for (int w = 0; w < nw; ++w) {
        const bse_c z(omega[w], eta);
        for (int r = 0; r < nr; ++r) g[r] = bse_cfrac(n_used[r], alpha + (size_t)r * nsteps, beta + (size_t)r * nsteps, norm2[r], z);
        bse_tensor(dim_k, da, db, g.data(), 1.0 / (double)npts, o.data());
        for (int i = 0; i < no; ++i) out[2 * ((size_t)w * no + i)] = o[i].real(), out[2 * ((size_t)w * no + i) + 1] = o[i].imag();
    }
    return TBK_OK;
}
