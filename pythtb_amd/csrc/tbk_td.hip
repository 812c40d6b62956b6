// tbk_td.hip -- real-time propagation of Bloch states under a uniform time-dependent field: the current J(t) and
// the energy E(t) of a crystal on a k mesh, the final band populations, and the propagator of a driven window on a k list (Floquet).
//
// Velocity gauge: the field is a rigid shift of every k-point, k -> k + kappa(t), kappa[j] given at the times t_j = j dt, j = 0..nt, in
// reduced coordinates.  H and d_a H are the convention-II matrices of tbk_gen_ham / tbk_gen_dham.  With (E, V) the solver's eigenpairs:
//   start    psi_m = the eigenvectors of H(k + kappa_0) of the bands occ (weight f = 1), or all of them with the Fermi weights f_m of
//            (mu, kT) -- f = [E <= mu] at kT = 0, no spin factor
//   step     psi <- V diag(e^{-i E dt}) V^+ psi with (E, V) of H(k + (kappa_j + kappa_{j+1}) / 2): the exponential midpoint rule, exactly
//            unitary, second order in dt, a function of H alone (it does not depend on the solver's basis inside a degenerate group)
//   measure  rho(k) = sum_m f_m psi_m psi_m^+;  E(t_j) = (1 / N_k) sum_k tr H rho,  J_a(t_j) = (1 / N_k) sum_k tr d_a H rho at k + kappa_j,
//            from one walk of the non-empty slots (dham_terms): no n x n matrix of H is formed
//   end      p_n(k) = sum_m f_m |<u_n(k + kappa_nt)|psi_m>|^2 and their mesh means
// States whose weight is exactly 0 are neither advanced nor measured.
//
// The carried states psi[nprop][N_k][nsta] stay on the device for the whole call.  A time step goes through the mesh in tbk_kubo.h's
// chunk length; per chunk
//   tbk_k_uniform_mesh_range_dev, k_td_shift   the chunk's k + kappa in the chunk's k buffer: the solver is called unchanged
//   n <= 32  k_td_step_lds: a workgroup takes P points; their eigenvectors (rows of LD = n | 1 c128), phases e^{-i E dt} (sincos of
//            E dt) and carried states come into LDS, every lane forms up to TD_ES coefficients c[m][b] = <V_b|psi_m> in registers,
//            writes c e^{-i E_b dt} over the staged states, and a second pass transforms back, in place in the resident array
//   n > 32   k_td_tile<1>: X[m][b] = e^{-i E_b dt} <V_b|psi_m> in 16 x 16 tiles through LDS on the plain VALU, into the chunk's
//            workspace; k_td_tile<2>: psi_m = sum_b V_b X[m][b], the same tiles
//   k_td_observe   k-group g: a lane per (point, non-empty slot) forms rho_ba and adds Re H_ab rho_ba and the dim_k derivatives;
//            block_sum per quantity; part[g][1 + dim_k].  k_td_observe_rvec, for 5 .. 16 states whose terms are also kept by lattice
//            vector: the same sums with one phase per (point, R) -- a property of the model alone
//   k_group_rows (tbk_kubo.h)   obs[j][c] (+)= (1 / N_k) sum_g part[g][c], the groups in index order, chunk after chunk
// No floating-point atomics.  The partition (tbk_td.h) is a function of (mesh or nk, nsta, dim_k, nprop) alone: two calls give the same
// bits, and a run of nt' < nt steps gives the bits of the first nt' + 1 entries of the longer run.
#include <math.h>
#include "tbk_td.h"

// ---------------------------------------------------------------- the shifted k list
// kc[p][d] = kb[p][d] + kappa[d]
__global__ __launch_bounds__(256) void k_td_shift(const double* __restrict__ kb, const int64_t cnt, const int dk, const TdKappa kap,
                                                  double* __restrict__ kc) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= cnt * dk) return;
    const int d = (int)(e % dk);
    kc[e] = kb[e] + kap.v[d];
}

// ---------------------------------------------------------------- start
// psi[m][first + p][:] = eigenvector sel[m] (null: m) of point p of the chunk; fw[m][first + p] = its weight
__global__ __launch_bounds__(256) void k_td_init(const cd* __restrict__ evec, const double* __restrict__ ev, const int64_t cnt, const int n,
                                                 const int nprop, const int32_t* __restrict__ sel, const int64_t first, const int64_t npts,
                                                 const double mu, const double kT, cd* __restrict__ psi, double* __restrict__ fw) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= cnt * nprop * n) return;
    const int64_t p = e / ((int64_t)nprop * n);
    const int r = (int)(e - p * nprop * n), m = r / n, i = r - m * n;
    const int b = sel ? sel[m] : m;
    psi[((int64_t)m * npts + first + p) * n + i] = evec[((int64_t)b * cnt + p) * n + i];
    if (i != 0) return;
    double f = 1.0;
    if (!sel) {
        const double en = ev[(int64_t)b * cnt + p];
        f = kT == 0.0 ? (en <= mu ? 1.0 : 0.0) : fermi_terms((en - mu) / kT).f();
    }
    fw[(int64_t)m * npts + first + p] = f;
}
// the list call: psi_m = the unit vector m
__global__ __launch_bounds__(256) void k_td_identity(const int64_t total, const int64_t nk, const int n, cd* __restrict__ psi) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int i = (int)(e % n);
    const int64_t m = e / ((int64_t)nk * n);
    psi[e] = cd{i == m ? 1.0 : 0.0, 0.0};
}

// ---------------------------------------------------------------- the step, up to 32 states
// Workgroup = the points [blockIdx.x P, + np) of the chunk.  U[(p n + b) LD + i] = component i of eigenvector b; ph[p n + b] = e^{-i E_b dt};
// S[(p nprop + m) n + i] = psi_m[i], then c[m][b] e^{-i E_b dt} at the same place.  A lane owns the elements e = t, t + 256, ... of S
// (at most TD_ES): in the first pass e = (p, m, b) and the lanes of a ds_read group read U along different rows b at the same i -- the
// odd row length keeps them on different banks -- and S as a broadcast; in the second e = (p, m, i) and they read U along i.
__global__ __launch_bounds__(256) void k_td_step_lds(const cd* __restrict__ evec, const double* __restrict__ ev, const int64_t cnt, const int n,
                                                     const int nprop, const int P, const int LD, const double dt, const int64_t first,
                                                     const int64_t npts, const double* __restrict__ fw, cd* __restrict__ psi) {
    __shared__ cd U[TD_LDS_U];
    __shared__ cd S[TD_LDS_C];
    __shared__ cd ph[TD_LDS_PN];
    const int t = threadIdx.x, nn = n * n, pn = nprop * n;
    const int64_t ik0 = (int64_t)blockIdx.x * P;
    const int np = (int)std::min<int64_t>(P, cnt - ik0);
    for (int e = t; e < np * nn; e += 256) {
        const int p = e / nn, r = e - p * nn, b = r / n, i = r - b * n;
        U[(p * n + b) * LD + i] = evec[((int64_t)b * cnt + ik0 + p) * n + i];
    }
    for (int e = t; e < np * n; e += 256) {
        const int p = e / n, b = e - p * n;
        double s, c;
        sincos(ev[(int64_t)b * cnt + ik0 + p] * dt, &s, &c);
        ph[e] = cd{c, -s};
    }
    bool live[TD_ES];
    int64_t at[TD_ES];
#pragma unroll
    for (int s = 0; s < TD_ES; ++s) {
        const int e = t + 256 * s;
        live[s] = false;
        at[s] = 0;
        if (e >= np * pn) continue;
        const int p = e / pn, r = e - p * pn, m = r / n, i = r - m * n;
        const int64_t ik = first + ik0 + p;
        live[s] = !fw || fw[(int64_t)m * npts + ik] != 0.0;
        at[s] = ((int64_t)m * npts + ik) * n + i;
        S[e] = live[s] ? psi[at[s]] : cd{0.0, 0.0};
    }
    __syncthreads();
    cd c[TD_ES];
#pragma unroll
    for (int s = 0; s < TD_ES; ++s) {
        const int e = t + 256 * s;
        c[s] = cd{0.0, 0.0};
        if (!live[s]) continue;
        const int p = e / pn, r = e - p * pn, m = r / n, b = r - m * n;
        const cd* ub = U + (p * n + b) * LD;
        const cd* sm = S + (p * nprop + m) * n;
        cd a{0.0, 0.0};
        for (int i = 0; i < n; ++i) cfmac_x(a, sm[i], ub[i]);      // += psi[i] conj(u_b[i])
        c[s] = cmul_x(a, ph[p * n + b]);
    }
    __syncthreads();                                               // (every lane has read the staged states)
#pragma unroll
    for (int s = 0; s < TD_ES; ++s)
        if (live[s]) S[t + 256 * s] = c[s];
    __syncthreads();
#pragma unroll
    for (int s = 0; s < TD_ES; ++s) {
        const int e = t + 256 * s;
        if (!live[s]) continue;
        const int p = e / pn, r = e - p * pn, m = r / n, i = r - m * n;
        const cd* up = U + p * n * LD + i;
        const cd* xm = S + (p * nprop + m) * n;
        cd a{0.0, 0.0};
        for (int b = 0; b < n; ++b) cfma_x(a, up[b * LD], xm[b]);
        psi[at[s]] = a;
    }
}

// ---------------------------------------------------------------- the step, 33 .. 2048 states
// Workgroup (point p, tile (tm, tc)): lane (ty, tx) owns the element (16 tm + ty, 16 tc + tx) of
//   PHASE 1   X[m][b] = e^{-i E_b dt} sum_i psi_m[i] conj(V_b[i])      (both operands read along i)
//   PHASE 2   psi_m[i] = sum_b X[m][b] V_b[i]
// strips of 16 through LDS (rows of 17: a column read of Bs falls on 16 different banks).  A tile whose 16 states all have weight 0 at
// this point is skipped by both phases (uniform over the workgroup).
template <int PHASE>
__global__ __launch_bounds__(256) void k_td_tile(const cd* __restrict__ evec, const double* __restrict__ ev, const int64_t cnt, const int n,
                                                 const int nprop, const int T, const double dt, const int64_t first, const int64_t npts,
                                                 const double* __restrict__ fw, cd* __restrict__ psi, cd* __restrict__ X) {
    __shared__ cd As[16][17], Bs[16][17];
    __shared__ double fs[16];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int64_t p = blockIdx.x;
    const int tm = blockIdx.y / T, tc = blockIdx.y - tm * T;
    const int m0 = tm * 16, c0 = tc * 16, m = m0 + ty, col = c0 + tx;
    if (fw) {
        if (t < 16) fs[t] = m0 + t < nprop ? fw[(int64_t)(m0 + t) * npts + first + p] : 0.0;
        __syncthreads();
        bool any = false;
#pragma unroll
        for (int q = 0; q < 16; ++q) any = any || fs[q] != 0.0;
        if (!any) return;
    }
    const cd* pm = psi + ((int64_t)(m < nprop ? m : 0) * npts + first + p) * n;
    const cd* xm = X + ((int64_t)p * nprop + (m < nprop ? m : 0)) * n;
    cd acc{0.0, 0.0};
    for (int k0 = 0; k0 < n; k0 += 16) {
        __syncthreads();                                           // (the previous strip is consumed)
        const int kx = k0 + tx;
        if (PHASE == 1) {
            As[ty][tx] = (m < nprop && kx < n) ? pm[kx] : cd{0.0, 0.0};
            const int b = c0 + ty;
            Bs[ty][tx] = (b < n && kx < n) ? evec[((int64_t)b * cnt + p) * n + kx] : cd{0.0, 0.0};
        } else {
            As[ty][tx] = (m < nprop && kx < n) ? xm[kx] : cd{0.0, 0.0};
            const int b = k0 + ty;
            Bs[ty][tx] = (b < n && col < n) ? evec[((int64_t)b * cnt + p) * n + col] : cd{0.0, 0.0};
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            if (PHASE == 1) cfmac_x(acc, As[ty][kk], Bs[tx][kk]);
            else cfma_x(acc, As[ty][kk], Bs[kk][tx]);
        }
    }
    if (m >= nprop || col >= n) return;
    if (PHASE == 1) {
        double s, c;
        sincos(ev[(int64_t)col * cnt + p] * dt, &s, &c);
        X[((int64_t)p * nprop + m) * n + col] = cmul_x(acc, cd{c, -s});
    } else {
        psi[((int64_t)m * npts + first + p) * n + col] = acc;
    }
}

// ---------------------------------------------------------------- the measurement
// k-group g (blockIdx.x): the points [g cnt / G, (g + 1) cnt / G) of the chunk.  Lane t takes the items (point, non-empty slot)
// t, t + 256, ... of the group in order: rho_ba = sum_m f_m psi_m[b] conj(psi_m[a]) for the slot (a, b), a <= b, and the slot's part of
// tr H rho -- H_aa rho_aa, or H_ab rho_ba + its conjugate -- with the same for every d_d H, at k + kappa.  part[g][nr]: E, J_0, ...
__global__ __launch_bounds__(256) void k_td_observe(const ModelView mv, const double* __restrict__ kb, const TdKappa kap, const int64_t cnt,
                                                    const int64_t first, const int64_t npts, const int nprop, const double* __restrict__ fw,
                                                    const cd* __restrict__ psi, const int G, double* __restrict__ part) {
    __shared__ double red[TD_NR][4];
    const int n = mv.nsta, dk = mv.dim_k, nr = 1 + dk, g = blockIdx.x;
    const int64_t p0 = (int64_t)g * cnt / G, p1 = (int64_t)(g + 1) * cnt / G;
    const int64_t items = (p1 - p0) * mv.nnz;
    double acc[TD_NR] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t e = threadIdx.x; e < items; e += 256) {
        const int64_t pl = e / mv.nnz, p = p0 + pl;
        const int4 z4 = mv.nz[e - pl * mv.nnz];
        const int a = z4.x & 0xffff, b = z4.x >> 16;
        double kk[4];
        cd z[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            kk[d] = d < dk ? kb[p * dk + d] + kap.v[d < 3 ? d : 0] : 0.0;
            z[d] = d < dk ? expi2pi(kk[d]) : cd{1.0, 0.0};
        }
        cd h, v[3], hx, vx;
        dham_terms(mv, a, b, z4.y, z4.z, kk, z, 0, 1, h, v[0], v[1]);
        v[2] = cd{0.0, 0.0};
        if (dk == 3) dham_terms(mv, a, b, z4.y, z4.z, kk, z, 2, 2, hx, v[2], vx);
        cd r{0.0, 0.0};
        for (int m = 0; m < nprop; ++m) {
            const double f = fw[(int64_t)m * npts + first + p];
            if (f == 0.0) continue;
            const cd* pm = psi + ((int64_t)m * npts + first + p) * n;
            cfmac_x(r, cscale(pm[b], f), pm[a]);                   // += f psi[b] conj(psi[a])
        }
        const double w = a == b ? 1.0 : 2.0;
        acc[0] += w * fma(h.x, r.x, -(h.y * r.y));
#pragma unroll
        for (int d = 0; d < 3; ++d)
            if (d < dk) acc[1 + d] += w * fma(v[d].x, r.x, -(v[d].y * r.y));
    }
#pragma unroll
    for (int c = 0; c < TD_NR; ++c) {
        if (c >= nr) break;
        const double tot = block_sum(acc[c], red[c]);
        if (threadIdx.x == 0) part[(int64_t)g * nr + c] = tot;
    }
}

// The same sums for 5 .. 16 states whose terms are also kept by lattice vector (ModelView.rblock: every Wannier-type table): one phase
// e^{2 pi i k.R} per (point, R) instead of one per term.  With sigma_s = w_s p_s rho_ba for the slot s = (a, b) -- w = 1 on the diagonal,
// else 2 and p = conj(e_a) e_b the orbital phases -- and dtau_s = tau_b - tau_a:
//   tr H rho = sum_R Re [e^{2 pi i k.R} T_0(R)],   tr d_d H rho = -2 pi sum_R Im [e^{2 pi i k.R} (R_d T_0(R) + T_d(R))],
//   T_0(R) = sum_s U_R[s] sigma_s,   T_d(R) = sum_s U_R[s] dtau_s,d sigma_s.
// k-group g as k_td_observe, in batches of TD_OB_PB points: the orbital phases of the batch, then sigma (a lane per (point, slot);
// an empty slot gives 0), then a lane per (point, R), which walks the slots of U_R in order.
__global__ __launch_bounds__(256) void k_td_observe_rvec(const ModelView mv, const double* __restrict__ kb, const TdKappa kap, const int64_t cnt,
                                                         const int64_t first, const int64_t npts, const int nprop,
                                                         const double* __restrict__ fw, const cd* __restrict__ psi, const int G,
                                                         double* __restrict__ part) {
    __shared__ cd sig[TD_OB_PB][TD_OB_SLOTS];
    __shared__ double dtau[3][TD_OB_SLOTS];
    __shared__ cd eo[TD_OB_PB][16];
    __shared__ cd zs[TD_OB_PB][4];
    __shared__ double red[TD_NR][4];
    const int n = mv.nsta, dk = mv.dim_k, nr = 1 + dk, ns = mv.nslot, g = blockIdx.x, t = threadIdx.x;
    const int64_t p0 = (int64_t)g * cnt / G, p1 = (int64_t)(g + 1) * cnt / G;
    for (int s = t; s < ns; s += 256) {
        const int ab = mv.slot_ab[s];
        const double4 oa = mv.orb[ab & 0xffff], ob = mv.orb[ab >> 16];
#pragma unroll
        for (int d = 0; d < 3; ++d) dtau[d][s] = comp4(ob, d) - comp4(oa, d);
    }
    double acc[TD_NR] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t b0 = p0; b0 < p1; b0 += TD_OB_PB) {
        const int np = (int)std::min<int64_t>(TD_OB_PB, p1 - b0);
        __syncthreads();                                           // (the previous batch is consumed; dtau is written)
        for (int e = t; e < np * n; e += 256) {
            const int pp = e / n, o = e - pp * n;
            double kk[4];
#pragma unroll
            for (int d = 0; d < 4; ++d) kk[d] = d < dk ? kb[(b0 + pp) * dk + d] + kap.v[d < 3 ? d : 0] : 0.0;
            eo[pp][o] = expi2pi(kdot(kk, mv.orb[o]));
            if (o == 0)
#pragma unroll
                for (int d = 0; d < 4; ++d) zs[pp][d] = d < dk ? expi2pi(kk[d]) : cd{1.0, 0.0};
        }
        __syncthreads();
        for (int e = t; e < np * ns; e += 256) {
            const int pp = e / ns, s = e - pp * ns;
            cd sg{0.0, 0.0};
            if (mv.slot_ptr[s + 1] > mv.slot_ptr[s]) {
                const int ab = mv.slot_ab[s], a = ab & 0xffff, b = ab >> 16;
                const int64_t ik = first + b0 + pp;
                cd r{0.0, 0.0};
                for (int m = 0; m < nprop; ++m) {
                    const double f = fw[(int64_t)m * npts + ik];
                    if (f == 0.0) continue;
                    const cd* pm = psi + ((int64_t)m * npts + ik) * n;
                    cfmac_x(r, cscale(pm[b], f), pm[a]);           // += f psi[b] conj(psi[a])
                }
                sg = a == b ? cd{r.x, 0.0} : cscale(cmul(cmulc(eo[pp][a], eo[pp][b]), r), 2.0);
            }
            sig[pp][s] = sg;
        }
        __syncthreads();
        for (int e = t; e < np * mv.nR; e += 256) {
            const int pp = e / mv.nR, r = e - pp * mv.nR;
            const int4 R = mv.rvec[r];
            const cd z[4] = {zs[pp][0], zs[pp][1], zs[pp][2], zs[pp][3]};
            const cd ph = phase_of_R(z, R);
            const cd* u = mv.rblock + (size_t)r * ns;
            cd t0{0.0, 0.0}, td[3] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
            for (int s = 0; s < ns; ++s) {
                const cd amp = u[s];
                if (amp.x == 0.0 && amp.y == 0.0) continue;
                const cd x = cmul(amp, sig[pp][s]);
                t0 = cadd(t0, x);
#pragma unroll
                for (int d = 0; d < 3; ++d) td[d] = cadd(td[d], cscale(x, dtau[d][s]));
            }
            acc[0] += ph.x * t0.x - ph.y * t0.y;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                if (d >= dk) break;
                const cd y = cadd(cscale(t0, (double)comp4i(R, d)), td[d]);
                acc[1 + d] -= 2.0 * M_PI * (ph.x * y.y + ph.y * y.x);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < TD_NR; ++c) {
        if (c >= nr) break;
        const double tot = block_sum(acc[c], red[c]);
        if (t == 0) part[(int64_t)g * nr + c] = tot;
    }
}

// ---------------------------------------------------------------- the final populations
// kpop[b][first + p] = sum_m f_m |<u_b|psi_m>|^2, a lane per (band b, point p) of the chunk
__global__ __launch_bounds__(256) void k_td_pop(const cd* __restrict__ evec, const int64_t cnt, const int n, const int nprop, const int64_t first,
                                                const int64_t npts, const double* __restrict__ fw, const cd* __restrict__ psi,
                                                double* __restrict__ kpop) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= cnt * n) return;
    const int64_t b = e / cnt, p = e - b * cnt;
    const cd* u = evec + (b * cnt + p) * n;
    double s = 0.0;
    for (int m = 0; m < nprop; ++m) {
        const double f = fw[(int64_t)m * npts + first + p];
        if (f == 0.0) continue;
        const cd* pm = psi + ((int64_t)m * npts + first + p) * n;
        cd o{0.0, 0.0};
        for (int i = 0; i < n; ++i) cfmac_x(o, pm[i], u[i]);
        s = fma(f, fma(o.x, o.x, o.y * o.y), s);
    }
    kpop[b * npts + first + p] = s;
}

// ---------------------------------------------------------------- host side
struct TdRun {
    tbk_model* m;
    tbk_ctx* ctx;
    TdPlan pl;
    KuboChunks cw;
    const int32_t* mesh;      // null: the list call
    double* k_all;            // the list's k on the device (list call)
    cd* psi;
    double* fw;               // null: the list call (every state is carried)
    double* part;
    double dt;
};

// body(first, cnt, kbase, eval, evec) for every chunk, solved at kbase + kap
template <class Body>
static int td_for_chunks(const TdRun& R, const TdKappa& kap, Body&& body) {
    tbk_ctx* ctx = R.ctx;
    const int dk = R.pl.dk;
    double* kc = (double*)(R.cw.base + R.cw.off[0]);
    double* ec = (double*)(R.cw.base + R.cw.off[1]);
    cd* vc = (cd*)(R.cw.base + R.cw.off[2]);
    for (int64_t first = 0; first < R.pl.npts; first += R.pl.chunk) {
        const int64_t cnt = std::min<int64_t>(R.pl.chunk, R.pl.npts - first);
        const double* kb = R.k_all + first * dk;
        if (R.mesh) {
            double* kbuf = R.cw.extra<double>(0);
            int rc = tbk_k_uniform_mesh_range_dev(ctx, dk, R.mesh, first, cnt, kbuf);
            if (rc) return rc;
            kb = kbuf;
        }
        {
            ProfScope ps(ctx, "td_shift");
            hipLaunchKernelGGL(k_td_shift, dim3(nblk(cnt * dk)), dim3(256), 0, ctx->stream, kb, cnt, dk, kap, kc);
            TBK_HIP(hipGetLastError());
        }
        int rc = tbk_solve_list_dev_checked(R.m, kc, cnt, ec, (double*)vc);
        if (rc) return rc;
        rc = body(first, cnt, kb, (const double*)ec, (const cd*)vc);
        if (rc) return rc;
    }
    return TBK_OK;
}

// psi <- exp(-i H(k + kap) dt) psi on the chunk
static int td_step_chunk(const TdRun& R, int64_t first, int64_t cnt, const double* ec, const cd* vc) {
    tbk_ctx* ctx = R.ctx;
    const TdPlan& pl = R.pl;
    if (pl.lds) {
        ProfScope ps(ctx, "td_step_lds");
        hipLaunchKernelGGL(k_td_step_lds, dim3((unsigned)((cnt + pl.P - 1) / pl.P)), dim3(256), 0, ctx->stream, vc, ec, cnt, pl.n, pl.nprop,
                           pl.P, pl.LD, R.dt, first, pl.npts, (const double*)R.fw, R.psi);
        TBK_HIP(hipGetLastError());
        return TBK_OK;
    }
    cd* X = R.cw.extra<cd>(1);
    const dim3 grid((unsigned)cnt, (unsigned)(pl.TM * pl.T));
    {
        ProfScope ps(ctx, "td_tile_c");
        hipLaunchKernelGGL(k_td_tile<1>, grid, dim3(256), 0, ctx->stream, vc, ec, cnt, pl.n, pl.nprop, pl.T, R.dt, first, pl.npts,
                           (const double*)R.fw, R.psi, X);
        TBK_HIP(hipGetLastError());
    }
    ProfScope ps(ctx, "td_tile_psi");
    hipLaunchKernelGGL(k_td_tile<2>, grid, dim3(256), 0, ctx->stream, vc, ec, cnt, pl.n, pl.nprop, pl.T, R.dt, first, pl.npts,
                       (const double*)R.fw, R.psi, X);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

// obs[row] (+)= the chunk's E and J at kbase + kap
static int td_observe_chunk(const TdRun& R, int64_t first, int64_t cnt, const double* kb, const TdKappa& kap, double* row) {
    tbk_ctx* ctx = R.ctx;
    const TdPlan& pl = R.pl;
    if (td_observe_by_vector(pl.n, R.m->view.nR)) {
        ProfScope ps(ctx, "td_observe_rvec");
        hipLaunchKernelGGL(k_td_observe_rvec, dim3((unsigned)pl.G), dim3(256), 0, ctx->stream, R.m->view, kb, kap, cnt, first, pl.npts,
                           pl.nprop, (const double*)R.fw, (const cd*)R.psi, pl.G, R.part);
        TBK_HIP(hipGetLastError());
    } else {
        ProfScope ps(ctx, "td_observe");
        hipLaunchKernelGGL(k_td_observe, dim3((unsigned)pl.G), dim3(256), 0, ctx->stream, R.m->view, kb, kap, cnt, first, pl.npts, pl.nprop,
                           (const double*)R.fw, (const cd*)R.psi, pl.G, R.part);
        TBK_HIP(hipGetLastError());
    }
    ProfScope ps(ctx, "td_rows");
    hipLaunchKernelGGL(k_group_rows, dim3((unsigned)pl.nr), dim3(256), 0, ctx->stream, (const double*)R.part, pl.G, (int64_t)pl.nr,
                       1.0 / (double)pl.npts, first > 0 ? 1 : 0, row);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

extern "C" int tbk_propagate_mesh(tbk_model* m, const int32_t* mesh, int nt, const double* shift, double dt, int nocc, const int32_t* occ,
                                  double mu, double kT, double* current, double* energy, double* pop_or_null, double* kpop_or_null) {
    const char* fn = "tbk_propagate_mesh";
    TBK_REQUIRE(m && current && energy, TBK_EINVAL, "%s: null argument", fn);
    const int dk = m->dim_k, n = m->nsta;
    int64_t npts;
    int nprop;
    int rc = td_mesh_check(fn, dk, n, mesh, nt, shift, dt, nocc, occ, mu, kT, npts, nprop);
    if (rc) return rc;
    TdRun R;
    R.m = m, R.ctx = m->ctx, R.mesh = mesh, R.dt = dt;
    R.pl = td_plan(n, dk, npts, nprop, nt, true);
    const TdPlan& pl = R.pl;
    tbk_ctx* ctx = m->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    void* base = nullptr;
    rc = tbk_ctx_scratch(ctx, pl.total, &base);
    if (rc) return rc;
    unsigned char* b = (unsigned char*)base;
    int32_t* sel_dev = (int32_t*)(b + pl.off_sel);
    double* kpop = (double*)(b + pl.off_kpop);
    double* pop = (double*)(b + pl.off_pop);
    double* obs = (double*)(b + pl.off_obs);
    R.k_all = nullptr;
    R.psi = (cd*)(b + pl.off_psi);
    R.fw = (double*)(b + pl.off_fw);
    R.part = (double*)(b + pl.off_part);
    R.cw = pl.cw;
    R.cw.base = b + pl.off_chunks;
    if (occ) {
        TBK_HIP(hipMemcpyAsync(sel_dev, occ, (size_t)nocc * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        TBK_HIP(hipStreamSynchronize(ctx->stream));                 // (occ may be the caller's temporary)
    }
    const int nr = pl.nr;
    // t_0: the starting states and the first measurement
    const TdKappa k0 = td_kappa(shift, dk, 0);
    rc = td_for_chunks(R, k0, [&](int64_t first, int64_t cnt, const double* kb, const double* ec, const cd* vc) -> int {
        {
            ProfScope ps(ctx, "td_init");
            hipLaunchKernelGGL(k_td_init, dim3(nblk(cnt * nprop * n)), dim3(256), 0, ctx->stream, vc, ec, cnt, n, nprop,
                               occ ? (const int32_t*)sel_dev : (const int32_t*)nullptr, first, npts, mu, kT, R.psi, R.fw);
            TBK_HIP(hipGetLastError());
        }
        return td_observe_chunk(R, first, cnt, kb, k0, obs);
    });
    if (rc) return rc;
    for (int j = 0; j < nt; ++j) {
        const TdKappa mid = td_kappa_mid(shift, dk, j), next = td_kappa(shift, dk, (int64_t)j + 1);
        double* row = obs + (size_t)(j + 1) * nr;
        rc = td_for_chunks(R, mid, [&](int64_t first, int64_t cnt, const double* kb, const double* ec, const cd* vc) -> int {
            int r2 = td_step_chunk(R, first, cnt, ec, vc);
            return r2 ? r2 : td_observe_chunk(R, first, cnt, kb, next, row);
        });
        if (rc) return rc;
    }
    const bool want_pop = pop_or_null || kpop_or_null;
    if (want_pop) {
        rc = td_for_chunks(R, td_kappa(shift, dk, nt), [&](int64_t first, int64_t cnt, const double*, const double*, const cd* vc) -> int {
            ProfScope ps(ctx, "td_pop");
            hipLaunchKernelGGL(k_td_pop, dim3(nblk(cnt * n)), dim3(256), 0, ctx->stream, vc, cnt, n, nprop, first, npts, (const double*)R.fw,
                               (const cd*)R.psi, kpop);
            TBK_HIP(hipGetLastError());
            return TBK_OK;
        });
        if (rc) return rc;
        ProfScope ps(ctx, "td_pop_rows");                           // the mesh mean of every band: one workgroup per band, a fixed order
        rc = kubo_rows_launch(ctx, kpop, (int)npts, n, pop);
        if (rc) return rc;
    }
    std::vector<double> host((size_t)(nt + 1) * nr), ph((size_t)n);
    TBK_HIP(hipMemcpyAsync(host.data(), obs, host.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (pop_or_null) TBK_HIP(hipMemcpyAsync(ph.data(), pop, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (kpop_or_null)
        TBK_HIP(hipMemcpyAsync(kpop_or_null, kpop, (size_t)n * npts * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    for (int j = 0; j <= nt; ++j) {
        energy[j] = host[(size_t)j * nr];
        for (int d = 0; d < dk; ++d) current[(size_t)j * dk + d] = host[(size_t)j * nr + 1 + d];
    }
    if (pop_or_null)
        for (int i = 0; i < n; ++i) pop_or_null[i] = ph[(size_t)i] / (double)npts;
    return TBK_OK;
}

extern "C" int tbk_propagator_list(tbk_model* m, const double* k, int64_t nk, int nt, const double* shift, double dt, double* u_out) {
    const char* fn = "tbk_propagator_list";
    TBK_REQUIRE(m && u_out, TBK_EINVAL, "%s: null argument", fn);
    const int dk = m->dim_k, n = m->nsta;
    int rc = td_list_check(fn, dk, n, nk, k, nt, shift, dt);
    if (rc) return rc;
    TdRun R;
    R.m = m, R.ctx = m->ctx, R.mesh = nullptr, R.dt = dt;
    R.pl = td_plan(n, dk, nk, n, nt, false);
    const TdPlan& pl = R.pl;
    tbk_ctx* ctx = m->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    void* base = nullptr;
    rc = tbk_ctx_scratch(ctx, pl.total, &base);
    if (rc) return rc;
    unsigned char* b = (unsigned char*)base;
    R.k_all = (double*)(b + pl.off_k);
    R.psi = (cd*)(b + pl.off_psi);
    R.fw = nullptr;
    R.part = nullptr;
    R.cw = pl.cw;
    R.cw.base = b + pl.off_chunks;
    TBK_HIP(hipMemcpyAsync(R.k_all, k, (size_t)nk * dk * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));                     // (k may be the caller's temporary)
    {
        ProfScope ps(ctx, "td_identity");
        hipLaunchKernelGGL(k_td_identity, dim3(nblk(pl.psi_cd)), dim3(256), 0, ctx->stream, pl.psi_cd, nk, n, R.psi);
        TBK_HIP(hipGetLastError());
    }
    for (int j = 0; j < nt; ++j) {
        rc = td_for_chunks(R, td_kappa_mid(shift, dk, j), [&](int64_t first, int64_t cnt, const double*, const double* ec, const cd* vc) -> int {
            return td_step_chunk(R, first, cnt, ec, vc);
        });
        if (rc) return rc;
    }
    // psi[j][k][i] = <i|U(k)|j>  ->  u_out[k][i][j]
    std::vector<cd> host((size_t)pl.psi_cd);
    TBK_HIP(hipMemcpyAsync(host.data(), R.psi, host.size() * sizeof(cd), hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    cd* out = (cd*)u_out;
    for (int64_t q = 0; q < nk; ++q)
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) out[(q * n + i) * n + j] = host[(size_t)(((int64_t)j * nk + q) * n + i)];
    return TBK_OK;
}
