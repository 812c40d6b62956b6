// tbk_dham.h -- the gradient form of the model's slot sums and its second derivative, the degeneracy rule and the groups of levels it
// defines, the 2 x 2 spin action of the spin current, the n = 2 closed form and the mesh-plane geometry of the Kubo-formula translation
// units (tbk_curv.hip, tbk_optics.hip, tbk_orbmag.hip, tbk_transport.hip, tbk_shift.hip; DESIGN.md sections 11 to 13 and 15 to 17).
// The kernels and the host pipeline they share are in tbk_kubo.h, which includes this file.
#pragma once
#include "tbk_solve_dev.h"

__device__ __forceinline__ double comp4(const double4 v, const int d) {
    return d == 0 ? v.x : (d == 1 ? v.y : (d == 2 ? v.z : v.w));
}
__device__ __forceinline__ int comp4i(const int4 v, const int d) {
    return d == 0 ? v.x : (d == 1 ? v.y : (d == 2 ? v.z : v.w));
}

// The gradient form of slot_sum: for the terms [t0, t1) of slot (a, b), a <= b, the matrix element h = H_ab(k) and its
// derivatives v0 = d_{d0} H_ab, v1 = d_{d1} H_ab.  With S = sum amp e^{2 pi i k.R}, G_d = sum amp R_d e^{2 pi i k.R} and
// p = e^{2 pi i k.(tau_b - tau_a)}:  h = p S,  d_d h = 2 pi i p (G_d + (tau_b - tau_a)_d S).  A diagonal slot holds both
// halves of every self-hopping, so S is real there and 2 pi i G_d is real (tbk_gen_ham keeps Re S).  The one copy of this
// formula: the parity hook k_gen_dham, the n = 2 lanes and the dense velocity matrices of the n != 2 path all call it.
__device__ __forceinline__ void dham_terms(const ModelView& mv, const int a, const int b, const int t0, const int t1,
                                           const double (&kk)[4], const cd (&z)[4], const int d0, const int d1, cd& h, cd& v0,
                                           cd& v1) {
    cd s{0.0, 0.0}, g0{0.0, 0.0}, g1{0.0, 0.0};
    for (int t = t0; t < t1; ++t) {
        const int4 R = mv.term_R[t];
        const cd e = cmul(mv.term_amp[t], phase_of_R(z, R));
        s = cadd(s, e);
        g0 = cadd(g0, cscale(e, (double)comp4i(R, d0)));
        g1 = cadd(g1, cscale(e, (double)comp4i(R, d1)));
    }
    const double tp = 2.0 * M_PI;
    if (a == b) {
        h = cd{s.x, 0.0};
        v0 = cd{-tp * g0.y, 0.0};
        v1 = cd{-tp * g1.y, 0.0};
        return;
    }
    const double4 oa = mv.orb[a], ob = mv.orb[b];
    const cd p = cmulc(expi2pi(kdot(kk, oa)), expi2pi(kdot(kk, ob)));   // conj(e_a) e_b, as tbk_gen_ham
    h = cmul(p, s);
    const cd q0 = cadd(g0, cscale(s, comp4(ob, d0) - comp4(oa, d0)));
    const cd q1 = cadd(g1, cscale(s, comp4(ob, d1) - comp4(oa, d1)));
    const cd pq0 = cmul(p, q0), pq1 = cmul(p, q1);
    v0 = cd{-tp * pq0.y, tp * pq0.x};
    v1 = cd{-tp * pq1.y, tp * pq1.x};
}

// The second derivative of the same slot sum: with G_de = sum amp R_d R_e e^{2 pi i k.R} and
// dt = tau_b - tau_a,  d_d d_e h = (2 pi i)^2 p (G_de + dt_d G_e + dt_e G_d + dt_d dt_e S); real on a diagonal slot, like the first
// derivative.  The one copy of this formula: the parity hook k_sh_ddham and the W matrices of tbk_shift.hip call it.
__device__ __forceinline__ cd ddham_terms(const ModelView& mv, const int a, const int b, const int t0, const int t1,
                                          const double (&kk)[4], const cd (&z)[4], const int d, const int e) {
    cd s{0.0, 0.0}, gd{0.0, 0.0}, ge{0.0, 0.0}, gde{0.0, 0.0};
    for (int t = t0; t < t1; ++t) {
        const int4 R = mv.term_R[t];
        const cd x = cmul(mv.term_amp[t], phase_of_R(z, R));
        const double rd = (double)comp4i(R, d), re = (double)comp4i(R, e);
        s = cadd(s, x);
        gd = cadd(gd, cscale(x, rd));
        ge = cadd(ge, cscale(x, re));
        gde = cadd(gde, cscale(x, rd * re));
    }
    const double c = -4.0 * M_PI * M_PI;
    if (a == b) return cd{c * gde.x, 0.0};
    const double4 oa = mv.orb[a], ob = mv.orb[b];
    const cd p = cmulc(expi2pi(kdot(kk, oa)), expi2pi(kdot(kk, ob)));   // conj(e_a) e_b, as dham_terms
    const double td = comp4(ob, d) - comp4(oa, d), te = comp4(ob, e) - comp4(oa, e);
    cd q = cadd(gde, cscale(ge, td));
    q = cadd(q, cscale(gd, te));
    q = cadd(q, cscale(s, td * te));
    return cscale(cmul(p, q), c);
}

__device__ __forceinline__ void k_phases(const ModelView& mv, const double* __restrict__ k, const int64_t ik, double (&kk)[4],
                                         cd (&z)[4]) {
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        kk[d] = d < mv.dim_k ? k[ik * mv.dim_k + d] : 0.0;
        z[d] = d < mv.dim_k ? expi2pi(kk[d]) : cd{1.0, 0.0};
    }
}

// the degeneracy rule of the interband sums: the pair (E_n, E_m), de = E_n - E_m of either sign, contributes nothing (NaN: nothing)
__device__ __forceinline__ bool kubo_degenerate(const double de, const double en, const double em) {
    return !(fabs(de) > 1e-9 * fmax(1.0, fmax(fabs(en), fabs(em))));
}

// the group [g0, g1) of band b at point ik (eval[n][nk]): a maximal run of consecutive levels, each degenerate with its predecessor
// (tbk_transport.hip and tbk_shift.hip)
__device__ __forceinline__ void band_group(const double* __restrict__ eval, const int64_t nk, const int64_t ik, const int n, const int b,
                                           int& g0, int& g1) {
    g0 = b;
    g1 = b + 1;
    double hi = eval[(int64_t)b * nk + ik];
    while (g0 > 0) {
        const double lo = eval[(int64_t)(g0 - 1) * nk + ik];
        if (!kubo_degenerate(hi - lo, hi, lo)) break;
        hi = lo;
        --g0;
    }
    double lo = eval[(int64_t)b * nk + ik];
    while (g1 < n) {
        const double up = eval[(int64_t)g1 * nk + ik];
        if (!kubo_degenerate(up - lo, up, lo)) break;
        lo = up;
        ++g1;
    }
}

// ---------------------------------------------------------------- spin current
// Sigma_s = 1_orb (x) s.sigma acts on the 2 x 2 spin blocks of a spinful model (state = 2 orbital + spin).  The one copy of its
// action: the LDS pass of k_kubo_lds, the wide build k_kubo_wsp_spin and the parity hook k_curv_jham all call these.
struct SpinVec {
    double s[3];
};
// (s.sigma)[al][be]
__device__ __forceinline__ cd spin_elem(const SpinVec& sv, const int al, const int be) {
    return al == be ? cd{al ? -sv.s[2] : sv.s[2], 0.0} : cd{sv.s[0], al ? sv.s[1] : -sv.s[1]};
}
// (Sigma_s u)[b] of a state vector u
__device__ __forceinline__ cd spin_vec(const SpinVec& sv, const cd* __restrict__ u, const int b) {
    const int be = b & 1;
    cd r = cscale(u[b], be ? -sv.s[2] : sv.s[2]);
    cfma(r, spin_elem(sv, be, be ^ 1), u[b ^ 1]);
    return r;
}
// J_ab = (Sigma_s D + D Sigma_s)_ab / 2 from dab = D_ab, dxb = D_{a^1, b} and dax = D_{a, b^1}
__device__ __forceinline__ cd spin_apply(const SpinVec& sv, const int a, const int b, const cd dab, const cd dxb, const cd dax) {
    const int al = a & 1, be = b & 1;
    cd r = cscale(dab, (al ? -sv.s[2] : sv.s[2]) + (be ? -sv.s[2] : sv.s[2]));
    cfma(r, spin_elem(sv, al, al ^ 1), dxb);
    cfma(r, dax, spin_elem(sv, be ^ 1, be));
    return cscale(r, 0.5);
}

// ---------------------------------------------------------------- n = 2: closed form in registers
struct Curv2 {
    double e0, e1, om;   // eigenvalues (ascending) and Omega_0 without the degeneracy rule (Omega_1 = -om)
    bool degenerate;     // the pair falls under the rule of (1)
};
__device__ __forceinline__ Curv2 curv2_point(const ModelView& mv, const double (&kk)[4], const int d0, const int d1) {
    cd z[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) z[d] = d < mv.dim_k ? expi2pi(kk[d]) : cd{1.0, 0.0};
    cd h[3], va[3], vb[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const int a = s == 2 ? 1 : 0, b = s == 0 ? 0 : 1;   // slots (0,0) (0,1) (1,1)
        dham_terms(mv, a, b, mv.slot_ptr[s], mv.slot_ptr[s + 1], kk, z, d0, d1, h[s], va[s], vb[s]);
    }
    // H = d0 + dx sx + dy sy + dz sz:  H_01 = dx - i dy,  H_00 - H_11 = 2 dz
    const double dx = h[1].x, dy = -h[1].y, dz = 0.5 * (h[0].x - h[2].x);
    const double ax = va[1].x, ay = -va[1].y, az = 0.5 * (va[0].x - va[2].x);
    const double bx = vb[1].x, by = -vb[1].y, bz = 0.5 * (vb[0].x - vb[2].x);
    const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
    const double d2 = dx * dx + dy * dy + dz * dz, dn = sqrt(d2);
    const double mid = 0.5 * (h[0].x + h[2].x);
    Curv2 r;
    r.e0 = mid - dn;
    r.e1 = mid + dn;
    r.om = (dx * cx + dy * cy + dz * cz) / (2.0 * d2 * dn);
    r.degenerate = kubo_degenerate(r.e1 - r.e0, r.e0, r.e1);
    return r;
}

// ---------------------------------------------------------------- mesh planes
// The (da, db) planes of k_uniform_mesh(N): slice s runs along the remaining axis (dc < 0: one slice); plane point p = ia N[db] + ib.
struct PlaneArgs {
    int N[3];
    int da, db, dc;
    int64_t nplane;
    int64_t npts;
    int nslice;
};
__device__ __forceinline__ int64_t plane_point(const PlaneArgs& P, const int s, const int64_t p, int (&ii)[3]) {
    ii[0] = ii[1] = ii[2] = 0;
    const int64_t ia = p / P.N[P.db];
    ii[P.da] = (int)ia;
    ii[P.db] = (int)(p - ia * P.N[P.db]);
    if (P.dc >= 0) ii[P.dc] = s;
    return ((int64_t)ii[0] * P.N[1] + ii[1]) * P.N[2] + ii[2];
}
// the inverse of that index: point idx of k_uniform_mesh(N) is (ii[0], ii[1], ii[2])
__device__ __forceinline__ void mesh_point(const int (&N)[3], const int64_t idx, int (&ii)[3]) {
    const int64_t i01 = idx / N[2];
    ii[2] = (int)(idx - i01 * N[2]);
    ii[0] = (int)(i01 / N[1]);
    ii[1] = (int)(i01 - (int64_t)ii[0] * N[1]);
}

// sum over the 256 threads of a workgroup in a fixed order (shuffle tree in each wavefront, then the four in order); thread 0 has it
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
