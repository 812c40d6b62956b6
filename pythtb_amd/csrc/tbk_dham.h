// tbk_dham.h -- the gradient form of the model's slot sums, shared by the Kubo-formula translation units (tbk_curv.hip,
// tbk_optics.hip; DESIGN.md sections 11 and 12).
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

__device__ __forceinline__ void k_phases(const ModelView& mv, const double* __restrict__ k, const int64_t ik, double (&kk)[4],
                                         cd (&z)[4]) {
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        kk[d] = d < mv.dim_k ? k[ik * mv.dim_k + d] : 0.0;
        z[d] = d < mv.dim_k ? expi2pi(kk[d]) : cd{1.0, 0.0};
    }
}
