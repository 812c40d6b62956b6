// tbk_sgf.h -- the decimation of the principal layer, once, for the two translation units built on it (tbk_surface.hip, DESIGN.md
// section 18; tbk_landauer.hip, section 19).  Device side: the fields both argument structs share (SgfCommon), H_ab of a slot and the
// kernel of the layer blocks H00 and H01, the 2 x 2 helpers and the decimation of the lane-per-problem regime (sgf_decimate_n2), the
// Gauss-Jordan elimination, the group maximum, a workgroup's problem and slots (sgf_problem), the decimation of the workgroup regimes
// (sgf_decimate_wg) and the resolvent solve xa = (z - E)^-1 R (sgf_resolve).  Host side: the limits of a call, the shape of a launch,
// the three-regime launcher (sgf_launch), the checks of the cut model and of the per-call arguments, and the chunk driver (sgf_plan,
// sgf_drive).  A unit adds what it does with es and et when the decimation ends.  Kernels are static: each unit holds its own copy.
// k_sgf_wg of tbk_surface.hip holds a literal copy of sgf_problem, sgf_decimate_wg and sgf_resolve (it is faster so): change them together.
#pragma once
#include "tbk_pairs.h"

static const size_t kSgfChunkBytes = (size_t)256 << 20;     // blocks + results of one chunk of k points
static const int64_t kSgfChunkProblems = (int64_t)1 << 20;  // (k, w) problems of one chunk at most
static const int kSgfMaxN = 128;
static const size_t kSgfMaxBytes = (size_t)4 << 30;         // device memory of one call (a chunk never holds less than one k point)

// what SgfArgs and LandArgs share: all the decimation reads and writes
struct SgfCommon {
    const cd* blk;        // [nk][2][N][N]: H00, H01 of the chunk's k points
    const double* omega;  // [nw]
    int nw, N;            // frequencies, layer size
    double eta, tol;
    int max_iter;
    int64_t nprob;        // nk nw, problem p = ik nw + iw
    int* info;            // [nprob] decimation steps taken, or null
    unsigned long long* fail;   // count of problems that missed a non-zero tol
};

// ---------------------------------------------------------------- H00, H01
// H_ab of the non-empty slot z4 = (a | b << 16, first term, end of terms) at k point ik, as gen_ham_entry forms it
__device__ __forceinline__ cd sgf_hab(const ModelView& mv, const double* __restrict__ k, const int64_t ik, const int4 z4) {
    const int a = z4.x & 0xffff, b = z4.x >> 16;
    double kk[4];
    cd z[4];
    k_phases(mv, k, ik, kk, z);
    cd s{0.0, 0.0};
    for (int t = z4.y; t < z4.z; ++t) cfma(s, mv.term_amp[t], phase_of_R(z, mv.term_R[t]));
    if (a == b) return cd{s.x, 0.0};
    const cd ea = expi2pi(kdot(kk, mv.orb[a])), eb = expi2pi(kdot(kk, mv.orb[b]));
    return cmul(cmulc(ea, eb), s);
}

// one thread per (k, non-empty slot (a, b), a <= b) of the cut model; rows a < N only
static __global__ __launch_bounds__(256) void k_sgf_blocks(const ModelView mv, const double* __restrict__ k, const int64_t nk, const int N,
                                                    cd* __restrict__ blk) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nk * mv.nnz) return;
    const int64_t ik = idx / mv.nnz;
    const int4 z4 = mv.nz[idx - ik * mv.nnz];
    const int a = z4.x & 0xffff, b = z4.x >> 16;
    if (a >= N || b >= 2 * N) return;
    const cd v = sgf_hab(mv, k, ik, z4);
    cd* h00 = blk + ik * 2 * N * N;
    cd* h01 = h00 + N * N;
    if (a == b) {
        h00[a * N + a] = v;
    } else if (b < N) {
        h00[a * N + b] = v;
        h00[b * N + a] = cconj(v);
    } else {
        h01[a * N + (b - N)] = v;
    }
}

// ---------------------------------------------------------------- N = 2: a lane per problem
struct M2 {
    cd a, b, c, d;   // [[a b] [c d]]
};
__device__ __forceinline__ M2 m2mul(const M2& x, const M2& y) {
    M2 r;
    r.a = cmul_x(x.a, y.a);
    cfma_x(r.a, x.b, y.c);
    r.b = cmul_x(x.a, y.b);
    cfma_x(r.b, x.b, y.d);
    r.c = cmul_x(x.c, y.a);
    cfma_x(r.c, x.d, y.c);
    r.d = cmul_x(x.c, y.b);
    cfma_x(r.d, x.d, y.d);
    return r;
}
__device__ __forceinline__ void m2acc(M2& x, const M2& y) {
    x.a = cadd(x.a, y.a);
    x.b = cadd(x.b, y.b);
    x.c = cadd(x.c, y.c);
    x.d = cadd(x.d, y.d);
}
__device__ __forceinline__ double m2max(const M2& x) { return fmax(fmax(cabs2(x.a), cabs2(x.b)), fmax(cabs2(x.c), cabs2(x.d))); }
// (z - e)^-1 by the adjugate
__device__ __forceinline__ M2 m2resolvent(const cd z, const M2& e) {
    const cd a = csub(z, e.a), d = csub(z, e.d), b = cd{-e.b.x, -e.b.y}, c = cd{-e.c.x, -e.c.y};
    cd det = cmul_x(a, d);
    cfma_x(det, cd{-b.x, -b.y}, c);
    const double q = 1.0 / cabs2(det);
    const cd id{det.x * q, -det.y * q};
    M2 r;
    r.a = cmul_x(d, id);
    r.b = cmul_x(cd{-b.x, -b.y}, id);
    r.c = cmul_x(cd{-c.x, -c.y}, id);
    r.d = cmul_x(a, id);
    return r;
}
// e = es + (et - h0): exactly h0 before the first step
__device__ __forceinline__ M2 m2bulk(const M2& es, const M2& et, const M2& h0) {
    M2 r;
    r.a = cadd(es.a, csub(et.a, h0.a));
    r.b = cadd(es.b, csub(et.b, h0.b));
    r.c = cadd(es.c, csub(et.c, h0.c));
    r.d = cadd(es.d, csub(et.d, h0.d));
    return r;
}

__device__ __forceinline__ M2 m2load(const cd* h) { return M2{h[0], h[1], h[2], h[3]}; }
__device__ __forceinline__ M2 m2dag(const M2& x) { return M2{cconj(x.a), cconj(x.c), cconj(x.b), cconj(x.d)}; }

// problem p of a lane decimated: what the loop ends with, and where the problem is
struct Sgf2 {
    int64_t ik;
    int iw;
    const cd* h;     // H00, H01 of the k point
    cd z;
    M2 h0, es, et;   // G_0 = (z - es)^-1, G_1 = (z - et)^-1, G_b = (z - m2bulk(es, et, h0))^-1
};
// stops at the first step count, 0 included, with max(|al|, |be|) <= tol max(|H00|, |H01|), or after max_iter steps; counts a
// problem that missed a non-zero tol in A.fail and stores its steps in A.info
__device__ __forceinline__ Sgf2 sgf_decimate_n2(const SgfCommon& A, const int64_t p) {
    Sgf2 D;
    D.ik = p / A.nw;
    D.iw = (int)(p - D.ik * A.nw);
    D.h = A.blk + D.ik * 8;
    D.h0 = m2load(D.h);
    M2 al = m2load(D.h + 4);
    M2 be = m2dag(al);
    D.es = D.h0, D.et = D.h0;
    D.z = cd{A.omega[D.iw], A.eta};
    const double scale = sqrt(fmax(m2max(D.h0), m2max(al)));
    double cur = sqrt(m2max(al));
    int steps = 0;
    bool conv = false;
    for (;;) {
        if (A.tol > 0.0 && cur <= A.tol * scale) {
            conv = true;
            break;
        }
        if (steps == A.max_iter) break;
        const M2 g = m2resolvent(D.z, m2bulk(D.es, D.et, D.h0));
        const M2 xa = m2mul(g, al), xb = m2mul(g, be);
        m2acc(D.es, m2mul(al, xb));
        m2acc(D.et, m2mul(be, xa));
        const M2 na = m2mul(al, xa), nb = m2mul(be, xb);
        al = na;
        be = nb;
        cur = sqrt(fmax(m2max(al), m2max(be)));
        ++steps;
    }
    if (A.tol > 0.0 && !conv) atomicAdd(A.fail, 1ull);
    if (A.info) A.info[p] = steps;
    return D;
}

// ---------------------------------------------------------------- N != 2: TP threads per problem, matrices in LDS or in a workspace
// column j of the augmented matrix [wm | xa | xb]
__device__ __forceinline__ cd* sgf_col(cd* wm, cd* xa, cd* xb, const int N, const int j) {
    return j < N ? wm + j : (j < 2 * N ? xa + (j - N) : xb + (j - 2 * N));
}

// [xa xb] := wm^-1 [xa xb] (W = 3 N) or xa := wm^-1 xa (W = 2 N); wm is used up.  Gauss-Jordan with partial pivoting: per column the
// pivot search (every thread for itself, the first largest modulus), the swap and scaling of the pivot row right of the column, the
// elimination of every other row.  Column c itself is never rewritten: the multiplier of the swapped row is read at its old place.
// Every thread of the workgroup passes the 2 N barriers; `on` masks the work of a finished problem.
__device__ __forceinline__ void sgf_solve(cd* wm, cd* xa, cd* xb, const int N, const int ld, const int W, const int t, const int tp_log,
                                          const bool on) {
    const int TP = 1 << tp_log, cw_log = tp_log < 5 ? tp_log : 5, CW = 1 << cw_log, RW = TP >> cw_log;
    const int tj = t & (CW - 1), tr = t >> cw_log;
    for (int c = 0; c < N; ++c) {
        int pr = c;
        if (on) {
            cd pv{1.0, 0.0};
            double best = -1.0;
            for (int r = c; r < N; ++r) {
                const cd v = wm[r * ld + c];
                const double m = cabs2(v);
                if (m > best) best = m, pr = r, pv = v;
            }
            const double q = 1.0 / cabs2(pv);
            const cd pinv{pv.x * q, -pv.y * q};
            for (int j = c + 1 + t; j < W; j += TP) {
                cd* col = sgf_col(wm, xa, xb, N, j);
                const cd top = col[c * ld], piv = col[pr * ld];
                col[pr * ld] = top;
                col[c * ld] = cmul_x(piv, pinv);
            }
        }
        __syncthreads();
        if (on) {
            for (int j = c + 1 + tj; j < W; j += CW) {
                cd* col = sgf_col(wm, xa, xb, N, j);
                const cd pj = col[c * ld];
                for (int r = tr; r < N; r += RW) {
                    if (r == c) continue;
                    const cd f = wm[(r == pr ? c : r) * ld + c];
                    cd v = col[r * ld];
                    v.x = fma(f.y, pj.y, fma(-f.x, pj.x, v.x));
                    v.y = fma(-f.y, pj.x, fma(-f.x, pj.y, v.y));
                    col[r * ld] = v;
                }
            }
        }
        __syncthreads();
    }
}

// the maxima of a and b over the TP threads of a problem (max does not depend on the order); every thread of the workgroup calls it
__device__ __forceinline__ void sgf_group_max(double& a, double& b, const int tp_log, double* red) {
    const int w = tp_log < 6 ? (1 << tp_log) : 64;
    for (int o = w >> 1; o > 0; o >>= 1) {
        a = fmax(a, __shfl_xor(a, o));
        b = fmax(b, __shfl_xor(b, o));
    }
    if (tp_log > 6) {
        const int wave = threadIdx.x >> 6, nwv = 1 << (tp_log - 6), w0 = (wave >> (tp_log - 6)) << (tp_log - 6);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) red[wave] = a, red[4 + wave] = b;
        __syncthreads();
        a = red[w0];
        b = red[4 + w0];
        for (int i = 1; i < nwv; ++i) {
            a = fmax(a, red[w0 + i]);
            b = fmax(b, red[4 + w0 + i]);
        }
    }
}

// the seven N x ld matrices of a problem.  The decimation rotates al <- wm <- be <- al, so which slot is which goes in and comes out
struct SgfSlots {
    cd *es, *et, *al, *be, *wm, *xa, *xb;
};
// the problem of this thread in group g of a workgroup kernel, and the thread's place in it
struct SgfProb {
    int N, ld, tp_log, t;   // t: the thread among the TP = 1 << tp_log of its problem
    int64_t p, ik;
    int iw;
    bool live;              // p < nprob; a thread without a problem only passes the barriers
    const cd *h00, *h01;
    cd z;
};
// the first call of a kernel's group loop: problem p = g P + sub, its blocks and z, and the slots in their first order in `mem` (the
// workgroup's dynamic LDS, or its part of the workspace, where P = 1); ends with the barrier after the previous group's last reads
__device__ __forceinline__ SgfProb sgf_problem(const SgfCommon& A, const int P, const int tp_log, const int ld, cd* mem, const int64_t g,
                                               SgfSlots& S) {
    const int sub = threadIdx.x >> tp_log, msz = A.N * ld;
    cd* B = mem + sub * 7 * msz;
    S = SgfSlots{B, B + msz, B + 2 * msz, B + 3 * msz, B + 4 * msz, B + 5 * msz, B + 6 * msz};
    SgfProb Q;
    Q.N = A.N, Q.ld = ld, Q.tp_log = tp_log, Q.t = threadIdx.x & ((1 << tp_log) - 1);
    Q.p = g * P + sub;
    Q.live = Q.p < A.nprob;
    Q.ik = Q.live ? Q.p / A.nw : 0;
    Q.iw = Q.live ? (int)(Q.p - Q.ik * A.nw) : 0;
    Q.h00 = A.blk + Q.ik * 2 * A.N * A.N;
    Q.h01 = Q.h00 + A.N * A.N;
    Q.z = cd{A.omega[Q.iw], A.eta};
    __syncthreads();
    return Q;
}

// the decimation of problem Q in the slots S: es = et = H00, al = H01, be = H01^+, then steps [X_a X_b] = (z - e)^-1 [al be], es += al X_b,
// et += be X_a, al <- al X_a, be <- be X_b to the stop rule of sgf_decimate_n2.  A finished problem is masked off and keeps its
// neighbours company at the barriers.  es and et hold the result; al, be, wm, xa, xb are free afterwards.  Every thread calls it.
__device__ __forceinline__ void sgf_decimate_wg(const SgfCommon& A, const SgfProb& Q, SgfSlots& S, double* red) {
    const int N = Q.N, ld = Q.ld, tp_log = Q.tp_log, t = Q.t, TP = 1 << tp_log, NN = N * N;
    const cd *h00 = Q.h00, *h01 = Q.h01;
    const cd z = Q.z;
    cd *es = S.es, *et = S.et, *al = S.al, *be = S.be, *wm = S.wm, *xa = S.xa, *xb = S.xb;
    double m0 = 0.0, m1 = 0.0;
    if (Q.live)
        for (int e = t; e < NN; e += TP) {
            const int i = e / N, j = e - i * N;
            const cd a0 = h00[e], a1 = h01[e];
            es[i * ld + j] = a0;
            et[i * ld + j] = a0;
            al[i * ld + j] = a1;
            be[i * ld + j] = cconj(h01[j * N + i]);
            m0 = fmax(m0, cabs2(a0));
            m1 = fmax(m1, cabs2(a1));
        }
    sgf_group_max(m0, m1, tp_log, red);
    const double scale = sqrt(fmax(m0, m1));
    double cur = sqrt(m1);
    int steps = 0;
    bool conv = false, active = Q.live;
    for (;;) {
        if (active) {
            if (A.tol > 0.0 && cur <= A.tol * scale) conv = true, active = false;
            else if (steps == A.max_iter) active = false;
        }
        if (!__syncthreads_or(active ? 1 : 0)) break;
        if (active)
            for (int e = t; e < NN; e += TP) {
                const int i = e / N, j = e - i * N, q = i * ld + j;
                const cd eb = cadd(es[q], csub(et[q], h00[e]));
                wm[q] = i == j ? csub(z, eb) : cd{-eb.x, -eb.y};
                xa[q] = al[q];
                xb[q] = be[q];
            }
        __syncthreads();
        sgf_solve(wm, xa, xb, N, ld, 3 * N, t, tp_log, active);
        double ma = 0.0, mb = 0.0;
        if (active)
            for (int e = t; e < NN; e += TP) {
                const int i = e / N, j = e - i * N, q = i * ld + j;
                cd s0{0.0, 0.0}, s1{0.0, 0.0}, na{0.0, 0.0};
                for (int k = 0; k < N; ++k) {
                    const cd a = al[i * ld + k], b = be[i * ld + k], ya = xa[k * ld + j], yb = xb[k * ld + j];
                    cfma_x(s0, a, yb);
                    cfma_x(s1, b, ya);
                    cfma_x(na, a, ya);
                }
                es[q] = cadd(es[q], s0);
                et[q] = cadd(et[q], s1);
                wm[q] = na;
                ma = fmax(ma, cabs2(na));
            }
        __syncthreads();
        if (active)
            for (int e = t; e < NN; e += TP) {
                const int i = e / N, j = e - i * N;
                cd nb{0.0, 0.0};
                for (int k = 0; k < N; ++k) cfma_x(nb, be[i * ld + k], xb[k * ld + j]);
                al[i * ld + j] = nb;
                mb = fmax(mb, cabs2(nb));
            }
        __syncthreads();
        if (active) {                                  // al <- al X_a (in wm), be <- be X_b (in al), the old be is the next wm
            cd* const o = al;
            al = wm;
            wm = be;
            be = o;
            ++steps;
        }
        sgf_group_max(ma, mb, tp_log, red);
        if (active) cur = sqrt(fmax(ma, mb));
    }
    if (Q.live && t == 0) {
        if (A.tol > 0.0 && !conv) atomicAdd(A.fail, 1ull);
        if (A.info) A.info[Q.p] = steps;
    }
    S.al = al, S.be = be, S.wm = wm;
}

// xa := (z - E)^-1 R in the slots S: wm takes z - E, xa takes R, one barrier, the elimination of width 2 N.  ev_of(e, q) and
// rhs_of(i, j, e) give E and R at element e = i N + j, which a slot holds at q = i ld + j.  Every thread calls it.
template <class EvOf, class RhsOf>
__device__ __forceinline__ void sgf_resolve(const SgfProb& Q, const SgfSlots& S, EvOf ev_of, RhsOf rhs_of) {
    if (Q.live)
        for (int e = Q.t; e < Q.N * Q.N; e += 1 << Q.tp_log) {
            const int i = e / Q.N, j = e - i * Q.N, q = i * Q.ld + j;
            const cd ev = ev_of(e, q);
            S.wm[q] = i == j ? csub(Q.z, ev) : cd{-ev.x, -ev.y};
            S.xa[q] = rhs_of(i, j, e);
        }
    __syncthreads();
    sgf_solve(S.wm, S.xa, S.xb, Q.N, Q.ld, 2 * Q.N, Q.t, Q.tp_log, Q.live);
}

// ---------------------------------------------------------------- host side
struct SgfShape {
    int P, tp_log, ld;
    size_t lds;    // bytes of dynamic LDS per workgroup (0: N = 2 or the workspace regime)
    bool global;
};
// TP = the power of two from N^2, 16 .. 256; P = 256 / TP problems per workgroup, halved while they pass 64 KiB of LDS together
static SgfShape sgf_shape(int N) {
    SgfShape S{1, 8, N + 1, 0, N > 32};
    if (S.global) return S;
    int tp_log = 4;
    while (tp_log < 8 && (1 << tp_log) < N * N) ++tp_log;
    const size_t foot = (size_t)7 * N * (N + 1) * sizeof(cd);
    while (tp_log < 8 && (size_t)(256 >> tp_log) * foot > 64 * 1024) ++tp_log;
    S.tp_log = tp_log;
    S.P = 256 >> tp_log;
    S.lds = S.P * foot;
    return S;
}

// the launch of a unit's kernels in the three storage regimes: N = 2 a lane per problem; N <= 32 P problems per workgroup in dynamic
// LDS, at most 32 workgroups per CU looping over the groups; beyond that one problem per workgroup on the workspace `ws` of ws_groups
// workgroups.  names: the profiling brackets of the three, in that order.
template <class Args, void (*KN2)(Args), void (*KLDS)(Args, int, int, int, cd*), void (*KGLOBAL)(Args, int, int, int, cd*)>
static int sgf_launch(tbk_ctx* ctx, const Args& A, cd* ws, int ws_groups, const char* const (&names)[3]) {
    if (A.N == 2) {
        ProfScope ps(ctx, names[0]);
        hipLaunchKernelGGL(KN2, dim3(nblk(A.nprob)), dim3(256), 0, ctx->stream, A);
        TBK_HIP(hipGetLastError());
        return TBK_OK;
    }
    const SgfShape S = sgf_shape(A.N);
    if (S.global) {
        ProfScope ps(ctx, names[2]);
        const unsigned grid = (unsigned)std::min<int64_t>(A.nprob, ws_groups);
        hipLaunchKernelGGL(KGLOBAL, dim3(grid), dim3(256), 0, ctx->stream, A, 1, S.tp_log, S.ld, ws);
        TBK_HIP(hipGetLastError());
        return TBK_OK;
    }
    ProfScope ps(ctx, names[1]);
    static bool big_lds = false;                           // the attribute belongs to the function KLDS: set once per process
    if (S.lds > 64 * 1024 && !big_lds) {
        TBK_HIP(hipFuncSetAttribute((const void*)KLDS, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
        big_lds = true;
    }
    const int64_t ngroups = (A.nprob + S.P - 1) / S.P;
    const unsigned grid = (unsigned)std::min<int64_t>(ngroups, (int64_t)std::max(ctx->cus, 1) * 32);
    hipLaunchKernelGGL(KLDS, dim3(grid), dim3(256), S.lds, ctx->stream, A, S.P, S.tp_log, S.ld, (cd*)nullptr);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

static int sgf_blocks_launch(tbk_model* cut, const double* k_dev, int64_t nk, int N, cd* blk) {
    tbk_ctx* ctx = cut->ctx;
    TBK_HIP(hipMemsetAsync(blk, 0, (size_t)nk * 2 * N * N * sizeof(cd), ctx->stream));
    if (cut->view.nnz == 0) return TBK_OK;
    ProfScope ps(ctx, "sgf_blocks");
    hipLaunchKernelGGL(k_sgf_blocks, dim3(nblk(nk * cut->view.nnz)), dim3(256), 0, ctx->stream, cut->view, k_dev, nk, N, blk);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

static int sgf_check_model(const char* who, tbk_model* cut, int nlayer, int ncell) {
    TBK_REQUIRE(cut, TBK_EINVAL, "%s: null model", who);
    TBK_REQUIRE(nlayer >= 1 && cut->nsta == 2 * nlayer, TBK_EINVAL,
                "%s: the model must be the cut piece of two principal layers (%d states for a layer of %d)", who, cut->nsta, nlayer);
    TBK_REQUIRE(nlayer <= kSgfMaxN, TBK_EUNSUPPORTED,
                "%s: a principal layer of %d states; the decimation kernels of this build take at most %d", who, nlayer, kSgfMaxN);
    TBK_REQUIRE(ncell >= 1 && nlayer % ncell == 0, TBK_EINVAL, "%s: a layer of %d states is no multiple of a cell of %d", who, nlayer,
                ncell);
    TBK_REQUIRE(cut->dim_k <= 3, TBK_EINVAL, "%s: surface zone of %d dimensions", who, cut->dim_k);
    return TBK_OK;
}

// the per-call arguments of every list and mesh form; the caller's check of its mode and side follows, then sgf_plan
static int sgf_check_call(const char* who, int nw, const double* omega, double eta, double tol, int max_iter, const double* out) {
    TBK_REQUIRE(omega && out, TBK_EINVAL, "%s: null argument", who);
    TBK_REQUIRE(nw >= 1 && nw <= 65536, TBK_EINVAL, "%s: nomega=%d (1..65536 frequencies)", who, nw);
    for (int j = 0; j < nw; ++j) TBK_REQUIRE(std::isfinite(omega[j]), TBK_EINVAL, "%s: frequency %d is not finite", who, j);
    TBK_REQUIRE(std::isfinite(eta) && eta > 0.0, TBK_EINVAL, "%s: eta must be finite and > 0", who);
    TBK_REQUIRE(std::isfinite(tol) && tol >= 0.0, TBK_EINVAL, "%s: tol must be finite and >= 0", who);
    TBK_REQUIRE(max_iter >= 0 && max_iter <= 64, TBK_EINVAL, "%s: max_iter=%d (0..64)", who, max_iter);
    return TBK_OK;
}

// ---------------------------------------------------------------- the chunk driver
// A call works through its k points in chunks.  The list forms take k[nk][dim_k] from the host (mesh == null), the mesh means
// generate k_uniform_mesh(mesh) per chunk and sum rows[] doubles per k point with the fixed-order k_group_rows.
struct SgfPlan {
    int N, nw;
    int64_t nk, chunk, nchunk, rows;   // rows: doubles per k point of the mesh mean
    const int32_t* mesh;
    int ws_groups;                     // the grid of the workspace regime
    size_t omb, kb, bb, xb, ob, ib, cb, wb, total;   // bytes: omega, k, H00/H01, the unit's extra table, results, steps, chunk sums, workspace
};
// k points per chunk, a function of (N, nk, nw) and the unit's bytes per k alone: min(256 MiB / bytes per k, 2^20 / nw), at least one
static int64_t sgf_chunk_len(int N, int64_t nk, int nw, size_t extra_perk, size_t out_perk) {
    const size_t perk = (size_t)2 * N * N * sizeof(cd) + extra_perk + (size_t)nw * sizeof(int) + out_perk;
    const int64_t c = std::min<int64_t>((int64_t)(kSgfChunkBytes / perk), kSgfChunkProblems / nw);
    return std::max<int64_t>(1, std::min<int64_t>(nk, c));
}
// extra_perk: bytes per k of a table of the unit's own (0: none); out_perk: bytes of results per k.  The caller compares P.total
// with kSgfMaxBytes under its own message.
static int sgf_plan(const char* who, tbk_model* cut, int N, int64_t nk, const int32_t* mesh, int nw, size_t extra_perk, size_t out_perk,
                    int64_t rows, SgfPlan& P) {
    TBK_REQUIRE(nk >= 1, TBK_EINVAL, "%s: no k point", who);
    tbk_ctx* ctx = cut->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    P = SgfPlan{};
    P.N = N, P.nw = nw, P.nk = nk, P.mesh = mesh, P.rows = rows;
    P.chunk = sgf_chunk_len(N, nk, nw, extra_perk, out_perk);
    P.nchunk = (nk + P.chunk - 1) / P.chunk;
    const SgfShape S = sgf_shape(N);
    P.ws_groups = (int)std::min<int64_t>(std::max(ctx->cus, 1), P.chunk * nw);
    P.omb = al256((size_t)nw * sizeof(double));
    P.kb = al256((size_t)(mesh ? P.chunk : nk) * std::max(cut->dim_k, 1) * sizeof(double));
    P.bb = al256((size_t)P.chunk * 2 * N * N * sizeof(cd));
    P.xb = extra_perk ? al256((size_t)P.chunk * extra_perk) : 0;
    P.ob = al256((size_t)P.chunk * out_perk);
    P.ib = al256((size_t)P.chunk * nw * sizeof(int));
    P.cb = mesh ? al256((size_t)(P.nchunk + 1) * rows * sizeof(double)) : 0;
    P.wb = S.global && N != 2 ? (size_t)P.ws_groups * 7 * N * S.ld * sizeof(cd) : 0;
    P.total = 512 + P.omb + P.kb + P.bb + P.xb + P.ob + P.ib + P.cb + P.wb;
    return TBK_OK;
}

// one chunk as the unit's callables see it
struct SgfChunk {
    int64_t first, cnt;   // k points first .. first + cnt of the call
    const double* k;      // their coordinates on the device
    SgfCommon args;       // filled in for the chunk
    cd* extra;            // the unit's own table (P.xb bytes)
    double* out;          // results of the chunk (P.ob bytes)
    cd* ws;
};
// work(chunk) launches the unit's kernels on a chunk whose H00, H01 are in place; download(chunk) copies the results of a list form
// to the host.  rows_name: the profiling bracket of the mesh sums.  Raises TBK_ENOCONV with the count of points that missed tol.
template <class Work, class Download>
static int sgf_drive(const char* who, tbk_model* cut, const SgfPlan& P, const double* k, const double* omega, double eta, double tol,
                     int max_iter, double* out, int32_t* info, const char* rows_name, Work work, Download download) {
    tbk_ctx* ctx = cut->ctx;
    const int dk = cut->dim_k, N = P.N, nw = P.nw;
    const int64_t nk = P.nk, rows = P.rows;
    void* base = nullptr;
    int rc = tbk_ctx_scratch(ctx, P.total, &base);
    if (rc) return rc;
    unsigned char* q = (unsigned char*)base + 256;
    unsigned long long* fail_dev = (unsigned long long*)q;
    q += 256;
    double* om_dev = (double*)q;
    q += P.omb;
    double* k_dev = (double*)q;
    q += P.kb;
    cd* blk = (cd*)q;
    q += P.bb;
    cd* extra = (cd*)q;
    q += P.xb;
    double* out_dev = (double*)q;
    q += P.ob;
    int* info_dev = (int*)q;
    q += P.ib;
    double* csum = (double*)q;                             // [nchunk][rows] chunk sums, then [rows] the mean
    q += P.cb;
    cd* ws = (cd*)q;
    TBK_HIP(hipMemsetAsync(fail_dev, 0, sizeof(unsigned long long), ctx->stream));
    TBK_HIP(hipMemcpyAsync(om_dev, omega, (size_t)nw * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (!P.mesh && dk > 0) TBK_HIP(hipMemcpyAsync(k_dev, k, (size_t)nk * dk * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    for (int64_t c = 0; c < P.nchunk; ++c) {
        SgfChunk C{};
        C.first = c * P.chunk, C.cnt = std::min(P.chunk, nk - C.first);
        C.k = k_dev + (P.mesh ? 0 : C.first * dk);
        if (P.mesh) {
            rc = tbk_k_uniform_mesh_range_dev(ctx, dk, P.mesh, C.first, C.cnt, k_dev);
            if (rc) return rc;
        }
        rc = sgf_blocks_launch(cut, C.k, C.cnt, N, blk);
        if (rc) return rc;
        C.args = SgfCommon{blk, om_dev, nw, N, eta, tol, max_iter, C.cnt * nw, info ? info_dev : nullptr, fail_dev};
        C.extra = extra, C.out = out_dev, C.ws = ws;
        rc = work(C);
        if (rc) return rc;
        if (P.mesh) {
            ProfScope ps(ctx, rows_name);
            hipLaunchKernelGGL(k_group_rows, dim3((unsigned)rows), dim3(256), 0, ctx->stream, (const double*)out_dev, (int)C.cnt, rows, 1.0,
                               0, csum + c * rows);
            TBK_HIP(hipGetLastError());
        } else {
            rc = download(C);
            if (rc) return rc;
        }
        if (info)
            TBK_HIP(hipMemcpyAsync(info + C.first * nw, info_dev, (size_t)C.cnt * nw * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        if (P.nchunk > 1) TBK_HIP(hipStreamSynchronize(ctx->stream));   // the next chunk reuses the buffers the copies read
    }
    if (P.mesh) {
        ProfScope ps(ctx, rows_name);
        hipLaunchKernelGGL(k_group_rows, dim3((unsigned)rows), dim3(256), 0, ctx->stream, (const double*)csum, (int)P.nchunk, rows,
                           1.0 / (double)nk, 0, csum + P.nchunk * rows);
        TBK_HIP(hipGetLastError());
        TBK_HIP(hipMemcpyAsync(out, csum + P.nchunk * rows, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    unsigned long long nfail = 0;
    TBK_HIP(hipMemcpyAsync(&nfail, fail_dev, sizeof(nfail), hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    TBK_REQUIRE(nfail == 0, TBK_ENOCONV, "%s: %llu of %lld (k, omega) points did not reach tol=%g within max_iter=%d decimation steps", who,
                nfail, (long long)(nk * nw), tol, max_iter);
    return TBK_OK;
}
