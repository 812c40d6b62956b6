// tbk_sgf.h -- what the two translation units built on the decimation of the principal layer share (tbk_surface.hip, DESIGN.md
// section 18; tbk_landauer.hip, section 19): the limits of a call, the kernel of the layer blocks H00 and H01 and its launch, the
// 2 x 2 helpers of the lane-per-problem regime, the Gauss-Jordan elimination and the group maximum of the workgroup regimes, the
// shape of a launch and the check of the cut model.  Kernels are static: each unit holds its own copy.
#pragma once
#include "tbk_pairs.h"

static const size_t kSgfChunkBytes = (size_t)256 << 20;     // blocks + results of one chunk of k points
static const int64_t kSgfChunkProblems = (int64_t)1 << 20;  // (k, w) problems of one chunk at most
static const int kSgfMaxN = 128;
static const size_t kSgfMaxBytes = (size_t)4 << 30;         // device memory of one call (a chunk never holds less than one k point)

// ---------------------------------------------------------------- H00, H01
// one thread per (k, non-empty slot (a, b), a <= b) of the cut model: H_ab as gen_ham_entry forms it; rows a < N only
static __global__ __launch_bounds__(256) void k_sgf_blocks(const ModelView mv, const double* __restrict__ k, const int64_t nk, const int N,
                                                    cd* __restrict__ blk) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nk * mv.nnz) return;
    const int64_t ik = idx / mv.nnz;
    const int4 z4 = mv.nz[idx - ik * mv.nnz];
    const int a = z4.x & 0xffff, b = z4.x >> 16;
    if (a >= N || b >= 2 * N) return;
    double kk[4];
    cd z[4];
    k_phases(mv, k, ik, kk, z);
    cd s{0.0, 0.0};
    for (int t = z4.y; t < z4.z; ++t) cfma(s, mv.term_amp[t], phase_of_R(z, mv.term_R[t]));
    cd* h00 = blk + ik * 2 * N * N;
    cd* h01 = h00 + N * N;
    if (a == b) {
        h00[a * N + a] = cd{s.x, 0.0};
        return;
    }
    const cd ea = expi2pi(kdot(kk, mv.orb[a])), eb = expi2pi(kdot(kk, mv.orb[b]));
    const cd v = cmul(cmulc(ea, eb), s);
    if (b < N) {
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
