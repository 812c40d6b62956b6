// tbk_surface.hip -- Green's functions of the semi-infinite crystal by iterative decimation (Lopez Sancho, Lopez Sancho and Rubio,
// J. Phys. F 15, 851 (1985)) and the edge / bulk spectral functions made from them.
//
// The caller uploads cut_piece(2 L, fin_dir) of its model as an ordinary model (2 N states, N = L nsta the principal layer, dim_k - 1
// periodic directions).  H00(k) and H01(k) are the top-left and top-right N x N blocks of that model's H(k); z = w + i eta.  With
//   es = et = H00,  al = H01,  be = H01^+,  e = es + (et - H00)
// one decimation step is
//   [X_a X_b] = (z - e)^-1 [al be]        (Gauss-Jordan elimination with partial pivoting on the augmented N x 3N matrix)
//   es += al X_b,  et += be X_a,  al <- al X_a,  be <- be X_b
// and after i steps G_0 = (z - es)^-1 (cell 0 exposed, crystal toward +fin_dir), G_1 = (z - et)^-1 (last cell exposed, crystal toward
// -fin_dir) and G_b = (z - e)^-1 are the first, last and middle diagonal blocks of the resolvent of slabs of L 2^i and L (2^(i+1) - 1)
// cells.  A problem is one (k, w); it stops at the first i, 0 included, with max(|al|_max, |be|_max) <= tol max(|H00|_max, |H01|_max),
// or after exactly max_iter steps when tol = 0.
//
// Kernels: k_sgf_blocks (H00, H01 of every k of a chunk, once, reused by every w), then ONE algorithm in three storage regimes:
//   N = 2        k_sgf_n2: a lane per problem, the matrices in registers, the 2 x 2 inverse in closed form
//   N <= 32      k_sgf_wg<false>: seven N x (N + 1) matrices per problem in LDS, P problems of TP threads per 256-thread workgroup
//   N <= 128     k_sgf_wg<true>: the same code, the seven matrices in a global workspace sized by the number of workgroups
// The last stage of the same kernels inverts z - es, z - et, z - e and writes whole matrices, exposed-cell diagonals or their traces.
// A problem's arithmetic depends on its own (k, w) alone -- a finished problem is masked off and only keeps its neighbours company at
// the barriers -- so its bits do not depend on the batch, its position in it or the chunk.  The mesh mean sums per-k rows with the
// fixed-order k_opt_rows of tbk_pairs.h.  No floating-point atomics anywhere.  (k_sgf_blocks, the elimination, the 2 x 2 helpers and
// the launch shape are in tbk_sgf.h, which tbk_landauer.hip shares.)
#include <math.h>
#include <string.h>
#include "tbk_sgf.h"

struct SgfArgs {
    const cd* blk;        // [nk][2][N][N]: H00, H01 of the chunk's k points
    const double* omega;  // [nw]
    int nw, N, ns;        // frequencies, layer size, states of one unit cell
    double eta, tol;
    int max_iter;
    int mode;             // 0: G of `side`, out[p][N][N] c128; 1: traces, 2: diagonals of the exposed cell, all three sides
    int side;
    int64_t nprob;        // nk nw, problem p = ik nw + iw
    double* out;
    int64_t s_side, s_k, s_w;   // modes 1, 2: value (side, ik, iw, q) at side s_side + ik s_k + iw s_w + q
    int* info;            // [nprob] steps taken, or null
    unsigned long long* fail;   // count of problems that missed a non-zero tol
};

// ---------------------------------------------------------------- N = 2: a lane per problem
__global__ __launch_bounds__(256) void k_sgf_n2(const SgfArgs A) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= A.nprob) return;
    const int64_t ik = p / A.nw;
    const int iw = (int)(p - ik * A.nw);
    const cd* h = A.blk + ik * 8;
    const M2 h0{h[0], h[1], h[2], h[3]};
    M2 al{h[4], h[5], h[6], h[7]};
    M2 be{cconj(al.a), cconj(al.c), cconj(al.b), cconj(al.d)};
    M2 es = h0, et = h0;
    const cd z{A.omega[iw], A.eta};
    const double scale = sqrt(fmax(m2max(h0), m2max(al)));
    double cur = sqrt(m2max(al));
    int steps = 0;
    bool conv = false;
    for (;;) {
        if (A.tol > 0.0 && cur <= A.tol * scale) {
            conv = true;
            break;
        }
        if (steps == A.max_iter) break;
        const M2 g = m2resolvent(z, m2bulk(es, et, h0));
        const M2 xa = m2mul(g, al), xb = m2mul(g, be);
        m2acc(es, m2mul(al, xb));
        m2acc(et, m2mul(be, xa));
        const M2 na = m2mul(al, xa), nb = m2mul(be, xb);
        al = na;
        be = nb;
        cur = sqrt(fmax(m2max(al), m2max(be)));
        ++steps;
    }
    if (A.tol > 0.0 && !conv) atomicAdd(A.fail, 1ull);
    if (A.info) A.info[p] = steps;
    const double mpi = -1.0 / M_PI;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        if (A.mode == 0 && s != A.side) continue;
        const M2 G = m2resolvent(z, s == 0 ? es : (s == 1 ? et : m2bulk(es, et, h0)));
        if (A.mode == 0) {
            cd* o = (cd*)A.out + p * 4;
            o[0] = G.a;
            o[1] = G.b;
            o[2] = G.c;
            o[3] = G.d;
            continue;
        }
        double* o = A.out + s * A.s_side + ik * A.s_k + iw * A.s_w;
        // the exposed cell: ns = 2 the whole layer; ns = 1 (L = 2) state 0, or state 1 on side 1
        const double d0 = mpi * G.a.y, d1 = mpi * G.d.y;
        if (A.ns == 2) {
            if (A.mode == 1) o[0] = d0 + d1;
            else o[0] = d0, o[1] = d1;
        } else {
            o[0] = s == 1 ? d1 : d0;
        }
    }
}

// ---------------------------------------------------------------- N != 2: TP threads per problem, matrices in LDS or in a workspace
template <bool GLOBAL>
__global__ __launch_bounds__(256) void k_sgf_wg(const SgfArgs A, const int P, const int tp_log, const int ld, cd* ws) {
    extern __shared__ cd sgf_lds[];
    __shared__ double red[8];
    const int N = A.N, TP = 1 << tp_log, NN = N * N, msz = N * ld;
    const int sub = threadIdx.x >> tp_log, t = threadIdx.x & (TP - 1);
    cd* B;
    if constexpr (GLOBAL) B = ws + (int64_t)blockIdx.x * 7 * msz;
    else B = sgf_lds + sub * 7 * msz;
    const int64_t ngroups = (A.nprob + P - 1) / P;
    const double mpi = -1.0 / M_PI;
    for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        cd *es = B, *et = B + msz, *al = B + 2 * msz, *be = B + 3 * msz, *wm = B + 4 * msz, *xa = B + 5 * msz, *xb = B + 6 * msz;
        const int64_t p = g * P + sub;
        const bool live = p < A.nprob;
        const int64_t ik = live ? p / A.nw : 0;
        const int iw = live ? (int)(p - ik * A.nw) : 0;
        const cd* h00 = A.blk + ik * 2 * NN;
        const cd* h01 = h00 + NN;
        const cd z{A.omega[iw], A.eta};
        __syncthreads();                                   // the previous group's last reads
        double m0 = 0.0, m1 = 0.0;
        if (live)
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
        bool conv = false, active = live;
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
        if (live && t == 0) {
            if (A.tol > 0.0 && !conv) atomicAdd(A.fail, 1ull);
            if (A.info) A.info[p] = steps;
        }
        for (int s = 0; s < 3; ++s) {
            if (A.mode == 0 && s != A.side) continue;
            if (live)
                for (int e = t; e < NN; e += TP) {
                    const int i = e / N, j = e - i * N, q = i * ld + j;
                    const cd ev = s == 0 ? es[q] : (s == 1 ? et[q] : cadd(es[q], csub(et[q], h00[e])));
                    wm[q] = i == j ? csub(z, ev) : cd{-ev.x, -ev.y};
                    xa[q] = i == j ? cd{1.0, 0.0} : cd{0.0, 0.0};
                }
            __syncthreads();
            sgf_solve(wm, xa, xb, N, ld, 2 * N, t, tp_log, live);
            if (live) {
                if (A.mode == 0) {
                    cd* o = (cd*)A.out + p * NN;
                    for (int e = t; e < NN; e += TP) {
                        const int i = e / N;
                        o[e] = xa[i * ld + (e - i * N)];
                    }
                } else {
                    const int c0 = s == 1 ? N - A.ns : 0;  // the exposed unit cell
                    double* o = A.out + s * A.s_side + ik * A.s_k + iw * A.s_w;
                    if (A.mode == 2) {
                        for (int q = t; q < A.ns; q += TP) o[q] = mpi * xa[(c0 + q) * ld + c0 + q].y;
                    } else if (t == 0) {
                        double acc = 0.0;
                        for (int q = 0; q < A.ns; ++q) acc += mpi * xa[(c0 + q) * ld + c0 + q].y;
                        o[0] = acc;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// ---------------------------------------------------------------- host side
static int sgf_launch(tbk_ctx* ctx, const SgfArgs& A, cd* ws, int ws_groups) {
    if (A.N == 2) {
        ProfScope ps(ctx, "sgf_n2");
        hipLaunchKernelGGL(k_sgf_n2, dim3(nblk(A.nprob)), dim3(256), 0, ctx->stream, A);
        TBK_HIP(hipGetLastError());
        return TBK_OK;
    }
    const SgfShape S = sgf_shape(A.N);
    if (S.global) {
        ProfScope ps(ctx, "sgf_wg_global");
        const unsigned grid = (unsigned)std::min<int64_t>(A.nprob, ws_groups);
        hipLaunchKernelGGL(k_sgf_wg<true>, dim3(grid), dim3(256), 0, ctx->stream, A, 1, S.tp_log, S.ld, ws);
        TBK_HIP(hipGetLastError());
        return TBK_OK;
    }
    ProfScope ps(ctx, "sgf_wg_lds");
    static bool big_lds = false;                           // the attribute belongs to the function: set once per process
    if (S.lds > 64 * 1024 && !big_lds) {
        TBK_HIP(hipFuncSetAttribute((const void*)k_sgf_wg<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
        big_lds = true;
    }
    const int64_t ngroups = (A.nprob + S.P - 1) / S.P;
    const unsigned grid = (unsigned)std::min<int64_t>(ngroups, (int64_t)std::max(ctx->cus, 1) * 32);
    hipLaunchKernelGGL(k_sgf_wg<false>, dim3(grid), dim3(256), S.lds, ctx->stream, A, S.P, S.tp_log, S.ld, (cd*)nullptr);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

extern "C" int tbk_surface_blocks(tbk_model* cut, int nlayer, const double* k, int64_t nk, double* h00, double* h01) {
    int rc = sgf_check_model("tbk_surface_blocks", cut, nlayer, nlayer);
    if (rc) return rc;
    TBK_REQUIRE(h00 && h01 && nk >= 1 && (k || cut->dim_k == 0), TBK_EINVAL, "tbk_surface_blocks: bad argument");
    tbk_ctx* ctx = cut->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    const int dk = cut->dim_k, N = nlayer;
    const size_t kb = al256((size_t)nk * std::max(dk, 1) * sizeof(double)), mb = (size_t)N * N * sizeof(cd);
    void* base = nullptr;
    rc = tbk_ctx_scratch(ctx, 256 + kb + (size_t)nk * 2 * mb, &base);
    if (rc) return rc;
    double* k_dev = (double*)((unsigned char*)base + 256);
    cd* blk = (cd*)((unsigned char*)k_dev + kb);
    if (dk > 0) TBK_HIP(hipMemcpyAsync(k_dev, k, (size_t)nk * dk * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    rc = sgf_blocks_launch(cut, k_dev, nk, N, blk);
    if (rc) return rc;
    for (int64_t i = 0; i < nk; ++i) {
        TBK_HIP(hipMemcpyAsync((char*)h00 + i * mb, blk + i * 2 * N * N, mb, hipMemcpyDeviceToHost, ctx->stream));
        TBK_HIP(hipMemcpyAsync((char*)h01 + i * mb, blk + i * 2 * N * N + N * N, mb, hipMemcpyDeviceToHost, ctx->stream));
    }
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    return TBK_OK;
}

// k points per chunk: a function of (N, nk, nw, mode, cell) alone
static int64_t sgf_chunk_len(int N, int64_t nk, int nw, int mode, int ns) {
    const size_t perk = (size_t)2 * N * N * sizeof(cd) + (size_t)nw * sizeof(int) +
                        (mode == 0 ? (size_t)nw * N * N * sizeof(cd) : (size_t)3 * nw * (mode == 2 ? ns : 1) * sizeof(double));
    const int64_t c = std::min<int64_t>((int64_t)(kSgfChunkBytes / perk), kSgfChunkProblems / nw);
    return std::max<int64_t>(1, std::min<int64_t>(nk, c));
}

// the list forms (mesh == null: k[nk][dim_k] from the host) and the mesh mean (mesh given: k_uniform_mesh(mesh) generated per chunk)
static int sgf_run(const char* who, tbk_model* cut, int N, int ns, const double* k, int64_t nk, const int32_t* mesh, int nw,
                   const double* omega, double eta, double tol, int max_iter, int mode, int side, double* out, int32_t* info) {
    TBK_REQUIRE(omega && out, TBK_EINVAL, "%s: null argument", who);
    TBK_REQUIRE(nw >= 1 && nw <= 65536, TBK_EINVAL, "%s: nomega=%d (1..65536 frequencies)", who, nw);
    for (int j = 0; j < nw; ++j) TBK_REQUIRE(std::isfinite(omega[j]), TBK_EINVAL, "%s: frequency %d is not finite", who, j);
    TBK_REQUIRE(std::isfinite(eta) && eta > 0.0, TBK_EINVAL, "%s: eta must be finite and > 0", who);
    TBK_REQUIRE(std::isfinite(tol) && tol >= 0.0, TBK_EINVAL, "%s: tol must be finite and >= 0", who);
    TBK_REQUIRE(max_iter >= 0 && max_iter <= 64, TBK_EINVAL, "%s: max_iter=%d (0..64)", who, max_iter);
    TBK_REQUIRE(mode >= 0 && mode <= 2 && side >= 0 && side <= 2, TBK_EINVAL, "%s: mode %d, side %d", who, mode, side);
    TBK_REQUIRE(nk >= 1, TBK_EINVAL, "%s: no k point", who);
    tbk_ctx* ctx = cut->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    const int dk = cut->dim_k, nv = mode == 2 ? ns : 1;
    const int64_t chunk = sgf_chunk_len(N, nk, nw, mode, ns), nchunk = (nk + chunk - 1) / chunk;
    const int64_t rows = (int64_t)3 * nw * nv;             // values per k point of modes 1, 2
    const SgfShape S = sgf_shape(N);
    const int ws_groups = (int)std::min<int64_t>(std::max(ctx->cus, 1), chunk * nw);   // the grid of the workspace regime
    const size_t omb = al256((size_t)nw * sizeof(double));
    const size_t kb = al256((size_t)(mesh ? chunk : nk) * std::max(dk, 1) * sizeof(double));
    const size_t bb = al256((size_t)chunk * 2 * N * N * sizeof(cd));
    const size_t ob = al256(mode == 0 ? (size_t)chunk * nw * N * N * sizeof(cd) : (size_t)chunk * rows * sizeof(double));
    const size_t ib = al256((size_t)chunk * nw * sizeof(int));
    const size_t cb = mesh ? al256((size_t)(nchunk + 1) * rows * sizeof(double)) : 0;
    const size_t wb = S.global && N != 2 ? (size_t)ws_groups * 7 * N * S.ld * sizeof(cd) : 0;
    const size_t total = 512 + omb + kb + bb + ob + ib + cb + wb;
    TBK_REQUIRE(total <= kSgfMaxBytes, TBK_EUNSUPPORTED,
                "%s: %d frequencies of a layer of %d states need %zu bytes of results per k point (at most %zu per call): split omega", who,
                nw, N, ob / (size_t)chunk, kSgfMaxBytes);
    void* base = nullptr;
    int rc = tbk_ctx_scratch(ctx, total, &base);
    if (rc) return rc;
    unsigned char* q = (unsigned char*)base + 256;
    unsigned long long* fail_dev = (unsigned long long*)q;
    q += 256;
    double* om_dev = (double*)q;
    q += omb;
    double* k_dev = (double*)q;
    q += kb;
    cd* blk = (cd*)q;
    q += bb;
    double* out_dev = (double*)q;
    q += ob;
    int* info_dev = (int*)q;
    q += ib;
    double* csum = (double*)q;                             // [nchunk][rows] chunk sums, then [rows] the mean
    q += cb;
    cd* ws = (cd*)q;
    TBK_HIP(hipMemsetAsync(fail_dev, 0, sizeof(unsigned long long), ctx->stream));
    TBK_HIP(hipMemcpyAsync(om_dev, omega, (size_t)nw * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (!mesh && dk > 0) TBK_HIP(hipMemcpyAsync(k_dev, k, (size_t)nk * dk * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    for (int64_t c = 0; c < nchunk; ++c) {
        const int64_t first = c * chunk, cnt = std::min(chunk, nk - first);
        const double* kc = k_dev + (mesh ? 0 : first * dk);
        if (mesh) {
            rc = tbk_k_uniform_mesh_range_dev(ctx, dk, mesh, first, cnt, k_dev);
            if (rc) return rc;
        }
        rc = sgf_blocks_launch(cut, kc, cnt, N, blk);
        if (rc) return rc;
        SgfArgs A{};
        A.blk = blk;
        A.omega = om_dev;
        A.nw = nw;
        A.N = N;
        A.ns = ns;
        A.eta = eta;
        A.tol = tol;
        A.max_iter = max_iter;
        A.mode = mode;
        A.side = side;
        A.nprob = cnt * nw;
        A.out = out_dev;
        A.s_w = nv;
        if (mesh) A.s_k = rows, A.s_side = (int64_t)nw * nv;      // part[k][side][w][q]
        else A.s_k = (int64_t)nw * nv, A.s_side = cnt * nw * nv;  // [side][k][w][q] of the chunk
        A.info = info ? info_dev : nullptr;
        A.fail = fail_dev;
        rc = sgf_launch(ctx, A, ws, ws_groups);
        if (rc) return rc;
        if (mesh) {
            ProfScope ps(ctx, "sgf_rows");
            hipLaunchKernelGGL(k_opt_rows, dim3((unsigned)rows), dim3(256), 0, ctx->stream, (const double*)out_dev, (int)cnt, rows, 1.0,
                               csum + c * rows);
            TBK_HIP(hipGetLastError());
        } else if (mode == 0) {
            TBK_HIP(hipMemcpyAsync(out + first * nw * 2 * N * N, out_dev, (size_t)cnt * nw * N * N * sizeof(cd), hipMemcpyDeviceToHost,
                                   ctx->stream));
        } else {
            for (int s = 0; s < 3; ++s)
                TBK_HIP(hipMemcpyAsync(out + (s * nk + first) * nw * nv, out_dev + s * A.s_side, (size_t)cnt * nw * nv * sizeof(double),
                                       hipMemcpyDeviceToHost, ctx->stream));
        }
        if (info)
            TBK_HIP(hipMemcpyAsync(info + first * nw, info_dev, (size_t)cnt * nw * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        if (nchunk > 1) TBK_HIP(hipStreamSynchronize(ctx->stream));   // the next chunk reuses the buffers the copies read
    }
    if (mesh) {
        ProfScope ps(ctx, "sgf_rows");
        hipLaunchKernelGGL(k_opt_rows, dim3((unsigned)rows), dim3(256), 0, ctx->stream, (const double*)csum, (int)nchunk, rows,
                           1.0 / (double)nk, csum + nchunk * rows);
        TBK_HIP(hipGetLastError());
        TBK_HIP(hipMemcpyAsync(out, csum + nchunk * rows, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    unsigned long long nfail = 0;
    TBK_HIP(hipMemcpyAsync(&nfail, fail_dev, sizeof(nfail), hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    TBK_REQUIRE(nfail == 0, TBK_ENOCONV, "%s: %llu of %lld (k, omega) points did not reach tol=%g within max_iter=%d decimation steps", who,
                nfail, (long long)(nk * nw), tol, max_iter);
    return TBK_OK;
}

extern "C" int tbk_surface_green_list(tbk_model* cut, int nlayer, int ncell, const double* k, int64_t nk, int nomega,
                                      const double* omega, double eta, double tol, int max_iter, int mode, int side, double* out,
                                      int32_t* info) {
    int rc = sgf_check_model("tbk_surface_green_list", cut, nlayer, ncell);
    if (rc) return rc;
    TBK_REQUIRE(k || cut->dim_k == 0, TBK_EINVAL, "tbk_surface_green_list: null k");
    TBK_REQUIRE(cut->dim_k > 0 || nk == 1, TBK_EINVAL, "tbk_surface_green_list: a model without a surface zone has one point");
    return sgf_run("tbk_surface_green_list", cut, nlayer, ncell, k, nk, nullptr, nomega, omega, eta, tol, max_iter, mode, side, out, info);
}

extern "C" int tbk_surface_dos_mesh(tbk_model* cut, int nlayer, int ncell, const int32_t* mesh, int nomega, const double* omega,
                                    double eta, double tol, int max_iter, int per_state, double* out) {
    int rc = sgf_check_model("tbk_surface_dos_mesh", cut, nlayer, ncell);
    if (rc) return rc;
    TBK_REQUIRE(mesh && cut->dim_k >= 1, TBK_EINVAL, "tbk_surface_dos_mesh: needs a surface zone of 1 to 3 dimensions and its mesh");
    int64_t nk = 1;
    for (int d = 0; d < cut->dim_k; ++d) {
        TBK_REQUIRE(mesh[d] >= 1, TBK_EINVAL, "tbk_surface_dos_mesh: mesh[%d]=%d", d, mesh[d]);
        nk *= mesh[d];
    }
    return sgf_run("tbk_surface_dos_mesh", cut, nlayer, ncell, nullptr, nk, mesh, nomega, omega, eta, tol, max_iter, per_state ? 2 : 1, 0,
                   out, nullptr);
}
