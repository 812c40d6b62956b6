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
// The decimation itself is in tbk_sgf.h (sgf_decimate_n2, sgf_decimate_wg), which tbk_landauer.hip shares, with k_sgf_blocks, the
// elimination, the launcher of the three regimes, the argument checks and the chunk driver.  This unit holds what follows the loop:
// the last stage of the same kernels inverts z - es, z - et, z - e and writes whole matrices, exposed-cell diagonals or their
// traces.  k_sgf_wg alone keeps the text of the shared workgroup functions in its body, for its speed (see the kernel).  A problem's arithmetic depends on its own (k, w) alone -- a finished problem is masked off and only keeps its
// neighbours company at the barriers -- so its bits do not depend on the batch, its position in it or the chunk.  The mesh mean sums
// per-k rows with the fixed-order k_group_rows of tbk_kubo.h.  No floating-point atomics anywhere.
#include <math.h>
#include <string.h>
#include "tbk_sgf.h"

struct SgfArgs : SgfCommon {
    int ns;               // states of one unit cell
    int mode;             // 0: G of `side`, out[p][N][N] c128; 1: traces, 2: diagonals of the exposed cell, all three sides
    int side;
    double* out;
    int64_t s_side, s_k, s_w;   // modes 1, 2: value (side, ik, iw, q) at side s_side + ik s_k + iw s_w + q
};

// ---------------------------------------------------------------- N = 2: a lane per problem
__global__ __launch_bounds__(256) void k_sgf_n2(const SgfArgs A) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= A.nprob) return;
    const Sgf2 D = sgf_decimate_n2(A, p);
    const double mpi = -1.0 / M_PI;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        if (A.mode == 0 && s != A.side) continue;
        const M2 G = m2resolvent(D.z, s == 0 ? D.es : (s == 1 ? D.et : m2bulk(D.es, D.et, D.h0)));
        if (A.mode == 0) {
            cd* o = (cd*)A.out + p * 4;
            o[0] = G.a;
            o[1] = G.b;
            o[2] = G.c;
            o[3] = G.d;
            continue;
        }
        double* o = A.out + s * A.s_side + D.ik * A.s_k + D.iw * A.s_w;
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
// This kernel keeps the text of sgf_problem, sgf_decimate_wg and sgf_resolve (tbk_sgf.h) instead of calling them: built from the calls
// the LDS regime measured 0.4 .. 1.2 % slower.  The loop must stay that of sgf_decimate_wg, statement for
// statement; tests/test_landauer.py compares the step counts of the two.
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

// the list forms (mesh == null: k[nk][dim_k] from the host) and the mesh mean (mesh given: k_uniform_mesh(mesh) generated per chunk)
static int sgf_run(const char* who, tbk_model* cut, int N, int ns, const double* k, int64_t nk, const int32_t* mesh, int nw,
                   const double* omega, double eta, double tol, int max_iter, int mode, int side, double* out, int32_t* info) {
    int rc = sgf_check_call(who, nw, omega, eta, tol, max_iter, out);
    if (rc) return rc;
    TBK_REQUIRE(mode >= 0 && mode <= 2 && side >= 0 && side <= 2, TBK_EINVAL, "%s: mode %d, side %d", who, mode, side);
    const int nv = mode == 2 ? ns : 1;
    const int64_t rows = (int64_t)3 * nw * nv;             // values per k point of modes 1, 2
    SgfPlan P;
    rc = sgf_plan(who, cut, N, nk, mesh, nw, 0, mode == 0 ? (size_t)nw * N * N * sizeof(cd) : (size_t)rows * sizeof(double), rows, P);
    if (rc) return rc;
    TBK_REQUIRE(P.total <= kSgfMaxBytes, TBK_EUNSUPPORTED,
                "%s: %d frequencies of a layer of %d states need %zu bytes of results per k point (at most %zu per call): split omega", who,
                nw, N, P.ob / (size_t)P.chunk, kSgfMaxBytes);
    static const char* const names[3] = {"sgf_n2", "sgf_wg_lds", "sgf_wg_global"};
    return sgf_drive(
        who, cut, P, k, omega, eta, tol, max_iter, out, info, "sgf_rows",
        [&](const SgfChunk& C) {
            SgfArgs A{};
            static_cast<SgfCommon&>(A) = C.args;
            A.ns = ns;
            A.mode = mode;
            A.side = side;
            A.out = C.out;
            A.s_w = nv;
            if (mesh) A.s_k = rows, A.s_side = (int64_t)nw * nv;        // part[k][side][w][q]
            else A.s_k = (int64_t)nw * nv, A.s_side = C.cnt * nw * nv;  // [side][k][w][q] of the chunk
            return sgf_launch<SgfArgs, k_sgf_n2, k_sgf_wg<false>, k_sgf_wg<true>>(cut->ctx, A, C.ws, P.ws_groups, names);
        },
        [&](const SgfChunk& C) -> int {
            hipStream_t st = cut->ctx->stream;
            if (mode == 0) {
                TBK_HIP(hipMemcpyAsync(out + C.first * nw * 2 * N * N, C.out, (size_t)C.cnt * nw * N * N * sizeof(cd), hipMemcpyDeviceToHost,
                                       st));
                return TBK_OK;
            }
            for (int s = 0; s < 3; ++s)
                TBK_HIP(hipMemcpyAsync(out + (s * nk + C.first) * nw * nv, C.out + s * C.cnt * nw * nv, (size_t)C.cnt * nw * nv * sizeof(double),
                                       hipMemcpyDeviceToHost, st));
            return TBK_OK;
        });
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
