// tbk_landauer.hip -- the Landauer transmission T(k, w) = Tr[Gamma_R G Gamma_L G^+] of a scattering region of M principal layers between
// two pristine semi-infinite leads of the crystal (Caroli et al. 1971, Fisher and Lee 1981), and the lead self-energies themselves
// (DESIGN.md section 19).
//
// Notation of tbk_surface.hip: H00(k), H01(k) the blocks of cut_piece(2 L, fin_dir), N = L nsta, z = w + i eta.  The decimation of that
// unit ends with es and et on chip; G_0 = (z - es)^-1 is the exposed first layer of the right lead, G_1 = (z - et)^-1 the exposed last
// layer of the left one, so
//   Sigma_L = H01^+ G_1 H01   (on layer 1),     Sigma_R = H01 G_0 H01^+   (on layer M),     Gamma = i (Sigma - Sigma^+)
// The device is an uploaded model of M N states, block-tridiagonal in layers: D_i (i = 1..M) and U_i = H_{i,i+1} (i = 1..M-1).  The
// forward sweep of the recursive Green's function, one Gauss-Jordan elimination of the augmented N x 3N matrix per layer:
//   A_1 = z - D_1 - Sigma_L,   A_i = z - D_i - U_{i-1}^+ X_b,   A_M additionally - Sigma_R
//   [X_a X_b] = A_i^-1 [U_{i-1}^+ P_{i-1}   U_i]      (layer 1: X_a = A_1^-1; layer M: no X_b)
//   P_i = X_a   (P_M = G_{M,1}),      T = Re Tr[Gamma_R P_M Gamma_L P_M^+]
//
// Kernels: k_land_blocks (D, U of every k of a chunk, once) and the three storage regimes of tbk_surface.hip, each kernel the
// decimation (sgf_decimate_n2 / sgf_decimate_wg of tbk_sgf.h, the calls tbk_surface.hip makes), then this unit's own part: the two
// self-energies, the sweep and the trace:
//   N = 2        k_land_n2: a lane per problem, the matrices in registers, 2 x 2 inverses by the adjugate
//   N <= 32      k_land_wg<false>: the seven N x (N + 1) slots per problem in LDS (Sigma_L, Sigma_R, A, X_a, X_b, U^+ P, one spare)
//   N <= 128     k_land_wg<true>: the same code on the global workspace
// mode 1 of the same kernels stops after the self-energies and writes one of them whole.  A problem's arithmetic depends on its own
// (k, w) alone; the trace is summed over the problem's own threads in a fixed order (shuffle tree, then the `red` array): a point's
// bits do not depend on the batch, its position in it or the chunk.  No floating-point atomics.  The host side is the launcher, the
// argument checks and the chunk driver of tbk_sgf.h around this unit's kernels, block table and downloads.
#include <math.h>
#include <string.h>
#include "tbk_sgf.h"

static const int kLandMaxLayers = 1024;

struct LandArgs : SgfCommon {
    const cd* dblk;       // [nk][2 M - 1][N][N]: D_1 .. D_M, U_1 .. U_{M-1} of the device; null: M = 1 and D_1 = H00
    int M;                // layers of the device
    int mode;             // 0: T, out[p] double; 1: the self-energy of `side` (0: Sigma_R, 1: Sigma_L), out[p][N][N] c128
    int side;
    double* out;
};

// ---------------------------------------------------------------- D, U
// one thread per (k, non-empty slot (a, b), a <= b) of the device model, H_ab by sgf_hab: both states in layer i -> D_i,
// b in the next layer -> U_i.  (Slots further apart do not exist: the caller has rejected such a device.)
__global__ __launch_bounds__(256) void k_land_blocks(const ModelView mv, const double* __restrict__ k, const int64_t nk, const int N,
                                                     const int M, cd* __restrict__ dblk) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nk * mv.nnz) return;
    const int64_t ik = idx / mv.nnz;
    const int4 z4 = mv.nz[idx - ik * mv.nnz];
    const int a = z4.x & 0xffff, b = z4.x >> 16;
    const int la = a / N, lb = b / N;
    if (a > b || lb >= M || lb - la > 1) return;
    const cd v = sgf_hab(mv, k, ik, z4);
    const int64_t NN = (int64_t)N * N;
    cd* d = dblk + (ik * (2 * M - 1) + la) * NN;
    const int ra = a - la * N, rb = b - lb * N;
    if (a == b) {
        d[ra * N + ra] = v;
    } else if (la == lb) {
        d[ra * N + rb] = v;
        d[rb * N + ra] = cconj(v);
    } else {
        d[(int64_t)M * NN + ra * N + rb] = v;              // U_la follows the M diagonal blocks
    }
}

// ---------------------------------------------------------------- N = 2: a lane per problem
// i (x - conj(y))
__device__ __forceinline__ cd land_gamma(const cd x, const cd y) { return cd{-(x.y + y.y), x.x - y.x}; }
__device__ __forceinline__ M2 m2gamma(const M2& s) {
    return M2{land_gamma(s.a, s.a), land_gamma(s.b, s.c), land_gamma(s.c, s.b), land_gamma(s.d, s.d)};
}
__device__ __forceinline__ double land_re(const double acc, const cd g, const cd c) { return fma(-g.y, c.y, fma(g.x, c.x, acc)); }

__global__ __launch_bounds__(256) void k_land_n2(const LandArgs A) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= A.nprob) return;
    const Sgf2 D = sgf_decimate_n2(A, p);
    const cd* h = D.h;
    const cd z = D.z;
    const M2 h1 = m2load(h + 4), h1d = m2dag(h1);
    const M2 sl = m2mul(h1d, m2mul(m2resolvent(z, D.et), h1));
    const M2 sr = m2mul(h1, m2mul(m2resolvent(z, D.es), h1d));
    if (A.mode == 1) {
        cd* o = (cd*)A.out + p * 4;
        if (A.side == 0) o[0] = sr.a, o[1] = sr.b, o[2] = sr.c, o[3] = sr.d;
        else o[0] = sl.a, o[1] = sl.b, o[2] = sl.c, o[3] = sl.d;
        return;
    }
    const int M = A.M;
    const cd* d = A.dblk ? A.dblk + D.ik * (2 * M - 1) * 4 : h;
    const cd* u = d + (int64_t)M * 4;
    M2 e = m2load(d);
    m2acc(e, sl);
    if (M == 1) m2acc(e, sr);
    M2 g = m2resolvent(z, e), P = g;                       // g_1 = P_1
    for (int i = 1; i < M; ++i) {
        const M2 ui = m2load(u + 4 * (i - 1)), ud = m2dag(ui);
        e = m2load(d + 4 * i);
        m2acc(e, m2mul(ud, m2mul(g, ui)));
        if (i == M - 1) m2acc(e, sr);
        g = m2resolvent(z, e);
        P = m2mul(g, m2mul(ud, P));
    }
    const M2 gl = m2gamma(sl), gr = m2gamma(sr);
    const M2 c = m2mul(m2mul(P, gl), m2dag(P));
    A.out[p] = land_re(land_re(land_re(land_re(0.0, gr.a, c.a), gr.b, c.c), gr.c, c.b), gr.d, c.d);
}

// ---------------------------------------------------------------- N != 2: TP threads per problem, matrices in LDS or in a workspace
// the sum of a over the TP threads of a problem in a fixed order (the shuffle tree, then the waves in turn); every thread of the
// workgroup calls it
__device__ __forceinline__ double land_group_sum(double a, const int tp_log, double* red) {
    const int w = tp_log < 6 ? (1 << tp_log) : 64;
    for (int o = w >> 1; o > 0; o >>= 1) a += __shfl_xor(a, o);
    if (tp_log > 6) {
        const int wave = threadIdx.x >> 6, nwv = 1 << (tp_log - 6), w0 = (wave >> (tp_log - 6)) << (tp_log - 6);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) red[wave] = a;
        __syncthreads();
        a = red[w0];
        for (int i = 1; i < nwv; ++i) a += red[w0 + i];
    }
    return a;
}

template <bool GLOBAL>
__global__ __launch_bounds__(256) void k_land_wg(const LandArgs A, const int P, const int tp_log, const int ld, cd* ws) {
    extern __shared__ cd sgf_lds[];
    __shared__ double red[8];
    const int N = A.N, TP = 1 << tp_log, NN = N * N, M = A.M;
    cd* const mem = GLOBAL ? ws + (int64_t)blockIdx.x * 7 * N * ld : sgf_lds;
    const int64_t ngroups = (A.nprob + P - 1) / P;
    for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        SgfSlots S;
        const SgfProb Q = sgf_problem(A, P, tp_log, ld, mem, g, S);
        const int t = Q.t;
        const bool live = Q.live;
        const cd *h00 = Q.h00, *h01 = Q.h01;
        const cd z = Q.z;
        sgf_decimate_wg(A, Q, S, red);
        // the self-energies: two eliminations with right-hand sides H01 and H01^+, two products; al and be are free and take them
        cd *sl = S.al, *sr = S.be, *wm = S.wm, *xa = S.xa, *xb = S.xb;
        sgf_resolve(                                       // xa = G_1 H01
            Q, S, [&](int, int q) { return S.et[q]; }, [&](int, int, int e) { return h01[e]; });
        if (live)
            for (int e = t; e < NN; e += TP) {
                const int i = e / N, j = e - i * N, q = i * ld + j;
                cd s{0.0, 0.0};
                for (int k = 0; k < N; ++k) cfma_x(s, cconj(h01[k * N + i]), xa[k * ld + j]);
                sl[q] = s;
            }
        __syncthreads();
        sgf_resolve(                                       // xa = G_0 H01^+
            Q, S, [&](int, int q) { return S.es[q]; }, [&](int i, int j, int) { return cconj(h01[j * N + i]); });
        if (live)
            for (int e = t; e < NN; e += TP) {
                const int i = e / N, j = e - i * N, q = i * ld + j;
                cd s{0.0, 0.0};
                for (int k = 0; k < N; ++k) cfma_x(s, h01[i * N + k], xa[k * ld + j]);
                sr[q] = s;
            }
        __syncthreads();
        if (A.mode == 1) {
            if (live) {
                const cd* s = A.side == 0 ? sr : sl;
                cd* o = (cd*)A.out + Q.p * NN;
                for (int e = t; e < NN; e += TP) {
                    const int i = e / N;
                    o[e] = s[i * ld + (e - i * N)];
                }
            }
            continue;
        }
        // the sweep over the layers; es is free and takes the product U^+ P, et is spare
        cd* up = S.es;
        const cd* D = A.dblk ? A.dblk + Q.ik * (2 * M - 1) * NN : h00;
        const cd* U = D + (int64_t)M * NN;
        for (int l = 0; l < M; ++l) {
            const bool last = l == M - 1;
            const cd* Dl = D + (int64_t)l * NN;
            const cd* Up = U + (int64_t)(l > 0 ? l - 1 : 0) * NN;   // couples the previous layer to this one (read for l > 0)
            if (live)
                for (int e = t; e < NN; e += TP) {
                    const int i = e / N, j = e - i * N, q = i * ld + j;
                    cd v = Dl[e];
                    if (l == 0) {
                        v = cadd(v, sl[q]);
                        up[q] = i == j ? cd{1.0, 0.0} : cd{0.0, 0.0};
                    } else {
                        cd sa{0.0, 0.0}, sb{0.0, 0.0};
                        for (int k = 0; k < N; ++k) {
                            const cd uc = cconj(Up[k * N + i]);
                            cfma_x(sa, uc, xa[k * ld + j]);
                            cfma_x(sb, uc, xb[k * ld + j]);
                        }
                        v = cadd(v, sb);
                        up[q] = sa;
                    }
                    if (last) v = cadd(v, sr[q]);
                    wm[q] = i == j ? csub(z, v) : cd{-v.x, -v.y};
                }
            __syncthreads();
            {                                              // the right-hand side U^+ P becomes X_a
                cd* const o = xa;
                xa = up;
                up = o;
            }
            if (live && !last)
                for (int e = t; e < NN; e += TP) {
                    const int i = e / N;
                    xb[i * ld + (e - i * N)] = U[(int64_t)l * NN + e];
                }
            __syncthreads();
            sgf_solve(wm, xa, xb, N, ld, last ? 2 * N : 3 * N, t, tp_log, live);
        }
        // the trace: B = P Gamma_L (in wm), C = B P^+ (in up), T = Re sum_ab Gamma_R[a, b] C[b, a]; P = xa
        if (live)
            for (int e = t; e < NN; e += TP) {
                const int i = e / N, j = e - i * N;
                cd s{0.0, 0.0};
                for (int k = 0; k < N; ++k) cfma_x(s, xa[i * ld + k], land_gamma(sl[k * ld + j], sl[j * ld + k]));
                wm[i * ld + j] = s;
            }
        __syncthreads();
        if (live)
            for (int e = t; e < NN; e += TP) {
                const int i = e / N, j = e - i * N;
                cd s{0.0, 0.0};
                for (int k = 0; k < N; ++k) cfmac_x(s, wm[i * ld + k], xa[j * ld + k]);
                up[i * ld + j] = s;
            }
        __syncthreads();
        double tr = 0.0;
        if (live)
            for (int e = t; e < NN; e += TP) {
                const int i = e / N, j = e - i * N;
                tr = land_re(tr, land_gamma(sr[i * ld + j], sr[j * ld + i]), up[j * ld + i]);
            }
        tr = land_group_sum(tr, tp_log, red);
        if (live && t == 0) A.out[Q.p] = tr;
    }
}

// ---------------------------------------------------------------- host side
static int land_blocks_launch(tbk_model* dev, const double* k_dev, int64_t nk, int N, int M, cd* dblk) {
    tbk_ctx* ctx = dev->ctx;
    TBK_HIP(hipMemsetAsync(dblk, 0, (size_t)nk * (2 * M - 1) * N * N * sizeof(cd), ctx->stream));
    if (dev->view.nnz == 0) return TBK_OK;
    ProfScope ps(ctx, "land_blocks");
    hipLaunchKernelGGL(k_land_blocks, dim3(nblk(nk * dev->view.nnz)), dim3(256), 0, ctx->stream, dev->view, k_dev, nk, N, M, dblk);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

// `dev` (nullable where the caller allows it) against the leads' cut model
static int land_check_device(const char* who, tbk_model* cut, tbk_model* dev, int nlayer, int nlayers) {
    TBK_REQUIRE(nlayers >= 1 && nlayers <= kLandMaxLayers, TBK_EINVAL, "%s: nlayers=%d (1..%d principal layers)", who, nlayers,
                kLandMaxLayers);
    if (!dev) {
        TBK_REQUIRE(nlayers == 1, TBK_EINVAL, "%s: no device model means one pristine layer, not %d", who, nlayers);
        return TBK_OK;
    }
    TBK_REQUIRE((int64_t)dev->nsta == (int64_t)nlayers * nlayer, TBK_EINVAL, "%s: a device of %d states is not %d layers of %d", who,
                dev->nsta, nlayers, nlayer);
    TBK_REQUIRE(!cut || (dev->dim_k == cut->dim_k && dev->ctx == cut->ctx), TBK_EINVAL,
                "%s: the device must have the surface zone (dim_k %d) and the context of the leads' model", who, cut ? cut->dim_k : 0);
    return TBK_OK;
}

extern "C" int tbk_landauer_blocks(tbk_model* dev, int nlayer, int nlayers, const double* k, int64_t nk, double* d, double* u) {
    const char* who = "tbk_landauer_blocks";
    TBK_REQUIRE(dev, TBK_EINVAL, "%s: null model", who);
    TBK_REQUIRE(nlayer >= 1, TBK_EINVAL, "%s: a principal layer of %d states", who, nlayer);
    TBK_REQUIRE(nlayer <= kSgfMaxN, TBK_EUNSUPPORTED,
                "%s: a principal layer of %d states; the decimation kernels of this build take at most %d", who, nlayer, kSgfMaxN);
    int rc = land_check_device(who, nullptr, dev, nlayer, nlayers);
    if (rc) return rc;
    TBK_REQUIRE(dev->dim_k <= 3, TBK_EINVAL, "%s: surface zone of %d dimensions", who, dev->dim_k);
    TBK_REQUIRE(d && (u || nlayers == 1) && nk >= 1 && (k || dev->dim_k == 0), TBK_EINVAL, "%s: bad argument", who);
    tbk_ctx* ctx = dev->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    const int dk = dev->dim_k, N = nlayer, M = nlayers;
    const size_t kb = al256((size_t)nk * std::max(dk, 1) * sizeof(double)), mb = (size_t)N * N * sizeof(cd);
    const size_t total = 256 + kb + (size_t)nk * (2 * M - 1) * mb;
    TBK_REQUIRE(total <= kSgfMaxBytes, TBK_EUNSUPPORTED, "%s: the blocks of %lld k points need %zu bytes (at most %zu per call): split k",
                who, (long long)nk, total, kSgfMaxBytes);
    void* base = nullptr;
    rc = tbk_ctx_scratch(ctx, total, &base);
    if (rc) return rc;
    double* k_dev = (double*)((unsigned char*)base + 256);
    cd* dblk = (cd*)((unsigned char*)k_dev + kb);
    if (dk > 0) TBK_HIP(hipMemcpyAsync(k_dev, k, (size_t)nk * dk * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    rc = land_blocks_launch(dev, k_dev, nk, N, M, dblk);
    if (rc) return rc;
    for (int64_t i = 0; i < nk; ++i) {
        const cd* src = dblk + i * (2 * M - 1) * N * N;
        TBK_HIP(hipMemcpyAsync((char*)d + i * M * mb, src, M * mb, hipMemcpyDeviceToHost, ctx->stream));
        if (M > 1)
            TBK_HIP(hipMemcpyAsync((char*)u + i * (M - 1) * mb, src + (size_t)M * N * N, (M - 1) * mb, hipMemcpyDeviceToHost,
                                   ctx->stream));
    }
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    return TBK_OK;
}

// the list forms (mesh == null: k[nk][dim_k] from the host) and the mesh mean of T (mesh given: k_uniform_mesh(mesh) generated per
// chunk), through the chunk driver of tbk_sgf.h; the device's blocks are the driver's extra table
static int land_run(const char* who, tbk_model* cut, tbk_model* dev, int N, int M, const double* k, int64_t nk, const int32_t* mesh,
                    int nw, const double* omega, double eta, double tol, int max_iter, int mode, int side, double* out, int32_t* info) {
    int rc = sgf_check_call(who, nw, omega, eta, tol, max_iter, out);
    if (rc) return rc;
    TBK_REQUIRE(mode >= 0 && mode <= 1 && side >= 0 && side <= 1, TBK_EINVAL, "%s: mode %d, side %d", who, mode, side);
    const size_t mb = (size_t)N * N * sizeof(cd);
    SgfPlan P;
    rc = sgf_plan(who, cut, N, nk, mesh, nw, dev ? (size_t)(2 * M - 1) * mb : 0, mode == 1 ? (size_t)nw * mb : (size_t)nw * sizeof(double), nw,
                  P);
    if (rc) return rc;
    TBK_REQUIRE(P.total <= kSgfMaxBytes, TBK_EUNSUPPORTED,
                "%s: %lld k points x %d frequencies of %d layers of %d states need %zu bytes on the device (at most %zu per call): split "
                "omega, or the k list",
                who, (long long)nk, nw, M, N, P.total, kSgfMaxBytes);
    static const char* const names[3] = {"land_n2", "land_wg_lds", "land_wg_global"};
    return sgf_drive(
        who, cut, P, k, omega, eta, tol, max_iter, out, info, "land_rows",
        [&](const SgfChunk& C) {
            if (dev) {
                const int rb = land_blocks_launch(dev, C.k, C.cnt, N, M, C.extra);
                if (rb) return rb;
            }
            LandArgs A{};
            static_cast<SgfCommon&>(A) = C.args;
            A.dblk = dev ? C.extra : nullptr;
            A.M = M;
            A.mode = mode;
            A.side = side;
            A.out = C.out;
            return sgf_launch<LandArgs, k_land_n2, k_land_wg<false>, k_land_wg<true>>(cut->ctx, A, C.ws, P.ws_groups, names);
        },
        [&](const SgfChunk& C) -> int {
            const size_t perw = mode == 1 ? mb : sizeof(double);   // bytes per (k, w): a whole Sigma, or T
            TBK_HIP(hipMemcpyAsync((char*)out + C.first * nw * perw, C.out, (size_t)C.cnt * nw * perw, hipMemcpyDeviceToHost,
                                   cut->ctx->stream));
            return TBK_OK;
        });
}

extern "C" int tbk_lead_self_energy_list(tbk_model* cut, int nlayer, const double* k, int64_t nk, int nomega, const double* omega,
                                         double eta, double tol, int max_iter, int side, double* out, int32_t* info) {
    const char* who = "tbk_lead_self_energy_list";
    int rc = sgf_check_model(who, cut, nlayer, nlayer);
    if (rc) return rc;
    TBK_REQUIRE(k || cut->dim_k == 0, TBK_EINVAL, "%s: null k", who);
    TBK_REQUIRE(cut->dim_k > 0 || nk == 1, TBK_EINVAL, "%s: a model without a surface zone has one point", who);
    return land_run(who, cut, nullptr, nlayer, 1, k, nk, nullptr, nomega, omega, eta, tol, max_iter, 1, side, out, info);
}

extern "C" int tbk_transmission_list(tbk_model* cut, tbk_model* dev, int nlayer, int nlayers, const double* k, int64_t nk, int nomega,
                                     const double* omega, double eta, double tol, int max_iter, double* out, int32_t* info) {
    const char* who = "tbk_transmission_list";
    int rc = sgf_check_model(who, cut, nlayer, nlayer);
    if (rc) return rc;
    rc = land_check_device(who, cut, dev, nlayer, nlayers);
    if (rc) return rc;
    TBK_REQUIRE(k || cut->dim_k == 0, TBK_EINVAL, "%s: null k", who);
    TBK_REQUIRE(cut->dim_k > 0 || nk == 1, TBK_EINVAL, "%s: a model without a surface zone has one point", who);
    return land_run(who, cut, dev, nlayer, nlayers, k, nk, nullptr, nomega, omega, eta, tol, max_iter, 0, 0, out, info);
}

extern "C" int tbk_transmission_mesh(tbk_model* cut, tbk_model* dev, int nlayer, int nlayers, const int32_t* mesh, int nomega,
                                     const double* omega, double eta, double tol, int max_iter, double* out) {
    const char* who = "tbk_transmission_mesh";
    int rc = sgf_check_model(who, cut, nlayer, nlayer);
    if (rc) return rc;
    rc = land_check_device(who, cut, dev, nlayer, nlayers);
    if (rc) return rc;
    TBK_REQUIRE(mesh && cut->dim_k >= 1, TBK_EINVAL, "%s: needs a surface zone of 1 to 3 dimensions and its mesh", who);
    int64_t nk = 1;
    for (int d = 0; d < cut->dim_k; ++d) {
        TBK_REQUIRE(mesh[d] >= 1, TBK_EINVAL, "%s: mesh[%d]=%d", who, d, mesh[d]);
        nk *= mesh[d];
    }
    return land_run(who, cut, dev, nlayer, nlayers, nullptr, nk, mesh, nomega, omega, eta, tol, max_iter, 0, 0, out, nullptr);
}
