// tbk_qgt.hip -- the quantum geometric tensor by the Kubo formula on k lists and uniform meshes.
//
// k in reduced coordinates, H the convention-II matrix of tbk_gen_ham, V^d_nm = <n| d_d H |m>, a and b over ALL dim_k axes (a = b too):
//   per band   Q^n_ab = sum_{m != n} V^a_nm V^b_mn / (E_n - E_m)^2; a pair with |E_n - E_m| <= 1e-9 max(1, |E_n|, |E_m|) contributes
//              nothing to either band (kubo_degenerate, the rule of section 11)
//   band set   Q^occ_ab = sum_{n in occ, m not in occ} of the same terms (no degeneracy rule) = Tr[P d_a P d_b P]
// Q = g - i Omega / 2: g_ab = Re Q_ab is the quantum metric, Omega_ab = -2 Im Q_ab the Berry curvature of tbk_berry_curv_list.
// A (band or set, point) result is dim_k^2 real doubles: g_ab for a <= b in row-major upper-triangle order, then Omega_ab for a < b
// in the same order (QgtOut says where they go).  All of them come from ONE solve and ONE pass over the pairs:
//   n = 2          k_qgt2: one lane per k, H = d0 + d.sigma and every d_a d in registers, no eigen-solve; on a mesh the lane makes
//                  its own k and feeds the reduction
//   n = 1, 3..32   k_qgt_lds: the tiling of k_kubo_lds with one LDS slot per direction: U, T and dim_k slots of n^2 per point
//   33..2048       per chunk and per pair a <= b: k_kubo_wsp (as it is) builds W^a and W^b, k_qgt_contract keeps both parts of the
//                  pair sums, k_qgt_occ_sum adds a band set's shares
// Mesh means: per-workgroup partials in a grid-stride order that depends on the mesh shape alone (k_qgt2's own sums at n = 2,
// tbk_kubo.h's k_kubo_plane over a chunk's buffer otherwise), block_sum inside a workgroup, k_kubo_rows across workgroups, chunk
// results added in chunk order on the host.  No floating-point atomics anywhere.
#include <math.h>
#include <string.h>
#include "tbk_kubo.h"

// where component c of (channel ch, point i) goes: p[ch sch + i sk + c sc]
struct QgtOut {
    double* p;
    int64_t sch, sk, sc;
};
__device__ __forceinline__ double& qgt_at(const QgtOut& o, const int64_t ch, const int64_t i, const int c) {
    return o.p[ch * o.sch + i * o.sk + c * o.sc];
}

// ---------------------------------------------------------------- n = 2: closed form in registers
// With d_a = d_a d and x_a = d_a x d:  g_ab = (d_a.d_b - (dhat.d_a)(dhat.d_b)) / (4 |d|^2) = x_a.x_b / (4 |d|^4) for both bands (the
// second form is Lagrange's identity; it does not subtract two nearly equal products where d_a is nearly parallel to d), and
// Omega_ab = d.(d_a x d_b) / (2 |d|^3) for band 0, the expression of curv2_point, with the other sign for band 1.
// q: the DK^2 doubles of band 0 without the degeneracy rule; returns whether the pair falls under it.
template <int DK>
__device__ __forceinline__ bool qgt2_point(const ModelView& mv, const double (&kk)[4], double (&q)[DK * DK]) {
    cd z[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) z[d] = d < mv.dim_k ? expi2pi(kk[d]) : cd{1.0, 0.0};
    double dv[3] = {0.0, 0.0, 0.0}, dd[DK][3], mid = 0.0;
#pragma unroll
    for (int w = 0; w < (DK + 1) / 2; ++w) {               // dham_terms gives two directions per walk
        const int d0 = 2 * w, d1 = 2 * w + 1 < DK ? 2 * w + 1 : 2 * w;
        cd h[3], va[3], vb[3];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const int a = s == 2 ? 1 : 0, b = s == 0 ? 0 : 1;   // slots (0,0) (0,1) (1,1)
            dham_terms(mv, a, b, mv.slot_ptr[s], mv.slot_ptr[s + 1], kk, z, d0, d1, h[s], va[s], vb[s]);
        }
        if (w == 0) {                                      // H = d0 + dx sx + dy sy + dz sz:  H_01 = dx - i dy,  H_00 - H_11 = 2 dz
            dv[0] = h[1].x;
            dv[1] = -h[1].y;
            dv[2] = 0.5 * (h[0].x - h[2].x);
            mid = 0.5 * (h[0].x + h[2].x);
        }
        dd[d0][0] = va[1].x;
        dd[d0][1] = -va[1].y;
        dd[d0][2] = 0.5 * (va[0].x - va[2].x);
        if (d1 != d0) {
            dd[d1][0] = vb[1].x;
            dd[d1][1] = -vb[1].y;
            dd[d1][2] = 0.5 * (vb[0].x - vb[2].x);
        }
    }
    const double dx = dv[0], dy = dv[1], dz = dv[2];
    const double d2 = dx * dx + dy * dy + dz * dz, dn = sqrt(d2);
    double x[DK][3];
#pragma unroll
    for (int a = 0; a < DK; ++a) {
        x[a][0] = dd[a][1] * dz - dd[a][2] * dy;
        x[a][1] = dd[a][2] * dx - dd[a][0] * dz;
        x[a][2] = dd[a][0] * dy - dd[a][1] * dx;
    }
    const double ig = 1.0 / (4.0 * d2 * d2), io = 1.0 / (2.0 * d2 * dn);
    int c = 0;
#pragma unroll
    for (int a = 0; a < DK; ++a)
#pragma unroll
        for (int b = a; b < DK; ++b) q[c++] = (x[a][0] * x[b][0] + x[a][1] * x[b][1] + x[a][2] * x[b][2]) * ig;
#pragma unroll
    for (int a = 0; a < DK; ++a)
#pragma unroll
        for (int b = a + 1; b < DK; ++b) {
            const double cx = dd[a][1] * dd[b][2] - dd[a][2] * dd[b][1], cy = dd[a][2] * dd[b][0] - dd[a][0] * dd[b][2],
                         cz = dd[a][0] * dd[b][1] - dd[a][1] * dd[b][0];
            q[c++] = (dx * cx + dy * cy + dz * cz) * io;
        }
    const double e0 = mid - dn, e1 = mid + dn;
    return kubo_degenerate(e1 - e0, e0, e1);
}

// sel = 0: per band (two channels, the rule applied); +1 / -1: the set {0} / {1} (one channel, no rule).
// List (k given): one lane per point, results to `out`.  Mesh (k null): the points of k_uniform_mesh(N) in a grid-stride order, the
// sums of band 0 (or of the set) over the workgroup's points to part[c][gridDim.x]; band 1 has the same g and -Omega.
template <int DK>
__global__ __launch_bounds__(256) void k_qgt2(const ModelView mv, const double* __restrict__ k, const int64_t nk, const int N0, const int N1,
                                              const int N2, const int sel, const QgtOut out, double* __restrict__ part) {
    constexpr int NC = DK * DK, NG = DK * (DK + 1) / 2;
    __shared__ double red[4];
    double acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = 0.0;
    for (int64_t ik = (int64_t)blockIdx.x * 256 + threadIdx.x; ik < nk; ik += (int64_t)gridDim.x * 256) {
        double kk[4] = {0.0, 0.0, 0.0, 0.0};
        if (k) {
#pragma unroll
            for (int d = 0; d < DK; ++d) kk[d] = k[ik * DK + d];
        } else {                                           // k_uniform_mesh's point, bit for bit
            const int N[3] = {N0, N1, N2};
            int ii[3];
            mesh_point(N, ik, ii);
#pragma unroll
            for (int d = 0; d < DK; ++d) kk[d] = (double)ii[d] / (double)N[d];
        }
        double q[NC];
        const bool deg = qgt2_point<DK>(mv, kk, q);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if (sel == 0 && deg) q[c] = 0.0;
            if (sel < 0 && c >= NG) q[c] = -q[c];
        }
        if (k) {
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                qgt_at(out, 0, ik, c) = q[c];
                if (sel == 0) qgt_at(out, 1, ik, c) = c >= NG ? -q[c] : q[c];
            }
        } else {
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[c] += q[c];
        }
    }
    if (k) return;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const double t = block_sum(acc[c], red);
        if (threadIdx.x == 0) part[(int64_t)c * gridDim.x + blockIdx.x] = t;
        __syncthreads();                                   // (red is reused by the next component)
    }
}

// ---------------------------------------------------------------- n = 1, 3..32: everything of a point in LDS
// P = min(64, 4096 / ((2 + DK) n^2)) points per workgroup (at least one): U (read once from HBM), T and one slot per direction.  For
// every d: slot d = d_d H from the non-empty slots, T = d_d H U^T, slot d := V^d = conj(U) T.  Then one lane per (point, band) walks
// m once and adds, for every a <= b, Re and Im of V^a_bm conj(V^b_bm) / (E_b - E_m)^2 in m order.  A band set's shares go over the
// then dead U and T (DK^2 n doubles per point <= 4 n^2 from n = 3) and are added in band order.  Dynamic LDS: 64 KiB at most but for
// DK = 3 at n = 27..32 (one point, 5 n^2 cd: up to 80 KiB, requested with the attribute by qgt_lds_launch).
#define QGT_LDS_CD 4096
static inline int qgt_lds_points(int n, int dk) { return std::max(1, std::min(64, QGT_LDS_CD / ((2 + dk) * n * n))); }
template <int DK>
__global__ __launch_bounds__(256) void k_qgt_lds(const ModelView mv, const double* __restrict__ k, const cd* __restrict__ evec,
                                                 const double* __restrict__ eval, const int64_t nk, const int P,
                                                 const int* __restrict__ occ, const int64_t first, const QgtOut out) {
    constexpr int NC = DK * DK, NG = DK * (DK + 1) / 2;
    extern __shared__ __align__(16) unsigned char qgt_raw[];
    cd* L = (cd*)qgt_raw;
    const int n = mv.nsta, nn = n * n;
    const int64_t ik0 = (int64_t)blockIdx.x * P;
    const int np = (int)std::min<int64_t>(P, nk - ik0);
    cd* U = L;
    cd* T = L + P * nn;
    cd* V = L + 2 * P * nn;                                        // slot d at V + d P nn
    kubo_lds_load(U, evec, nk, ik0, np, n, nn, [&](const int e) {
#pragma unroll
        for (int d = 0; d < DK; ++d) V[d * P * nn + e] = cd{0.0, 0.0};
    });
    __syncthreads();
    for (int e = threadIdx.x; e < np * mv.nnz; e += 256) {
        const int p = e / mv.nnz;
        const int4 z4 = mv.nz[e - p * mv.nnz];
        const int a = z4.x & 0xffff, b = z4.x >> 16;
        double kk[4];
        cd z[4];
        k_phases(mv, k, ik0 + p, kk, z);
#pragma unroll
        for (int w = 0; w < (DK + 1) / 2; ++w) {                   // dham_terms gives two directions per walk
            const int d0 = 2 * w, d1 = 2 * w + 1 < DK ? 2 * w + 1 : 2 * w;
            cd h, v0, v1;
            dham_terms(mv, a, b, z4.y, z4.z, kk, z, d0, d1, h, v0, v1);
            cd* D0 = V + d0 * P * nn + p * nn;
            D0[a * n + b] = v0;
            D0[b * n + a] = cconj(v0);
            if (d1 != d0) {
                cd* D1 = V + d1 * P * nn + p * nn;
                D1[a * n + b] = v1;
                D1[b * n + a] = cconj(v1);
            }
        }
    }
    __syncthreads();
    for (int d = 0; d < DK; ++d) kubo_lds_rotate(V + d * P * nn, T, U, np, n, nn);   // slot d := V^d
    double* share = (double*)L;                                    // (U and T are dead)
    for (int e = threadIdx.x; e < np * n; e += 256) {
        const int p = e / n, b = e - p * n;
        const int64_t ik = ik0 + p;
        const double eb = eval[(int64_t)b * nk + ik];
        const cd* vr = V + p * nn + b * n;
        double acc[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[c] = 0.0;
        if (!occ || occ[b]) {
            for (int mm = 0; mm < n; ++mm) {
                if (mm == b) continue;
                const double em = eval[(int64_t)mm * nk + ik];
                const double de = eb - em;
                if (occ ? occ[mm] != 0 : kubo_degenerate(de, eb, em)) continue;
                const double inv = 1.0 / (de * de);
                cd v[DK];
#pragma unroll
                for (int d = 0; d < DK; ++d) v[d] = vr[d * P * nn + mm];
                int c = 0;
#pragma unroll
                for (int a = 0; a < DK; ++a)
#pragma unroll
                    for (int bb = a; bb < DK; ++bb) acc[c++] += (v[a].x * v[bb].x + v[a].y * v[bb].y) * inv;   // Re V^a_bm conj(V^b_bm)
#pragma unroll
                for (int a = 0; a < DK; ++a)
#pragma unroll
                    for (int bb = a + 1; bb < DK; ++bb) acc[c++] += (v[a].y * v[bb].x - v[a].x * v[bb].y) * inv;   // Im
            }
        }
#pragma unroll
        for (int c = NG; c < NC; ++c) acc[c] *= -2.0;
        if (occ) {
#pragma unroll
            for (int c = 0; c < NC; ++c) share[NC * e + c] = acc[c];
        } else {
#pragma unroll
            for (int c = 0; c < NC; ++c) qgt_at(out, b, first + ik, c) = acc[c];
        }
    }
    if (occ) {
        __syncthreads();
        for (int p = threadIdx.x; p < np; p += 256) {
            double s[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) s[c] = 0.0;
            for (int b = 0; b < n; ++b)
#pragma unroll
                for (int c = 0; c < NC; ++c) s[c] += share[NC * (p * n + b) + c];
#pragma unroll
            for (int c = 0; c < NC; ++c) qgt_at(out, 0, first + ik0 + p, c) = s[c];
        }
    }
}

template <int DK>
static int qgt_lds_launch(tbk_model* m, const double* kp, const cd* vc, const double* ec, int64_t cnt, const int* occ, int64_t first,
                          const QgtOut& out) {
    tbk_ctx* ctx = m->ctx;
    const int n = m->nsta, P = qgt_lds_points(n, DK);
    const size_t lds = (size_t)(2 + DK) * P * n * n * sizeof(cd);
    if (lds > 64 * 1024)                                           // (DK = 3 at n = 27..32)
        TBK_HIP(hipFuncSetAttribute((const void*)k_qgt_lds<DK>, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024));
    ProfScope ps(ctx, "qgt_lds");
    hipLaunchKernelGGL(k_qgt_lds<DK>, dim3((unsigned)((cnt + P - 1) / P)), dim3(256), lds, ctx->stream, m->view, kp, vc, ec, cnt, P, occ,
                       first, out);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

// ---------------------------------------------------------------- 33..2048 states: the pair (a, b) on k_kubo_wsp's W^a, W^b
// One lane per (ik, band b), as k_kubo_contract, keeping both parts: sum_m V^a_bm conj(V^b_bm) / (E_b - E_m)^2 in m order.  Component
// cg gets the real part, com (a < b; -1 for a = b, where W^b is W^a and is not read) -2 times the imaginary part.  A band set's
// shares go to tmp[ik][b][2], summed per point by k_qgt_occ_sum.
__global__ __launch_bounds__(256) void k_qgt_contract(const cd* __restrict__ evec, const double* __restrict__ eval,
                                                      const cd* __restrict__ wt, const int64_t nk, const int n,
                                                      const int* __restrict__ occ, const int64_t first, const int cg, const int com,
                                                      const QgtOut out, double* __restrict__ tmp) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nk * n) return;
    const int64_t ik = idx / n;
    const int b = (int)(idx - ik * n);
    const int64_t nn = (int64_t)n * n;
    const cd* u = evec + ((int64_t)b * nk + ik) * n;
    const cd* w0 = wt + (2 * ik) * nn;
    const cd* w1 = w0 + nn;
    const double eb = eval[(int64_t)b * nk + ik];
    double re = 0.0, im = 0.0;
    if (!occ || occ[b]) {
        for (int m = 0; m < n; ++m) {
            if (m == b) continue;
            const double em = eval[(int64_t)m * nk + ik];
            const double de = eb - em;
            if (occ ? occ[m] != 0 : kubo_degenerate(de, eb, em)) continue;
            const double inv = 1.0 / (de * de);
            cd va{0.0, 0.0}, vb{0.0, 0.0};
            if (com >= 0) {
                for (int i = 0; i < n; ++i) {
                    cfmac(va, u[i], w0[(int64_t)i * n + m]);
                    cfmac(vb, u[i], w1[(int64_t)i * n + m]);
                }
            } else {
                for (int i = 0; i < n; ++i) cfmac(va, u[i], w0[(int64_t)i * n + m]);
                vb = va;
            }
            re += (va.x * vb.x + va.y * vb.y) * inv;
            im += (va.y * vb.x - va.x * vb.y) * inv;
        }
    }
    if (occ) {
        tmp[2 * idx] = re;
        tmp[2 * idx + 1] = -2.0 * im;
    } else {
        qgt_at(out, b, first + ik, cg) = re;
        if (com >= 0) qgt_at(out, b, first + ik, com) = -2.0 * im;
    }
}

__global__ __launch_bounds__(256) void k_qgt_occ_sum(const double* __restrict__ tmp, const int64_t nk, const int n, const int64_t first,
                                                     const int cg, const int com, const QgtOut out) {
    const int64_t ik = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (ik >= nk) return;
    double s0 = 0.0, s1 = 0.0;
    for (int b = 0; b < n; ++b) {
        s0 += tmp[2 * (ik * n + b)];
        s1 += tmp[2 * (ik * n + b) + 1];
    }
    qgt_at(out, 0, first + ik, cg) = s0;
    if (com >= 0) qgt_at(out, 0, first + ik, com) = s1;
}

// ---------------------------------------------------------------- mesh means of the chunked forms
// k_kubo_plane's source: channel `row` of buf[row][stride], the chunk's first P.nplane entries as the plane
struct QgtBufSrc {
    const double* buf;
    int64_t stride;
    __device__ __forceinline__ void plane(const PlaneArgs&, int, const int64_t p, const int row, double (&w)[1]) const {
        w[0] = buf[row * stride + p];
    }
};

// ---------------------------------------------------------------- host side
// this unit's own checks (kubo_check demands dim_k >= 2 and two different axes); mask as kubo_check's
static int qgt_check(const char* fn, tbk_model* m, const int32_t* occ, int nocc, std::vector<int>& mask) {
    TBK_REQUIRE(m, TBK_EINVAL, "%s: null model", fn);
    TBK_REQUIRE(m->dim_k >= 1 && m->dim_k <= 3, TBK_EINVAL, "%s: the quantum geometric tensor needs dim_k 1..3 (the model has %d)", fn,
                m->dim_k);
    return kubo_occ_mask(fn, m, occ, nocc, mask);
}

static int qgt2_launch(tbk_model* m, const double* k_dev, int64_t nk, const int32_t* mesh, int sel, const QgtOut& out, int gx,
                       double* part) {
    tbk_ctx* ctx = m->ctx;
    const int dk = m->dim_k;
    const int N0 = mesh ? mesh[0] : 1, N1 = mesh && dk > 1 ? mesh[1] : 1, N2 = mesh && dk > 2 ? mesh[2] : 1;
    const dim3 grid(mesh ? (unsigned)gx : nblk(nk));
    ProfScope ps(ctx, "qgt2");
    if (dk == 1) hipLaunchKernelGGL(k_qgt2<1>, grid, dim3(256), 0, ctx->stream, m->view, k_dev, nk, N0, N1, N2, sel, out, part);
    else if (dk == 2) hipLaunchKernelGGL(k_qgt2<2>, grid, dim3(256), 0, ctx->stream, m->view, k_dev, nk, N0, N1, N2, sel, out, part);
    else hipLaunchKernelGGL(k_qgt2<3>, grid, dim3(256), 0, ctx->stream, m->view, k_dev, nk, N0, N1, N2, sel, out, part);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

// n != 2 over points [0, nk) of a k list or a mesh: ONE solve per chunk, every component from it; `after(first, cnt)` runs behind a
// chunk's kernels.  `out` is indexed by first + (point in the chunk) when `absolute`, else by the point in the chunk.
template <class After>
static int qgt_contract(tbk_model* m, const double* k_all_dev, const int32_t* mesh, int64_t nk, const std::vector<int>& mask,
                        const KuboChunks& w, const QgtOut& out, bool absolute, After&& after) {
    tbk_ctx* ctx = m->ctx;
    const int n = m->nsta, dk = m->dim_k, ng = dk * (dk + 1) / 2;
    cd* wt = w.extra<cd>(0);
    int* occ_dev = w.extra<int>(1);
    double* tmp = w.extra<double>(2);
    const bool manifold = !mask.empty();
    const int* occ = manifold ? (const int*)occ_dev : (const int*)nullptr;
    if (manifold) TBK_HIP(hipMemcpyAsync(occ_dev, mask.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    return kubo_for_chunks(m, w, k_all_dev, mesh, nk, [&](int64_t first, int64_t cnt, const double* kp, const double* ec, const cd* vc) -> int {
        const int64_t at = absolute ? first : 0;
        if (n <= 32) {
            int rc = dk == 1 ? qgt_lds_launch<1>(m, kp, vc, ec, cnt, occ, at, out)
                             : (dk == 2 ? qgt_lds_launch<2>(m, kp, vc, ec, cnt, occ, at, out)
                                        : qgt_lds_launch<3>(m, kp, vc, ec, cnt, occ, at, out));
            if (rc) return rc;
            return after(first, cnt);
        }
        int cg = 0, com = ng;
        for (int a = 0; a < dk; ++a)
            for (int b = a; b < dk; ++b, ++cg) {
                {
                    ProfScope ps(ctx, "qgt_wsp");
                    hipLaunchKernelGGL(k_kubo_wsp, dim3((unsigned)cnt, (unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, m->view, kp,
                                       vc, cnt, a, b, wt);
                    TBK_HIP(hipGetLastError());
                }
                const int co = a < b ? com++ : -1;
                {
                    ProfScope ps(ctx, "qgt_contract");
                    hipLaunchKernelGGL(k_qgt_contract, dim3(nblk(cnt * n)), dim3(256), 0, ctx->stream, vc, ec, (const cd*)wt, cnt, n, occ,
                                       at, cg, co, out, tmp);
                    TBK_HIP(hipGetLastError());
                }
                if (manifold) {
                    ProfScope ps(ctx, "qgt_occ_sum");
                    hipLaunchKernelGGL(k_qgt_occ_sum, dim3(nblk(cnt)), dim3(256), 0, ctx->stream, (const double*)tmp, cnt, n, at, cg, co,
                                       out);
                    TBK_HIP(hipGetLastError());
                }
            }
        return after(first, cnt);
    });
}

extern "C" int tbk_qgt_list(tbk_model* m, const double* k, int64_t nk, const int32_t* occ, int nocc, double* out) {
    const char* fn = "tbk_qgt_list";
    std::vector<int> mask;
    int rc = qgt_check(fn, m, occ, nocc, mask);
    if (rc) return rc;
    TBK_REQUIRE(nk >= 0 && out && (k || nk == 0), TBK_EINVAL, "%s: bad k list or output", fn);
    const int n = m->nsta, dk = m->dim_k, nc = dk * dk;
    const bool manifold = occ != nullptr;
    const int nch = manifold ? 1 : n;
    const int64_t nout = (int64_t)nch * nk * nc;
    if (nk == 0) return TBK_OK;
    if (manifold && nocc == n) {           // the complement is empty: nothing to sum
        std::fill(out, out + nout, 0.0);
        return TBK_OK;
    }
    tbk_ctx* ctx = m->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    KuboChunks cw = n != 2 ? kubo_contract_chunks(n, dk, nk, manifold, 2) : KuboChunks();
    double *k_dev, *o_dev;
    KuboCarve ws;
    ws.add(k_dev, (size_t)nk * dk * sizeof(double)), ws.add(o_dev, (size_t)nout * sizeof(double)), ws.add(cw.base, cw.bytes());
    rc = kubo_carve(ctx, ws);
    if (rc) return rc;
    const QgtOut o{o_dev, nk * nc, nc, 1};                         // out[ch][ik][c]
    TBK_HIP(hipMemcpyAsync(k_dev, k, (size_t)nk * dk * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (n == 2) {
        rc = qgt2_launch(m, k_dev, nk, nullptr, manifold ? (mask[0] ? 1 : -1) : 0, o, 0, nullptr);
    } else {
        rc = qgt_contract(m, k_dev, nullptr, nk, mask, cw, o, true, [](int64_t, int64_t) -> int { return TBK_OK; });
    }
    if (rc) return rc;
    TBK_HIP(hipMemcpyAsync(out, o_dev, (size_t)nout * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    return TBK_OK;
}

extern "C" int tbk_qgt_mesh(tbk_model* m, const int32_t* mesh, const int32_t* occ, int nocc, double* out) {
    const char* fn = "tbk_qgt_mesh";
    std::vector<int> mask;
    int rc = qgt_check(fn, m, occ, nocc, mask);
    if (rc) return rc;
    TBK_REQUIRE(mesh && out, TBK_EINVAL, "%s: null argument", fn);
    const int n = m->nsta, dk = m->dim_k, nc = dk * dk, ng = dk * (dk + 1) / 2;
    PlaneArgs P;                           // one "plane": the whole mesh
    rc = kubo_whole_mesh(fn, mesh, dk, P);
    if (rc) return rc;
    const int64_t npts = P.npts;
    const bool manifold = occ != nullptr;
    const int nch = manifold ? 1 : n;
    if (manifold && nocc == n) {
        std::fill(out, out + (size_t)nch * nc, 0.0);
        return TBK_OK;
    }
    tbk_ctx* ctx = m->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    const double inv = 1.0 / (double)npts;
    double *buf, *part, *rows;
    KuboCarve ws;
    std::vector<double> sums;
    if (n == 2) {                          // the lanes make their own k: nothing per point touches HBM
        const int gx = kubo_plane_gx(P);
        ws.add(part, (size_t)nc * gx * sizeof(double)), ws.add(rows, (size_t)nc * sizeof(double));
        rc = kubo_carve(ctx, ws);
        if (rc) return rc;
        rc = qgt2_launch(m, nullptr, npts, mesh, manifold ? (mask[0] ? 1 : -1) : 0, QgtOut{nullptr, 0, 0, 0}, gx, part);
        if (rc) return rc;
        rc = kubo_rows_to_host(ctx, "qgt_rows", part, gx, nc, rows, sums);
        if (rc) return rc;
        for (int c = 0; c < nc; ++c) {
            out[c] = sums[c] * inv;
            if (!manifold) out[nc + c] = c >= ng ? -out[c] : out[c];   // band 1: the same g, -Omega, bit for bit
        }
        return TBK_OK;
    }
    // chunked forms: a chunk's values buf[c][ch][chunk], its partials, one row of sums per chunk
    KuboChunks cw = kubo_contract_chunks(n, dk, npts, manifold, 2);
    const int64_t chunk = cw.chunk, nchunks = (npts + chunk - 1) / chunk, nrows = (int64_t)nc * nch;
    P.nplane = chunk;
    const int gx = kubo_plane_gx(P);
    ws.add(buf, (size_t)nrows * chunk * sizeof(double)), ws.add(part, (size_t)nrows * gx * sizeof(double));
    ws.add(rows, (size_t)nchunks * nrows * sizeof(double)), ws.add(cw.base, cw.bytes());
    rc = kubo_carve(ctx, ws);
    if (rc) return rc;
    const QgtOut o{buf, chunk, 1, (int64_t)nch * chunk};           // buf[c][ch][i]: row = c nch + ch
    rc = qgt_contract(m, nullptr, mesh, npts, mask, cw, o, false, [&](int64_t first, int64_t cnt) -> int {
        ProfScope ps(ctx, "qgt_rows");
        P.nplane = cnt;
        int rc = kubo_plane_launch<1>(ctx, QgtBufSrc{buf, chunk}, P, (int)nrows, nrows, gx, part);
        return rc ? rc : kubo_rows_launch(ctx, part, gx, nrows, rows + (first / chunk) * nrows);
    });
    if (rc) return rc;
    rc = kubo_to_host(ctx, rows, nchunks * nrows, sums);
    if (rc) return rc;
    for (int ch = 0; ch < nch; ++ch)
        for (int c = 0; c < nc; ++c) {
            double acc = 0.0;                                      // chunk results in chunk order
            for (int64_t q = 0; q < nchunks; ++q) acc += sums[(size_t)(q * nrows + (int64_t)c * nch + ch)];
            out[(size_t)ch * nc + c] = acc * inv;
        }
    return TBK_OK;
}
