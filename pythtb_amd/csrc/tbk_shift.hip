// tbk_shift.hip -- shift and injection photocurrents: the interband second-order optical response.
//
// k reduced, H the convention-II matrix of tbk_gen_ham, V^a = d_a H (tbk_gen_dham), W^{ab} = d_a d_b H (tbk_gen_ddham), E_n and |n> the
// eigenpairs of the solver, E_nm = E_n - E_m, G(n) the group of band n (band_group, tbk_dham.h).  For G(n) != G(m):
//   r^b_nm   = -i V^b_nm / E_nm                                                  (0 inside a group)
//   r^b_nm;a = (i / E_nm) [ T^{ba}_nm / E_nm - W^{ba}_nm + sum_{p not in G(n) u G(m)} (V^b_np V^a_pm / E_pm - V^a_np V^b_pm / E_np) ]
//   T^{ba}_nm = sum_{p in G(n)} (V^a_np V^b_pm + V^b_np V^a_pm) - sum_{p in G(m)} (V^b_np V^a_pm + V^a_np V^b_pm)
//   X^{abc}_nm = r^b_mn r^c_nm;a + r^c_mn r^b_nm;a
//   Y^{abc}_nm = sum_{m' in G(m)} V^a_mm' r^c_m'n r^b_nm - sum_{n' in G(n)} r^c_mn V^a_nn' r^b_n'm
//   K_abc(w) = mean_k sum_{E_m > E_n, G(n) != G(m)} (f_n - f_m) Im X^{abc}_nm D(E_m - E_n, w)        (shift, real)
//   N_abc(w) = the same sum of Y^{abc}_nm                                                             (injection, complex)
//   D(eps, w) = (eta / pi) [1 / ((eps - w)^2 + eta^2) + 1 / ((eps + w)^2 + eta^2)]
// The sums over (n in G1, m in G2) do not change when the solver's eigenvectors are rotated inside a group.
//
// Pipeline (tbk_pairs.h's sweep driver on tbk_kubo.h's chunk loop): the device k generator, the eigen-solver with vectors, then per
// current direction a one PASS:
// the PAIR stage writes a record (eps, fields...) per (point, pair i < j) -- eps = -1 for a pair that adds nothing, which is decided
// before the walk over p -- and the FREQUENCY stage (k_pair_omega over ShOmega) adds each k-group's sums into part[G][row]; k_group_rows
// sums the groups.
//   n <= 32    k_sh_pairs: U, the V^d and W^{da} of the pass and one scratch matrix of several points in LDS
//   n > 32     k_pair_wsp (d H U^T and d d H U^T from the sparse slots), k_opt_vprod (conj(U) times it), k_sh_pairs_wide
// A pass of the full tensor holds at most 3 V + 3 W: at 32 states 8 matrices of 16 KiB with U and the scratch, 128 KiB of the CU's 160.
// Every partition depends on the mesh, n, dim_k, n_omega and the components alone, and nothing uses atomics: two calls give the same bits.
#include <math.h>
#include <string.h>
#include "tbk_pairs.h"

#define SH_LDS_CD 4096                                   // c128 of LDS per workgroup of k_sh_pairs while more than one point fits

// One pass: the current direction a and the light directions bdir[nb].  Operator j < nv is V^{vdir[j]}; operator nv + j (shift only) is
// W^{bdir[j] a}.  Field f is the light pair (bdir[f1[f]], bdir[f2[f]]): one double (Im X, shift) or two (Re Y, Im Y; injection).
// The small index lists are packed two bits per entry (sh_get, sh_set), so that no kernel indexes an argument array with a loop
// variable: the pass stays in scalar registers.
__host__ __device__ __forceinline__ int sh_get(const unsigned pk, const int i) { return (int)((pk >> (2 * i)) & 3u); }
struct ShiftPass {
    int kind;   // 0 shift, 1 injection
    int a, ia;  // V^a is operator ia
    int nv, nb, nfld;
    unsigned vdir, bdir, ib, f1, f2;
    __host__ __device__ int nops() const { return kind == 0 ? nv + nb : nv; }
    __host__ __device__ int nf() const { return kind == 0 ? nfld : 2 * nfld; }
    // as the SLOTS of tbk_pairs.h: the slot value of operator op, d_{vdir[op]} H_ab or d_{bdir[op - nv]} d_a H_ab
    __device__ __forceinline__ cd one(const ModelView& mv, const int op, const int4 z4, const double (&kk)[4], const cd (&z)[4]) const {
        const int sa = z4.x & 0xffff, sb = z4.x >> 16;
        if (op < nv) {
            cd h, v0, v1;
            dham_terms(mv, sa, sb, z4.y, z4.z, kk, z, sh_get(vdir, op), sh_get(vdir, op), h, v0, v1);
            return v0;
        }
        return ddham_terms(mv, sa, sb, z4.y, z4.z, kk, z, sh_get(bdir, op - nv), a);
    }
    __device__ __forceinline__ void all(const ModelView& mv, const int4 z4, const double (&kk)[4], const cd (&z)[4],
                                        cd (&sv)[6][256]) const {
        for (int d = 0; d < nops(); ++d) sv[d][threadIdx.x] = one(mv, d, z4, kk, z);
    }
};

static inline void sh_set(unsigned& pk, const int i, const int v) { pk = (pk & ~(3u << (2 * i))) | ((unsigned)v << (2 * i)); }

// the weight of the pair (i, j), E_j >= E_i: f_i - f_j on a mesh; with a band set, +1 for i in occ and j outside, -1 the other way
__device__ __forceinline__ double sh_weight(const double en, const double em, const double mu, const double kT,
                                            const int* __restrict__ occ, const int i, const int j) {
    if (occ) return occ[i] ? (occ[j] ? 0.0 : 1.0) : (occ[j] ? -1.0 : 0.0);
    if (kT == 0.0) return (en <= mu && !(em <= mu)) ? 1.0 : 0.0;
    const double eps = em - en;
    return -opt_weight(en, em, eps, mu, kT) * eps;
}

// v[i] of three without a dynamic index: the three values are read first, so that the choice is between registers, not addresses
__device__ __forceinline__ cd sh_pick(const cd (&v)[3], const int i) {
    const cd v0 = v[0], v1 = v[1], v2 = v[2];
    return i == 0 ? v0 : (i == 1 ? v1 : v2);
}

// One record at r for the pair (i, j), i < j, of a point: M(op, row, col) the operators in the eigenbasis, E(b) the levels.
// Every lane walks p upwards, so the members of a group sum in the same order.
template <int KIND, class Mat, class Eig>
__device__ __forceinline__ void sh_record(double* __restrict__ r, const ShiftPass& S, const int n, const int i, const int j,
                                          const int gi0, const int gi1, const int gj0, const int gj1, const double wgt, const Mat& M,
                                          const Eig& E) {
    const int nf = S.nf();
    const double en = E(i), em = E(j), enm = en - em;
    if (wgt == 0.0 || j < gi1 || !(enm < 0.0)) {                   // no weight, one group, or not a number
        r[0] = -1.0;
        for (int f = 0; f < nf; ++f) r[1 + f] = 0.0;
        return;
    }
    const double inv = 1.0 / enm;
    r[0] = -enm;
    cd rmn[3], q[3];                                               // r^b_ji; r^b_ij;a (shift) or the two group sums' difference
    if constexpr (KIND == 0) {
        cd T[3], Ps[3];
#pragma unroll
        for (int b = 0; b < 3; ++b) T[b] = Ps[b] = cd{0.0, 0.0};
        for (int p = 0; p < n; ++p) {
            const bool in_n = p >= gi0 && p < gi1, in_m = p >= gj0 && p < gj1;
            const cd va_ip = M(S.ia, i, p), va_pj = M(S.ia, p, j);
            double ipm = 0.0, inp = 0.0;
            if (!in_n && !in_m) {
                const double ep = E(p);
                ipm = 1.0 / (ep - em);
                inp = 1.0 / (en - ep);
            }
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                if (b >= S.nb) continue;
                const cd vb_ip = M(sh_get(S.ib, b), i, p), vb_pj = M(sh_get(S.ib, b), p, j);
                const cd t1 = cmul(vb_ip, va_pj), t2 = cmul(va_ip, vb_pj);
                if (in_n) T[b] = cadd(T[b], cadd(t1, t2));
                else if (in_m) T[b] = csub(T[b], cadd(t1, t2));
                else Ps[b] = cadd(Ps[b], csub(cscale(t1, ipm), cscale(t2, inp)));
            }
        }
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            if (b >= S.nb) continue;
            const cd x = cadd(csub(cscale(T[b], inv), M(S.nv + b, i, j)), Ps[b]);
            q[b] = cd{-x.y * inv, x.x * inv};                      // r^b_ij;a = (i / E_ij) x
            const cd v = M(sh_get(S.ib, b), j, i);
            rmn[b] = cd{-v.y * inv, v.x * inv};                    // r^b_ji = -i V^b_ji / E_ji = i V^b_ji / E_ij
        }
        for (int f = 0; f < S.nfld; ++f) {
            const int b = sh_get(S.f1, f), c = sh_get(S.f2, f);
            const cd x = cadd(cmul(sh_pick(rmn, b), sh_pick(q, c)), cmul(sh_pick(rmn, c), sh_pick(q, b)));
            r[1 + f] = wgt * x.y;
        }
    } else {
        cd A[3], B[3], rnm[3];
#pragma unroll
        for (int b = 0; b < 3; ++b) A[b] = B[b] = cd{0.0, 0.0};
        for (int p = gi0; p < gi1; ++p) {                          // B_b = sum_{n' in G(i)} V^a_in' r^b_n'j
            const cd va = M(S.ia, i, p);
            const double ie = 1.0 / (E(p) - em);
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                if (b >= S.nb) continue;
                const cd v = M(sh_get(S.ib, b), p, j);
                B[b] = cadd(B[b], cmul(va, cd{v.y * ie, -v.x * ie}));
            }
        }
        for (int p = gj0; p < gj1; ++p) {                          // A_c = sum_{m' in G(j)} V^a_jm' r^c_m'i
            const cd va = M(S.ia, j, p);
            const double ie = 1.0 / (E(p) - en);
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                if (b >= S.nb) continue;
                const cd v = M(sh_get(S.ib, b), p, i);
                A[b] = cadd(A[b], cmul(va, cd{v.y * ie, -v.x * ie}));
            }
        }
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            if (b >= S.nb) continue;
            const cd v = M(sh_get(S.ib, b), i, j), u = M(sh_get(S.ib, b), j, i);
            rnm[b] = cd{v.y * inv, -v.x * inv};                    // r^b_ij = -i V^b_ij / E_ij
            rmn[b] = cd{-u.y * inv, u.x * inv};
        }
        for (int f = 0; f < S.nfld; ++f) {
            const int b = sh_get(S.f1, f), c = sh_get(S.f2, f);
            const cd y = csub(cmul(sh_pick(A, c), sh_pick(rnm, b)), cmul(sh_pick(rmn, c), sh_pick(B, b)));
            r[1 + 2 * f] = wgt * y.x;
            r[2 + 2 * f] = wgt * y.y;
        }
    }
}

// ---------------------------------------------------------------- pair stage, 1 .. 32 states
// P points per workgroup; per point U and nops + 1 matrices in LDS (pair_lds_ops), as k_opt_pairs.  One lane per (point, pair) then
// walks p once.
static inline int sh_lds_points(int n, int nops) { return std::max(1, std::min(64, SH_LDS_CD / ((nops + 2) * n * n))); }
template <int KIND>
__global__ __launch_bounds__(256) void k_sh_pairs(const ModelView mv, const double* __restrict__ k, const cd* __restrict__ evec,
                                                  const double* __restrict__ eval, const int64_t nk, const ShiftPass S, const int P,
                                                  const double mu, const double kT, const int* __restrict__ occ,
                                                  double* __restrict__ rec) {
    extern __shared__ cd L[];
    const int n = mv.nsta, nn = n * n;
    const int64_t ik0 = (int64_t)blockIdx.x * P;
    const int np = (int)std::min<int64_t>(P, nk - ik0);
    pair_lds_ops(mv, k, evec, nk, ik0, np, P, S, L);
    const cd* Bf = L + P * nn;                                     // buffer j at Bf + j P nn
    const int npair = n * (n - 1) / 2, R = 1 + S.nf();
    for (int e = threadIdx.x; e < np * npair; e += 256) {
        const int p = e / npair, q = e - p * npair;
        int i, j;
        opt_pair_of(n, q, i, j);
        const int64_t ik = ik0 + p;
        const double* ev = eval + ik;
        int gi0, gi1, gj0, gj1;
        band_group(eval, nk, ik, n, i, gi0, gi1);
        band_group(eval, nk, ik, n, j, gj0, gj1);
        const double wgt = sh_weight(ev[(int64_t)i * nk], ev[(int64_t)j * nk], mu, kT, occ, i, j);
        const cd* V = Bf + p * nn;
        sh_record<KIND>(
            rec + (ik * npair + q) * R, S, n, i, j, gi0, gi1, gj0, gj1, wgt,
            [&](const int op, const int row, const int col) __attribute__((always_inline)) { return V[op * P * nn + row * n + col]; },
            [&](const int b) __attribute__((always_inline)) { return ev[(int64_t)b * nk]; });
    }
}

// ---------------------------------------------------------------- pair stage, 33 .. 2048 states (behind tbk_pairs.h's k_pair_wsp, k_opt_vprod)
// one lane per (point, pair): the records from vt[ik][op][n][n] (k_opt_vprod's).  Neighbouring lanes hold neighbouring columns j, so
// the walk down column j is coalesced and row i is shared by most of a wavefront.
template <int KIND>
__global__ __launch_bounds__(256) void k_sh_pairs_wide(const double* __restrict__ eval, const cd* __restrict__ vt, const int64_t nk,
                                                       const int n, const ShiftPass S, const double mu, const double kT,
                                                       const int* __restrict__ occ, double* __restrict__ rec) {
    const int64_t npair = (int64_t)n * (n - 1) / 2, nn = (int64_t)n * n;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nk * npair) return;
    const int64_t ik = idx / npair, q = idx - ik * npair;
    int i, j;
    opt_pair_of(n, q, i, j);
    const double* ev = eval + ik;
    int gi0, gi1, gj0, gj1;
    band_group(eval, nk, ik, n, i, gi0, gi1);
    band_group(eval, nk, ik, n, j, gj0, gj1);
    const double wgt = sh_weight(ev[(int64_t)i * nk], ev[(int64_t)j * nk], mu, kT, occ, i, j);
    const cd* V = vt + ik * S.nops() * nn;
    sh_record<KIND>(
        rec + idx * (1 + S.nf()), S, n, i, j, gi0, gi1, gj0, gj1, wgt,
        [&](const int op, const int row, const int col) __attribute__((always_inline)) { return V[op * nn + (int64_t)row * n + col]; },
        [&](const int b) __attribute__((always_inline)) { return ev[(int64_t)b * nk]; });
}

// ---------------------------------------------------------------- frequency stage
// The policy of tbk_pairs.h's k_pair_omega for the one sum that is needed: of records (eps, fields...) of R doubles, eps < 0 adding
// nothing, the NF fields f0 .. f0 + NF - 1; per lane and frequency
//   y_f = sum field_f [1 / ((eps - w)^2 + eta^2) + 1 / ((eps + w)^2 + eta^2)]
// goes to part[g][(row0 + f) nw + w].  A pass with more than 6 fields takes several launches.
template <int NF>
struct ShOmega {
    static constexpr int NV = 1 + NF, NQ = NF;
    int R, f0;
    __device__ __forceinline__ int rlen() const { return R; }
    __device__ __forceinline__ bool load(const double* __restrict__ p, double (&v)[NV]) const {
        v[0] = p[0];
#pragma unroll
        for (int f = 0; f < NF; ++f) v[1 + f] = p[1 + f0 + f];
        return !(v[0] < 0.0);                                      // a pair that adds nothing
    }
    __device__ __forceinline__ void add(const double (&v)[NV], const double om, const double eta2, double (&s)[NQ]) const {
        const double xp = v[0] - om, xm = -v[0] - om;
        const double d = opt_rcp(fma(xp, xp, eta2)) + opt_rcp(fma(xm, xm, eta2));
#pragma unroll
        for (int f = 0; f < NF; ++f) s[f] = fma(v[1 + f], d, s[f]);
    }
};

// out[first + ik] = the sum of the one-field records of point ik in pair order (the k-list call)
__global__ __launch_bounds__(256) void k_sh_list_sum(const double* __restrict__ rec, const int64_t nk, const int64_t npair,
                                                     const int64_t first, double* __restrict__ out) {
    const int64_t ik = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (ik >= nk) return;
    const double* p = rec + ik * npair * 2;
    double acc = 0.0;
    for (int64_t q = 0; q < npair; ++q) acc += p[2 * q + 1];
    out[first + ik] = acc;
}

// dense d_{d0} d_{d1} H of nk points from the non-empty slots (out zeroed by the caller): the parity hook
__global__ __launch_bounds__(256) void k_sh_ddham(const ModelView mv, const int64_t nk, const double* __restrict__ k, const int d0,
                                                  const int d1, cd* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nk * mv.nnz) return;
    const int64_t ik = idx / mv.nnz;
    const int4 e = mv.nz[(int)(idx - ik * mv.nnz)];
    const int a = e.x & 0xffff, b = e.x >> 16, n = mv.nsta;
    double kk[4];
    cd z[4];
    k_phases(mv, k, ik, kk, z);
    const cd w = ddham_terms(mv, a, b, e.y, e.z, kk, z, d0, d1);
    cd* o = out + ik * (int64_t)n * n;
    o[a * n + b] = w;
    o[b * n + a] = cconj(w);
}

// ---------------------------------------------------------------- host side
// the pass of current direction a with the light directions b[nb] (distinct) and the fields (f1, f2) given as indices into b[]
static ShiftPass sh_pass(int kind, int a, int nb, const int* b) {
    ShiftPass S{};
    S.kind = kind;
    S.a = a;
    S.nb = nb;
    S.ia = -1;
    for (int j = 0; j < nb; ++j) {
        sh_set(S.bdir, j, b[j]);
        sh_set(S.ib, j, S.nv);
        sh_set(S.vdir, S.nv++, b[j]);
        if (b[j] == a) S.ia = sh_get(S.ib, j);
    }
    if (S.ia < 0) {                                                // (nb = 3 spans every direction: a is among them)
        S.ia = S.nv;
        sh_set(S.vdir, S.nv++, a);
    }
    return S;
}
static ShiftPass sh_pass_full(int kind, int a, int dk) {
    const int b[3] = {0, 1, 2};
    ShiftPass S = sh_pass(kind, a, dk, b);
    for (int x = 0; x < dk; ++x)
        for (int y = kind == 0 ? x : 0; y < dk; ++y) sh_set(S.f1, S.nfld, x), sh_set(S.f2, S.nfld, y), ++S.nfld;
    return S;
}
static ShiftPass sh_pass_one(int kind, int a, int b, int c) {
    const int bb[2] = {b, c};
    ShiftPass S = sh_pass(kind, a, b == c ? 1 : 2, bb);
    S.nfld = 1;
    sh_set(S.f1, 0, 0);
    sh_set(S.f2, 0, b == c ? 0 : 1);
    return S;
}

template <int KIND>
static int sh_lds_attr(size_t lds) {
    if (lds > 64 * 1024)
        TBK_HIP(hipFuncSetAttribute((const void*)k_sh_pairs<KIND>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    return TBK_OK;
}

// the pair stage of one pass over a chunk: records of 1 + S.nf() doubles at rec
static int sh_pair_stage(tbk_model* m, const ShiftPass& S, int64_t cnt, const double* kc, const double* ec, const cd* vc, double mu,
                         double kT, const int* occ, cd* wt, cd* vt, double* rec) {
    tbk_ctx* ctx = m->ctx;
    const int n = m->nsta, nops = S.nops();
    const int64_t npair = (int64_t)n * (n - 1) / 2;
    if (n <= 32) {
        const int P = sh_lds_points(n, nops);
        const size_t lds = (size_t)(nops + 2) * P * n * n * sizeof(cd);
        int rc = S.kind == 0 ? sh_lds_attr<0>(lds) : sh_lds_attr<1>(lds);
        if (rc) return rc;
        ProfScope ps(ctx, "shift_pairs");
        const dim3 grid((unsigned)((cnt + P - 1) / P));
        if (S.kind == 0)
            hipLaunchKernelGGL(k_sh_pairs<0>, grid, dim3(256), lds, ctx->stream, m->view, kc, vc, ec, cnt, S, P, mu, kT, occ, rec);
        else
            hipLaunchKernelGGL(k_sh_pairs<1>, grid, dim3(256), lds, ctx->stream, m->view, kc, vc, ec, cnt, S, P, mu, kT, occ, rec);
        TBK_HIP(hipGetLastError());
        return TBK_OK;
    }
    return pair_wide_stage<6>(m, S, cnt, kc, vc, wt, vt, "shift_wide", "shift_pairs", [&] {
        const dim3 grid(nblk(cnt * npair));
        if (S.kind == 0)
            hipLaunchKernelGGL(k_sh_pairs_wide<0>, grid, dim3(256), 0, ctx->stream, ec, (const cd*)vt, cnt, n, S, mu, kT, occ, rec);
        else
            hipLaunchKernelGGL(k_sh_pairs_wide<1>, grid, dim3(256), 0, ctx->stream, ec, (const cd*)vt, cnt, n, S, mu, kT, occ, rec);
    });
}

template <int NF>
static int sh_omega_launch(tbk_ctx* ctx, dim3 grid, const PairSweep& w, int64_t cnt, int R, int f0, int nw, double eta, int accumulate,
                           int row0) {
    return pair_omega_launch(ctx, grid, ShOmega<NF>{R, f0}, w.rec, cnt, w.npair, w.G, w.om, nw, eta, accumulate, w.nrows, row0, w.part);
}

extern "C" int tbk_gen_ddham(tbk_model* m, const double* k, int64_t nk, int dir0, int dir1, double* out) {
    TBK_REQUIRE(m && out && nk >= 0, TBK_EINVAL, "tbk_gen_ddham: bad argument");
    TBK_REQUIRE(m->dim_k >= 1 && dir0 >= 0 && dir0 < m->dim_k && dir1 >= 0 && dir1 < m->dim_k, TBK_EINVAL,
                "tbk_gen_ddham: dirs (%d, %d) outside [0, dim_k=%d)", dir0, dir1, m->dim_k);
    TBK_REQUIRE(k || nk == 0, TBK_EINVAL, "tbk_gen_ddham: null k");
    if (nk == 0) return TBK_OK;
    tbk_ctx* ctx = m->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    const int n = m->nsta;
    const size_t kb = (size_t)nk * m->dim_k * sizeof(double), hb = (size_t)nk * n * n * sizeof(cd);
    void* base = nullptr;
    int rc = tbk_ctx_scratch(ctx, 256 + al256(kb) + al256(hb), &base);
    if (rc) return rc;
    double* k_dev = (double*)((unsigned char*)base + 256);
    cd* h_dev = (cd*)((unsigned char*)k_dev + al256(kb));
    TBK_HIP(hipMemcpyAsync(k_dev, k, kb, hipMemcpyHostToDevice, ctx->stream));
    TBK_HIP(hipMemsetAsync(h_dev, 0, hb, ctx->stream));
    if (m->view.nnz > 0) {
        ProfScope ps(ctx, "gen_ddham");
        hipLaunchKernelGGL(k_sh_ddham, dim3(nblk(nk * m->view.nnz)), dim3(256), 0, ctx->stream, m->view, nk, (const double*)k_dev, dir0,
                           dir1, h_dev);
        TBK_HIP(hipGetLastError());
    }
    TBK_HIP(hipMemcpyAsync(out, h_dev, hb, hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    return TBK_OK;
}

extern "C" int tbk_shift_list(tbk_model* m, const double* k, int64_t nk, int a, int b, int c, const int32_t* occ, int nocc,
                              double* out) {
    TBK_REQUIRE(m && out && occ && nk >= 0 && (k || nk == 0), TBK_EINVAL, "tbk_shift_list: null argument");
    const int dk = m->dim_k, n = m->nsta;
    TBK_REQUIRE(dk >= 1 && dk <= 3, TBK_EINVAL, "tbk_shift_list: dim_k=%d (1, 2 or 3)", dk);
    TBK_REQUIRE(a >= 0 && a < dk && b >= 0 && b < dk && c >= 0 && c < dk, TBK_EINVAL,
                "tbk_shift_list: dirs (%d, %d, %d) must be axes in [0, %d)", a, b, c, dk);
    TBK_REQUIRE(nocc >= 1 && nocc <= n, TBK_EINVAL, "tbk_shift_list: nocc=%d (1..%d)", nocc, n);
    std::vector<int> mask((size_t)n, 0);
    for (int i = 0; i < nocc; ++i) {
        TBK_REQUIRE(occ[i] >= 0 && occ[i] < n, TBK_EINVAL, "tbk_shift_list: occ[%d]=%d outside [0, %d)", i, occ[i], n);
        TBK_REQUIRE(!mask[occ[i]], TBK_EINVAL, "tbk_shift_list: band %d appears twice in occ", occ[i]);
        mask[occ[i]] = 1;
    }
    if (nk == 0) return TBK_OK;
    if (nocc == n) {                       // the complement is empty: nothing to sum
        std::fill(out, out + nk, 0.0);
        return TBK_OK;
    }
    const ShiftPass S = sh_pass_one(0, a, b, c);
    const int64_t npair = (int64_t)n * (n - 1) / 2;
    KuboChunks cw = pair_chunks(n, dk, nk, 2, S.nops());
    tbk_ctx* ctx = m->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    const size_t kb = al256((size_t)nk * dk * sizeof(double)), ob = al256((size_t)nk * sizeof(double)), mb = al256((size_t)n * sizeof(int));
    void* base = nullptr;
    int rc = tbk_ctx_scratch(ctx, 256 + kb + ob + mb + cw.bytes(), &base);
    if (rc) return rc;
    unsigned char* p = (unsigned char*)base + 256;
    double* k_dev = (double*)p;
    double* o_dev = (double*)(p + kb);
    int* occ_dev = (int*)(p + kb + ob);
    cw.base = p + kb + ob + mb;
    TBK_HIP(hipMemcpyAsync(k_dev, k, (size_t)nk * dk * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    TBK_HIP(hipMemcpyAsync(occ_dev, mask.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    double* rec = cw.extra<double>(0);
    rc = kubo_for_chunks(m, cw, k_dev, nullptr, nk, [&](int64_t first, int64_t cnt, const double* kc, const double* ec, const cd* vc) -> int {
        int r2 = sh_pair_stage(m, S, cnt, kc, ec, vc, 0.0, 0.0, occ_dev, cw.extra<cd>(1), cw.extra<cd>(2), rec);
        if (r2) return r2;
        ProfScope ps(ctx, "shift_list_sum");
        hipLaunchKernelGGL(k_sh_list_sum, dim3(nblk(cnt)), dim3(256), 0, ctx->stream, (const double*)rec, cnt, npair, first, o_dev);
        TBK_HIP(hipGetLastError());
        return TBK_OK;
    });
    if (rc) return rc;
    TBK_HIP(hipMemcpyAsync(out, o_dev, (size_t)nk * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    return TBK_OK;
}

extern "C" int tbk_photocurrent_mesh(tbk_model* m, const int32_t* mesh, int kind, int nomega, const double* omega, double eta, double mu,
                                     double kT, int a, int b, int c, double* out) {
    const char* fn = "tbk_photocurrent_mesh";
    TBK_REQUIRE(m && mesh && omega && out, TBK_EINVAL, "%s: null argument", fn);
    const int dk = m->dim_k;
    TBK_REQUIRE(kind == 0 || kind == 1, TBK_EINVAL, "%s: kind=%d (0 shift, 1 injection)", fn, kind);
    int64_t npts;
    int rc = pair_sweep_check(fn, m, mesh, nomega, omega, eta, mu, kT, npts);
    if (rc) return rc;
    const bool full = a == -1 && b == -1 && c == -1;
    TBK_REQUIRE(full || (a >= 0 && a < dk && b >= 0 && b < dk && c >= 0 && c < dk), TBK_EINVAL,
                "%s: dirs (%d, %d, %d) must be axes in [0, %d), or all -1 for the full tensor", fn, a, b, c, dk);
    const int n = m->nsta, cplx = kind == 1 ? 2 : 1;
    const int64_t nout = (full ? (int64_t)nomega * dk * dk * dk : (int64_t)nomega) * cplx;   // doubles
    std::fill(out, out + nout, 0.0);
    if (n < 2) return TBK_OK;                                      // no pair
    ShiftPass pass[3];
    int npass = 0, row0[4] = {0, 0, 0, 0}, rmax = 0;
    if (full)
        for (int d = 0; d < dk; ++d) pass[npass++] = sh_pass_full(kind, d, dk);
    else
        pass[npass++] = sh_pass_one(kind, a, b, c);
    for (int s = 0; s < npass; ++s) {
        row0[s + 1] = row0[s] + pass[s].nf();
        rmax = std::max(rmax, 1 + pass[s].nf());
    }
    const int nft = row0[npass], nopmax = pass[0].nops();          // (every pass of a call has as many operators)
    tbk_ctx* ctx = m->ctx;
    std::vector<double> sums;
    rc = pair_sweep(m, mesh, npts, nomega, omega, rmax, (int64_t)nft * nomega, nopmax, "shift_rows", sums,
                    [&](const PairSweep& w, int64_t first, int64_t cnt, const double* kc, const double* ec, const cd* vc) -> int {
        const dim3 grid(w.ntile, (unsigned)w.G);
        const int acc = first > 0 ? 1 : 0;
        for (int s = 0; s < npass; ++s) {
            const ShiftPass& S = pass[s];
            int r2 = sh_pair_stage(m, S, cnt, kc, ec, vc, mu, kT, nullptr, w.wt, w.vt, w.rec);
            if (r2) return r2;
            ProfScope ps(ctx, "shift_omega");
            const int nf = S.nf(), R = 1 + nf;
            for (int f0 = 0; f0 < nf;) {
                const int left = nf - f0, wd = left >= 6 ? 6 : (left >= 3 ? 3 : (left >= 2 ? 2 : 1));
                auto go = wd == 6 ? sh_omega_launch<6> : (wd == 3 ? sh_omega_launch<3> : (wd == 2 ? sh_omega_launch<2> : sh_omega_launch<1>));
                r2 = go(ctx, grid, w, cnt, R, f0, nomega, eta, acc, row0[s] + f0);
                if (r2) return r2;
                f0 += wd;
            }
        }
        return TBK_OK;
    });
    if (rc) return rc;
    const double pref = eta / M_PI;
    for (int w = 0; w < nomega; ++w)
        for (int s = 0; s < npass; ++s) {
            const ShiftPass& S = pass[s];
            for (int f = 0; f < S.nfld; ++f) {
                const int x = sh_get(S.bdir, sh_get(S.f1, f)), y = sh_get(S.bdir, sh_get(S.f2, f));
                if (kind == 0) {
                    const double v = pref * sums[(size_t)(row0[s] + f) * nomega + w];
                    if (!full) {
                        out[w] = v;
                        continue;
                    }
                    double* o = out + (size_t)w * dk * dk * dk + (size_t)S.a * dk * dk;
                    o[x * dk + y] = v;
                    o[y * dk + x] = v;
                } else {
                    const double re = pref * sums[(size_t)(row0[s] + 2 * f) * nomega + w];
                    const double im = pref * sums[(size_t)(row0[s] + 2 * f + 1) * nomega + w];
                    double* o = full ? out + 2 * ((size_t)w * dk * dk * dk + (size_t)S.a * dk * dk + x * dk + y) : out + 2 * (size_t)w;
                    o[0] = re;
                    o[1] = im;
                }
            }
        }
    return TBK_OK;
}
