// tbk_optics.hip -- interband optical conductivity on uniform meshes by the Kubo formula.
//
// k in reduced coordinates, H the convention-II matrix of tbk_gen_ham, V^d = d_d H (tbk_gen_dham), E_n and |n> the eigenpairs of
// the solver, f_n = [E_n <= mu] (kT = 0) or 1 / (1 + exp((E_n - mu) / kT)):
//   S_ab(w) = (i / N_k) sum_k sum_{n != m} [(f_m - f_n) / (E_m - E_n)] V^a_nm V^b_mn / (E_m - E_n - w - i eta)
// pairs with |E_m - E_n| <= 1e-9 max(1, |E_n|, |E_m|) left out (the rule of tbk_curv.hip: interband only).
// Per unordered pair n < m, eps = E_m - E_n >= 0, c = (f_m - f_n) / eps and P_ab = V^a_nm V^b_mn (P_ba = conj P_ab):
//   S_ab += i c Re(P_ab) G+ - c Im(P_ab) G-,   g+- = 1 / (+-eps - w - i eta),  G+ = g+ + g-,  G- = g+ - g-
// so a pair is a RECORD of 1 + ns + na doubles: eps (-1: the pair adds nothing), the symmetric weights A = c Re P_ab (a <= b) and
// the antisymmetric ones B = c Im P_ab (a < b) of the components asked for.
//
// Pipeline, in chunks of a fixed number of points (tbk_pairs.h's sweep driver on tbk_kubo.h's chunk pipeline: kKuboChunkBytes of
// eigenvectors, kPairRecBytes of records): the device k generator, the eigen-solver with vectors, then the PAIR stage writes the
// chunk's records at a fixed stride of n (n - 1) / 2 per point
//   n <= 32    k_opt_pairs: U, d_d H for every direction asked for, and V^d = conj(U) d_d H U^T of several points in LDS
//   n > 32     k_pair_wsp (W^d = d_d H U^T from the sparse slots), k_opt_vprod (V^d = conj(U) W^d, LDS tiles), k_opt_pairs_wide
// and the FREQUENCY stage (k_pair_omega over OptOmega: two frequencies per lane, the records read as wave-uniform values) adds each
// k-group's sums into part[G][row]; k_group_rows sums the G groups in a fixed order.  Every partition depends on the mesh, n, dim_k, n_omega and the
// components alone, and nothing uses atomics: two calls give the same bits on any machine.
// This unit holds the components (OptFields), the record writer and the frequency policy; the pair stage around the record writer, the
// frequency walk and the sweep driver live in tbk_pairs.h, which tbk_shift.hip shares.
#include <math.h>
#include <string.h>
#include "tbk_pairs.h"

#define OPT_LDS_CD 5120                                  // c128 of LDS per workgroup of k_opt_pairs at most (80 KiB)

// The components of one call: the velocity matrices of nd directions dir[] are formed; record field f < ns is A of the direction
// pair (dir[fa[f]], dir[fb[f]]), field ns + f is B of (dir[fa[ns + f]], dir[fb[ns + f]]).  As the SLOTS of tbk_pairs.h: operator d
// is d_{dir[d]} H.
struct OptFields {
    int nd;
    int dir[3];
    int ns, na;
    int fa[9], fb[9];
    __host__ __device__ int nops() const { return nd; }
    __device__ __forceinline__ cd one(const ModelView& mv, const int d, const int4 z4, const double (&kk)[4], const cd (&z)[4]) const {
        cd h, v0, v1;
        dham_terms(mv, z4.x & 0xffff, z4.x >> 16, z4.y, z4.z, kk, z, dir[d], dir[d], h, v0, v1);
        return v0;
    }
    __device__ __forceinline__ void all(const ModelView& mv, const int4 z4, const double (&kk)[4], const cd (&z)[4],
                                        cd (&sv)[3][256]) const {
        for (int d = 0; d < nd; d += 2) {                          // dham_terms gives two directions per walk
            cd h, v0, v1;
            const int d1 = d + 1 < nd ? d + 1 : d;
            dham_terms(mv, z4.x & 0xffff, z4.x >> 16, z4.y, z4.z, kk, z, dir[d], dir[d1], h, v0, v1);
            sv[d][threadIdx.x] = v0;
            if (d + 1 < nd) sv[d + 1][threadIdx.x] = v1;
        }
    }
};

// one record at r: vel(d, 0) = V^{dir[d]}_nm, vel(d, 1) = V^{dir[d]}_mn
template <class Vel>
__device__ __forceinline__ void opt_record(double* __restrict__ r, const OptFields& F, const double en, const double em, const double mu,
                                           const double kT, const Vel& vel) {
    const double eps = em - en;
    const double c = kubo_degenerate(eps, en, em) ? 0.0 : opt_weight(en, em, eps, mu, kT);
    const int nf = F.ns + F.na;
    if (c == 0.0) {
        r[0] = -1.0;
        for (int f = 0; f < nf; ++f) r[1 + f] = 0.0;
        return;
    }
    r[0] = eps;
    for (int f = 0; f < nf; ++f) {
        const cd p = cmul(vel(F.fa[f], 0), vel(F.fb[f], 1));   // V^a_nm V^b_mn
        r[1 + f] = c * (f < F.ns ? p.x : p.y);
    }
}

// ---------------------------------------------------------------- pair stage, 1 .. 32 states
// P points per workgroup; per point U and nd + 1 matrices in LDS (pair_lds_ops): buffers 0 .. nd - 1 end up holding V^0 .. V^{nd-1}.
// One lane per (point, pair) then writes the records.
static inline int opt_lds_points(int n, int nd) { return std::max(1, std::min(64, OPT_LDS_CD / ((nd + 2) * n * n))); }
__global__ __launch_bounds__(256) void k_opt_pairs(const ModelView mv, const double* __restrict__ k, const cd* __restrict__ evec,
                                                   const double* __restrict__ eval, const int64_t nk, const OptFields F, const int P,
                                                   const double mu, const double kT, double* __restrict__ rec) {
    extern __shared__ cd L[];
    const int n = mv.nsta, nn = n * n;
    const int64_t ik0 = (int64_t)blockIdx.x * P;
    const int np = (int)std::min<int64_t>(P, nk - ik0);
    pair_lds_ops(mv, k, evec, nk, ik0, np, P, F, L);
    const cd* Bf = L + P * nn;                                     // buffer j at Bf + j P nn
    const int npair = n * (n - 1) / 2, R = 1 + F.ns + F.na;
    for (int e = threadIdx.x; e < np * npair; e += 256) {
        const int p = e / npair, q = e - p * npair;
        int i, j;
        opt_pair_of(n, q, i, j);
        const int64_t ik = ik0 + p;
        const double ei = eval[(int64_t)i * nk + ik], ej = eval[(int64_t)j * nk + ik];
        const bool sw = ej < ei;                                   // (n, m) of the formula: E_m >= E_n
        const int a = sw ? j : i, b = sw ? i : j;
        const cd* V = Bf + p * nn;
        opt_record(rec + (ik * npair + q) * R, F, sw ? ej : ei, sw ? ei : ej, mu, kT, [&](const int d, const int mn) {
            return mn ? V[d * P * nn + b * n + a] : V[d * P * nn + a * n + b];
        });
    }
}

// ---------------------------------------------------------------- pair stage, 33 .. 2048 states (behind tbk_pairs.h's k_pair_wsp, k_opt_vprod)
// one lane per (point, pair): the records from vt
__global__ __launch_bounds__(256) void k_opt_pairs_wide(const double* __restrict__ eval, const cd* __restrict__ vt, const int64_t nk,
                                                        const int n, const OptFields F, const double mu, const double kT,
                                                        double* __restrict__ rec) {
    const int64_t npair = (int64_t)n * (n - 1) / 2, nn = (int64_t)n * n;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nk * npair) return;
    const int64_t ik = idx / npair, q = idx - ik * npair;
    int i, j;
    opt_pair_of(n, q, i, j);
    const double ei = eval[(int64_t)i * nk + ik], ej = eval[(int64_t)j * nk + ik];
    const bool sw = ej < ei;
    const int a = sw ? j : i, b = sw ? i : j;
    const cd* V = vt + ik * F.nd * nn;
    opt_record(rec + idx * (1 + F.ns + F.na), F, sw ? ej : ei, sw ? ei : ej, mu, kT, [&](const int d, const int mn) {
        return mn ? V[d * nn + (int64_t)b * n + a] : V[d * nn + (int64_t)a * n + b];
    });
}

// ---------------------------------------------------------------- frequency stage
// The policy of tbk_pairs.h's k_pair_omega: a record is (eps, NS fields A, NA fields B), eps < 0 adds nothing.  Per lane and frequency
//   x_f = sum A_f G+.x (f < NS) or B_f G-.x,   y_f = sum A_f (r+ + r-) or B_f (r+ - r-)     (G+-.y = eta (r+ +- r-))
// are sums 2 f and 2 f + 1: part[g][row], row = (2 f + {0: x, 1: y}) nw + w.
template <int NS, int NA>
struct OptOmega {
    static constexpr int NF = NS + NA, NV = 1 + NF, NQ = 2 * NF;
    __device__ __forceinline__ int rlen() const { return NV; }
    __device__ __forceinline__ bool load(const double* __restrict__ p, double (&v)[NV]) const {
#pragma unroll
        for (int f = 0; f < NV; ++f) v[f] = p[f];
        return !(v[0] < 0.0);                                      // c = 0 or a degenerate pair
    }
    __device__ __forceinline__ void add(const double (&v)[NV], const double om, const double eta2, double (&s)[NQ]) const {
        const double xp = v[0] - om, xm = -v[0] - om;
        const double rp = opt_rcp(fma(xp, xp, eta2)), rm = opt_rcp(fma(xm, xm, eta2));
        const double gp = xp * rp, gm = xm * rm;
        const double Gpx = gp + gm, Gmx = gp - gm, Gpy = rp + rm, Gmy = rp - rm;
#pragma unroll
        for (int f = 0; f < NS; ++f) {
            s[2 * f] = fma(v[1 + f], Gpx, s[2 * f]);
            s[2 * f + 1] = fma(v[1 + f], Gpy, s[2 * f + 1]);
        }
#pragma unroll
        for (int f = NS; f < NF; ++f) {
            s[2 * f] = fma(v[1 + f], Gmx, s[2 * f]);
            s[2 * f + 1] = fma(v[1 + f], Gmy, s[2 * f + 1]);
        }
    }
};

// ---------------------------------------------------------------- host side
template <int NS, int NA>
static int opt_omega_launch(tbk_ctx* ctx, dim3 grid, const PairSweep& w, int64_t cnt, int nw, double eta, int accumulate) {
    return pair_omega_launch(ctx, grid, OptOmega<NS, NA>{}, w.rec, cnt, w.npair, w.G, w.om, nw, eta, accumulate, w.nrows, 0, w.part);
}

extern "C" int tbk_optical_cond_mesh(tbk_model* m, const int32_t* mesh, int nomega, const double* omega, double eta, double mu,
                                     double kT, int dir0, int dir1, double* out) {
    const char* fn = "tbk_optical_cond_mesh";
    TBK_REQUIRE(m && mesh && omega && out, TBK_EINVAL, "%s: null argument", fn);
    const int dk = m->dim_k;
    int64_t npts;
    int rc = pair_sweep_check(fn, m, mesh, nomega, omega, eta, mu, kT, npts);
    if (rc) return rc;
    const bool full = dir0 == -1 && dir1 == -1;
    TBK_REQUIRE(full || (dir0 >= 0 && dir0 < dk && dir1 >= 0 && dir1 < dk), TBK_EINVAL,
                "%s: dirs (%d, %d) must be axes in [0, %d), or both -1 for the full tensor", fn, dir0, dir1, dk);
    const int n = m->nsta;
    const int64_t nout = full ? (int64_t)nomega * dk * dk : (int64_t)nomega;   // complex values
    if (n < 2) {                                                   // no pair
        std::fill(out, out + 2 * nout, 0.0);
        return TBK_OK;
    }
    // the components: full tensor -> A of every a <= b, B of every a < b; one component -> A (and B when a != b)
    OptFields F{};
    if (full) {
        F.nd = dk;
        for (int d = 0; d < dk; ++d) F.dir[d] = d;
        for (int a = 0; a < dk; ++a)
            for (int b = a; b < dk; ++b) F.fa[F.ns] = a, F.fb[F.ns] = b, ++F.ns;
        for (int a = 0; a < dk; ++a)
            for (int b = a + 1; b < dk; ++b) F.fa[F.ns + F.na] = a, F.fb[F.ns + F.na] = b, ++F.na;
    } else if (dir0 == dir1) {
        F.nd = 1;
        F.dir[0] = dir0;
        F.ns = 1;
        F.fa[0] = F.fb[0] = 0;
    } else {
        F.nd = 2;
        F.dir[0] = dir0;
        F.dir[1] = dir1;
        F.ns = F.na = 1;
        F.fa[0] = F.fa[1] = 0;
        F.fb[0] = F.fb[1] = 1;
    }
    const int nf = F.ns + F.na;
    tbk_ctx* ctx = m->ctx;
    const int P = opt_lds_points(n, F.nd);
    const size_t lds = (size_t)(F.nd + 2) * P * n * n * sizeof(cd);
    if (n <= 32 && lds > 64 * 1024) {
        TBK_HIP(hipSetDevice(ctx->device));
        TBK_HIP(hipFuncSetAttribute((const void*)k_opt_pairs, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    }
    std::vector<double> sums;
    rc = pair_sweep(m, mesh, npts, nomega, omega, 1 + nf, 2 * (int64_t)nf * nomega, F.nd, "opt_rows", sums,
                    [&](const PairSweep& w, int64_t first, int64_t cnt, const double* kc, const double* ec, const cd* vc) -> int {
        if (n <= 32) {
            ProfScope ps(ctx, "opt_pairs");
            hipLaunchKernelGGL(k_opt_pairs, dim3((unsigned)((cnt + P - 1) / P)), dim3(256), lds, ctx->stream, m->view,
                               kc, vc, ec, cnt, F, P, mu, kT, w.rec);
            TBK_HIP(hipGetLastError());
        } else {
            int r2 = pair_wide_stage<3>(m, F, cnt, kc, vc, w.wt, w.vt, "opt_wide", "opt_pairs", [&] {
                hipLaunchKernelGGL(k_opt_pairs_wide, dim3(nblk(cnt * w.npair)), dim3(256), 0, ctx->stream, ec, (const cd*)w.vt, cnt, n, F,
                                   mu, kT, w.rec);
            });
            if (r2) return r2;
        }
        ProfScope ps(ctx, "opt_omega");
        const dim3 grid(w.ntile, (unsigned)w.G);
        const int acc = first > 0 ? 1 : 0;
        if (F.ns == 1 && F.na == 0) return opt_omega_launch<1, 0>(ctx, grid, w, cnt, nomega, eta, acc);
        if (F.ns == 1 && F.na == 1) return opt_omega_launch<1, 1>(ctx, grid, w, cnt, nomega, eta, acc);
        if (F.ns == 3) return opt_omega_launch<3, 1>(ctx, grid, w, cnt, nomega, eta, acc);
        return opt_omega_launch<6, 3>(ctx, grid, w, cnt, nomega, eta, acc);
    });
    if (rc) return rc;
    // S_ab = i SA - SB, S_ba = i SA + SB with SA = (x_A, eta y_A), SB = (x_B, eta y_B) of the pair (a, b), a < b; S_aa = i SA
    auto X = [&](int f, int w) { return sums[(size_t)(2 * f) * nomega + w]; };
    auto Y = [&](int f, int w) { return eta * sums[(size_t)(2 * f + 1) * nomega + w]; };
    auto B_of = [&](int a, int b) {   // the B field of (a, b), a < b, or -1
        for (int f = F.ns; f < nf; ++f)
            if (F.fa[f] == a && F.fb[f] == b) return f;
        return -1;
    };
    for (int w = 0; w < nomega; ++w) {
        for (int f = 0; f < F.ns; ++f) {
            const int a = F.fa[f], b = F.fb[f];
            const int fb = a == b ? -1 : B_of(a, b);
            const double bx = fb >= 0 ? X(fb, w) : 0.0, by = fb >= 0 ? Y(fb, w) : 0.0;
            const double re = -Y(f, w), im = X(f, w);
            if (!full) {
                out[2 * w] = re - bx;
                out[2 * w + 1] = im - by;
                continue;
            }
            double* o = out + (size_t)w * 2 * dk * dk;
            o[2 * (a * dk + b)] = re - bx;
            o[2 * (a * dk + b) + 1] = im - by;
            if (a != b) {
                o[2 * (b * dk + a)] = re + bx;
                o[2 * (b * dk + a) + 1] = im + by;
            }
        }
    }
    return TBK_OK;
}
