// tbk_orbmag.hip -- orbital moments and orbital magnetization by the Kubo formula on k lists and uniform meshes (DESIGN.md
// section 13).
//
// k reduced, H the convention-II matrix of tbk_gen_ham, V^d = d_d H (tbk_gen_dham), E_n and |n> the eigenpairs of the solver,
// (a, b) = (dir0, dir1), P_nm = Im V^a_nm V^b_mn, Delta_nm = E_n - E_m:
//   moment (1)       m_n = sum_{m != n} P_nm / (E_m - E_n), beside Omega_n = -2 sum_{m != n} P_nm / Delta^2 (tbk_curv.hip); a pair with
//                    |Delta| <= 1e-9 max(1, |E_n|, |E_m|) contributes to neither
//   band set (2)     over n in occ, m not in occ (no degeneracy rule): LC = sum P_nm E_m / Delta^2, IC = sum P_nm E_n / Delta^2,
//                    Omega_occ = -2 sum P_nm / Delta^2
//   T = 0 scan (3)   M(mu) = mean_k sum_{E_n <= mu} [m_n + (mu - E_n) Omega_n] = A(mu) + mu I(mu), A the same sum of m_n - E_n Omega_n
//   kT > 0 (4)       M(mu, T) = mean_k sum_n [f_n m_n + g_n Omega_n], f = 1 / (1 + e^x), g = kT ln(1 + e^-x), x = (E_n - mu) / kT
//
// Forms, routed as in tbk_curv.hip:
//   n = 2     one lane per k from curv2_point (no eigen-solve): m_0 = m_1 = (E_0 - E_1) Omega_0 / 2.  On a mesh the lane feeds the
//             plane and T = 0 reductions directly; for kT > 0 it writes the (E, m, Omega) records.
//   n != 2    the chunk pipeline and the contraction kernels of tbk_kubo.h with the policy OrbQ: two accumulators per (point, band)
//             lane, three shares for a band set.
// Reductions, all of tbk_kubo.h: k_kubo_plane with three quantities (the band-set sums in one pass), k_kubo_fermi with two per item,
// k_kubo_thermal with the policy OrbThermal (levels across lanes, records read as wave-uniform values, sums in registers),
// k_kubo_rows.  This unit owns the sources, OrbThermal's arithmetic and OrbQ.  Every partition depends on the mesh, n and the
// number of levels alone, and nothing uses atomics: two calls give the same bits.
#include <math.h>
#include <string.h>
#include "tbk_kubo.h"

// ---------------------------------------------------------------- n = 2: closed form in registers
// list form: out[2][nk] = m (occ_sign == 0), or out[nk] = LC + IC of the band set {0} (occ_sign = +1) or {1} (-1)
__global__ __launch_bounds__(256) void k_orb2_list(const ModelView mv, const int64_t nk, const double* __restrict__ k, const int d0,
                                                   const int d1, const int occ_sign, double* __restrict__ out) {
    const int64_t ik = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (ik >= nk) return;
    double kk[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) kk[d] = d < mv.dim_k ? k[ik * mv.dim_k + d] : 0.0;
    const Curv2 c = curv2_point(mv, kk, d0, d1);
    if (occ_sign == 0) {
        const double w = c.degenerate ? 0.0 : 0.5 * (c.e0 - c.e1) * c.om;
        out[ik] = w;
        out[nk + ik] = w;
    } else {
        out[ik] = -0.5 * (c.e0 + c.e1) * (occ_sign > 0 ? c.om : -c.om);   // P / Delta^2 = -Omega_occ / 2, times E_0 + E_1
    }
}

// Sources of per-point values for the reductions.  band(): w = (Omega_ch (degeneracy rule), m_ch - E_ch Omega_ch) and E_ch
// (k_kubo_fermi); plane(): (LC, IC, Omega_occ) of the band set (k_kubo_plane; each sum in the order of the curvature's plane
// sums, and the Omega sum is its manifold sum, bit for bit).
struct Orb2Src : Kubo2Src {
    __device__ __forceinline__ void band(const PlaneArgs& P, const int (&ii)[3], int64_t, const int ch, double& e, double (&w)[2]) const {
        const Curv2 c = at(P, ii);
        e = ch ? c.e1 : c.e0;
        const double o = c.degenerate ? 0.0 : c.om;
        w[0] = ch ? -o : o;
        w[1] = -0.5 * (c.e0 + c.e1) * w[0];   // sum_m P_nm (E_n + E_m) / Delta^2
    }
    __device__ __forceinline__ void plane(const PlaneArgs& P, const int s, const int64_t p, int, double (&w)[3]) const {
        int ii[3];
        plane_point(P, s, p, ii);
        const Curv2 c = at(P, ii);
        w[2] = occ_sign > 0 ? c.om : -c.om;   // the manifold value of tbk_curv.hip, bit for bit
        const double h = -0.5 * w[2];
        w[0] = h * (occ_sign > 0 ? c.e1 : c.e0);
        w[1] = h * (occ_sign > 0 ? c.e0 : c.e1);
    }
};
struct OrbArraySrc {
    const double* ev;   // [n][npts] (per band)
    const double* mm;
    const double* om;
    const double* st;   // [3][npts] (band set)
    __device__ __forceinline__ void band(const PlaneArgs& P, const int (&)[3], const int64_t idx, const int ch, double& e,
                                         double (&w)[2]) const {
        const int64_t i = (int64_t)ch * P.npts + idx;
        e = ev[i];
        w[0] = om[i];
        w[1] = mm[i] - e * w[0];
    }
    __device__ __forceinline__ void plane(const PlaneArgs& P, const int s, const int64_t p, int, double (&w)[3]) const {
        int ii[3];
        const int64_t idx = plane_point(P, s, p, ii);
        w[0] = st[idx];
        w[1] = st[P.npts + idx];
        w[2] = st[2 * P.npts + idx];
    }
};

// n = 2 records for kT > 0: ev, mm, om [2][npts] of every mesh point (degenerate pairs: m = Omega = 0)
__global__ __launch_bounds__(256) void k_orb2_records(const ModelView mv, const PlaneArgs P, const int d0, const int d1,
                                                      double* __restrict__ ev, double* __restrict__ mm, double* __restrict__ om) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= P.npts) return;
    int ii[3];
    mesh_point(P.N, idx, ii);
    const Curv2 c = Kubo2Src{mv, d0, d1, 0}.at(P, ii);
    const double w = c.degenerate ? 0.0 : c.om;
    const double m = c.degenerate ? 0.0 : 0.5 * (c.e0 - c.e1) * c.om;
    ev[idx] = c.e0;
    ev[P.npts + idx] = c.e1;
    mm[idx] = m;
    mm[P.npts + idx] = m;
    om[idx] = w;
    om[P.npts + idx] = -w;
}

// ---------------------------------------------------------------- reductions
// kT > 0 (k_kubo_thermal): the records (m, Omega) beside E.  Per (record, level) one exp, one log1p and one division:
// t = e^{-|x|},  f = 1 / (1 + t) (x < 0) or t / (1 + t) (tbk_kubo.h's fermi_terms),  g = kT log1p(t) (x >= 0) or mu - E + kT log1p(t)
struct OrbThermal {
    static constexpr int NR = 2, NQ = 1;
    static constexpr bool kWhole = false;
    static __device__ __forceinline__ void add(const double e, const double (&rc)[2], const double u, const double kT, const double ikT,
                                               double (&acc)[1]) {
        const double m = rc[0], o = rc[1];
        const FermiTerms ft = fermi_terms((e - u) * ikT);
        const double l = kT * log1p(ft.t);
        const double gg = ft.x >= 0.0 ? l : (u - e) + l;
        acc[0] = fma(ft.f(), m, fma(gg, o, acc[0]));
    }
};

// ---------------------------------------------------------------- n != 2: what a (point, band) lane of tbk_kubo.h's contraction keeps
// Omega's and m's weights of the same P_nm (per band: mm[b], om[b] and ev[b] at [nfull] stride, om and ev nullable) or the band's
// shares of LC, IC and Omega_occ, summed per point into st[c][nfull] (c = LC, IC, Omega; Omega_occ as CurvQ forms it, bit for bit).
struct OrbQ {
    static constexpr int NSET = 3;
    static constexpr const char* kLabel[4] = {"orb_lds", "orb_wsp", "orb_contract", "orb_occ_sum"};
    struct Out {
        double *mm, *om, *ev, *st;
    };
    double acc = 0.0, acm = 0.0;                                   // sum P / Delta^2; sum P / (E_m - E_b) or sum P E_m / Delta^2
    __device__ __forceinline__ void pair(const double pr, const double de, const double eb, const double em, const bool set) {
        const double w = pr / (de * de);
        acc += w;
        if (set) acm += w * em;
        else acm += pr / (em - eb);
    }
    __device__ __forceinline__ void band(const Out& o, const int64_t i, const double eb) const {
        o.mm[i] = acm;
        if (o.om) o.om[i] = -2.0 * acc;
        if (o.ev) o.ev[i] = eb;
    }
    __device__ __forceinline__ void share(double* s, const double eb) const {
        s[0] = acm;
        s[1] = eb * acc;
        s[2] = -2.0 * acc;
    }
    static __device__ __forceinline__ void set(const Out& o, const int64_t i, const int64_t nfull, const double (&s)[3]) {
        o.st[i] = s[0];
        o.st[nfull + i] = s[1];
        o.st[2 * nfull + i] = s[2];
    }
};

// ---------------------------------------------------------------- host side
extern "C" int tbk_orb_moment_list(tbk_model* m, const double* k, int64_t nk, int dir0, int dir1, const int32_t* occ, int nocc,
                                   double* out) {
    std::vector<int> mask;
    int rc = kubo_check("tbk_orb_moment_list", "orbital moment", m, dir0, dir1, occ, nocc, mask);
    if (rc) return rc;
    TBK_REQUIRE(nk >= 0 && out && (k || nk == 0), TBK_EINVAL, "tbk_orb_moment_list: bad k list or output");
    const int n = m->nsta, dk = m->dim_k;
    const bool manifold = occ != nullptr;
    const int64_t nout = manifold ? nk : (int64_t)n * nk;
    if (nk == 0) return TBK_OK;
    if (n < 2 || (manifold && nocc == n)) {   // no pair to sum
        std::fill(out, out + nout, 0.0);
        return TBK_OK;
    }
    tbk_ctx* ctx = m->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    const int64_t ndev = manifold && n != 2 ? 3 * nk : nout;   // a band set of the n != 2 path: st[3][nk]
    KuboChunks cw = n == 2 ? KuboChunks() : kubo_contract_chunks(n, dk, nk, manifold, OrbQ::NSET);
    double *k_dev, *o_dev;
    KuboCarve ws;
    ws.add(k_dev, (size_t)nk * dk * sizeof(double)), ws.add(o_dev, (size_t)ndev * sizeof(double)), ws.add(cw.base, cw.bytes());
    rc = kubo_carve(ctx, ws);
    if (rc) return rc;
    TBK_HIP(hipMemcpyAsync(k_dev, k, (size_t)nk * dk * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (n == 2) {
        ProfScope ps(ctx, "orb2_list");
        const int sign = manifold ? (mask[0] ? 1 : -1) : 0;
        hipLaunchKernelGGL(k_orb2_list, dim3(nblk(nk)), dim3(256), 0, ctx->stream, m->view, nk, (const double*)k_dev, dir0, dir1, sign,
                           o_dev);
        TBK_HIP(hipGetLastError());
    } else {
        rc = kubo_contract<OrbQ>(m, k_dev, nullptr, nk, dir0, dir1, mask, cw,
                                 OrbQ::Out{manifold ? nullptr : o_dev, nullptr, nullptr, manifold ? o_dev : nullptr});
        if (rc) return rc;
    }
    if (manifold && n != 2) {                 // LC + IC
        std::vector<double> lcic((size_t)2 * nk);
        TBK_HIP(hipMemcpyAsync(lcic.data(), o_dev, (size_t)2 * nk * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        TBK_HIP(hipStreamSynchronize(ctx->stream));
        for (int64_t i = 0; i < nk; ++i) out[i] = lcic[(size_t)i] + lcic[(size_t)(nk + i)];
        return TBK_OK;
    }
    TBK_HIP(hipMemcpyAsync(out, o_dev, (size_t)nout * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    return TBK_OK;
}

extern "C" int tbk_orb_mag_mesh(tbk_model* m, const int32_t* mesh, int dir0, int dir1, const int32_t* occ, int nocc, int nmu,
                                const double* mu, double kT, double* out) {
    std::vector<int> mask;
    int rc = kubo_check("tbk_orb_mag_mesh", "orbital moment", m, dir0, dir1, occ, nocc, mask);
    if (rc) return rc;
    TBK_REQUIRE(mesh && out, TBK_EINVAL, "tbk_orb_mag_mesh: null argument");
    TBK_REQUIRE(m->dim_k == 2 || m->dim_k == 3, TBK_EINVAL, "tbk_orb_mag_mesh: dim_k=%d (meshes of 2 or 3 dimensions)", m->dim_k);
    rc = kubo_levels_check("tbk_orb_mag_mesh", nmu, mu, 0);
    if (rc) return rc;
    TBK_REQUIRE((nmu > 0) != (occ != nullptr), TBK_EINVAL, "tbk_orb_mag_mesh: give exactly one of a band set and Fermi levels");
    rc = kubo_kt_check("tbk_orb_mag_mesh", kT, false);
    if (rc) return rc;
    TBK_REQUIRE(kT == 0.0 || nmu > 0, TBK_EINVAL, "tbk_orb_mag_mesh: kT > 0 needs Fermi levels");
    rc = kubo_levels_finite("tbk_orb_mag_mesh", nmu, mu);
    if (rc) return rc;
    const int n = m->nsta, dk = m->dim_k;
    PlaneArgs P;
    rc = kubo_planes("tbk_orb_mag_mesh", mesh, dir0, dir1, dk, P);
    if (rc) return rc;
    const int64_t npts = P.npts;
    const int nslice = P.nslice;
    const bool manifold = occ != nullptr, hot = kT > 0.0;
    const int nch = manifold ? 3 : nmu;
    const int64_t nout = (int64_t)nch * nslice;
    if (n < 2 || (manifold && nocc == n)) {   // no pair to sum
        std::fill(out, out + nout, 0.0);
        return TBK_OK;
    }
    tbk_ctx* ctx = m->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    // T = 0: levels sorted on the host (ties by index) for the bins; results come back in input order
    std::vector<int> ord;
    std::vector<double> mus;
    kubo_levels(mu, nmu, !hot, ord, mus);
    // partial layouts and counts: the grid shapes depend on the mesh shape, n and nmu alone
    int gx;
    int64_t nrows;
    if (manifold) {
        gx = kubo_plane_gx(P);
        nrows = (int64_t)nslice * 3;
    } else if (!hot) {
        gx = kubo_fermi_gx(P, n, nmu, 2);
        nrows = (int64_t)nslice * nmu * 2;
    } else {
        gx = kubo_thermal_groups(P, n, nmu, 1);
        nrows = (int64_t)nslice * nmu;
    }
    const bool general = n != 2;
    // per-point arrays: band set st[3][npts] (n != 2); per band rec[3][n][npts] = ev, mm, om (n != 2, or n = 2 with kT > 0)
    const bool recs = (general && !manifold) || hot;
    const size_t recn = (size_t)n * npts;
    KuboChunks cw = general ? kubo_contract_chunks(n, dk, npts, manifold, OrbQ::NSET) : KuboChunks();
    double *part, *rows, *mu_dev, *st_dev, *ev_dev;
    KuboCarve ws;
    ws.add(part, (size_t)nrows * gx * sizeof(double)), ws.add(rows, (size_t)nrows * sizeof(double));
    ws.add(mu_dev, (size_t)std::max(nmu, 1) * sizeof(double));
    ws.add(st_dev, general && manifold ? (size_t)3 * npts * sizeof(double) : 0);
    ws.add(ev_dev, recs ? 3 * recn * sizeof(double) : 0), ws.add(cw.base, cw.bytes());
    rc = kubo_carve(ctx, ws);
    if (rc) return rc;
    double* mm_dev = recs ? ev_dev + recn : nullptr;
    double* om_dev = recs ? ev_dev + 2 * recn : nullptr;
    if (nmu) TBK_HIP(hipMemcpyAsync(mu_dev, mus.data(), (size_t)nmu * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    auto reduce = [&](auto src) -> int {
        if (manifold) {
            ProfScope ps(ctx, n == 2 ? "orb2_plane" : "orb_plane");
            return kubo_plane_launch<3>(ctx, src, P, 1, nslice, gx, part);
        }
        ProfScope ps(ctx, n == 2 ? "orb2_fermi" : "orb_fermi");
        return kubo_fermi_launch<2>(ctx, src, P, n, mu_dev, nmu, gx, part);
    };
    if (general) {
        rc = kubo_contract<OrbQ>(m, nullptr, mesh, npts, dir0, dir1, mask, cw, OrbQ::Out{mm_dev, om_dev, ev_dev, st_dev});
        if (rc) return rc;
    } else if (hot) {
        ProfScope ps(ctx, "orb2_records");
        hipLaunchKernelGGL(k_orb2_records, dim3(nblk(npts)), dim3(256), 0, ctx->stream, m->view, P, dir0, dir1, ev_dev, mm_dev, om_dev);
        TBK_HIP(hipGetLastError());
    }
    if (hot) {
        ProfScope ps(ctx, "orb_kt");
        rc = kubo_thermal_launch<OrbThermal>(ctx, P, n, ev_dev, mu_dev, nmu, kT, gx, part);
    } else if (general) {
        rc = reduce(OrbArraySrc{ev_dev, mm_dev, om_dev, st_dev});
    } else {
        rc = reduce(Orb2Src{{m->view, dir0, dir1, manifold ? (mask[0] ? 1 : -1) : 0}});
    }
    if (rc) return rc;
    std::vector<double> sums;
    rc = kubo_rows_to_host(ctx, "orb_rows", part, gx, nrows, rows, sums);
    if (rc) return rc;
    const double inv = 1.0 / (double)P.nplane;
    // out[ch][s]: the Python shapes (nch,) for a 2-D mesh, (nch, nslice) for a 3-D one
    for (int s = 0; s < nslice; ++s) {
        if (manifold) {
            for (int c = 0; c < 3; ++c) out[(size_t)c * nslice + s] = sums[(size_t)s * 3 + c] * inv;
        } else if (hot) {
            for (int j = 0; j < nmu; ++j) out[(size_t)j * nslice + s] = sums[(size_t)s * nmu + j] * inv;
        } else {
            double ai = 0.0, aa = 0.0;             // I(mu_j), A(mu_j): prefix sums of the bins over the sorted levels
            for (int j = 0; j < nmu; ++j) {
                ai += sums[((size_t)s * nmu + j) * 2];
                aa += sums[((size_t)s * nmu + j) * 2 + 1];
                out[(size_t)ord[j] * nslice + s] = aa * inv + mus[j] * (ai * inv);
            }
        }
    }
    return TBK_OK;
}
