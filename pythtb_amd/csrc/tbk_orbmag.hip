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
// Reductions: k_orb_plane (the three band-set sums in one pass), k_kubo_fermi with two quantities per item, k_orb_kt (levels across
// lanes, records read as wave-uniform values, sums in registers), k_kubo_rows.  Every partition depends on the mesh, n and the
// number of levels alone, and nothing uses atomics: two calls give the same bits.
#include <math.h>
#include <string.h>
#include "tbk_kubo.h"

static const int kOrbKtTile = 256;                       // levels per workgroup of k_orb_kt (one per lane)
static const int kOrbKtGroupsMax = 1024;                 // k-groups of k_orb_kt at most

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

// Sources of per-point values for the reductions.  band(): w = (Omega_ch (degeneracy rule), m_ch - E_ch Omega_ch) and E_ch;
// set(): (LC, IC, Omega_occ) of the band set.
struct Orb2Src : Kubo2Src {
    __device__ __forceinline__ void band(const PlaneArgs& P, const int (&ii)[3], int64_t, const int ch, double& e, double (&w)[2]) const {
        const Curv2 c = at(P, ii);
        e = ch ? c.e1 : c.e0;
        const double o = c.degenerate ? 0.0 : c.om;
        w[0] = ch ? -o : o;
        w[1] = -0.5 * (c.e0 + c.e1) * w[0];   // sum_m P_nm (E_n + E_m) / Delta^2
    }
    __device__ __forceinline__ void set(const PlaneArgs& P, const int (&ii)[3], int64_t, double& lc, double& ic, double& om) const {
        const Curv2 c = at(P, ii);
        om = occ_sign > 0 ? c.om : -c.om;   // the manifold value of tbk_curv.hip, bit for bit
        const double h = -0.5 * om;
        lc = h * (occ_sign > 0 ? c.e1 : c.e0);
        ic = h * (occ_sign > 0 ? c.e0 : c.e1);
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
    __device__ __forceinline__ void set(const PlaneArgs& P, const int (&)[3], const int64_t idx, double& lc, double& ic,
                                        double& om) const {
        lc = st[idx];
        ic = st[P.npts + idx];
        om = st[2 * P.npts + idx];
    }
};

// n = 2 records for kT > 0: ev, mm, om [2][npts] of every mesh point (degenerate pairs: m = Omega = 0)
__global__ __launch_bounds__(256) void k_orb2_records(const ModelView mv, const PlaneArgs P, const int d0, const int d1,
                                                      double* __restrict__ ev, double* __restrict__ mm, double* __restrict__ om) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= P.npts) return;
    int ii[3];
    const int64_t i01 = idx / P.N[2];
    ii[2] = (int)(idx - i01 * P.N[2]);
    ii[0] = (int)(i01 / P.N[1]);
    ii[1] = (int)(i01 - (int64_t)ii[0] * P.N[1]);
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
// band-set plane sums: blockIdx.x = g of gx, blockIdx.y = slice s (and every gridDim.y after it); part[s][c][gx], c = LC, IC, Omega.
// Each sum runs in k_curv_plane's order (and the Omega sum is its manifold sum, bit for bit).
template <class Src>
__global__ __launch_bounds__(256) void k_orb_plane(const Src src, const PlaneArgs P, double* __restrict__ part) {
    __shared__ double red[3][4];
    for (int s = blockIdx.y; s < P.nslice; s += gridDim.y) {
        double acc[3] = {0.0, 0.0, 0.0};
        for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < P.nplane; p += (int64_t)gridDim.x * 256) {
            int ii[3];
            const int64_t idx = plane_point(P, s, p, ii);
            double lc, ic, om;
            src.set(P, ii, idx, lc, ic, om);
            acc[0] += lc;
            acc[1] += ic;
            acc[2] += om;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double t = block_sum(acc[c], red[c]);
            if (threadIdx.x == 0) part[((int64_t)s * 3 + c) * gridDim.x + blockIdx.x] = t;
        }
        __syncthreads();                                          // (red is reused by the next slice)
    }
}

// kT > 0 scan.  Workgroup (tile of kOrbKtTile levels, k-group g, slice s): lane t takes level j = tile + t and walks the records
// (E, m, Omega) of the plane points [g nplane / G, (g + 1) nplane / G) of slice s, every band of a point in order; a record's
// address depends on the workgroup and the loop alone, so it is read as a wave-uniform value.  Per (record, level) one exp, one
// log1p and one division:  t = e^{-|x|},  f = 1 / (1 + t) (x < 0) or t / (1 + t),  g = kT log1p(t) (x >= 0) or
// mu - E + kT log1p(t).  part[s][j][G]
__global__ __launch_bounds__(256) void k_orb_kt(const PlaneArgs P, const int nb, const double* __restrict__ ev,
                                                const double* __restrict__ mm, const double* __restrict__ om,
                                                const double* __restrict__ mu, const int nmu, const double kT, const int G,
                                                double* __restrict__ part) {
    const int base = blockIdx.x * kOrbKtTile;
    if (base + (int)(threadIdx.x & ~63u) >= nmu) return;            // a wavefront without a level (uniform)
    const int j = base + threadIdx.x, g = blockIdx.y;
    const double u = j < nmu ? mu[j] : 0.0;
    const double ikT = 1.0 / kT;
    const int64_t p0 = (int64_t)g * P.nplane / G, p1 = (int64_t)(g + 1) * P.nplane / G;
    for (int s = blockIdx.z; s < P.nslice; s += gridDim.z) {
        double acc = 0.0;
        for (int64_t p = p0; p < p1; ++p) {
            int ii[3];
            const int64_t idx = plane_point(P, s, p, ii);
            for (int b = 0; b < nb; ++b) {
                const int64_t i = (int64_t)b * P.npts + idx;
                const double e = ev[i], m = mm[i], o = om[i];
                const double x = (e - u) * ikT;
                const double t = exp(-fabs(x));
                const double r = 1.0 / (1.0 + t);
                const double l = kT * log1p(t);
                const bool up = x >= 0.0;
                const double f = up ? t * r : r;
                const double gg = up ? l : (u - e) + l;
                acc = fma(f, m, fma(gg, o, acc));
            }
        }
        if (j < nmu) part[((int64_t)s * nmu + j) * G + g] = acc;
    }
}

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
    const size_t kb = al256((size_t)nk * dk * sizeof(double)), ob = al256((size_t)ndev * sizeof(double));
    KuboChunks cw = n == 2 ? KuboChunks() : kubo_contract_chunks(n, dk, nk, manifold, OrbQ::NSET);
    void* base = nullptr;
    rc = tbk_ctx_scratch(ctx, 256 + kb + ob + cw.bytes(), &base);
    if (rc) return rc;
    unsigned char* p = (unsigned char*)base + 256;
    double* k_dev = (double*)p;
    double* o_dev = (double*)(p + kb);
    TBK_HIP(hipMemcpyAsync(k_dev, k, (size_t)nk * dk * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (n == 2) {
        ProfScope ps(ctx, "orb2_list");
        const int sign = manifold ? (mask[0] ? 1 : -1) : 0;
        hipLaunchKernelGGL(k_orb2_list, dim3(nblk(nk)), dim3(256), 0, ctx->stream, m->view, nk, (const double*)k_dev, dir0, dir1, sign,
                           o_dev);
        TBK_HIP(hipGetLastError());
    } else {
        cw.base = p + kb + ob;
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
    TBK_REQUIRE(nmu >= 0 && nmu <= 8192 && (nmu == 0 || mu), TBK_EINVAL, "tbk_orb_mag_mesh: nmu=%d (0..8192 levels)", nmu);
    TBK_REQUIRE((nmu > 0) != (occ != nullptr), TBK_EINVAL, "tbk_orb_mag_mesh: give exactly one of a band set and Fermi levels");
    TBK_REQUIRE(std::isfinite(kT) && kT >= 0.0, TBK_EINVAL, "tbk_orb_mag_mesh: kT must be finite and >= 0");
    TBK_REQUIRE(kT == 0.0 || nmu > 0, TBK_EINVAL, "tbk_orb_mag_mesh: kT > 0 needs Fermi levels");
    for (int j = 0; j < nmu; ++j)
        TBK_REQUIRE(std::isfinite(mu[j]), TBK_EINVAL, "tbk_orb_mag_mesh: Fermi level %d is not finite", j);
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
        const int64_t cap = std::max<int64_t>(1, ((int64_t)1 << 22) / ((int64_t)nslice * nmu));
        gx = (int)std::max<int64_t>(1, std::min<int64_t>({(P.nplane * n + 1023) / 1024, (int64_t)kOrbKtGroupsMax, cap}));
        nrows = (int64_t)nslice * nmu;
    }
    const size_t partb = al256((size_t)nrows * gx * sizeof(double)), rowb = al256((size_t)nrows * sizeof(double));
    const size_t mub = al256((size_t)std::max(nmu, 1) * sizeof(double));
    const bool general = n != 2;
    // per-point arrays: band set st[3][npts] (n != 2); per band ev, mm, om [n][npts] (n != 2, or n = 2 with kT > 0)
    const size_t stb = general && manifold ? al256((size_t)3 * npts * sizeof(double)) : 0;
    const size_t recb = (general && !manifold) || hot ? al256((size_t)n * npts * sizeof(double)) : 0;
    KuboChunks cw = general ? kubo_contract_chunks(n, dk, npts, manifold, OrbQ::NSET) : KuboChunks();
    void* base = nullptr;
    rc = tbk_ctx_scratch(ctx, 256 + partb + rowb + mub + stb + 3 * recb + cw.bytes(), &base);
    if (rc) return rc;
    unsigned char* p = (unsigned char*)base + 256;
    double* part = (double*)p;
    p += partb;
    double* rows = (double*)p;
    p += rowb;
    double* mu_dev = (double*)p;
    p += mub;
    double* st_dev = stb ? (double*)p : nullptr;
    p += stb;
    double* ev_dev = recb ? (double*)p : nullptr;
    double* mm_dev = recb ? (double*)(p + recb) : nullptr;
    double* om_dev = recb ? (double*)(p + 2 * recb) : nullptr;
    p += 3 * recb;
    cw.base = p;
    if (nmu) TBK_HIP(hipMemcpyAsync(mu_dev, mus.data(), (size_t)nmu * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    auto reduce = [&](auto src) -> int {
        if (manifold) {
            ProfScope ps(ctx, n == 2 ? "orb2_plane" : "orb_plane");
            hipLaunchKernelGGL(k_orb_plane<decltype(src)>, dim3(gx, (unsigned)std::min(nslice, 65535)), dim3(256), 0, ctx->stream, src,
                               P, part);
            TBK_HIP(hipGetLastError());
        } else {
            ProfScope ps(ctx, n == 2 ? "orb2_fermi" : "orb_fermi");
            int rc = kubo_fermi_launch<2>(ctx, src, P, n, mu_dev, nmu, gx, part);
            if (rc) return rc;
        }
        return TBK_OK;
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
        const unsigned ntile = (unsigned)((nmu + kOrbKtTile - 1) / kOrbKtTile);
        hipLaunchKernelGGL(k_orb_kt, dim3(ntile, (unsigned)gx, (unsigned)std::min(nslice, 65535)), dim3(256), 0, ctx->stream, P, n,
                           (const double*)ev_dev, (const double*)mm_dev, (const double*)om_dev, (const double*)mu_dev, nmu, kT, gx,
                           part);
        TBK_HIP(hipGetLastError());
    } else if (general) {
        rc = reduce(OrbArraySrc{ev_dev, mm_dev, om_dev, st_dev});
    } else {
        rc = reduce(Orb2Src{{m->view, dir0, dir1, manifold ? (mask[0] ? 1 : -1) : 0}});
    }
    if (rc) return rc;
    {
        ProfScope ps(ctx, "orb_rows");
        hipLaunchKernelGGL(k_kubo_rows, dim3((unsigned)nrows), dim3(256), 0, ctx->stream, (const double*)part, gx, rows);
        TBK_HIP(hipGetLastError());
    }
    std::vector<double> sums((size_t)nrows);
    TBK_HIP(hipMemcpyAsync(sums.data(), rows, (size_t)nrows * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
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
