// tbk_curv.hip -- Berry curvature by the Kubo formula on k lists and uniform meshes.
//
// k in reduced coordinates, H the convention-II matrix of tbk_gen_ham: H_ab(k) = sum_t amp_t exp(2 pi i k.(R_t + tau_b - tau_a)).
//   velocity      d_d H_ab(k) = sum_t amp_t 2 pi i (R_t + tau_b - tau_a)_d exp(2 pi i k.(R_t + tau_b - tau_a))
//   per band (1)  Omega_n = -2 Im sum_{m != n} V^a_nm V^b_mn / (E_n - E_m)^2,  V^d_nm = <n| d_d H |m>;
//                 a pair with |E_n - E_m| <= 1e-9 max(1, |E_n|, |E_m|) contributes nothing to either band
//   manifold (2)  Omega_occ = -2 Im sum_{n in occ, m not in occ} V^a_nm V^b_mn / (E_n - E_m)^2   (no degeneracy rule)
//
// Two forms:
//   n = 2     one lane per k, H = d0 + d.sigma and d_a d, d_b d in registers: Omega_0 = d.(d_a d x d_b d) / (2 |d|^3) = -Omega_1,
//             no eigen-solve.  On a mesh the lane generates its own k and feeds the plane / Fermi reductions directly.
//   n != 2    the chunk pipeline and the contraction kernels of tbk_kubo.h with the policy CurvQ: up to 32 states ONE kernel with
//             several points' U, d H and products in LDS (k_kubo_lds); from 33 states W^d = d_d H U^T from the sparse slots
//             (k_kubo_wsp) and a lane per (k, band) contraction (k_kubo_contract).
// Spin form (section 15): Omega^s_n with the first velocity replaced by the spin current J^{s,a} = (Sigma_s d_a H + d_a H Sigma_s) / 2,
// Sigma_s = 1_orb (x) s.sigma, for spinful models.  The policy SpinQ (CurvQ's sums, kSpin) takes the same kernels at every n -- the n = 2
// closed form is for two velocities and is not used; the mesh reductions are those of the charge form.
// Reductions are tbk_kubo.h's (k_kubo_plane, k_kubo_fermi, k_kubo_rows over this unit's sources): fixed-shape trees (per-workgroup
// partials in a grid-stride order that depends on the mesh shape alone, then one workgroup per output): two calls on the same input
// give the same bits.  No floating-point atomics anywhere.
#include <math.h>
#include <string.h>
#include "tbk_kubo.h"

// dense d_{d0} H and d_{d1} H of nk points from the non-empty slots: the n x n matrices of point ik at out0 + ik pstride and
// out1 + ik pstride (zeroed by the caller); out1 nullable
__global__ __launch_bounds__(256) void k_curv_dham(const ModelView mv, const int64_t nk, const double* __restrict__ k, const int d0,
                                                   const int d1, const int64_t pstride, cd* __restrict__ out0, cd* __restrict__ out1) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nk * mv.nnz) return;
    const int64_t ik = idx / mv.nnz;
    const int4 e = mv.nz[(int)(idx - ik * mv.nnz)];
    const int a = e.x & 0xffff, b = e.x >> 16, n = mv.nsta;
    double kk[4];
    cd z[4];
    k_phases(mv, k, ik, kk, z);
    cd h, v0, v1;
    dham_terms(mv, a, b, e.y, e.z, kk, z, d0, d1, h, v0, v1);
    cd* o0 = out0 + ik * pstride;
    o0[a * n + b] = v0;
    o0[b * n + a] = cconj(v0);
    if (out1) {
        cd* o1 = out1 + ik * pstride;
        o1[a * n + b] = v1;
        o1[b * n + a] = cconj(v1);
    }
}

// J = (Sigma_s D + D Sigma_s) / 2 of nk dense n x n matrices D (k_curv_dham's), one lane per entry
__global__ __launch_bounds__(256) void k_curv_jham(const int n, const int64_t total, const SpinVec sv, const cd* __restrict__ dh,
                                                   cd* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int64_t nn = (int64_t)n * n, ik = idx / nn;
    const int r = (int)(idx - ik * nn), i = r / n, j = r - i * n;
    const cd* dp = dh + ik * nn;
    out[idx] = spin_apply(sv, i, j, dp[r], dp[(i ^ 1) * n + j], dp[i * n + (j ^ 1)]);
}

// ---------------------------------------------------------------- n = 2: closed form in registers (curv2_point, tbk_dham.h)
// list form: out[2][nk] per band (occ_sign == 0) or out[nk] = occ_sign * Omega_0 (the manifold of band 0: +1, of band 1: -1)
__global__ __launch_bounds__(256) void k_curv2_list(const ModelView mv, const int64_t nk, const double* __restrict__ k, const int d0,
                                                    const int d1, const int occ_sign, double* __restrict__ out) {
    const int64_t ik = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (ik >= nk) return;
    double kk[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) kk[d] = d < mv.dim_k ? k[ik * mv.dim_k + d] : 0.0;
    const Curv2 c = curv2_point(mv, kk, d0, d1);
    if (occ_sign == 0) {
        const double w = c.degenerate ? 0.0 : c.om;
        out[ik] = w;
        out[nk + ik] = -w;
    } else {
        out[ik] = occ_sign > 0 ? c.om : -c.om;
    }
}

// ---------------------------------------------------------------- mesh planes (PlaneArgs, plane_point: tbk_dham.h)
// sources of per-point values for the reductions.  band(): Omega_ch with the degeneracy rule and E_ch (k_kubo_fermi); plane(): that
// Omega_ch, or the manifold value of a band set (k_kubo_plane)
struct Curv2Src : Kubo2Src {
    __device__ __forceinline__ void band(const PlaneArgs& P, const int (&ii)[3], int64_t, const int ch, double& e, double (&w)[1]) const {
        const Curv2 c = at(P, ii);
        e = ch ? c.e1 : c.e0;
        const double o = c.degenerate ? 0.0 : c.om;
        w[0] = ch ? -o : o;
    }
    __device__ __forceinline__ void plane(const PlaneArgs& P, const int s, const int64_t p, const int ch, double (&w)[1]) const {
        int ii[3];
        const int64_t idx = plane_point(P, s, p, ii);
        double e;
        if (occ_sign == 0) return band(P, ii, idx, ch, e, w);
        const Curv2 c = at(P, ii);
        w[0] = occ_sign > 0 ? c.om : -c.om;
    }
};
struct ArraySrc {
    const double* om;   // [nch][npts]
    const double* ev;   // [n][npts] (Fermi scan only)
    __device__ __forceinline__ void band(const PlaneArgs& P, const int (&)[3], const int64_t idx, const int ch, double& e,
                                         double (&w)[1]) const {
        e = ev ? ev[(int64_t)ch * P.npts + idx] : 0.0;
        w[0] = om[(int64_t)ch * P.npts + idx];
    }
    __device__ __forceinline__ void plane(const PlaneArgs& P, const int s, const int64_t p, const int ch, double (&w)[1]) const {
        int ii[3];
        w[0] = om[(int64_t)ch * P.npts + plane_point(P, s, p, ii)];   // (a band set: one channel)
    }
};

// ---------------------------------------------------------------- n != 2: what a (point, band) lane of tbk_kubo.h's contraction keeps
// (CurvQ, the policy of the charge curvature, is in tbk_kubo.h: tbk_transport.hip sums with it too)
// the spin form: CurvQ's sums of Im J_bm V^b_mb; the kernels that form the first operator read Out::spin (kubo_spin, tbk_kubo.h)
struct SpinQ : CurvQ {
    static constexpr bool kSpin = true;
    static constexpr const char* kLabel[4] = {"spin_curv_lds", "spin_curv_wsp", "spin_curv_contract", "spin_curv_occ_sum"};
    using Contract = CurvQ;
    struct Out : CurvQ::Out {
        SpinVec spin;
    };
};

// ---------------------------------------------------------------- host side
// the checks of a spin direction: a spinful model and three finite components
static int spin_check(const char* fn, tbk_model* m, const double* spin, SpinVec& sv) {
    TBK_REQUIRE(m && spin, TBK_EINVAL, "%s: null argument", fn);
    TBK_REQUIRE(m->nspin == 2, TBK_EINVAL, "%s: the spin current needs a model with nspin = 2 (the model has %d)", fn, m->nspin);
    for (int c = 0; c < 3; ++c) {
        TBK_REQUIRE(std::isfinite(spin[c]), TBK_EINVAL, "%s: spin[%d] is not finite", fn, c);
        sv.s[c] = spin[c];
    }
    return TBK_OK;
}

// tbk_gen_dham (spin null) and tbk_gen_jham
static int gen_dham(const char* fn, tbk_model* m, const double* k, int64_t nk, int dir, const double* spin, double* out) {
    TBK_REQUIRE(m && out && nk >= 0, TBK_EINVAL, "%s: bad argument", fn);
    TBK_REQUIRE(m->dim_k >= 1 && dir >= 0 && dir < m->dim_k, TBK_EINVAL, "%s: dir=%d outside [0, dim_k=%d)", fn, dir, m->dim_k);
    TBK_REQUIRE(k || nk == 0, TBK_EINVAL, "%s: null k", fn);
    SpinVec sv{};
    if (spin) {
        int rc = spin_check(fn, m, spin, sv);
        if (rc) return rc;
    }
    if (nk == 0) return TBK_OK;
    tbk_ctx* ctx = m->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    const int n = m->nsta;
    const size_t kb = (size_t)nk * m->dim_k * sizeof(double), hb = (size_t)nk * n * n * sizeof(cd);
    double* k_dev;
    cd *h_dev, *j_dev;
    KuboCarve ws;
    ws.add(k_dev, kb), ws.add(h_dev, hb), ws.add(j_dev, spin ? hb : 0);
    int rc = kubo_carve(ctx, ws);
    if (rc) return rc;
    if (!spin) j_dev = h_dev;
    TBK_HIP(hipMemcpyAsync(k_dev, k, kb, hipMemcpyHostToDevice, ctx->stream));
    TBK_HIP(hipMemsetAsync(h_dev, 0, hb, ctx->stream));
    if (m->view.nnz > 0) {
        ProfScope ps(ctx, "gen_dham");
        hipLaunchKernelGGL(k_curv_dham, dim3(nblk(nk * m->view.nnz)), dim3(256), 0, ctx->stream, m->view, nk, (const double*)k_dev, dir, dir,
                           (int64_t)n * n, h_dev, (cd*)nullptr);
        TBK_HIP(hipGetLastError());
    }
    if (spin) {
        ProfScope ps(ctx, "gen_jham");
        hipLaunchKernelGGL(k_curv_jham, dim3(nblk(nk * n * n)), dim3(256), 0, ctx->stream, n, nk * n * n, sv, (const cd*)h_dev, j_dev);
        TBK_HIP(hipGetLastError());
    }
    TBK_HIP(hipMemcpyAsync(out, j_dev, hb, hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    return TBK_OK;
}
extern "C" int tbk_gen_dham(tbk_model* m, const double* k, int64_t nk, int dir, double* out) {
    return gen_dham("tbk_gen_dham", m, k, nk, dir, nullptr, out);
}
extern "C" int tbk_gen_jham(tbk_model* m, const double* k, int64_t nk, int dir, const double* spin, double* out) {
    TBK_REQUIRE(spin, TBK_EINVAL, "tbk_gen_jham: null spin");
    return gen_dham("tbk_gen_jham", m, k, nk, dir, spin, out);
}

// tbk_berry_curv_list (spin null) and tbk_spin_curv_list
static int curv_list(const char* fn, tbk_model* m, const double* k, int64_t nk, int dir0, int dir1, const int32_t* occ, int nocc,
                     const double* spin, double* out) {
    std::vector<int> mask;
    int rc = kubo_check(fn, spin ? "spin curvature" : "curvature", m, dir0, dir1, occ, nocc, mask);
    if (rc) return rc;
    SpinVec sv{};
    if (spin) {
        rc = spin_check(fn, m, spin, sv);
        if (rc) return rc;
    }
    TBK_REQUIRE(nk >= 0 && out && (k || nk == 0), TBK_EINVAL, "%s: bad k list or output", fn);
    const int n = m->nsta, dk = m->dim_k;
    const bool manifold = occ != nullptr;
    const int64_t nout = manifold ? nk : (int64_t)n * nk;
    if (nk == 0) return TBK_OK;
    if (manifold && nocc == n) {           // the complement is empty: nothing to sum
        std::fill(out, out + nout, 0.0);
        return TBK_OK;
    }
    tbk_ctx* ctx = m->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    const bool general = n != 2 || spin;   // (the n = 2 closed form is for two velocities)
    KuboChunks cw = general ? kubo_contract_chunks(n, dk, nk, manifold, CurvQ::NSET) : KuboChunks();
    double *k_dev, *o_dev;
    KuboCarve ws;
    ws.add(k_dev, (size_t)nk * dk * sizeof(double)), ws.add(o_dev, (size_t)nout * sizeof(double)), ws.add(cw.base, cw.bytes());
    rc = kubo_carve(ctx, ws);
    if (rc) return rc;
    TBK_HIP(hipMemcpyAsync(k_dev, k, (size_t)nk * dk * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (!general) {
        ProfScope ps(ctx, "curv2_list");
        const int sign = manifold ? (mask[0] ? 1 : -1) : 0;
        hipLaunchKernelGGL(k_curv2_list, dim3(nblk(nk)), dim3(256), 0, ctx->stream, m->view, nk, (const double*)k_dev, dir0, dir1,
                           sign, o_dev);
        TBK_HIP(hipGetLastError());
    } else {
        if (spin) rc = kubo_contract<SpinQ>(m, k_dev, nullptr, nk, dir0, dir1, mask, cw, SpinQ::Out{{o_dev, nullptr}, sv});
        else rc = kubo_contract<CurvQ>(m, k_dev, nullptr, nk, dir0, dir1, mask, cw, CurvQ::Out{o_dev, nullptr});
        if (rc) return rc;
    }
    TBK_HIP(hipMemcpyAsync(out, o_dev, (size_t)nout * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    return TBK_OK;
}
extern "C" int tbk_berry_curv_list(tbk_model* m, const double* k, int64_t nk, int dir0, int dir1, const int32_t* occ, int nocc,
                                   double* out) {
    return curv_list("tbk_berry_curv_list", m, k, nk, dir0, dir1, occ, nocc, nullptr, out);
}
extern "C" int tbk_spin_curv_list(tbk_model* m, const double* k, int64_t nk, int dir0, int dir1, const int32_t* occ, int nocc,
                                  const double* spin, double* out) {
    TBK_REQUIRE(spin, TBK_EINVAL, "tbk_spin_curv_list: null spin");
    return curv_list("tbk_spin_curv_list", m, k, nk, dir0, dir1, occ, nocc, spin, out);
}

// tbk_berry_curv_mesh (spin null) and tbk_spin_curv_mesh
static int curv_mesh(const char* fn, tbk_model* m, const int32_t* mesh, int dir0, int dir1, const int32_t* occ, int nocc, int nmu,
                     const double* mu, const double* spin, double* out) {
    std::vector<int> mask;
    int rc = kubo_check(fn, spin ? "spin curvature" : "curvature", m, dir0, dir1, occ, nocc, mask);
    if (rc) return rc;
    SpinVec sv{};
    if (spin) {
        rc = spin_check(fn, m, spin, sv);
        if (rc) return rc;
    }
    TBK_REQUIRE(mesh && out, TBK_EINVAL, "%s: null argument", fn);
    TBK_REQUIRE(m->dim_k == 2 || m->dim_k == 3, TBK_EINVAL, "%s: dim_k=%d (meshes of 2 or 3 dimensions)", fn, m->dim_k);
    rc = kubo_levels_check(fn, nmu, mu, 0);
    if (rc) return rc;
    TBK_REQUIRE(!(nmu > 0 && occ), TBK_EINVAL, "%s: a band set and a Fermi scan are exclusive", fn);
    rc = kubo_levels_finite(fn, nmu, mu);
    if (rc) return rc;
    const int n = m->nsta, dk = m->dim_k;
    PlaneArgs P;
    rc = kubo_planes(fn, mesh, dir0, dir1, dk, P);
    if (rc) return rc;
    const int64_t npts = P.npts;
    const int nslice = P.nslice;
    const bool manifold = occ != nullptr, fermi = nmu > 0;
    const int nch = fermi ? nmu : (manifold ? 1 : n);
    const int64_t nout = (int64_t)nch * nslice;
    if (manifold && nocc == n) {
        std::fill(out, out + nout, 0.0);
        return TBK_OK;
    }
    tbk_ctx* ctx = m->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    // levels sorted on the host (ties by index); results come back in input order
    std::vector<int> ord;
    std::vector<double> mus;
    kubo_levels(mu, nmu, true, ord, mus);
    // partial layout and counts: the grid-stride shapes depend on the mesh shape alone
    const bool general = n != 2 || spin;                                // (the n = 2 closed form is for two velocities)
    const int nplane_ch = (!fermi && !manifold && !general) ? 1 : nch;   // n = 2 per band: band 1 is -band 0, bit for bit
    const int gx = fermi ? kubo_fermi_gx(P, n, nmu, 1) : kubo_plane_gx(P);
    const int64_t nrows = (int64_t)nslice * nplane_ch;
    KuboChunks cw = general ? kubo_contract_chunks(n, dk, npts, manifold, CurvQ::NSET) : KuboChunks();
    double *part, *rows, *mu_dev, *om_dev, *ev_dev;
    KuboCarve ws;
    ws.add(part, (size_t)nrows * gx * sizeof(double)), ws.add(rows, (size_t)nrows * sizeof(double));
    ws.add(mu_dev, (size_t)std::max(nmu, 1) * sizeof(double));
    ws.add(om_dev, general ? (size_t)(manifold ? 1 : n) * npts * sizeof(double) : 0);
    ws.add(ev_dev, general && fermi ? (size_t)n * npts * sizeof(double) : 0);
    ws.add(cw.base, cw.bytes());
    rc = kubo_carve(ctx, ws);
    if (rc) return rc;
    if (fermi) TBK_HIP(hipMemcpyAsync(mu_dev, mus.data(), (size_t)nmu * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    auto reduce = [&](auto src) -> int {
        if (fermi) {
            ProfScope ps(ctx, general ? "curv_fermi" : "curv2_fermi");
            return kubo_fermi_launch<1>(ctx, src, P, n, mu_dev, nmu, gx, part);
        }
        ProfScope ps(ctx, general ? "curv_plane" : "curv2_plane");
        return kubo_plane_launch<1>(ctx, src, P, nplane_ch, nrows, gx, part);
    };
    if (general) {
        if (spin) rc = kubo_contract<SpinQ>(m, nullptr, mesh, npts, dir0, dir1, mask, cw, SpinQ::Out{{om_dev, ev_dev}, sv});
        else rc = kubo_contract<CurvQ>(m, nullptr, mesh, npts, dir0, dir1, mask, cw, CurvQ::Out{om_dev, ev_dev});
        if (rc) return rc;
        rc = reduce(ArraySrc{om_dev, ev_dev});
    } else {
        rc = reduce(Curv2Src{{m->view, dir0, dir1, manifold ? (mask[0] ? 1 : -1) : 0}});
    }
    if (rc) return rc;
    std::vector<double> sums;
    rc = kubo_rows_to_host(ctx, "curv_rows", part, gx, nrows, rows, sums);
    if (rc) return rc;
    const double inv = 1.0 / (double)P.nplane;
    // out[ch][s]: the Python shapes (nch,) for a 2-D mesh, (nch, nslice) for a 3-D one
    for (int s = 0; s < nslice; ++s) {
        if (fermi) {
            double acc = 0.0;                       // I(mu_j) = sum of the bins up to j: a prefix sum over the sorted levels
            for (int j = 0; j < nmu; ++j) {
                acc += sums[(size_t)s * nmu + j];
                out[(size_t)ord[j] * nslice + s] = acc * inv;
            }
        } else if (nplane_ch == 1 && !manifold) {   // n = 2 per band
            const double v = sums[(size_t)s] * inv;
            out[s] = v;
            out[(size_t)nslice + s] = -v;
        } else {
            for (int c = 0; c < nch; ++c) out[(size_t)c * nslice + s] = sums[(size_t)s * nch + c] * inv;
        }
    }
    return TBK_OK;
}
extern "C" int tbk_berry_curv_mesh(tbk_model* m, const int32_t* mesh, int dir0, int dir1, const int32_t* occ, int nocc, int nmu,
                                   const double* mu, double* out) {
    return curv_mesh("tbk_berry_curv_mesh", m, mesh, dir0, dir1, occ, nocc, nmu, mu, nullptr, out);
}
extern "C" int tbk_spin_curv_mesh(tbk_model* m, const int32_t* mesh, int dir0, int dir1, const int32_t* occ, int nocc, int nmu,
                                  const double* mu, const double* spin, double* out) {
    TBK_REQUIRE(spin, TBK_EINVAL, "tbk_spin_curv_mesh: null spin");
    return curv_mesh("tbk_spin_curv_mesh", m, mesh, dir0, dir1, occ, nocc, nmu, mu, spin, out);
}
