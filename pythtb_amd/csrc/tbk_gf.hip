// tbk_gf.hip -- the retarded lattice Green's function of the bulk crystal on uniform meshes, the T-matrix of a local impurity and the
// LDOS around it.
//
// E_n(k) and u_n(k) are the eigenpairs of the solver (the convention-II matrix of tbk_gen_ham), z = w + i eta, eta > 0.  With N_k the
// points of k_uniform_mesh(mesh), in the index layout and phase convention of tbk_density_matrix_mesh (and of the hopping table):
//   P_ij(k, w) = sum_n u_n[i] conj(u_n[j]) / (z - E_n(k))
//   G_ij(R, w) = (1 / N_k) sum_k P_ij(k, w) e^{-2 pi i k.(R + tau_j - tau_i)} = <i,0| (z - H)^-1 |j,R>
// exactly the resolvent of the torus of the mesh.  A local impurity V on the sites (i_a, R_a):
//   g_ab(w) = G_{i_a i_b}(R_b - R_a, w),   T(w) = V (1 - g V)^-1,   det(w) = det(1 - g V)
//   ldos0[w][a]    = -(1 / pi) Im G_{s_a s_a}(0, w)
//   dldos[w][r][a] = -(1 / pi) Im sum_{bc} G_{s_a i_b}(R_b - R_r) T_bc G_{i_c s_a}(R_r - R_c)
//
// The mesh goes through tbk_kubo.h's chunks (solve with eigenvectors); per chunk and per launch tile of frequencies and lattice vectors
// the lattice sum of tbk_lat_dev.h -- the walk of the density matrix -- under the weight policy GfWt below:
//   n <= 32  k_lat_lds: the selected components of a batch's eigenvectors in LDS with the weights 1 / (z - E_n) of GF_WB frequencies; a
//            lane forms P_ij(k, w) once per (point, frequency) -- one product w_n[i] conj(w_n[j]) per state, shared by the frequencies
//            -- and adds P_ij e^{-2 pi i k.R} for GF_RB lattice vectors in registers
//   n > 32   k_lat_tile: 16 x 16 tiles of the selected block of P(k, w), strips of 16 states through LDS, plain VALU
//            both write part[g][w][R][i][j] for the k-group g of the chunk
//   k_group_rows_lanes (tbk_kubo.h)  acc[w][R][i][j] (+)= sum_g part, the groups in index order, chunk after chunk in stream order;
//            the rows of a launch tile of RT < nR lattice vectors are runs of acc, one per frequency
// then k_gf_scale (acc / N_k), and for the impurity calls k_gf_tmatrix (a wavefront per frequency on tbk_small_solve.h's solver) and
// k_gf_ldos (a lane per (frequency, probe cell, probe state)).  A selection costs n na^2 per point and frequency.  Nothing uses
// floating-point atomics and no partition depends on the frequencies, lattice vectors or selection: two calls give the same bits.
#include <math.h>
#include "tbk_gf.h"
#include "tbk_lat_dev.h"
#include "tbk_small_solve.h"

// 1 / (w + i eta - e)
__device__ __forceinline__ cd gf_weight(const double w, const double eta, const double e) {
    const double d = w - e;
    const double r = 1.0 / fma(d, d, eta * eta);
    return cd{d * r, -(eta * r)};
}
// a conj(b), every operation spelled out
__device__ __forceinline__ cd gf_outer(const cd a, const cd b) { return cd{fma(a.x, b.x, a.y * b.y), fma(a.y, b.x, -(a.x * b.y))}; }

// The weight policy of the lattice sum (tbk_lat_dev.h): the complex weights 1 / (z - E_n) of GF_WB frequencies per state, GF_RB lattice
// vectors per workgroup, a selection of the states.  The product w_n[i] conj(w_n[j]) is formed once per state and shared by the
// block's frequencies; no weight is skipped.
struct GfWt {
    static constexpr int WB = GF_WB, RB = GF_RB, NSEL = kGfSelMax;
    static constexpr bool GROUP_X = false;   // (the blocks of a launch tile can outnumber the 65 535 of the y axis)
    static constexpr const char* kLabel[3] = {"gf_lds", "gf_tile", "gf_rows"};
    typedef cd W;
    const double* omega;   // the launch tile's frequencies
    double eta;
    const int32_t* sel;    // [na], on the device
    int na, all;           // all: sel = 0 .. n - 1 in order (k_lat_lds then loads through kubo_lds_load)
    __device__ __forceinline__ double freq(const int w) const { return omega[w]; }
    __device__ __forceinline__ cd weight(const double om, const double e) const { return gf_weight(om, eta, e); }
    static __device__ __forceinline__ bool empty(const cd&) { return false; }
    template <bool FULL>
    static __device__ __forceinline__ void add(cd (&pij)[GF_WB], const cd a, const cd b, const cd* c, const int nwl) {
        const cd x = gf_outer(a, b);
#pragma unroll
        for (int w = 0; w < GF_WB; ++w)
            if (FULL || w < nwl) cfma_x(pij[w], x, c[w]);
    }
};

// acc / N_k, one lane per double
__global__ __launch_bounds__(256) void k_gf_scale(double* __restrict__ acc, const int64_t nd, const double nk) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nd) acc[i] /= nk;
}

// ---------------------------------------------------------------- the impurity
// One frequency per workgroup of ONE wavefront: g_ab = G[w][pair[a][b]][pos a][pos b] gathered from the internal blocks, M =
// [1 - g V | 1] in LDS, tbk_small_solve.h's elimination with partial pivoting, T = V (1 - g V)^-1, det = det(1 - g V).  A pivot
// of squared modulus exactly 0 sets the frequency's flag (the host reports it); its T is not written.
__global__ __launch_bounds__(64) void k_gf_tmatrix(const cd* __restrict__ Gr, const int nR, const int na, const int ns,
                                                   const int32_t* __restrict__ pos, const int32_t* __restrict__ pair,
                                                   const cd* __restrict__ V, cd* __restrict__ Tm, cd* __restrict__ det,
                                                   int32_t* __restrict__ flag) {
    __shared__ cd Mx[kGfSiteMax][2 * kGfSiteMax + 1];
    __shared__ cd gl[kGfSiteMax * kGfSiteMax], Vs[kGfSiteMax * kGfSiteMax];
    const int t = threadIdx.x, nss = ns * ns;
    const int64_t iw = blockIdx.x;
    const cd* Gw = Gr + iw * nR * na * na;
    for (int e = t; e < nss; e += 64) {
        const int a = e / ns, b = e - a * ns;
        gl[e] = Gw[((int64_t)pair[e] * na + pos[a]) * na + pos[b]];
        Vs[e] = V[e];
    }
    __syncthreads();
    for (int e = t; e < nss; e += 64) {
        const int a = e / ns, b = e - a * ns;
        cd s{a == b ? 1.0 : 0.0, 0.0};
        for (int c = 0; c < ns; ++c) {
            const cd x = gl[a * ns + c], y = Vs[c * ns + b];
            s.x = fma(x.y, y.y, fma(-x.x, y.x, s.x));
            s.y = fma(-x.y, y.x, fma(-x.x, y.y, s.y));
        }
        Mx[a][b] = s;
        Mx[a][ns + b] = cd{a == b ? 1.0 : 0.0, 0.0};
    }
    __syncthreads();
    cd d;
    if (!small_solve<kGfSiteMax>(Mx, ns, t, d)) {                  // (uniform over the workgroup)
        if (t == 0) {
            flag[iw] = 1;
            det[iw] = cd{0.0, 0.0};
        }
        return;
    }
    for (int e = t; e < nss; e += 64) {
        const int a = e / ns, b = e - a * ns;
        cd s{0.0, 0.0};
        for (int c = 0; c < ns; ++c) cfma_x(s, Vs[a * ns + c], Mx[c][ns + b]);
        Tm[iw * nss + e] = s;
    }
    if (t == 0) {
        flag[iw] = 0;
        det[iw] = d;
    }
}

// One lane per (frequency w, probe cell r, probe state a), r = nprobe standing for the bulk: ldos0[w][a] = -(1 / pi) Im G_aa(0)
// (index 0 of the internal list is R = 0), dldos[w][r][a] = -(1 / pi) Im sum_bc G[out[r][b]][a][pos b] T_bc G[in[r][c]][pos c][a].
// A frequency whose flag is set is left alone.
__global__ __launch_bounds__(256) void k_gf_ldos(const cd* __restrict__ Gr, const int nw, const int nR, const int na, const int ns,
                                                 const int nprobe, const int np, const int32_t* __restrict__ pos,
                                                 const int32_t* __restrict__ tout, const int32_t* __restrict__ tin,
                                                 const cd* __restrict__ Tm, const int32_t* __restrict__ flag, double* __restrict__ ldos0,
                                                 double* __restrict__ dldos) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)nw * (nprobe + 1) * np) return;
    const int64_t wr = idx / np;
    const int a = (int)(idx - wr * np), iw = (int)(wr / (nprobe + 1)), r = (int)(wr - (int64_t)iw * (nprobe + 1));
    const int64_t nab = (int64_t)na * na;
    const cd* Gw = Gr + (int64_t)iw * nR * nab;
    const double ipi = 0.31830988618379067154;
    if (r == nprobe) {
        ldos0[(int64_t)iw * np + a] = -ipi * Gw[(int64_t)a * na + a].y;
        return;
    }
    if (flag[iw]) return;
    const cd* Tw = Tm + (int64_t)iw * ns * ns;
    cd s{0.0, 0.0};
    for (int b = 0; b < ns; ++b) {
        cd tb{0.0, 0.0};                                           // sum_c T_bc G_{i_c s_a}(R_r - R_c)
        for (int c = 0; c < ns; ++c) cfma_x(tb, Tw[b * ns + c], Gw[(int64_t)tin[(int64_t)r * ns + c] * nab + (int64_t)pos[c] * na + a]);
        cfma_x(s, Gw[(int64_t)tout[(int64_t)r * ns + b] * nab + (int64_t)a * na + pos[b]], tb);
    }
    dldos[((int64_t)iw * nprobe + r) * np + a] = -ipi * s.y;
}

// ---------------------------------------------------------------- host side
// G[nw][nR][na][na] of the selection into acc on the device (scratch at `b`, laid out by `pl`); omega, R and sel are host arrays
static int gf_run(tbk_model* m, const int32_t* mesh, const GfPlan& pl, unsigned char* b, int nw, const double* omega, double eta, int nR,
                  const int32_t* R, const int32_t* sel) {
    tbk_ctx* ctx = m->ctx;
    const int dk = m->dim_k, na = pl.na;
    const int64_t nab = pl.nab, npts = pl.npts;
    double* om_dev = (double*)(b + pl.off_om);
    int32_t* R_dev = (int32_t*)(b + pl.off_R);
    int32_t* sel_dev = (int32_t*)(b + pl.off_sel);
    cd* acc = (cd*)(b + pl.off_acc);
    cd* part = (cd*)(b + pl.off_part);
    KuboChunks cw = pl.cw;
    cw.base = b + pl.off_chunks;
    TBK_HIP(hipMemcpyAsync(om_dev, omega, (size_t)nw * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    TBK_HIP(hipMemcpyAsync(R_dev, R, (size_t)nR * dk * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    TBK_HIP(hipMemcpyAsync(sel_dev, sel, (size_t)na * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));                     // (the host arrays may be the caller's temporaries)
    OccMesh M{{1, 1, 1}, dk};
    for (int d = 0; d < dk; ++d) M.N[d] = mesh[d];
    int all = na == m->nsta ? 1 : 0;                               // every state in order
    for (int a = 0; a < na && all; ++a) all = sel[a] == a;
    int rc = kubo_for_chunks(m, cw, nullptr, mesh, npts, [&](int64_t first, int64_t cnt, const double* kp, const double* ec, const cd* vc) -> int {
        const LatChunk c{m->view, kp, vc, ec, cnt, first, M};
        for (int w0 = 0; w0 < nw; w0 += pl.WT)
            for (int r0 = 0; r0 < nR; r0 += pl.RT) {
                const int rc = lat_launch(ctx, pl, c, GfWt{om_dev + w0, eta, sel_dev, na, all}, na, std::min(pl.WT, nw - w0),
                                          R_dev + (int64_t)r0 * dk, std::min(pl.RT, nR - r0), nR, part, acc + ((int64_t)w0 * nR + r0) * nab,
                                          first > 0 ? 1 : 0);
                if (rc) return rc;
            }
        return TBK_OK;
    });
    if (rc) return rc;
    ProfScope ps(ctx, "gf_scale");
    hipLaunchKernelGGL(k_gf_scale, dim3(nblk(pl.acc_cd * 2)), dim3(256), 0, ctx->stream, (double*)acc, pl.acc_cd * 2, (double)npts);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

extern "C" int tbk_green_function_mesh(tbk_model* m, const int32_t* mesh, int nomega, const double* omega, double eta, int nR, const int32_t* R,
                                       int nsel, const int32_t* sel, double* out) {
    const char* fn = "tbk_green_function_mesh";
    TBK_REQUIRE(m && mesh && out, TBK_EINVAL, "%s: null argument", fn);
    const int dk = m->dim_k, n = m->nsta;
    int64_t npts;
    int na;
    int rc = gf_green_check(fn, dk, n, mesh, nomega, omega, eta, nR, R, nsel, sel, npts, na);
    if (rc) return rc;
    const GfPlan pl = gf_plan(n, dk, npts, nomega, nR, na, 0);
    tbk_ctx* ctx = m->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    void* base = nullptr;
    rc = tbk_ctx_scratch(ctx, pl.total, &base);
    if (rc) return rc;
    std::vector<int32_t> all;
    if (!sel) {
        all.resize((size_t)n);
        std::iota(all.begin(), all.end(), 0);
        sel = all.data();
    }
    rc = gf_run(m, mesh, pl, (unsigned char*)base, nomega, omega, eta, nR, R, sel);
    if (rc) return rc;
    TBK_HIP(hipMemcpyAsync(out, (unsigned char*)base + pl.off_acc, (size_t)pl.acc_cd * sizeof(cd), hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    return TBK_OK;
}

// both impurity calls: the internal problem, G into scratch, the T-matrix per frequency; ldos0 != null: the contraction as well
static int gf_impurity(const char* fn, tbk_model* m, const int32_t* mesh, int nomega, const double* omega, double eta, int ns, const int32_t* st,
                       const int32_t* Rs, const double* V, int nprobe, const int32_t* Rp, int np, const int32_t* probe, double* t_out,
                       double* det_out, double* ldos0, double* dldos) {
    const int dk = m->dim_k, n = m->nsta;
    int64_t npts;
    int rc = gf_mesh_omega_check(fn, dk, n, mesh, nomega, omega, eta, npts);
    if (!rc) rc = gf_sites_check(fn, dk, n, mesh, ns, st, Rs, V);
    if (rc) return rc;
    const bool want_ldos = ldos0 != nullptr;
    std::vector<int32_t> all;
    if (want_ldos) {
        rc = lat_R_check(fn, dk, nprobe, Rp);
        int na_probe = 0;
        if (!rc) rc = gf_sel_check(fn, n, np, probe, na_probe);
        if (rc) return rc;
        if (!probe) {
            TBK_REQUIRE(n <= kGfSelMax, TBK_EINVAL, "%s: all states as probes needs nsta <= %d (the model has %d): give states", fn, kGfSelMax, n);
            all.resize((size_t)n);
            std::iota(all.begin(), all.end(), 0);
            probe = all.data();
            np = n;
        }
    } else {
        nprobe = 0, np = 0;
    }
    const GfImpurity g = gf_impurity_build(dk, mesh, ns, st, Rs, nprobe, Rp, np, probe);
    rc = gf_impurity_caps(fn, g, nomega, (int64_t)nomega * nprobe * np);
    if (rc) return rc;
    const GfImpLayout lay = gf_imp_layout(ns, nomega, nprobe, np);
    const GfPlan pl = gf_plan(n, dk, npts, nomega, g.nR, g.na, lay.total);
    tbk_ctx* ctx = m->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    void* base = nullptr;
    rc = tbk_ctx_scratch(ctx, pl.total, &base);
    if (rc) return rc;
    unsigned char* b = (unsigned char*)base;
    unsigned char* x = b + pl.off_x;
    cd* v_dev = (cd*)(x + lay.off_v);
    int32_t* tab = (int32_t*)(x + lay.off_tab);
    cd* t_dev = (cd*)(x + lay.off_t);
    cd* det_dev = (cd*)(x + lay.off_det);
    int32_t* flag_dev = (int32_t*)(x + lay.off_flag);
    double* l0_dev = (double*)(x + lay.off_ldos0);
    double* dl_dev = (double*)(x + lay.off_dldos);
    std::vector<int32_t> tabs(lay.tab_ints);
    std::copy(g.pos_site.begin(), g.pos_site.end(), tabs.begin() + lay.tab_pos_site);
    std::copy(g.pair.begin(), g.pair.end(), tabs.begin() + lay.tab_pair);
    std::copy(g.out.begin(), g.out.end(), tabs.begin() + lay.tab_out);
    std::copy(g.in.begin(), g.in.end(), tabs.begin() + lay.tab_in);
    TBK_HIP(hipMemcpyAsync(v_dev, V, (size_t)ns * ns * sizeof(cd), hipMemcpyHostToDevice, ctx->stream));
    TBK_HIP(hipMemcpyAsync(tab, tabs.data(), tabs.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    rc = gf_run(m, mesh, pl, b, nomega, omega, eta, g.nR, g.R.data(), g.sel.data());   // (synchronises behind the uploads)
    if (rc) return rc;
    const cd* Gr = (const cd*)(b + pl.off_acc);
    {
        ProfScope ps(ctx, "gf_tmatrix");
        hipLaunchKernelGGL(k_gf_tmatrix, dim3((unsigned)nomega), dim3(64), 0, ctx->stream, Gr, g.nR, g.na, ns,
                           (const int32_t*)(tab + lay.tab_pos_site), (const int32_t*)(tab + lay.tab_pair), (const cd*)v_dev, t_dev, det_dev,
                           flag_dev);
        TBK_HIP(hipGetLastError());
    }
    if (want_ldos) {
        ProfScope ps(ctx, "gf_ldos");
        const int64_t lanes = (int64_t)nomega * (nprobe + 1) * np;
        hipLaunchKernelGGL(k_gf_ldos, dim3(nblk(lanes)), dim3(256), 0, ctx->stream, Gr, nomega, g.nR, g.na, ns, nprobe, np,
                           (const int32_t*)(tab + lay.tab_pos_site), (const int32_t*)(tab + lay.tab_out), (const int32_t*)(tab + lay.tab_in),
                           (const cd*)t_dev, (const int32_t*)flag_dev, l0_dev, dl_dev);
        TBK_HIP(hipGetLastError());
    }
    std::vector<int32_t> flag((size_t)nomega);
    TBK_HIP(hipMemcpyAsync(flag.data(), flag_dev, flag.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (t_out) TBK_HIP(hipMemcpyAsync(t_out, t_dev, (size_t)nomega * ns * ns * sizeof(cd), hipMemcpyDeviceToHost, ctx->stream));
    if (det_out) TBK_HIP(hipMemcpyAsync(det_out, det_dev, (size_t)nomega * sizeof(cd), hipMemcpyDeviceToHost, ctx->stream));
    if (want_ldos) {
        TBK_HIP(hipMemcpyAsync(ldos0, l0_dev, (size_t)nomega * np * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        TBK_HIP(hipMemcpyAsync(dldos, dl_dev, (size_t)nomega * nprobe * np * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    for (int j = 0; j < nomega; ++j)
        TBK_REQUIRE(!flag[j], TBK_EINVAL, "%s: 1 - g V is singular at frequency %d (omega = %.17g): a bound state of the impurity at eta -> 0", fn,
                    j, omega[j]);
    return TBK_OK;
}

extern "C" int tbk_impurity_t_matrix_mesh(tbk_model* m, const int32_t* mesh, int nomega, const double* omega, double eta, int nsite,
                                          const int32_t* site_state, const int32_t* site_R, const double* potential, double* t_out,
                                          double* det_or_null) {
    const char* fn = "tbk_impurity_t_matrix_mesh";
    TBK_REQUIRE(m && mesh && t_out, TBK_EINVAL, "%s: null argument", fn);
    return gf_impurity(fn, m, mesh, nomega, omega, eta, nsite, site_state, site_R, potential, 0, nullptr, 0, nullptr, t_out, det_or_null, nullptr,
                       nullptr);
}

extern "C" int tbk_impurity_ldos_mesh(tbk_model* m, const int32_t* mesh, int nomega, const double* omega, double eta, int nsite,
                                      const int32_t* site_state, const int32_t* site_R, const double* potential, int nR, const int32_t* R,
                                      int nsel, const int32_t* sel, double* ldos0, double* dldos) {
    const char* fn = "tbk_impurity_ldos_mesh";
    TBK_REQUIRE(m && mesh && ldos0 && dldos, TBK_EINVAL, "%s: null argument", fn);
    return gf_impurity(fn, m, mesh, nomega, omega, eta, nsite, site_state, site_R, potential, nR, R, nsel, sel, nullptr, nullptr, ldos0, dldos);
}
