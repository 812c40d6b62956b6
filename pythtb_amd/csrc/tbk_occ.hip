// tbk_occ.hip -- the occupied states of a model on uniform meshes: the thermodynamic sums N, E, S at given Fermi
// levels, the Fermi level of a given filling, and the real-space density matrix D_ij(R).
//
// E_n(k) and u_n(k) are the eigenpairs of the solver (the convention-II matrix of tbk_gen_ham), f = [E <= mu] (kT = 0) or
// 1 / (1 + exp((E - mu) / kT)); a state counts once (no spin factor).  With N_k the points of k_uniform_mesh(mesh):
//   N(mu) = (1 / N_k) sum_{k,n} f,   E(mu) = (1 / N_k) sum f E_n,   S(mu) = -(1 / N_k) sum [f ln f + (1 - f) ln(1 - f)]
//   D_ij(R) = (1 / N_k) sum_k [sum_n f_n u_n[i] conj(u_n[j])] e^{-2 pi i k.(R + tau_j - tau_i)} = <c+_{j,R} c_{i,0}>
//
// tbk_thermodynamics_mesh and tbk_fermi_level_mesh solve for the eigenvalues of the whole mesh once and keep them on the device as one
// flat array of L = n N_k levels.  kT = 0 sums: tbk_kubo.h's Fermi scan k_kubo_fermi over the sorted levels and a prefix sum on the host;
// kT > 0 sums: k_occ_scan, one lane per Fermi level, group g of G walking the levels [g L / G, (g + 1) L / G) in order (k_kubo_thermal
// wants at least one record beside E: its shape does not fit), then k_kubo_rows and the tail kubo_rows_to_host.  The Fermi selection
// bisects on the ordered 64-bit key of a double (occ_key): kOccSteps times k_occ_count (the occupation of every filling's midpoint into
// per-group partials, the lanes over the levels) and k_occ_bisect (a wavefront per filling adds the partials in a fixed order and moves
// the bracket in device memory) -- no host synchronisation between steps and no workgroup that waits for another.  At kT = 0 the same pass
// counts with the step function and ends on the level e_{c-1} itself; one more pass (k_occ_count<true>, k_occ_edges) finds the next
// level above.
//
// tbk_density_matrix_mesh goes through the mesh in tbk_kubo.h's chunks (solve with eigenvectors), per chunk
//   k_dm_weights   f[n][cnt], once per (point, state)
// then the lattice sum of tbk_lat_dev.h under the weight policy DmWt below:
//   n <= 32  k_lat_lds: a batch of P points' eigenvectors in LDS, multiplied by the orbital phases e^{2 pi i k.tau_i} on the way in; a lane
//            owns an element (i, j) (and a share of the batch's points where n^2 < 256, or ES elements where n^2 > 256), forms
//            P_ij(k) = sum_n f_n w_n[i] conj(w_n[j]) skipping f_n = 0, and adds P_ij e^{-2 pi i k.R} for OCC_RB lattice vectors in registers
//   n > 32   k_lat_tile: 16 x 16 tiles of P(k), strips of 16 states through LDS, plain VALU
//            both write part[g][R][i][j] for the k-group g of the chunk
//   k_group_rows_lanes (tbk_kubo.h)  acc[R][i][j] (+)= sum_g part[g][R][i][j], the groups in index order, chunk after chunk in
//            stream order
// The phase e^{-2 pi i k.R} at mesh point (i_a / N_a) is formed from the exact integer (i_a R_a mod N_a).  Nothing uses floating-point
// atomics and no partition depends on the number of levels, fillings or lattice vectors: two calls give the same bits.
#include <math.h>
#include "tbk_occ_dev.h"

// ---------------------------------------------------------------- occupation: occ_fermi (tbk_occ_dev.h)
// the Fermi scan's source (k_kubo_fermi, the mesh as one row of N_k points): a level adds (1, E) to its bin
struct OccEvSrc {
    const double* ev;   // [n][npts]
    __device__ __forceinline__ void band(const PlaneArgs& P, const int (&)[3], const int64_t idx, const int b, double& e,
                                         double (&w)[2]) const {
        e = ev[(int64_t)b * P.npts + idx];
        w[0] = 1.0;
        w[1] = e;
    }
};

// ---------------------------------------------------------------- level scans
// The thermal sums of tbk_thermodynamics_mesh.  Workgroup (tile of 256 Fermi levels, group g): lane t takes level j = tile + t and
// walks the mesh levels [g L / G, (g + 1) L / G) in order (wave-uniform reads), adding N, E and S.  part[j][3][G] (the rows of
// k_kubo_rows).
__global__ __launch_bounds__(256) void k_occ_scan(const double* __restrict__ ev, const int64_t nlev, const int G, const double* __restrict__ mu,
                                                  const int nmu, const double kT, double* __restrict__ part) {
    const int base = blockIdx.x * 256;
    if (base + (int)(threadIdx.x & ~63u) >= nmu) return;            // a wavefront without a level (uniform)
    const int j = base + threadIdx.x, g = blockIdx.y;
    const double u = j < nmu ? mu[j] : 0.0;
    const int64_t l0 = (int64_t)g * nlev / G, l1 = (int64_t)(g + 1) * nlev / G;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int64_t l = l0; l < l1; ++l) {
        const double e = ev[l];
        double s;
        const double f = occ_fermi(e, u, kT, &s);
        a0 += f;
        a1 = fma(f, e, a1);
        a2 += s;
    }
    if (j >= nmu) return;
    double* p = part + ((int64_t)j * 3) * G + g;
    p[0] = a0;
    p[G] = a1;
    p[2 * (int64_t)G] = a2;
}

// A pass of the Fermi selection: the few fillings (at most 64) against all the levels, so the LANES take the levels.  Workgroup g
// holds the mesh levels [g L / G, (g + 1) L / G), lane t those at t, t + 256, ...; for every filling j in turn it adds the
// occupation at mu[j] (the step function at kT = 0) and block_sum leaves the group's sum in part[j][G] -- a filling's sum does not
// depend on the fillings beside it.  NEXT (kT = 0, after the last step; mu[j] is the KEY of the lower edge): the count of levels at
// or below the edge and the smallest level above it (+inf: none), part[j][2][G].
template <bool NEXT>
__global__ __launch_bounds__(256) void k_occ_count(const double* __restrict__ ev, const int64_t nlev, const int G, const double* __restrict__ mu,
                                                   const int nfill, const double kT, double* __restrict__ part) {
    __shared__ double red[4], low[4];
    const int g = blockIdx.x;
    const int64_t l0 = (int64_t)g * nlev / G, l1 = (int64_t)(g + 1) * nlev / G;
    for (int j = 0; j < nfill; ++j) {
        const double u = NEXT ? occ_unkey(((const uint64_t*)mu)[j]) : mu[j];
        double acc = 0.0, nxt = INFINITY;
        for (int64_t l = l0 + threadIdx.x; l < l1; l += 256) {
            const double e = ev[l];
            if constexpr (NEXT) {
                if (e <= u) acc += 1.0;
                else nxt = fmin(nxt, e);
            } else {
                acc += occ_fermi(e, u, kT, nullptr);
            }
        }
        if constexpr (NEXT) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) nxt = fmin(nxt, __shfl_xor(nxt, o));
            if ((threadIdx.x & 63) == 0) low[threadIdx.x >> 6] = nxt;
        }
        const double tot = block_sum(acc, red);                    // (its barrier also orders `low`)
        if (threadIdx.x == 0) {
            if constexpr (NEXT) {
                part[((int64_t)j * 2) * G + g] = tot;
                part[((int64_t)j * 2 + 1) * G + g] = fmin(fmin(low[0], low[1]), fmin(low[2], low[3]));
            } else {
                part[(int64_t)j * G + g] = tot;
            }
        }
        __syncthreads();                                           // (red and low are reused by the next filling)
    }
}

// One wavefront per filling j (blockIdx.x): lane t adds the partials t, t + 64, ... in order, a shuffle tree adds the lanes, and lane 0
// moves the bracket -- hi to the midpoint where the occupation reaches the target, lo otherwise -- then stores the next midpoint's
// double for the next pass.  The invariant: the occupation at lo is below the target, at hi it is not; a bracket of neighbouring
// keys stays as it is.
__global__ __launch_bounds__(64) void k_occ_bisect(const double* __restrict__ part, const int G, const double* __restrict__ target,
                                                   uint64_t* __restrict__ lo, uint64_t* __restrict__ hi, double* __restrict__ mu) {
    const int j = blockIdx.x;
    double tot = 0.0;
    for (int g = threadIdx.x; g < G; g += 64) tot += part[(int64_t)j * G + g];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o);
    if (threadIdx.x != 0) return;
    uint64_t a = lo[j], b = hi[j];
    const uint64_t mid = a + (b - a) / 2;
    if (b - a > 1) {
        if (tot >= target[j]) b = mid;
        else a = mid;
    }
    lo[j] = a;
    hi[j] = b;
    mu[j] = occ_unkey(a + (b - a) / 2);
}
// The same shape after the NEXT pass: edges[j] = (e_{c-1}, e_c) -- e_c = e_{c-1} where more than c levels lie at or below it
__global__ __launch_bounds__(64) void k_occ_edges(const double* __restrict__ part, const int G, const double* __restrict__ target,
                                                  const uint64_t* __restrict__ hi, double* __restrict__ edges) {
    const int j = blockIdx.x;
    double cnt = 0.0, nxt = INFINITY;
    for (int g = threadIdx.x; g < G; g += 64) {
        cnt += part[((int64_t)j * 2) * G + g];
        nxt = fmin(nxt, part[((int64_t)j * 2 + 1) * G + g]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o);
        nxt = fmin(nxt, __shfl_xor(nxt, o));
    }
    if (threadIdx.x != 0) return;
    const double lower = occ_unkey(hi[j]);
    edges[2 * j] = lower;
    edges[2 * j + 1] = cnt > target[j] ? lower : nxt;
}
// The bracket of every filling: every finite double (nothing is occupied at -DBL_MAX and everything at DBL_MAX), and the first midpoint
__global__ __launch_bounds__(64) void k_occ_arm(const int nfill, uint64_t* __restrict__ lo, uint64_t* __restrict__ hi, double* __restrict__ mu) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= nfill) return;
    const uint64_t klo = occ_key(-DBL_MAX), khi = occ_key(DBL_MAX);
    lo[j] = klo;
    hi[j] = khi;
    mu[j] = occ_unkey(klo + (khi - klo) / 2);
}
// The Fermi level of every filling, left in device memory: kT > 0 the double of the upper key, kT = 0 the midpoint of the edges
// (+ 0.0: -0 becomes +0)
__global__ __launch_bounds__(64) void k_occ_final(const int nfill, const int thermal, const uint64_t* __restrict__ hi,
                                                  const double* __restrict__ edges, double* __restrict__ mu) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= nfill) return;
    if (thermal) {
        mu[j] = occ_unkey(hi[j]) + 0.0;
        return;
    }
    const double e0 = edges[2 * j] + 0.0, e1 = edges[2 * j + 1] + 0.0;
    mu[j] = 0.5 * (e0 + e1);
}

// ---------------------------------------------------------------- density matrix
// f[b][ik] of a chunk
__global__ __launch_bounds__(256) void k_dm_weights(const double* __restrict__ ev, const int64_t total, const double mu, const double kT,
                                                    double* __restrict__ fw) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < total) fw[i] = occ_fermi(ev[i], mu, kT, nullptr);
}
// ... at the Fermi level the selection left in device memory (the mean-field driver: no round trip between the two stages)
__global__ __launch_bounds__(256) void k_dm_weights_ptr(const double* __restrict__ ev, const int64_t total, const double* __restrict__ mu,
                                                        const double kT, double* __restrict__ fw) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < total) fw[i] = occ_fermi(ev[i], mu[0], kT, nullptr);
}

// The weight policy of the lattice sum (tbk_lat_dev.h): a real weight f[b][ik] per state, one "frequency", OCC_RB lattice vectors per
// workgroup, every state in order.  A state of weight 0 is skipped (kT = 0: the empty states), and in the tiled form the first strip
// whose leading weight is 0 ends the point: the weights fall with the level.
struct DmWt {
    static constexpr int WB = 1, RB = OCC_RB, NSEL = 0;
    static constexpr bool GROUP_X = true;   // (at most 1024 blocks of lattice vectors, or 4096 / G with their tiles: they fit y)
    static constexpr const char* kLabel[3] = {"dm_lds", "dm_tile", "dm_rows"};
    typedef double W;
    __device__ __forceinline__ double freq(const int) const { return 0.0; }
    __device__ __forceinline__ double weight(const double, const double f) const { return f; }
    static __device__ __forceinline__ bool empty(const double f) { return f == 0.0; }
    template <bool FULL>
    static __device__ __forceinline__ void add(cd (&pij)[1], const cd a, const cd b, const double* f, const int) {
        cfmac_x(pij[0], cscale(a, f[0]), b);                        // += f w[i] conj(w[j])
    }
};

// ---------------------------------------------------------------- host side: the two resident stages (tbk_occ_dev.h)
int occ_fermi_stage(tbk_ctx* ctx, const double* e_dev, int64_t nlev, int G, int nfill, double kT, const OccFermiBufs& B) {
    const dim3 grid((unsigned)G), fgrid((unsigned)((nfill + 63) / 64));
    hipLaunchKernelGGL(k_occ_arm, fgrid, dim3(64), 0, ctx->stream, nfill, B.lo, B.hi, B.mu);
    TBK_HIP(hipGetLastError());
    for (int step = 0; step < kOccSteps; ++step) {
        {
            ProfScope ps(ctx, "occ_count");
            hipLaunchKernelGGL(k_occ_count<false>, grid, dim3(256), 0, ctx->stream, e_dev, nlev, G, (const double*)B.mu, nfill, kT, B.part);
            TBK_HIP(hipGetLastError());
        }
        ProfScope ps(ctx, "occ_bisect");
        hipLaunchKernelGGL(k_occ_bisect, dim3((unsigned)nfill), dim3(64), 0, ctx->stream, (const double*)B.part, G, B.target, B.lo, B.hi, B.mu);
        TBK_HIP(hipGetLastError());
    }
    if (kT == 0.0) {                                                // hi is the level e_{c-1} itself; the next one above
        {
            ProfScope ps(ctx, "occ_next");
            hipLaunchKernelGGL(k_occ_count<true>, grid, dim3(256), 0, ctx->stream, e_dev, nlev, G, (const double*)B.hi, nfill, 0.0, B.part);
            TBK_HIP(hipGetLastError());
        }
        ProfScope ps(ctx, "occ_edges");
        hipLaunchKernelGGL(k_occ_edges, dim3((unsigned)nfill), dim3(64), 0, ctx->stream, (const double*)B.part, G, B.target,
                           (const uint64_t*)B.hi, B.edges);
        TBK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_occ_final, fgrid, dim3(64), 0, ctx->stream, nfill, kT > 0.0 ? 1 : 0, (const uint64_t*)B.hi, (const double*)B.edges,
                       B.mu);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

int occ_dm_stage(tbk_ctx* ctx, const ModelView& mv, const OccDmPlan& pl, const OccMesh& M, int64_t first, int64_t cnt, const double* kp,
                 const double* ec, const cd* vc, const double* mu_dev, double mu, double kT, double* fw, const int32_t* R_dev, int nR,
                 cd* part, cd* acc, int accumulate) {
    const int n = mv.nsta, dk = mv.dim_k;
    const int64_t nn = (int64_t)n * n;
    {
        ProfScope ps(ctx, "dm_weights");
        if (mu_dev) hipLaunchKernelGGL(k_dm_weights_ptr, dim3(nblk(cnt * n)), dim3(256), 0, ctx->stream, ec, cnt * n, mu_dev, kT, fw);
        else hipLaunchKernelGGL(k_dm_weights, dim3(nblk(cnt * n)), dim3(256), 0, ctx->stream, ec, cnt * n, mu, kT, fw);
        TBK_HIP(hipGetLastError());
    }
    const LatChunk c{mv, kp, vc, fw, cnt, first, M};
    for (int r0 = 0; r0 < nR; r0 += pl.RT) {
        const int rc = lat_launch(ctx, pl, c, DmWt{}, n, 1, R_dev + (int64_t)r0 * dk, std::min(pl.RT, nR - r0), nR, part,
                                  acc + (int64_t)r0 * nn, accumulate);
        if (rc) return rc;
    }
    return TBK_OK;
}

// ---------------------------------------------------------------- host side
extern "C" int tbk_thermodynamics_mesh(tbk_model* m, const int32_t* mesh, int nmu, const double* mu, double kT, double* out) {
    const char* fn = "tbk_thermodynamics_mesh";
    TBK_REQUIRE(m && mesh && out, TBK_EINVAL, "%s: null argument", fn);
    const int dk = m->dim_k, n = m->nsta;
    int64_t npts;
    int rc = occ_thermo_check(fn, dk, n, mesh, nmu, mu, kT, npts);
    if (rc) return rc;
    const bool thermal = kT > 0.0;
    const OccScanPlan pl = occ_scan_plan(n, dk, npts, nmu, thermal, false);
    tbk_ctx* ctx = m->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    void* base = nullptr;
    rc = tbk_ctx_scratch(ctx, pl.total, &base);
    if (rc) return rc;
    unsigned char* b = (unsigned char*)base;
    double* k_dev = (double*)(b + pl.off_k);
    double* e_dev = (double*)(b + pl.off_e);
    double* part = (double*)(b + pl.off_part);
    double* rows = (double*)(b + pl.off_rows);
    double* mu_dev = (double*)(b + pl.off_mu);
    std::vector<int> ord;
    std::vector<double> mus;
    kubo_levels(mu, nmu, !thermal, ord, mus);                       // kT = 0: sorted (ties by index) for the bins of the Fermi scan
    TBK_HIP(hipMemcpyAsync(mu_dev, mus.data(), (size_t)nmu * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    rc = tbk_mesh_evals_dev(m, mesh, npts, k_dev, e_dev);
    if (rc) return rc;
    std::vector<double> sums;
    const double nk = (double)npts;
    if (thermal) {
        {
            ProfScope ps(ctx, "occ_scan");
            hipLaunchKernelGGL(k_occ_scan, dim3((unsigned)((nmu + 255) / 256), (unsigned)pl.G), dim3(256), 0, ctx->stream,
                               (const double*)e_dev, pl.nlev, pl.G, (const double*)mu_dev, nmu, kT, part);
            TBK_HIP(hipGetLastError());
        }
        rc = kubo_rows_to_host(ctx, "occ_rows", part, pl.G, pl.nrows, rows, sums);
        if (rc) return rc;
        for (int j = 0; j < nmu; ++j)
            for (int c = 0; c < 3; ++c) out[(size_t)c * nmu + j] = sums[(size_t)j * 3 + c] / nk;
        return TBK_OK;
    }
    PlaneArgs P{};                                                  // the mesh as one row of N_k points: plane point p is mesh point p
    P.N[0] = (int)npts, P.N[1] = P.N[2] = 1;
    P.da = 0, P.db = 1, P.dc = -1;
    P.nplane = P.npts = npts;
    P.nslice = 1;
    {
        ProfScope ps(ctx, "occ_fermi");
        rc = kubo_fermi_launch<2>(ctx, OccEvSrc{e_dev}, P, n, mu_dev, nmu, pl.gx, part);
        if (rc) return rc;
    }
    rc = kubo_rows_to_host(ctx, "occ_rows", part, pl.gx, pl.nrows, rows, sums);
    if (rc) return rc;
    double cnt = 0.0, en = 0.0;                                     // a level's sums: those of the bins up to it (counts: exact integers)
    for (int j = 0; j < nmu; ++j) {
        cnt += sums[(size_t)j * 2];
        en += sums[(size_t)j * 2 + 1];
        out[ord[j]] = cnt / nk;
        out[(size_t)nmu + ord[j]] = en / nk;
        out[(size_t)2 * nmu + ord[j]] = 0.0;
    }
    return TBK_OK;
}

extern "C" int tbk_fermi_level_mesh(tbk_model* m, const int32_t* mesh, int nfill, const double* n_electrons, double kT, double* mu_out,
                                    double* edges_or_null) {
    const char* fn = "tbk_fermi_level_mesh";
    TBK_REQUIRE(m && mesh && mu_out, TBK_EINVAL, "%s: null argument", fn);
    const int dk = m->dim_k, n = m->nsta;
    int64_t npts;
    std::vector<double> target;
    int rc = occ_fermi_check(fn, dk, n, mesh, nfill, n_electrons, kT, edges_or_null != nullptr, npts, target);
    if (rc) return rc;
    const OccScanPlan pl = occ_scan_plan(n, dk, npts, nfill, kT > 0.0, true);
    tbk_ctx* ctx = m->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    void* base = nullptr;
    rc = tbk_ctx_scratch(ctx, pl.total, &base);
    if (rc) return rc;
    unsigned char* b = (unsigned char*)base;
    double* k_dev = (double*)(b + pl.off_k);
    double* e_dev = (double*)(b + pl.off_e);
    double* part = (double*)(b + pl.off_part);
    double* mu_dev = (double*)(b + pl.off_mu);
    uint64_t* lo_dev = (uint64_t*)(b + pl.off_lo);
    uint64_t* hi_dev = (uint64_t*)(b + pl.off_hi);
    double* target_dev = (double*)(b + pl.off_target);
    double* edges_dev = (double*)(b + pl.off_edges);
    const size_t fb = (size_t)nfill * sizeof(double);
    TBK_HIP(hipMemcpyAsync(target_dev, target.data(), fb, hipMemcpyHostToDevice, ctx->stream));
    rc = tbk_mesh_evals_dev(m, mesh, npts, k_dev, e_dev);               // ONE eigen-solve for every filling and every step
    if (rc) return rc;
    rc = occ_fermi_stage(ctx, e_dev, pl.nlev, pl.G, nfill, kT, OccFermiBufs{part, mu_dev, lo_dev, hi_dev, target_dev, edges_dev});
    if (rc) return rc;
    if (kT > 0.0) {                                                 // the first double whose occupation reaches the target
        std::vector<uint64_t> hi((size_t)nfill);
        TBK_HIP(hipMemcpyAsync(hi.data(), hi_dev, fb, hipMemcpyDeviceToHost, ctx->stream));
        TBK_HIP(hipStreamSynchronize(ctx->stream));
        for (int j = 0; j < nfill; ++j) mu_out[j] = occ_unkey(hi[j]) + 0.0;
        return TBK_OK;
    }
    std::vector<double> edges((size_t)2 * nfill);
    TBK_HIP(hipMemcpyAsync(edges.data(), edges_dev, 2 * fb, hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    for (int j = 0; j < nfill; ++j) {
        const double e0 = edges[2 * j] + 0.0, e1 = edges[2 * j + 1] + 0.0;   // (+ 0.0: -0 becomes +0)
        mu_out[j] = 0.5 * (e0 + e1);
        if (edges_or_null) {
            edges_or_null[2 * j] = e0;
            edges_or_null[2 * j + 1] = e1;
        }
    }
    return TBK_OK;
}

extern "C" int tbk_density_matrix_mesh(tbk_model* m, const int32_t* mesh, double mu, double kT, int nR, const int32_t* R, double* out) {
    const char* fn = "tbk_density_matrix_mesh";
    TBK_REQUIRE(m && mesh && out, TBK_EINVAL, "%s: null argument", fn);
    const int dk = m->dim_k, n = m->nsta;
    int64_t npts;
    int rc = occ_dm_check(fn, dk, n, mesh, mu, kT, nR, R, npts);
    if (rc) return rc;
    const OccDmPlan pl = occ_dm_plan(n, dk, npts, nR);
    tbk_ctx* ctx = m->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    void* base = nullptr;
    rc = tbk_ctx_scratch(ctx, pl.total, &base);
    if (rc) return rc;
    unsigned char* b = (unsigned char*)base;
    int32_t* R_dev = (int32_t*)(b + pl.off_R);
    cd* acc = (cd*)(b + pl.off_acc);
    cd* part = (cd*)(b + pl.off_part);
    KuboChunks cw = pl.cw;
    cw.base = b + pl.off_chunks;
    double* fw = cw.extra<double>(0);
    TBK_HIP(hipMemcpyAsync(R_dev, R, (size_t)nR * dk * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    OccMesh M{{1, 1, 1}, dk};
    for (int d = 0; d < dk; ++d) M.N[d] = mesh[d];
    rc = kubo_for_chunks(m, cw, nullptr, mesh, npts, [&](int64_t first, int64_t cnt, const double* kp, const double* ec, const cd* vc) -> int {
        return occ_dm_stage(ctx, m->view, pl, M, first, cnt, kp, ec, vc, nullptr, mu, kT, fw, R_dev, nR, part, acc, first > 0 ? 1 : 0);
    });
    if (rc) return rc;
    const size_t nd = (size_t)pl.acc_cd * 2;
    TBK_HIP(hipMemcpyAsync(out, acc, nd * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    const double nk = (double)npts;
    for (size_t i = 0; i < nd; ++i) out[i] /= nk;
    return TBK_OK;
}
