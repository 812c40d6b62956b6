// tbk_tetra.hip -- the linear tetrahedron method on uniform meshes (Bloechl, Jepsen, Andersen, PRB 49, 16223):
// the density of states g(E) and its integral N(E), total, per band and projected on states; the per-(band, k) occupation weights
// w(mu), their derivative and Bloechl's curvature correction; and the T = 0 Fermi level of a filling from N(E).
//
// E_b(k) is the solver's b-th eigenvalue at each point of k_uniform_mesh(mesh) (periodic); every band is interpolated linearly
// inside the simplices of tbk_tetra.h and theta(E - e), delta(E - e) are integrated in closed form (tet_eval: w_i and d_i = dw_i/dE
// of a corner, the level at E occupied).  The eigenvalues of the whole mesh stay on the device as e[n][N_k] (tbk_mesh_evals_dev).
//
//   cell form (g and N, total or per band; the Fermi search)
//     k_tetra_cells  workgroup (k-group g, block of 256 energies, band tile z): a LANE owns an energy; the workgroup walks the cells
//                    [g N_k / G, (g + 1) N_k / G) of its bands in order, reads the 2^dim corner energies (the same address in every
//                    lane), sorts the corners of the dim! simplices once and lets every lane evaluate its own E.  part[g][z][2][et]
//   vertex form (weights, projected DOS)
//     k_tetra_weights  a lane per (band, point): the (dim + 1)! simplices around the point, the weight of its own corner in each
//     k_tetra_pdos   workgroup (k-group g of a chunk of kubo_for_chunks, block of 256 energies, band tile z): a lane owns an energy;
//                    per (band, point) the derivative weight D of the point's own corners, then acc[a] += D |u_b(k)[a]|^2 for the
//                    selected states from the chunk's eigenvectors (the corner energies come from the resident array of the whole
//                    mesh, so no simplex is split between chunks).  part[g][z][nsel][et]
//   k_group_rows (tbk_kubo.h)  acc[row] (+)= sum_g part[g][row], the groups in a fixed order -- ALWAYS the workgroup-per-row form: the
//                    lane-per-row form adds in another order, and a switch on the number of rows would make an energy's bits
//                    depend on how many energies stand beside it
//   k_tetra_minmax   the extrema of every band (the gap test of the Fermi level, the bracket of its search)
//
// The Fermi level: n_electrons within 1e-9 of an integer m with max E_{m-1} < min E_m gives the midpoint of the gap; else rounds of
// up to 256 trial energies (tet_trial_keys: even steps in the ordered key of a double between the bracket's ends), one launch of
// the cell form per round, until the bracket is two neighbouring doubles: eight or nine rounds and as many copies to the host.
//
// No floating-point atomics, no partition that depends on the energies, the bands of a launch or the selection: two calls give
// the same bits, and an energy gives the same bits alone and inside a longer list.
#include <math.h>
#include "tbk_tetra.h"

struct TetMesh {
    int N[3];   // the mesh, 1 beyond dim_k
};
// the index of the point ii + (o0, o1, o2), every offset in -1 .. 1, on the periodic mesh
__device__ __forceinline__ int64_t tet_index(const TetMesh& M, const int (&ii)[3], const int o0, const int o1, const int o2) {
    const int a = (ii[0] + o0 + M.N[0]) % M.N[0], b = (ii[1] + o1 + M.N[1]) % M.N[1], c = (ii[2] + o2 + M.N[2]) % M.N[2];
    return ((int64_t)a * M.N[1] + b) * M.N[2] + c;
}

// ---------------------------------------------------------------- cell form
template <int DIM>
__global__ __launch_bounds__(256) void k_tetra_cells(const double* __restrict__ ev, const int64_t npts, const TetMesh M, const int G,
                                                     const double* __restrict__ en, const int et, const int b0, const int bpz,
                                                     double* __restrict__ part) {
    constexpr int NC = 1 << DIM, NS = tet_simplices(DIM), NV = DIM + 1;
    const int base = blockIdx.y * 256;
    if (base + (int)(threadIdx.x & ~63u) >= et) return;            // a wavefront without an energy (uniform)
    const int j = base + threadIdx.x, g = blockIdx.x, z = blockIdx.z;
    const double E = j < et ? en[j] : 0.0;
    const int64_t c0 = (int64_t)g * npts / G, c1 = (int64_t)(g + 1) * npts / G;
    double aN = 0.0, aG = 0.0;
    for (int b = b0 + z * bpz; b < b0 + (z + 1) * bpz; ++b) {
        const double* __restrict__ eb = ev + (int64_t)b * npts;
        for (int64_t c = c0; c < c1; ++c) {
            int ii[3];
            mesh_point(M.N, c, ii);
            double ce[NC];
#pragma unroll
            for (int q = 0; q < NC; ++q) ce[q] = eb[tet_index(M, ii, q & 1, (q >> 1) & 1, (q >> 2) & 1)];
#pragma unroll
            for (int p = 0; p < NS; ++p) {
                double e[NV];
                int s[NV];
#pragma unroll
                for (int v = 0; v < NV; ++v) e[v] = ce[tet_corner(DIM, p, v)];
                tet_sort<NV>(e, s);
                Du w[NV];
                tet_eval<DIM>(e, E, w);
                double tn = w[0].v, tg = w[0].d;
#pragma unroll
                for (int v = 1; v < NV; ++v) {
                    tn += w[v].v;
                    tg += w[v].d;
                }
                aN += tn;
                aG += tg;
            }
        }
    }
    if (j >= et) return;
    double* p = part + (((int64_t)g * gridDim.z + z) * 2) * et + j;
    p[0] = aN;
    p[et] = aG;
}

// ---------------------------------------------------------------- vertex form
// The sum over the (dim + 1)! simplices with the point ii as a corner of the weight of that corner at E, band energies eb[N_k]:
// the occupation weight, with Bloechl's correction where asked (3-D), or its derivative.  Simplex p with ii in slot s has its origin
// at ii - corner(p, s).
template <int DIM>
__device__ __forceinline__ double tet_vertex(const double* __restrict__ eb, const TetMesh& M, const int (&ii)[3], const double E,
                                             const bool derivative, const bool correction) {
    constexpr int NS = tet_simplices(DIM), NV = DIM + 1;
    const double own = eb[tet_index(M, ii, 0, 0, 0)];
    double sum = 0.0;
#pragma unroll
    for (int p = 0; p < NS; ++p)
#pragma unroll
        for (int s = 0; s < NV; ++s) {
            const int ms = tet_corner(DIM, p, s);
            double e[NV];
            int o[NV];
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const int mv = tet_corner(DIM, p, v);
                e[v] = v == s ? own
                              : eb[tet_index(M, ii, (mv & 1) - (ms & 1), ((mv >> 1) & 1) - ((ms >> 1) & 1), ((mv >> 2) & 1) - ((ms >> 2) & 1))];
            }
            tet_sort<NV>(e, o);
            Du w[NV];
            tet_eval<DIM>(e, E, w);
#pragma unroll
            for (int v = 0; v < NV; ++v)
                if (o[v] == s) {
                    double x = derivative ? w[v].d : w[v].v;
                    if constexpr (DIM == 3)
                        if (correction) x += tet_correction(e, w, v);
                    sum += x;
                }
        }
    return sum;
}

// out[b][k] = tet_vertex / den, a lane per (band, point)
template <int DIM>
__global__ __launch_bounds__(256) void k_tetra_weights(const double* __restrict__ ev, const int64_t npts, const int n, const TetMesh M,
                                                       const double mu, const int derivative, const int correction, const double den,
                                                       double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npts * n) return;
    const int64_t b = i / npts, k = i - b * npts;
    int ii[3];
    mesh_point(M.N, k, ii);
    out[i] = tet_vertex<DIM>(ev + b * npts, M, ii, mu, derivative != 0, correction != 0) / den;
}

// The projected DOS of a chunk [first, first + cnt) of the mesh: ev[n][npts] the whole mesh's eigenvalues, evec[n][cnt][n] the
// chunk's eigenvectors.  part[g][z][nsel][et]
template <int DIM>
__global__ __launch_bounds__(256) void k_tetra_pdos(const double* __restrict__ ev, const int64_t npts, const cd* __restrict__ evec,
                                                    const int64_t cnt, const int64_t first, const int n, const TetMesh M, const int G,
                                                    const double* __restrict__ en, const int et, const int b0, const int bpz,
                                                    const int32_t* __restrict__ sel, const int nsel, double* __restrict__ part) {
    const int base = blockIdx.y * 256;
    if (base + (int)(threadIdx.x & ~63u) >= et) return;            // a wavefront without an energy (uniform)
    const int j = base + threadIdx.x, g = blockIdx.x, z = blockIdx.z;
    const double E = j < et ? en[j] : 0.0;
    const int64_t p0 = (int64_t)g * cnt / G, p1 = (int64_t)(g + 1) * cnt / G;
    double acc[kTetSelMax];
#pragma unroll
    for (int a = 0; a < kTetSelMax; ++a) acc[a] = 0.0;
    for (int b = b0 + z * bpz; b < b0 + (z + 1) * bpz; ++b) {
        const double* __restrict__ eb = ev + (int64_t)b * npts;
        for (int64_t ik = p0; ik < p1; ++ik) {
            int ii[3];
            mesh_point(M.N, first + ik, ii);
            const double D = tet_vertex<DIM>(eb, M, ii, E, true, false);
            const cd* __restrict__ u = evec + ((int64_t)b * cnt + ik) * n;
#pragma unroll
            for (int a = 0; a < kTetSelMax; ++a)
                if (a < nsel) {
                    const cd c = u[sel[a]];
                    acc[a] = fma(D, c.x * c.x + c.y * c.y, acc[a]);
                }
        }
    }
    if (j >= et) return;
    double* p = part + (((int64_t)g * gridDim.z + z) * nsel) * et + j;
#pragma unroll
    for (int a = 0; a < kTetSelMax; ++a)
        if (a < nsel) p[(int64_t)a * et] = acc[a];
}

// part[b][g][2] = (min, max) of band b over the points g 256 + t, then every gridDim.x 256 after it
__global__ __launch_bounds__(256) void k_tetra_minmax(const double* __restrict__ ev, const int64_t npts, double* __restrict__ part) {
    __shared__ double lo_s[4], hi_s[4];
    const double* e = ev + (int64_t)blockIdx.y * npts;
    double lo = INFINITY, hi = -INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npts; i += (int64_t)gridDim.x * 256) {
        lo = fmin(lo, e[i]);
        hi = fmax(hi, e[i]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fmin(lo, __shfl_xor(lo, o));
        hi = fmax(hi, __shfl_xor(hi, o));
    }
    if ((threadIdx.x & 63) == 0) {
        lo_s[threadIdx.x >> 6] = lo;
        hi_s[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double* p = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
        p[0] = fmin(fmin(lo_s[0], lo_s[1]), fmin(lo_s[2], lo_s[3]));
        p[1] = fmax(fmax(hi_s[0], hi_s[1]), fmax(hi_s[2], hi_s[3]));
    }
}

// ---------------------------------------------------------------- host side
static TetMesh tet_mesh(const int32_t* mesh, int dk) {
    TetMesh M{{1, 1, 1}};
    for (int d = 0; d < dk; ++d) M.N[d] = mesh[d];
    return M;
}
// the simplices of the mesh: the divisor of every sum over simplices of volume 1
static double tet_den(int dk, int64_t npts) { return (double)tet_simplices(dk) * (double)npts; }
// f(integral constant dim_k), for the kernels that are templates over the dimension
template <class F>
static void tet_for_dim(int dk, F&& f) {
    if (dk == 1) f(std::integral_constant<int, 1>{});
    else if (dk == 2) f(std::integral_constant<int, 2>{});
    else f(std::integral_constant<int, 3>{});
}

// one launch of the cell form over the energies en[0, et) and the band tile ib of `sw`, and its group sum into acc
static int tet_cells_launch(tbk_ctx* ctx, int dk, const double* e_dev, int64_t npts, const TetMesh& M, const TetSweep& sw, int n,
                            const double* en, int et, int ib, double* part, double* acc) {
    const int bt = sw.bt(ib, n);
    const dim3 grid((unsigned)sw.G, (unsigned)((et + 255) / 256), (unsigned)bt);
    {
        ProfScope ps(ctx, "tetra_cells");
        tet_for_dim(dk, [&](auto dim) {
            hipLaunchKernelGGL(k_tetra_cells<decltype(dim)::value>, grid, dim3(256), 0, ctx->stream, e_dev, npts, M, sw.G, en, et, sw.b0(ib),
                               sw.bpz(n), part);
        });
        TBK_HIP(hipGetLastError());
    }
    ProfScope ps(ctx, "tetra_rows");
    const int64_t nrows = (int64_t)bt * 2 * et;
    hipLaunchKernelGGL(k_group_rows, dim3((unsigned)nrows), dim3(256), 0, ctx->stream, (const double*)part, sw.G, nrows, 1.0, 0, acc);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

// out[q][band][energy] = acc's rows / den: the rows [bt][Q][et] of launch (ie, ib) sit at (ie * nbt + ib) * stride
static void tet_unpack(const TetSweep& sw, const std::vector<double>& acc, int n, int nE, double den, double* const* out) {
    for (int ie = 0; ie < sw.net; ++ie)
        for (int ib = 0; ib < sw.nbt; ++ib) {
            const int et = sw.et(ie, nE), bt = sw.bt(ib, n);
            const double* a = acc.data() + ((int64_t)ie * sw.nbt + ib) * sw.stride;
            for (int z = 0; z < bt; ++z)
                for (int q = 0; q < sw.Q; ++q)
                    for (int j = 0; j < et; ++j)
                        out[q][(int64_t)(sw.b0(ib) + z) * nE + (int64_t)ie * sw.ET + j] = a[((int64_t)z * sw.Q + q) * et + j] / den;
        }
}

extern "C" int tbk_tetrahedron_dos_mesh(tbk_model* m, const int32_t* mesh, int nE, const double* energies, int per_band, int nsel,
                                        const int32_t* sel, double* dos, double* idos, double* pdos_or_null) {
    const char* fn = "tbk_tetrahedron_dos_mesh";
    TBK_REQUIRE(m && mesh && dos && idos, TBK_EINVAL, "%s: null argument", fn);
    TBK_REQUIRE((nsel > 0) == (pdos_or_null != nullptr), TBK_EINVAL, "%s: a selection and the projected DOS go together", fn);
    const int dk = m->dim_k, n = m->nsta;
    int64_t npts;
    int rc = tet_dos_check(fn, dk, n, mesh, nE, energies, per_band, nsel, sel, npts);
    if (rc) return rc;
    const TetDosPlan pl = tet_dos_plan(n, dk, npts, nE, per_band != 0, nsel);
    tbk_ctx* ctx = m->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    void* base = nullptr;
    rc = tbk_ctx_scratch(ctx, pl.total, &base);
    if (rc) return rc;
    unsigned char* b = (unsigned char*)base;
    double* k_dev = (double*)(b + pl.off_k);
    double* e_dev = (double*)(b + pl.off_e);
    double* en_dev = (double*)(b + pl.off_en);
    int32_t* sel_dev = (int32_t*)(b + pl.off_sel);
    double* acc = (double*)(b + pl.off_acc);
    double* part = (double*)(b + pl.off_part);
    double* pacc = (double*)(b + pl.off_pacc);
    TBK_HIP(hipMemcpyAsync(en_dev, energies, (size_t)nE * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (pl.pdos) TBK_HIP(hipMemcpyAsync(sel_dev, sel, (size_t)nsel * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    rc = tbk_mesh_evals_dev(m, mesh, npts, k_dev, e_dev);
    if (rc) return rc;
    const TetMesh M = tet_mesh(mesh, dk);
    const double den = tet_den(dk, npts);
    const TetSweep& cs = pl.cell;
    for (int ie = 0; ie < cs.net; ++ie)
        for (int ib = 0; ib < cs.nbt; ++ib) {
            rc = tet_cells_launch(ctx, dk, e_dev, npts, M, cs, n, en_dev + (int64_t)ie * cs.ET, cs.et(ie, nE), ib, part,
                                  acc + ((int64_t)ie * cs.nbt + ib) * cs.stride);
            if (rc) return rc;
        }
    std::vector<double> host((size_t)cs.acc_doubles);
    TBK_HIP(hipMemcpyAsync(host.data(), acc, host.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    {
        double* const out[2] = {idos, dos};                        // the rows of a launch: N, then g
        tet_unpack(cs, host, n, nE, den, out);
    }
    if (!pl.pdos) return TBK_OK;
    // the projected DOS: the eigenvectors in chunks, the corner energies from the resident array
    const TetSweep& vs = pl.vert;
    KuboChunks cw = pl.cw;
    cw.base = b + pl.off_chunks;
    rc = kubo_for_chunks(m, cw, nullptr, mesh, npts, [&](int64_t first, int64_t cnt, const double*, const double*, const cd* vc) -> int {
        for (int ie = 0; ie < vs.net; ++ie)
            for (int ib = 0; ib < vs.nbt; ++ib) {
                const int et = vs.et(ie, nE), bt = vs.bt(ib, n);
                const double* en = en_dev + (int64_t)ie * vs.ET;
                const dim3 grid((unsigned)vs.G, (unsigned)((et + 255) / 256), (unsigned)bt);
                {
                    ProfScope ps(ctx, "tetra_pdos");
                    tet_for_dim(dk, [&](auto dim) {
                        hipLaunchKernelGGL(k_tetra_pdos<decltype(dim)::value>, grid, dim3(256), 0, ctx->stream, (const double*)e_dev, npts, vc, cnt,
                                           first, n, M, vs.G, en, et, vs.b0(ib), vs.bpz(n), (const int32_t*)sel_dev, nsel, part);
                    });
                    TBK_HIP(hipGetLastError());
                }
                ProfScope ps(ctx, "tetra_rows");
                const int64_t nrows = (int64_t)bt * nsel * et;
                hipLaunchKernelGGL(k_group_rows, dim3((unsigned)nrows), dim3(256), 0, ctx->stream, (const double*)part, vs.G, nrows, 1.0,
                                   first > 0 ? 1 : 0, pacc + ((int64_t)ie * vs.nbt + ib) * vs.stride);
                TBK_HIP(hipGetLastError());
            }
        return TBK_OK;
    });
    if (rc) return rc;
    host.resize((size_t)vs.acc_doubles);
    TBK_HIP(hipMemcpyAsync(host.data(), pacc, host.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    const int64_t per = (int64_t)(per_band ? n : 1) * nE;          // pdos[a][band][energy]
    double* out[kTetSelMax];
    for (int a = 0; a < nsel; ++a) out[a] = pdos_or_null + (int64_t)a * per;
    tet_unpack(vs, host, n, nE, den, out);
    return TBK_OK;
}

extern "C" int tbk_tetrahedron_weights_mesh(tbk_model* m, const int32_t* mesh, double mu, int correction, int derivative, double* out) {
    const char* fn = "tbk_tetrahedron_weights_mesh";
    TBK_REQUIRE(m && mesh && out, TBK_EINVAL, "%s: null argument", fn);
    const int dk = m->dim_k, n = m->nsta;
    int64_t npts;
    int rc = tet_weights_check(fn, dk, n, mesh, mu, correction, derivative, npts);
    if (rc) return rc;
    const TetWeightsPlan pl = tet_weights_plan(n, dk, npts);
    tbk_ctx* ctx = m->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    void* base = nullptr;
    rc = tbk_ctx_scratch(ctx, pl.total, &base);
    if (rc) return rc;
    unsigned char* b = (unsigned char*)base;
    double* k_dev = (double*)(b + pl.off_k);
    double* e_dev = (double*)(b + pl.off_e);
    double* w_dev = (double*)(b + pl.off_w);
    rc = tbk_mesh_evals_dev(m, mesh, npts, k_dev, e_dev);
    if (rc) return rc;
    const TetMesh M = tet_mesh(mesh, dk);
    const double den = tet_den(dk, npts);
    const int64_t total = npts * n;
    {
        ProfScope ps(ctx, "tetra_weights");
        const dim3 grid(nblk(total));
        tet_for_dim(dk, [&](auto dim) {
            hipLaunchKernelGGL(k_tetra_weights<decltype(dim)::value>, grid, dim3(256), 0, ctx->stream, (const double*)e_dev, npts, n, M, mu,
                               derivative, correction, den, w_dev);
        });
        TBK_HIP(hipGetLastError());
    }
    TBK_HIP(hipMemcpyAsync(out, w_dev, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    return TBK_OK;
}

extern "C" int tbk_tetrahedron_fermi_level_mesh(tbk_model* m, const int32_t* mesh, double n_electrons, double* mu_out) {
    const char* fn = "tbk_tetrahedron_fermi_level_mesh";
    TBK_REQUIRE(m && mesh && mu_out, TBK_EINVAL, "%s: null argument", fn);
    const int dk = m->dim_k, n = m->nsta;
    int64_t npts;
    int rc = tet_fermi_check(fn, dk, n, mesh, n_electrons, npts);
    if (rc) return rc;
    const TetFermiPlan pl = tet_fermi_plan(n, dk, npts);
    tbk_ctx* ctx = m->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    void* base = nullptr;
    rc = tbk_ctx_scratch(ctx, pl.total, &base);
    if (rc) return rc;
    unsigned char* b = (unsigned char*)base;
    double* k_dev = (double*)(b + pl.off_k);
    double* e_dev = (double*)(b + pl.off_e);
    double* en_dev = (double*)(b + pl.off_en);
    double* acc = (double*)(b + pl.off_acc);
    double* part = (double*)(b + pl.off_part);
    double* mm_dev = (double*)(b + pl.off_mm);
    rc = tbk_mesh_evals_dev(m, mesh, npts, k_dev, e_dev);               // ONE eigen-solve for the gap test and every round
    if (rc) return rc;
    {
        ProfScope ps(ctx, "tetra_minmax");
        hipLaunchKernelGGL(k_tetra_minmax, dim3((unsigned)pl.gx, (unsigned)n), dim3(256), 0, ctx->stream, (const double*)e_dev, npts, mm_dev);
        TBK_HIP(hipGetLastError());
    }
    std::vector<double> mm((size_t)n * pl.gx * 2), lo((size_t)n, INFINITY), hi((size_t)n, -INFINITY);
    TBK_HIP(hipMemcpyAsync(mm.data(), mm_dev, mm.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    for (int band = 0; band < n; ++band)
        for (int g = 0; g < pl.gx; ++g) {
            lo[band] = std::min(lo[band], mm[((size_t)band * pl.gx + g) * 2]);
            hi[band] = std::max(hi[band], mm[((size_t)band * pl.gx + g) * 2 + 1]);
        }
    const int filled = tet_integer_filling(n_electrons, n);
    if (filled && hi[filled - 1] < lo[filled]) {                    // an insulator: the middle of the gap
        *mu_out = 0.5 * (hi[filled - 1] + lo[filled]) + 0.0;
        return TBK_OK;
    }
    // nothing is occupied at the lowest level of the mesh and everything at the highest: N(klo) = 0 < n_electrons <= N(khi) = n
    uint64_t klo = occ_key(*std::min_element(lo.begin(), lo.end())), khi = occ_key(*std::max_element(hi.begin(), hi.end()));
    const TetMesh M = tet_mesh(mesh, dk);
    const double den = tet_den(dk, npts);
    uint64_t keys[kTetTrials];
    double trial[kTetTrials], rows[2 * kTetTrials];
    for (int round = 0; khi - klo > 1; ++round) {
        TBK_REQUIRE(round < kTetRoundsMax, TBK_ENOCONV, "%s: the bracket did not close in %d rounds", fn, kTetRoundsMax);
        const int nt = tet_trial_keys(klo, khi, keys);
        for (int j = 0; j < nt; ++j) trial[j] = occ_unkey(keys[j]);
        TBK_HIP(hipMemcpyAsync(en_dev, trial, (size_t)nt * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        rc = tet_cells_launch(ctx, dk, e_dev, npts, M, pl.cell, n, en_dev, nt, 0, part, acc);
        if (rc) return rc;
        TBK_HIP(hipMemcpyAsync(rows, acc, (size_t)2 * nt * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        TBK_HIP(hipStreamSynchronize(ctx->stream));
        int first = nt;                                             // the first trial whose N reaches the filling
        for (int j = nt - 1; j >= 0; --j)
            if (rows[j] / den >= n_electrons) first = j;
        if (first < nt) khi = keys[first];
        if (first > 0) klo = keys[first - 1];
    }
    *mu_out = occ_unkey(khi) + 0.0;
    return TBK_OK;
}
