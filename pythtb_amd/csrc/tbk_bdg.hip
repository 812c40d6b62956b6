// tbk_bdg.hip -- the self-consistent Bogoliubov-de Gennes driver on uniform k meshes.
//
// H_int = 1/2 sum_{a,b,R} V_ab(R) n_{a,0} n_{b,R} over state indices, decoupled in up to three channels with the density matrix D of the
// NAMBU model (tbk_bdg.h: N = 2 n states, Psi = (c, c+), Fermi level 0):
//   Hartree   the on-site energy of a gets sum V n_b, that of the hole n + a the negative
//   Fock      the entry (a, b, R) of the particle block gets -V D_ab(R), the hole block the negated conjugate
//   pairing   the hop (a -> n + b, R) gets Delta_ab(R) = V F_ab(R), F_ab(R) = D_{a,n+b}(R), its mirror (b -> n + a, -R) gets -Delta
// The unknown is the real vector x of tbk_bdg.h; with n_electrons given, mu is its last entry.  One iteration, all of it on the device
// and in stream order, nothing uploaded, downloaded or synchronised:
//   k_mf_apply       H[x_in] into the tables of the private Nambu model (tbk_mf.hip's kernel over tbk_mf.h's CSR map; mu is one more
//                    parameter, -1 on the particle diagonal and +1 on the hole diagonal)
//   per chunk        the solve with eigenvectors, the chunk's eigenvalues copied into the resident level array, then occ_pairs_stage
//                    (tbk_pairs_dm.hip) at the Fermi level 0: the n occupations and the D and F entries the interaction couples -- the
//                    eigenvectors of one chunk are all that is ever held
//   k_mf_gather      x_out[p] = acc[gidx[p]] / N_k
//   k_bdg_mu         ONE workgroup: the occupation row of the iteration, N_out = sum_a n_a by a fixed-order block sum, and
//                    x_out[mu] = x_in[mu] + mu_step (n_electrons - N_out)
//   k_mf_mix         tbk_mf.hip's: linear or Anderson
// The loop and its check cadence are tbk_mf_dev.h's.  No floating-point atomics; two calls give the same bits.
#include <math.h>
#include "tbk_bdg.h"
#include "tbk_mf_dev.h"
#include "tbk_occ_dev.h"

// ---------------------------------------------------------------- kernels
__global__ __launch_bounds__(256) void k_bdg_mu(const int n, const double* __restrict__ acc, const double nk, const int it, const int pmu,
                                                const double nel, const double mu_step, const double* __restrict__ xin,
                                                double* __restrict__ xout, double* __restrict__ occ_hist) {
    __shared__ double red[4];
    double s = 0.0;
    for (int a = threadIdx.x; a < n; a += 256) {
        const double o = acc[2 * a] / nk;
        occ_hist[(int64_t)it * n + a] = o;
        s += o;
    }
    const double tot = block_sum(s, red);
    if (threadIdx.x == 0 && pmu >= 0) xout[pmu] = fma(mu_step, nel - tot, xin[pmu]);
}

// min |E| over the levels [g L / G, (g + 1) L / G) into part[g]; then the minimum of the partials
__global__ __launch_bounds__(256) void k_bdg_gap(const double* __restrict__ ev, const int64_t nlev, const int G, double* __restrict__ part) {
    __shared__ double red[4];
    const int g = blockIdx.x;
    const int64_t l0 = (int64_t)g * nlev / G, l1 = (int64_t)(g + 1) * nlev / G;
    double m = INFINITY;
    for (int64_t l = l0 + threadIdx.x; l < l1; l += 256) m = fmin(m, fabs(ev[l]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmin(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) part[g] = fmin(fmin(red[0], red[1]), fmin(red[2], red[3]));
}
__global__ __launch_bounds__(64) void k_bdg_gap_min(const double* __restrict__ part, const int G, double* __restrict__ out) {
    double m = INFINITY;
    for (int g = threadIdx.x; g < G; g += 64) m = fmin(m, part[g]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmin(m, __shfl_xor(m, o));
    if (threadIdx.x == 0) out[0] = m;
}

// ---------------------------------------------------------------- host side
namespace {
struct BdgRun {
    MfFrame F;                 // the private Nambu model, the workspace and the loop's buffers (tbk_mf_dev.h)
    BdgPlan pl;
    OccMesh M;
    int n, dk, pmu;
    int64_t nt;
    double kT, nel, mu_step;
    template <class T>
    T* buf(int i) const { return (T*)(F.base + pl.off[i]); }
};

// x_in -> H[x_in] -> per chunk the eigenpairs and the selected entries of D at 0 -> x_out
int bdg_pass(const BdgRun& S, int it) {
    tbk_ctx* ctx = S.F.ctx;
    int rc = mf_launch_apply(S.F, "bdg_apply");
    if (rc) return rc;
    const int N = 2 * S.n;
    double* ec = S.buf<double>(BdgPlan::EC);
    cd* vec = S.buf<cd>(BdgPlan::VEC);
    for (int64_t c = 0; c < S.pl.pd.nchunks; ++c) {
        const int64_t first = c * S.pl.pd.chunk, cnt = std::min<int64_t>(S.pl.pd.chunk, S.pl.npts - first);
        const double* kp = S.buf<double>(BdgPlan::K_ALL) + first * S.dk;
        rc = tbk_solve_list_dev(S.F.m, kp, cnt, ec, (double*)vec);
        if (rc) return rc;
        TBK_HIP(hipMemcpyAsync(S.buf<double>(BdgPlan::LEV) + first * N, ec, (size_t)cnt * N * sizeof(double), hipMemcpyDeviceToDevice,
                               ctx->stream));
        rc = occ_pairs_stage(ctx, S.F.m->view, S.pl.pd, S.M, first, cnt, kp, ec, vec, nullptr, 0.0, S.kT, S.buf<int32_t>(BdgPlan::TIJ),
                             S.buf<int32_t>(BdgPlan::TR), S.nt, S.buf<cd>(BdgPlan::PART), S.buf<cd>(BdgPlan::ACC), c > 0 ? 1 : 0);
        if (rc) return rc;
    }
    const int64_t ng = S.F.np - (S.pmu >= 0 ? 1 : 0);
    ProfScope ps(ctx, "bdg_gather");
    if (ng > 0) {
        hipLaunchKernelGGL(k_mf_gather, dim3(nblk(ng)), dim3(256), 0, ctx->stream, ng, (const int64_t*)S.F.lp<int64_t>(MfLoopBufs::GIDX),
                           (const double*)S.buf<cd>(BdgPlan::ACC), (double)S.pl.npts, S.F.lp<double>(MfLoopBufs::XOUT));
        TBK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_bdg_mu, dim3(1), dim3(256), 0, ctx->stream, S.n, (const double*)S.buf<cd>(BdgPlan::ACC), (double)S.pl.npts, it, S.pmu,
                       S.nel, S.mu_step, (const double*)S.F.lp<double>(MfLoopBufs::XIN), S.F.lp<double>(MfLoopBufs::XOUT),
                       S.F.lp<double>(MfLoopBufs::OCCH));
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}
}  // namespace

extern "C" int tbk_bdg_mesh(tbk_ctx* ctx, int dim_k, int nsta, const double* orb, const double* onsite, int64_t nhop, const int32_t* hop_i,
                            const int32_t* hop_j, const int32_t* hop_R, const double* hop_amp, const int32_t* mesh, int nint,
                            const int32_t* int_ab, const int32_t* int_R, const double* int_V, int hartree, int fock, int pairing,
                            int have_nel, double nel_or_mu, double kT, const double* x_start, double mu_step, double mixing, int history,
                            double tol, int max_iter, int check_every, double* x_in, double* x_out, double* energies, double* res_hist,
                            double* occ_hist, int32_t* info) {
    const char* fn = "tbk_bdg_mesh";
    TBK_REQUIRE(ctx && mesh && x_start && x_in && x_out && energies && res_hist && occ_hist && info, TBK_EINVAL, "%s: null argument", fn);
    const int dk = dim_k, n = nsta, N = 2 * nsta;
    BdgArgs A;
    A.nint = nint, A.ab = int_ab, A.R = int_R, A.V = int_V, A.fock = fock, A.hartree = hartree, A.pairing = pairing, A.have_nel = have_nel;
    A.nel = have_nel ? nel_or_mu : 0.0, A.mu = have_nel ? 0.0 : nel_or_mu, A.kT = kT, A.mu_step = mu_step;
    A.mixing = mixing, A.history = history, A.tol = tol, A.max_iter = max_iter, A.check_every = check_every;
    int64_t npts;
    int rc = bdg_check(fn, dk, n, mesh, A, npts);
    if (rc) return rc;
    BdgProblem B;
    rc = bdg_problem(fn, dk, n, A, B);
    if (rc) return rc;
    for (int64_t p = 0; p < B.np; ++p) TBK_REQUIRE(std::isfinite(x_start[p]), TBK_EINVAL, "%s: the start field is not finite", fn);
    TBK_HIP(hipSetDevice(ctx->device));

    // the private Nambu model: spinless, N orbitals; the caller's tables hold the bare model, with the Fermi level where it is given
    BdgRun S{};
    S.n = n, S.dk = dk, S.pmu = B.par_mu, S.nt = B.nt, S.kT = kT, S.nel = A.nel, S.mu_step = mu_step;
    S.M = OccMesh{{1, 1, 1}, dk};
    for (int d = 0; d < dk; ++d) S.M.N[d] = mesh[d];
    rc = mf_frame_open(S.F, ctx, fn, dim_k, N, 1, orb, onsite, nhop, hop_i, hop_j, hop_R, hop_amp, B.P, B.np,
                       [&](MfFrame& F, int64_t nft, int64_t nnz) {
                           S.pl = bdg_plan(n, dk, npts, B.nt, B.np, history, max_iter, nft, nnz);
                           F.L = S.pl.loop, F.total = S.pl.total, F.k_all = S.pl.off[BdgPlan::K_ALL];
                       });
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    TBK_HIP(hipMemcpyAsync(S.buf<int32_t>(BdgPlan::TIJ), B.tij.data(), B.tij.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    TBK_HIP(hipMemcpyAsync(S.buf<int32_t>(BdgPlan::TR), B.tR.data(), B.tR.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if ((rc = mf_frame_upload(S.F, B.gidx, x_start))) return rc;
    // (SPART zeroed whole: behind the scan's partials and sums sits the level 0 it runs at)
    if ((rc = mf_frame_start(S.F, dk, mesh, S.buf<double>(BdgPlan::SPART), al256((size_t)3 * S.pl.G * sizeof(double) + 512)))) return rc;

    int iterations = 0, converged = 0, cur = 0;
    rc = mf_iterate(
        ctx, fn, N, max_iter, check_every, tol, S.F.lp<double>(MfLoopBufs::RESH), [&]() { return bdg_pass(S, cur); },
        [&](int it) {
            cur = it + 1;
            return mf_launch_mix(S.F, "bdg_mix", it, history, mixing, 0, (double)npts, S.buf<cd>(BdgPlan::ACC));   // (the row is k_bdg_mu's)
        },
        &iterations, &converged);
    if (rc) return rc;

    // once, from the last iteration's own levels: sum f E and S at the Fermi level 0 by the thermal scan of section 27, and min |E|
    double* spart = S.buf<double>(BdgPlan::SPART);
    double* zero_dev = spart + (size_t)3 * S.pl.G + 32;             // (the block was zeroed: the level the scan runs at)
    double* gpart = S.buf<double>(BdgPlan::GAPP);
    double* gmin = gpart + S.pl.G;
    double sums[3], gap = 0.0, *srows;
    rc = mf_frame_scan(S.F, "bdg_scan", S.buf<double>(BdgPlan::LEV), S.pl.nlev, S.pl.G, zero_dev, kT, spart, &srows);
    if (rc) return rc;
    {
        ProfScope ps(ctx, "bdg_gap");
        hipLaunchKernelGGL(k_bdg_gap, dim3((unsigned)S.pl.G), dim3(256), 0, st, (const double*)S.buf<double>(BdgPlan::LEV), S.pl.nlev, S.pl.G, gpart);
        TBK_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_bdg_gap_min, dim3(1), dim3(64), 0, st, (const double*)gpart, S.pl.G, gmin);
        TBK_HIP(hipGetLastError());
    }
    TBK_HIP(hipMemcpyAsync(sums, srows, sizeof sums, hipMemcpyDeviceToHost, st));
    TBK_HIP(hipMemcpyAsync(&gap, gmin, sizeof gap, hipMemcpyDeviceToHost, st));
    if ((rc = mf_frame_download_x(S.F, x_in, x_out))) return rc;
    if ((rc = mf_frame_download_hist(S.F, iterations, n, res_hist, occ_hist))) return rc;
    TBK_HIP(hipStreamSynchronize(st));
    const double nk = (double)npts;
    // <H - mu N> = 1/2 (1 / N_k) sum f E + 1/2 sum_a (eps_a + d eps_a^in - mu_in) - E_dc (mf_edc, every bracket with its channel:
    // tbk_bdg.h); the trace is that of the particle block's on-site energies in the field of x_in
    const double mu_in = have_nel ? x_in[B.par_mu] : nel_or_mu;
    double tr = 0.0, nout = 0.0;
    for (int a = 0; a < n; ++a) {
        tr += onsite[2 * a];                                        // (bare; minus the given Fermi level where the tables carry it)
        nout += occ_hist[(size_t)(iterations - 1) * n + a];
    }
    if (have_nel) tr -= (double)n * mu_in;
    for (int e = 0; B.hartree && e < nint; ++e) tr += int_V[e] * (x_in[B.occ_par[int_ab[2 * e]]] + x_in[B.occ_par[int_ab[2 * e + 1]]]);
    const double edc = mf_edc(nint, int_ab, int_V, B.occ_par, B.hartree, B.par_d, B.par_f, x_in, x_out);
    const double omega = 0.5 * sums[1] / nk + 0.5 * tr - edc, ent = 0.5 * sums[2] / nk;
    energies[0] = omega + mu_in * nout;                             // E = <H - mu N> + mu N
    energies[1] = ent;
    energies[2] = energies[0] - kT * ent;                           // F = E - kT S
    energies[3] = energies[2] - mu_in * nout;                       // the grand potential F - mu N
    energies[4] = nout;
    energies[5] = mu_in;
    energies[6] = gap;
    info[0] = iterations;
    info[1] = converged;
    info[2] = B.nR;
    info[3] = (int32_t)B.np;
    info[4] = (int32_t)B.nt;
    return TBK_OK;
}
