// tbk_mf.hip -- the self-consistent Hartree-Fock driver on uniform k meshes.
//
// H_int = 1/2 sum_{a,b,R} V_ab(R) n_{a,0} n_{b,R} over state indices, decoupled with D_ij(R) = <c+_{j,R} c_{i,0}> of section 27:
//   Hartree   the on-site energy of a gets sum_{b,R} V_ab(R) Re D_bb(0)
//   Fock      the entry (a, b, R) of the hopping table gets -V_ab(R) D_ab(R), its mirror the conjugate
// The unknown is the real vector x (tbk_mf.h: occupations, then Re and Im of every D_ab(R) a V couples).  One iteration, all of it on
// the device and in stream order, nothing uploaded, downloaded or synchronised:
//   k_mf_apply    term_amp[t] = base[t] + sum_p c_{t,p} x_p for every term that carries a field, one lane per term (a gather over the
//                 CSR map of tbk_mf.h, contributions in list order), the same value into the term's cell of rblock where that table
//                 exists.  The private model was uploaded with every such term pinned (tbk_model_upload_pinned): no table changes shape.
//   solve         the chunks of tbk_kubo.h (kubo_chunk_len) with eigenvectors, the chunk's eigenvalues copied into the resident level
//                 array.  Resident form (N_k nsta^2 <= 2^26 c128, or TBK_MF_RESIDENT_MAX): every chunk's eigenvectors stay.
//   mu            occ_fermi_stage (tbk_occ.hip): the bisection on the resident levels, mu left in device memory (skipped at a given mu)
//   D             occ_dm_stage per chunk, weights at the device's mu: over the resident chunks, or (two-pass form) over chunks solved a
//                 second time -- WITH vectors both times, so that the levels the bisection saw are the bits the weights see
//   k_mf_gather   x_out[p] = acc[gidx[p]] / N_k
//   k_mf_mix      ONE workgroup: r = x_out - x_in into the history ring, max |r| and the new row of the Gram matrix by fixed-order block
//                 sums (lane t takes the parameters t, t + 256, ...), the small solve (mf_anderson, tbk_mf.h) in lane 0, the next x_in,
//                 the residual and the occupation row of the iteration into the history arrays
// At a convergence check (every check_every iterations) the host reads the iteration's residual by a plain 8-byte copy behind a
// stream synchronisation, and the solver's status words with it.  No floating-point atomics; two calls give the same bits, and so do
// the resident and the two-pass form (same chunks, same groups, same order).
#include <math.h>
#include "tbk_mf_dev.h"
#include "tbk_occ_dev.h"

// ---------------------------------------------------------------- kernels
__global__ __launch_bounds__(256) void k_mf_apply(const int nft, const int32_t* __restrict__ tptr, const int32_t* __restrict__ tterm,
                                                  const int64_t* __restrict__ trblk, const double* __restrict__ tbase,
                                                  const double* __restrict__ ccoef, const int32_t* __restrict__ cpar,
                                                  const int32_t* __restrict__ cpart, const double* __restrict__ x, cd* __restrict__ amp,
                                                  cd* __restrict__ rblock) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= nft) return;
    cd v{tbase[2 * f], tbase[2 * f + 1]};
    for (int q = tptr[f]; q < tptr[f + 1]; ++q) {
        const double c = ccoef[q] * x[cpar[q]];
        if (cpart[q]) v.y += c;
        else v.x += c;
    }
    amp[tterm[f]] = v;
    const int64_t cell = trblk[f];
    if (cell >= 0) rblock[cell] = v;
}

__global__ __launch_bounds__(256) void k_mf_gather(const int64_t np, const int64_t* __restrict__ gidx, const double* __restrict__ acc,
                                                   const double nk, double* __restrict__ xout) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < np) xout[p] = acc[gidx[p]] / nk;
}

__global__ __launch_bounds__(256) void k_mf_copy(const int64_t np, const double* __restrict__ src, double* __restrict__ dst) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < np) dst[p] = src[p];
}

// One workgroup.  it: the iteration (0-based); m: the ring's length (0: linear mixing); slot = it % m.
__global__ __launch_bounds__(256) void k_mf_mix(const int64_t np, const int it, const int m, const double alpha, const int n, const double nk,
                                                const double* __restrict__ acc, double* __restrict__ xin, const double* __restrict__ xout,
                                                double* __restrict__ xprev, double* __restrict__ ringx, double* __restrict__ ringr,
                                                double* __restrict__ gram, double* __restrict__ res_hist, double* __restrict__ occ_hist) {
    __shared__ double red[kMfHistMax + 1][4];
    __shared__ double coef[kMfHistMax], work[MF_AND_WORK];
    __shared__ int mode;
    const int t = threadIdx.x;
    const int slot = m > 0 ? it % m : 0;
    const int cnt = m > 0 ? min(it + 1, m) : 0;
    double mx = 0.0, dot[kMfHistMax];
#pragma unroll
    for (int j = 0; j < kMfHistMax; ++j) dot[j] = 0.0;
    for (int64_t p = t; p < np; p += 256) {
        const double xi = xin[p], r = xout[p] - xi;
        xprev[p] = xi;
        mx = fmax(mx, fabs(r));
        if (!(fabs(r) <= 1.7e308)) mx = INFINITY;                    // (a NaN residual must not pass for converged)
        if (m > 0) {
            ringx[(int64_t)slot * np + p] = xi;
            ringr[(int64_t)slot * np + p] = r;
#pragma unroll
            for (int j = 0; j < kMfHistMax; ++j)
                if (j < cnt) dot[j] = fma(r, j == slot ? r : ringr[(int64_t)j * np + p], dot[j]);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
    if ((t & 63) == 0) red[kMfHistMax][t >> 6] = mx;
#pragma unroll
    for (int j = 0; j < kMfHistMax; ++j) {
        double v = dot[j];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if ((t & 63) == 0) red[j][t >> 6] = v;
    }
    __syncthreads();
    if (t == 0) {
        const double* q = red[kMfHistMax];
        res_hist[it] = fmax(fmax(q[0], q[1]), fmax(q[2], q[3]));
        int md = 0;
        if (m > 0) {
            for (int j = 0; j < cnt; ++j) {
                const double s = (red[j][0] + red[j][1]) + (red[j][2] + red[j][3]);
                gram[slot * kMfHistMax + j] = s;
                gram[j * kMfHistMax + slot] = s;
            }
            if (it >= m) {                                         // the first m steps are linear
                if (mf_anderson(cnt, gram, coef, work)) md = 1;
            }
        }
        mode = md;
    }
    __syncthreads();
    const int md = mode;
    for (int64_t p = t; p < np; p += 256) {
        double v;
        if (md) {
            v = 0.0;
            for (int j = 0; j < cnt; ++j) v = fma(coef[j], fma(alpha, ringr[(int64_t)j * np + p], ringx[(int64_t)j * np + p]), v);
        } else {
            v = fma(alpha, xout[p] - xprev[p], xprev[p]);
        }
        xin[p] = v;
    }
    for (int a = t; a < n; a += 256) occ_hist[(int64_t)it * n + a] = acc[2 * ((int64_t)a * n + a)] / nk;
}

// ---------------------------------------------------------------- host side
namespace {
struct MfRun {
    MfFrame F;                 // the private model, the workspace and the loop's buffers (tbk_mf_dev.h)
    MfPlan pl;
    OccMesh M;
    int n, dk, nR, fixed_mu;
    double kT;
    template <class T>
    T* buf(int i) const { return (T*)(F.base + pl.off[i]); }
    double* fsmall(int i) const { return (double*)(F.base + pl.off[MfPlan::FSMALL] + 256 * (size_t)i); }
    double* mu_dev() const { return fsmall(0); }
};

int mf_solve_chunk(const MfRun& S, int64_t c, cd* vec) {
    const int64_t first = c * S.pl.chunk, cnt = std::min<int64_t>(S.pl.chunk, S.pl.npts - first);
    double* ec = S.buf<double>(MfPlan::EC);
    int rc = tbk_solve_list_dev(S.F.m, S.buf<double>(MfPlan::K_ALL) + first * S.dk, cnt, ec, (double*)vec);
    if (rc) return rc;
    TBK_HIP(hipMemcpyAsync(S.buf<double>(MfPlan::LEV) + first * S.n, ec, (size_t)cnt * S.n * sizeof(double), hipMemcpyDeviceToDevice,
                           S.F.ctx->stream));
    return TBK_OK;
}
int mf_dm_chunk(const MfRun& S, int64_t c, const cd* vec) {
    const int64_t first = c * S.pl.chunk, cnt = std::min<int64_t>(S.pl.chunk, S.pl.npts - first);
    return occ_dm_stage(S.F.ctx, S.F.m->view, S.pl.dm, S.M, first, cnt, S.buf<double>(MfPlan::K_ALL) + first * S.dk,
                        S.buf<double>(MfPlan::LEV) + first * S.n, vec, S.mu_dev(), 0.0, S.kT, S.buf<double>(MfPlan::FW),
                        S.buf<int32_t>(MfPlan::RDEV), S.nR, S.buf<cd>(MfPlan::DPART), S.buf<cd>(MfPlan::ACC), c > 0 ? 1 : 0);
}
// x_in -> H[x_in] -> the levels -> mu -> D -> x_out
int mf_pass(const MfRun& S) {
    tbk_ctx* ctx = S.F.ctx;
    int rc = mf_launch_apply(S.F, "mf_apply");
    if (rc) return rc;
    cd* vec = S.buf<cd>(MfPlan::VEC);
    if (S.pl.resident || !S.fixed_mu)
        for (int64_t c = 0; c < S.pl.nchunks; ++c)
            if ((rc = mf_solve_chunk(S, c, vec + (S.pl.resident ? c * S.pl.vstride : 0)))) return rc;
    if (!S.fixed_mu) {
        const OccFermiBufs B{S.buf<double>(MfPlan::FPART), S.fsmall(0), (uint64_t*)S.fsmall(1), (uint64_t*)S.fsmall(2), S.fsmall(3), S.fsmall(4)};
        if ((rc = occ_fermi_stage(ctx, S.buf<double>(MfPlan::LEV), S.pl.nlev, S.pl.G, 1, S.kT, B))) return rc;
    }
    for (int64_t c = 0; c < S.pl.nchunks; ++c) {
        if (!S.pl.resident && (rc = mf_solve_chunk(S, c, vec))) return rc;
        if ((rc = mf_dm_chunk(S, c, vec + (S.pl.resident ? c * S.pl.vstride : 0)))) return rc;
    }
    ProfScope ps(ctx, "mf_gather");
    hipLaunchKernelGGL(k_mf_gather, dim3(nblk(S.F.np)), dim3(256), 0, ctx->stream, S.F.np, (const int64_t*)S.F.lp<int64_t>(MfLoopBufs::GIDX),
                       (const double*)S.buf<cd>(MfPlan::ACC), (double)S.pl.npts, S.F.lp<double>(MfLoopBufs::XOUT));
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}
int mf_loop(MfRun& S, const MfArgs& A, int start_mode, int* iterations, int* converged) {
    tbk_ctx* ctx = S.F.ctx;
    const int64_t np = S.F.np;
    int rc;
    if (start_mode == 0) {                                         // the field of the bare model at the same filling: x = 0 goes in
        TBK_HIP(hipMemsetAsync(S.F.lp<double>(MfLoopBufs::XIN), 0, (size_t)np * sizeof(double), ctx->stream));
        if ((rc = mf_pass(S))) return rc;
        hipLaunchKernelGGL(k_mf_copy, dim3(nblk(np)), dim3(256), 0, ctx->stream, np, (const double*)S.F.lp<double>(MfLoopBufs::XOUT),
                           S.F.lp<double>(MfLoopBufs::XIN));
        TBK_HIP(hipGetLastError());
    }
    return mf_iterate(
        ctx, "tbk_mean_field_mesh", S.n, A.max_iter, A.check_every, A.tol, S.F.lp<double>(MfLoopBufs::RESH), [&]() { return mf_pass(S); },
        [&](int it) { return mf_launch_mix(S.F, "mf_mix", it, A.history, A.mixing, S.n, (double)S.pl.npts, S.buf<cd>(MfPlan::ACC)); },
        iterations, converged);
}
}  // namespace

extern "C" int tbk_mean_field_mesh(tbk_ctx* ctx, int dim_k, int norb, int nspin, const double* orb, const double* onsite, int64_t nhop,
                                   const int32_t* hop_i, const int32_t* hop_j, const int32_t* hop_R, const double* hop_amp,
                                   const int32_t* mesh, int nint, const int32_t* int_ab, const int32_t* int_R, const double* int_V, int fock,
                                   int have_nel, double nel_or_mu, double kT, int start_mode, const double* x_start, double mixing,
                                   int history, double tol, int max_iter, int check_every, double* x_in, double* x_out, double* mu_out,
                                   double* dens, int32_t* R_out, double* energies, double* res_hist, double* occ_hist, int32_t* info) {
    const char* fn = "tbk_mean_field_mesh";
    TBK_REQUIRE(ctx && mesh && x_in && x_out && mu_out && dens && R_out && energies && res_hist && occ_hist && info, TBK_EINVAL,
                "%s: null argument", fn);
    TBK_REQUIRE(nspin == 1 || nspin == 2, TBK_EINVAL, "%s: nspin=%d", fn, nspin);
    TBK_REQUIRE(norb >= 1 && norb <= 2048, TBK_EINVAL, "%s: norb=%d", fn, norb);
    TBK_REQUIRE(start_mode == 0 || (start_mode == 1 && x_start), TBK_EINVAL, "%s: start_mode=%d", fn, start_mode);
    const int dk = dim_k, n = norb * nspin;
    MfArgs A;
    A.nint = nint, A.ab = int_ab, A.R = int_R, A.V = int_V, A.fock = fock, A.have_nel = have_nel;
    A.nel = have_nel ? nel_or_mu : 0.0, A.mu = have_nel ? 0.0 : nel_or_mu, A.kT = kT;
    A.mixing = mixing, A.history = history, A.tol = tol, A.max_iter = max_iter, A.check_every = check_every;
    int64_t npts;
    double target;
    int rc = mf_check(fn, dk, n, mesh, A, npts, target);
    if (rc) return rc;
    MfProblem P;
    rc = mf_problem(fn, dk, n, A, P);
    if (rc) return rc;
    if (start_mode == 1)
        for (int64_t p = 0; p < P.np; ++p) TBK_REQUIRE(std::isfinite(x_start[p]), TBK_EINVAL, "%s: the start field is not finite", fn);
    TBK_HIP(hipSetDevice(ctx->device));

    MfRun S{};
    S.n = n, S.dk = dk, S.nR = P.nR, S.kT = kT, S.fixed_mu = have_nel ? 0 : 1;
    S.M = OccMesh{{1, 1, 1}, dk};
    for (int d = 0; d < dk; ++d) S.M.N[d] = mesh[d];
    rc = mf_frame_open(S.F, ctx, fn, dim_k, norb, nspin, orb, onsite, nhop, hop_i, hop_j, hop_R, hop_amp, P, P.np,
                       [&](MfFrame& F, int64_t nft, int64_t nnz) {
                           S.pl = mf_plan(n, dk, npts, P.nR, P.np, history, max_iter, nft, nnz, mf_resident_cap(tbk_knobs().mf_resident_max));
                           F.L = S.pl.loop, F.total = S.pl.total, F.k_all = S.pl.off[MfPlan::K_ALL];
                       });
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    TBK_HIP(hipMemcpyAsync(S.buf<int32_t>(MfPlan::RDEV), P.Rl.data(), P.Rl.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if ((rc = mf_frame_upload(S.F, P.gidx, start_mode == 1 ? x_start : nullptr))) return rc;
    TBK_HIP(hipMemcpyAsync(S.fsmall(3), &target, sizeof(double), hipMemcpyHostToDevice, st));
    if (!have_nel) TBK_HIP(hipMemcpyAsync(S.mu_dev(), &A.mu, sizeof(double), hipMemcpyHostToDevice, st));
    if ((rc = mf_frame_start(S.F, dk, mesh))) return rc;

    int iterations = 0, converged = 0;
    rc = mf_loop(S, A, start_mode, &iterations, &converged);
    if (rc) return rc;

    // the energies, once, from the last iteration's own levels and mu: N, E_band, S by the thermal scan of section 27
    double sums[3], *srows;
    rc = mf_frame_scan(S.F, "mf_scan", S.buf<double>(MfPlan::LEV), S.pl.nlev, S.pl.G, S.mu_dev(), kT, S.buf<double>(MfPlan::SPART), &srows);
    if (rc) return rc;
    TBK_HIP(hipMemcpyAsync(sums, srows, sizeof sums, hipMemcpyDeviceToHost, st));
    TBK_HIP(hipMemcpyAsync(mu_out, S.mu_dev(), sizeof(double), hipMemcpyDeviceToHost, st));
    if ((rc = mf_frame_download_x(S.F, x_in, x_out))) return rc;
    const size_t nd = (size_t)P.nR * n * n * 2;
    TBK_HIP(hipMemcpyAsync(dens, S.buf<cd>(MfPlan::ACC), nd * sizeof(double), hipMemcpyDeviceToHost, st));
    if ((rc = mf_frame_download_hist(S.F, iterations, n, res_hist, occ_hist))) return rc;
    TBK_HIP(hipStreamSynchronize(st));
    const double nk = (double)npts;
    for (size_t i = 0; i < nd; ++i) dens[i] /= nk;
    memcpy(R_out, P.Rl.data(), P.Rl.size() * sizeof(int32_t));
    // E = <H_0> + <H_int> in the Hartree-Fock state of the last iteration (density x_out in the field of x_in): the band energy
    // minus E_dc (mf_edc), which is 1/2 sum V [n n - |D|^2] at the fixed point
    const double edc = mf_edc(nint, int_ab, int_V, P.occ_par, true, P.fock ? P.nocc : -1, -1, x_in, x_out);
    const double eband = sums[1] / nk, ent = sums[2] / nk;
    energies[0] = eband - edc;
    energies[1] = ent;
    energies[2] = energies[0] - kT * ent;
    energies[3] = eband;
    energies[4] = sums[0] / nk;
    info[0] = iterations;
    info[1] = converged;
    info[2] = P.nR;
    info[3] = (int32_t)P.np;
    info[4] = S.pl.resident ? 1 : 0;
    return TBK_OK;
}
