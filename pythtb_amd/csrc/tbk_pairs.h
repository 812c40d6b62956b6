// tbk_pairs.h -- what the translation units that turn (point, pair) records into frequency sums share (tbk_optics.hip, DESIGN.md
// section 12; tbk_shift.hip, section 17; constants, opt_rcp and the plan of the frequency stage also tbk_chi.hip, section 26):
//   device   the index of a pair, the occupation weight, the operators of a unit in the eigenbasis (pair_lds_ops up to 32 states;
//            k_pair_wsp and k_opt_vprod from 33), the frequency stage k_pair_omega over a policy and its reciprocal
//   host     the three launches of the wide pair stage (pair_wide_stage), the chunk plan of the records (pair_chunks) and the driver
//            of a frequency sweep over a mesh (pair_sweep_check, pair_sweep)
// A unit says what its operators are with a SLOTS type (OptFields, ShiftPass): nops() operators, one(mv, op, z4, kk, z) the value of
// operator op at the non-empty slot z4 (ModelView.nz), and all(mv, z4, kk, z, sv) the values of every operator at once into
// sv[op][threadIdx.x].  The unit keeps its record writer and the policy of its frequency stage.  Kernels are static or templates: each
// unit holds its own copy.
#pragma once
#include "tbk_kubo.h"

static const size_t kPairRecBytes = (size_t)256 << 20;   // pair records per chunk
static const int kPairTile = 512;                        // frequencies per workgroup of a frequency kernel (two per lane)
static const int64_t kPairPartCap = (int64_t)1 << 24;    // doubles of part[G][rows]: G shrinks as the frequencies grow
static const int kPairGroupsMax = 1024;                  // k-groups G at most

// the pair (i, j), i < j, of index q in the row-major order of the strict upper triangle of n x n
__device__ __forceinline__ void opt_pair_of(const int n, const int64_t q, int& i, int& j) {
    const double t = 2.0 * n - 1.0;
    int r = (int)((t - sqrt(fmax(t * t - 8.0 * (double)q, 0.0))) * 0.5);
    r = max(0, min(r, n - 2));
    while (r > 0 && (int64_t)r * (2 * n - r - 1) / 2 > q) --r;
    while (r < n - 2 && (int64_t)(r + 1) * (2 * n - r - 2) / 2 <= q) ++r;
    i = r;
    j = (int)(q - (int64_t)r * (2 * n - r - 1) / 2) + r + 1;
}

// c = (f_m - f_n) / eps for E_m = E_n + eps, eps > 0.  kT > 0: with h = eps / 2kT and u = ((E_n + E_m) / 2 - mu) / kT,
// f_m - f_n = -sinh h / (cosh h + cosh u) by tbk_kubo.h's FermiPair.
__device__ __forceinline__ double opt_weight(const double en, const double em, const double eps, const double mu, const double kT) {
    if (kT == 0.0) return (en <= mu && !(em <= mu)) ? -1.0 / eps : 0.0;
    const FermiPair p(0.5 * eps / kT, fabs((0.5 * (en + em) - mu) / kT));
    return p.num() / p.den / eps;
}

// ---------------------------------------------------------------- pair stage, 1 .. 32 states
// The operators of np <= P points in the eigenbasis, in the dynamic LDS L of (nops + 2) P n^2: U (the eigenvectors, read once from
// HBM) at L and buffer j at L + (1 + j) P n^2, j = 0 .. nops.  For operator op, buffer op takes its values from the non-empty slots,
// buffer op + 1 takes T = (operator) U^T, then buffer op := conj(U) T; after the last one buffers 0 .. nops - 1 hold the operators.
template <class Slots>
__device__ __forceinline__ void pair_lds_ops(const ModelView& mv, const double* __restrict__ k, const cd* __restrict__ evec,
                                             const int64_t nk, const int64_t ik0, const int np, const int P, const Slots& sl, cd* L) {
    const int n = mv.nsta, nn = n * n, nops = sl.nops();
    cd* U = L;
    cd* Bf = L + P * nn;
    kubo_lds_load(U, evec, nk, ik0, np, n, nn, [](int) {});
    for (int op = 0; op < nops; ++op) {
        cd* S = Bf + op * P * nn;
        cd* T = Bf + (op + 1) * P * nn;
        for (int e = threadIdx.x; e < np * nn; e += 256) S[e] = cd{0.0, 0.0};
        __syncthreads();
        for (int e = threadIdx.x; e < np * mv.nnz; e += 256) {
            const int p = e / mv.nnz;
            const int4 z4 = mv.nz[e - p * mv.nnz];
            const int a = z4.x & 0xffff, b = z4.x >> 16;
            double kk[4];
            cd z[4];
            k_phases(mv, k, ik0 + p, kk, z);
            const cd v = sl.one(mv, op, z4, kk, z);
            S[p * nn + a * n + b] = v;
            S[p * nn + b * n + a] = cconj(v);
        }
        __syncthreads();
        kubo_lds_rotate(S, T, U, np, n, nn);
    }
}

// ---------------------------------------------------------------- pair stage, 33 .. 2048 states
// W^op[ik][i][m] = sum_j (operator op)_ij u_m[j] of the nops <= MAXOPS operators from the non-empty slots (the form of k_kubo_wsp):
// workgroup (point, block of 256 columns), lane m owns column m of every W^op; the slot values are computed once per point and staged
// in LDS.  wt[ik][op][n][n].
template <int MAXOPS, class Slots>
__global__ __launch_bounds__(256) void k_pair_wsp(const ModelView mv, const double* __restrict__ k, const cd* __restrict__ evec,
                                                  const int64_t nk, const Slots sl, cd* __restrict__ wt) {
    __shared__ int sab[256];
    __shared__ cd sv[MAXOPS][256];
    const int n = mv.nsta, nops = sl.nops();
    const int64_t ik = blockIdx.x, nn = (int64_t)n * n;
    const int m = blockIdx.y * 256 + threadIdx.x;
    const bool live = m < n;
    cd* w = wt + ik * nops * nn;
    if (live)
        for (int d = 0; d < nops; ++d)
            for (int i = 0; i < n; ++i) w[d * nn + (int64_t)i * n + m] = cd{0.0, 0.0};
    double kk[4];
    cd z[4];
    k_phases(mv, k, ik, kk, z);
    const cd* u = evec + ((int64_t)(live ? m : 0) * nk + ik) * n;
    for (int q0 = 0; q0 < mv.nnz; q0 += 256) {
        __syncthreads();
        if (q0 + (int)threadIdx.x < mv.nnz) {
            const int4 z4 = mv.nz[q0 + threadIdx.x];
            sl.all(mv, z4, kk, z, sv);
            sab[threadIdx.x] = z4.x;
        }
        __syncthreads();
        const int cnt = min(256, mv.nnz - q0);
        if (!live) continue;
        for (int q = 0; q < cnt; ++q) {
            const int a = sab[q] & 0xffff, b = sab[q] >> 16;
            const cd ub = u[b], ua = u[a];
            for (int d = 0; d < nops; ++d) {
                const cd v = sv[d][q];
                cd* pa = w + d * nn + (int64_t)a * n + m;
                cd t = *pa;
                cfma(t, v, ub);
                *pa = t;
                if (a != b) {
                    cd* pb = w + d * nn + (int64_t)b * n + m;
                    cd s = *pb;
                    cfma(s, cconj(v), ua);
                    *pb = s;
                }
            }
        }
    }
}

// V^d = conj(U) W^d for every (point, operator) z = ik nd + d (blockIdx.z): 16 x 16 output tiles, the 16-wide slices of conj(U) and
// W^d staged in LDS.  vt[ik][d][n][n], V^d[b][m] = <b| d_d H |m>.
static __global__ __launch_bounds__(256) void k_opt_vprod(const cd* __restrict__ evec, const cd* __restrict__ wt, const int64_t nk, const int n,
                                                   const int nd, cd* __restrict__ vt) {
    __shared__ cd Ut[16][17], Wt[16][17];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int64_t zi = blockIdx.z, nn = (int64_t)n * n;
    const int64_t ik = zi / nd;
    const int row = blockIdx.y * 16 + ty, col = blockIdx.x * 16 + tx;
    const cd* w = wt + zi * nn;
    cd acc{0.0, 0.0};
    for (int k0 = 0; k0 < n; k0 += 16) {
        const int uc = k0 + tx, wr = k0 + ty;
        Ut[ty][tx] = (row < n && uc < n) ? evec[((int64_t)row * nk + ik) * n + uc] : cd{0.0, 0.0};
        Wt[ty][tx] = (wr < n && col < n) ? w[(int64_t)wr * n + col] : cd{0.0, 0.0};
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 16; ++q) cfmac(acc, Ut[ty][q], Wt[q][tx]);
        __syncthreads();
    }
    if (row < n && col < n) vt[zi * nn + (int64_t)row * n + col] = acc;
}

// 1 / x by v_rcp_f64 and two Newton steps (x > 0, normal)
__device__ __forceinline__ double opt_rcp(const double x) {
    double r = __builtin_amdgcn_rcp(x);
    double e = fma(-x, r, 1.0);
    r = fma(r, e, r);
    e = fma(-x, r, 1.0);
    return fma(r, e, r);
}

// ---------------------------------------------------------------- frequency stage
// Workgroup (tile of kPairTile frequencies, k-group g): lane t takes w[tile + t] and w[tile + 256 + t] and walks the records of the
// points [g nk / G, (g + 1) nk / G) of the chunk (nrec records per point) in order, as wave-uniform values.  The policy says what a
// record is (OptOmega in tbk_optics.hip, ShOmega in tbk_shift.hip; tbk_chi.hip's k_chi_omega is this plan in its own text):
//   NV, NQ               doubles a lane keeps of a record; sums per frequency
//   rlen()               doubles per record
//   load(p, v)           v = what it reads of the record at p; false: the record adds nothing (uniform branch)
//   add(v, om, eta2, s)  the arithmetic of one (record, frequency) on its NQ sums
// Sum q of frequency w goes to part[g][(row0 + q) nw + w], nrows doubles per group: written, or added to (accumulate: the later
// chunks, in stream order).
template <class Pol>
__global__ __launch_bounds__(256) void k_pair_omega(const Pol pol, const double* __restrict__ rec, const int64_t nk, const int64_t nrec,
                                                    const int G, const double* __restrict__ omega, const int nw, const double eta,
                                                    const int accumulate, const int64_t nrows, const int row0,
                                                    double* __restrict__ part) {
    constexpr int NQ = Pol::NQ;
    const int base = blockIdx.x * kPairTile;
    if (base + (int)(threadIdx.x & ~63u) >= nw) return;            // a wavefront without a frequency (uniform)
    const int g = blockIdx.y;
    int wi[2];
    double om[2], s[2][NQ];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        wi[h] = base + h * 256 + threadIdx.x;
        om[h] = wi[h] < nw ? omega[wi[h]] : 0.0;
#pragma unroll
        for (int q = 0; q < NQ; ++q) s[h][q] = 0.0;
    }
    const int64_t r0 = (int64_t)g * nk / G * nrec, r1 = (int64_t)(g + 1) * nk / G * nrec;
    const double eta2 = eta * eta;
    const int R = pol.rlen();
    const double* __restrict__ p = rec + r0 * R;
    for (int64_t r = r0; r < r1; ++r, p += R) {
        double v[Pol::NV];
        if (!pol.load(p, v)) continue;
#pragma unroll
        for (int h = 0; h < 2; ++h) pol.add(v, om[h], eta2, s[h]);
    }
    double* out = part + (int64_t)g * nrows + (int64_t)row0 * nw;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (wi[h] >= nw) continue;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            double* py = out + (int64_t)q * nw + wi[h];
            *py = accumulate ? *py + s[h][q] : s[h][q];
        }
    }
}
template <class Pol>
static int pair_omega_launch(tbk_ctx* ctx, dim3 grid, const Pol& pol, const double* rec, int64_t cnt, int64_t nrec, int G, const double* om,
                             int nw, double eta, int accumulate, int64_t nrows, int row0, double* part) {
    hipLaunchKernelGGL(k_pair_omega<Pol>, grid, dim3(256), 0, ctx->stream, pol, rec, cnt, nrec, G, om, nw, eta, accumulate, nrows, row0,
                       part);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

// ---------------------------------------------------------------- host side
// The wide pair stage of a chunk: k_pair_wsp (W = (operator) U^T from the slots, wt), k_opt_vprod (V = conj(U) W, vt), then the unit's
// record kernel, launched by pairs() on vt.
template <int MAXOPS, class Slots, class Pairs>
static int pair_wide_stage(tbk_model* m, const Slots& sl, int64_t cnt, const double* kc, const cd* vc, cd* wt, cd* vt,
                           const char* wide_label, const char* pairs_label, Pairs&& pairs) {
    tbk_ctx* ctx = m->ctx;
    const int n = m->nsta, nops = sl.nops();
    {
        ProfScope ps(ctx, wide_label);
        hipLaunchKernelGGL((k_pair_wsp<MAXOPS, Slots>), dim3((unsigned)cnt, (unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                           m->view, kc, vc, cnt, sl, wt);
        TBK_HIP(hipGetLastError());
    }
    {
        // cnt nops <= 6 kKuboChunkBytes / (33^2 16 B) < 65536 (the grid's z limit)
        ProfScope ps(ctx, wide_label);
        const unsigned t = (unsigned)((n + 15) / 16);
        hipLaunchKernelGGL(k_opt_vprod, dim3(t, t, (unsigned)(cnt * nops)), dim3(256), 0, ctx->stream, vc, (const cd*)wt, cnt, n, nops, vt);
        TBK_HIP(hipGetLastError());
    }
    ProfScope ps(ctx, pairs_label);
    pairs();
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

// The chunk workspace of a pair stage over nk points of a model of at least two states: records of R doubles per pair (extra 0),
// then W and V of the wide form's wops operators (extras 1 and 2).  The chunk holds at most kKuboChunkBytes of eigenvectors and
// kPairRecBytes of records.
static KuboChunks pair_chunks(int n, int dk, int64_t nk, int R, int wops) {
    const size_t rb = (size_t)n * (n - 1) / 2 * R * sizeof(double);
    const int64_t chunk = std::min<int64_t>(kubo_chunk_len(n, nk), std::max<int64_t>(1, (int64_t)(kPairRecBytes / rb)));
    const size_t wb = n > 32 ? (size_t)chunk * wops * n * n * sizeof(cd) : 0;
    return KuboChunks(n, dk, chunk, (size_t)chunk * rb, wb, wb);
}

// The argument checks that the frequency sweeps over a mesh share, in the name of the unit's function fn; npts = the points of the
// mesh.  The unit checks its pointers before and its directions after.
static int pair_sweep_check(const char* fn, tbk_model* m, const int32_t* mesh, int nomega, const double* omega, double eta, double mu,
                            double kT, int64_t& npts) {
    int rc = kubo_mesh_dim(fn, m->dim_k);
    if (!rc) rc = kubo_omega_check(fn, nomega, omega, eta);
    if (!rc) rc = kubo_occupation_check(fn, kT, mu);
    return rc ? rc : kubo_mesh_points(fn, m->dim_k, mesh, npts);
}

// One frequency sweep over the npts points of a mesh (checked; at least two states): sums[row] = (1 / npts) sum over the points of
// what body adds to row `row` of the nrows rows (nomega per field).  The chunk, the G k-groups and the tiles are functions of (mesh, n,
// dim_k, nomega, R, nrows, wops) only.  body(w, first, cnt, k, eval, evec) writes the chunk's records (R doubles per pair at w.rec,
// through w.wt and w.vt from 33 states) and adds every k-group's sums into w.part[G][nrows] with grid (w.ntile, w.G): written by the
// first chunk, added to by the later ones (stream order).
struct PairSweep {
    int64_t npair, nrows;
    int G;
    unsigned ntile;
    const double* om;      // the nomega frequencies on the device
    double *part, *rec;
    cd *wt, *vt;
};
template <class Body>
static int pair_sweep(tbk_model* m, const int32_t* mesh, int64_t npts, int nomega, const double* omega, int R, int64_t nrows, int wops,
                      const char* rows_label, std::vector<double>& sums, Body&& body) {
    const int n = m->nsta;
    KuboChunks cw = pair_chunks(n, m->dim_k, npts, R, wops);
    const int G = (int)std::max<int64_t>(1, std::min<int64_t>({kPairPartCap / nrows, (int64_t)kPairGroupsMax, cw.chunk}));
    const size_t omb = al256((size_t)nomega * sizeof(double)), partb = al256((size_t)G * nrows * sizeof(double)),
                 rowb = al256((size_t)nrows * sizeof(double));
    tbk_ctx* ctx = m->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    void* base = nullptr;
    int rc = tbk_ctx_scratch(ctx, 256 + omb + partb + rowb + cw.bytes(), &base);
    if (rc) return rc;
    unsigned char* p = (unsigned char*)base + 256;
    double* om_dev = (double*)p;
    double* part = (double*)(p + omb);
    double* rows = (double*)(p + omb + partb);
    cw.base = p + omb + partb + rowb;
    const PairSweep w{(int64_t)n * (n - 1) / 2, nrows, G, (unsigned)((nomega + kPairTile - 1) / kPairTile), om_dev, part,
                      cw.extra<double>(0), cw.extra<cd>(1), cw.extra<cd>(2)};
    TBK_HIP(hipMemcpyAsync(om_dev, omega, (size_t)nomega * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    rc = kubo_for_chunks(m, cw, nullptr, mesh, npts, [&](int64_t first, int64_t cnt, const double* kc, const double* ec, const cd* vc) -> int {
        return body(w, first, cnt, kc, ec, vc);
    });
    if (rc) return rc;
    {
        ProfScope ps(ctx, rows_label);
        hipLaunchKernelGGL(k_group_rows, dim3((unsigned)nrows), dim3(256), 0, ctx->stream, (const double*)part, G, nrows,
                           1.0 / (double)npts, 0, rows);
        TBK_HIP(hipGetLastError());
    }
    sums.resize((size_t)nrows);
    TBK_HIP(hipMemcpyAsync(sums.data(), rows, (size_t)nrows * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    return TBK_OK;
}
