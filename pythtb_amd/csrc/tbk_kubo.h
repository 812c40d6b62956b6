// tbk_kubo.h -- what the Kubo-formula translation units share beyond the d H formula of tbk_dham.h (DESIGN.md sections 11 to 14):
//   device   the rotation of d H into the eigenbasis for several points in LDS (kubo_lds_load, kubo_lds_dut, kubo_lds_ut,
//            kubo_lds_rotate: every kernel up to 32 states here, in tbk_qgt.hip and in tbk_pairs.h); the contraction of the solver's
//            eigenvectors with d_a H, d_b H (k_kubo_lds up to 32 states; k_kubo_wsp, k_kubo_contract and k_kubo_occ_sum from 33),
//            templates over a policy Q that says what a (point, band) lane keeps of a pair; the n = 2 mesh source; the mesh
//            reductions behind a chunk's per-point values: the plane sum k_kubo_plane over a source, the T = 0 Fermi scan
//            k_kubo_fermi, the thermal scan k_kubo_thermal over a policy, and the row sum k_kubo_rows
//   host     the argument checks (bands, Fermi levels, kT), the mesh planes, the sort of the Fermi levels, the tail
//            kubo_rows_to_host, the workspace carver KuboCarve and the chunk pipeline (KuboChunks, kubo_for_chunks)
// tbk_curv.hip, tbk_orbmag.hip and tbk_transport.hip use all of it, tbk_qgt.hip everything but the contraction and the scans, and
// tbk_pairs.h (tbk_optics.hip, tbk_shift.hip) the rotation and the chunk pipeline.  The library is built without relocatable device code, so every kernel here is a template or static: each unit
// that launches one holds its own definition and host stub.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <type_traits>
#include <vector>
#include "tbk_dham.h"

static inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
static inline unsigned nblk(int64_t threads) { return (unsigned)((threads + 255) / 256); }

// ---------------------------------------------------------------- the occupation arithmetic (kT > 0), overflow-safe
// One level at x = (E - mu) / kT, formed by the caller: t = e^{-|x|}, q = 1 / (1 + t), tq = t q.  From them f, -df/dx and the entropy
// term -f ln f - (1 - f) ln(1 - f) = |x| t q + log1p(t).  t is 0 from |x| = 746 on; |x| is cut at 1024 there, so that no 0 * inf is
// formed and the sum is 0 once t has underflowed -- one v_min_f64, where a test of tq compiles to a divergent branch around log1p in
// the thermal scans' inner loop.
struct FermiTerms {
    double x, t, q, tq;
    __device__ __forceinline__ double f() const { return x >= 0.0 ? tq : q; }
    __device__ __forceinline__ double mdf() const { return tq * q; }
    __device__ __forceinline__ double entropy() const { return fma(fmin(fabs(x), 1024.0), tq, log1p(t)); }
};
__device__ __forceinline__ FermiTerms fermi_terms(const double x) {
    const double t = exp(-fabs(x)), q = 1.0 / (1.0 + t);
    return FermiTerms{x, t, q, t * q};
}
// Two levels a = |E_m - E_n| / 2kT and u = |(E_n + E_m) / 2 - mu| / kT apart: |f_n - f_m| = sinh a / (cosh a + cosh u) = -num() / den
// with both scaled by e^{-M}, M = max(a, u): no cancellation for close levels, no overflow far from mu.
struct FermiPair {
    double a, M, den;
    __device__ __forceinline__ FermiPair(const double a_, const double u) : a(a_), M(fmax(a_, u)) {
        den = exp(a - M) + exp(-a - M) + exp(u - M) + exp(-u - M);
    }
    __device__ __forceinline__ double num() const { return exp(a - M) * expm1(-2.0 * a); }
};

// ---------------------------------------------------------------- n = 2 on a mesh: the closed form at plane point ii
struct Kubo2Src {
    ModelView mv;
    int d0, d1, occ_sign;   // occ_sign: the band set {0} (+1) or {1} (-1); 0 per band
    __device__ __forceinline__ Curv2 at(const PlaneArgs& P, const int (&ii)[3]) const {
        double kk[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int d = 0; d < 3; ++d)
            if (d < mv.dim_k) kk[d] = (double)ii[d] / (double)P.N[d];   // k_uniform_mesh's point, bit for bit
        return curv2_point(mv, kk, d0, d1);
    }
};

// ---------------------------------------------------------------- reductions
// T = 0 Fermi scan: every (point, band) item of slice s adds its NQ quantities (Src::band) to the bins of the first sorted level
// mu_j >= E_n.  A tile of 256 items is staged in LDS as (bin, quantities); each lane owns a fixed range of the window's bins and adds
// the tile's items in item order.  blockIdx.x = g of gx (tiles g, g + gx, ...), blockIdx.y = slice (and every gridDim.y after it),
// blockIdx.z = window of 4096 / NQ levels (32 KiB of bins).  part[s][j][NQ][gx]
static const int kFermiBins = 4096;
template <class Src, int NQ>
__global__ __launch_bounds__(256) void k_kubo_fermi(const Src src, const PlaneArgs P, const int nb, const double* __restrict__ mu,
                                                    const int nmu, double* __restrict__ part) {
    constexpr int WIN = kFermiBins / NQ;
    __shared__ double bins[NQ][WIN];
    __shared__ double tw[NQ][256];
    __shared__ int tb[256];
    for (int s = blockIdx.y; s < P.nslice; s += gridDim.y) {   // (slices beyond the grid's y limit: the next pass)
        const int w0 = blockIdx.z * WIN, wn = min(WIN, nmu - w0);
        for (int j = threadIdx.x; j < WIN; j += 256)
#pragma unroll
            for (int c = 0; c < NQ; ++c) bins[c][j] = 0.0;
        const int per = (wn + 255) / 256;
        const int lo = threadIdx.x * per, hi = min(wn, lo + per);
        const int64_t total = P.nplane * nb;
        for (int64_t t0 = (int64_t)blockIdx.x * 256; t0 < total; t0 += (int64_t)gridDim.x * 256) {
            const int64_t it = t0 + threadIdx.x;
            int bin = -1;
            double w[NQ];
#pragma unroll
            for (int c = 0; c < NQ; ++c) w[c] = 0.0;
            if (it < total) {
                const int64_t p = it / nb;
                const int band = (int)(it - p * nb);
                int ii[3];
                const int64_t idx = plane_point(P, s, p, ii);
                double e;
                src.band(P, ii, idx, band, e, w);
                int l = 0, r = nmu;                  // first j with mu[j] >= e (nmu: above every level; NaN: nowhere)
                while (l < r) {
                    const int m = (l + r) >> 1;
                    if (mu[m] < e) l = m + 1;
                    else r = m;
                }
                bin = e == e ? l - w0 : -1;
            }
            __syncthreads();                         // the previous tile's items are consumed
            tb[threadIdx.x] = bin;
#pragma unroll
            for (int c = 0; c < NQ; ++c) tw[c][threadIdx.x] = w[c];
            __syncthreads();
            for (int q = 0; q < 256; ++q) {
                const int b = tb[q];
                if (b >= lo && b < hi)
#pragma unroll
                    for (int c = 0; c < NQ; ++c) bins[c][b] += tw[c][q];
            }
        }
        __syncthreads();
        for (int j = threadIdx.x; j < wn; j += 256)
#pragma unroll
            for (int c = 0; c < NQ; ++c) part[(((int64_t)s * nmu + w0 + j) * NQ + c) * gridDim.x + blockIdx.x] = bins[c][j];
        __syncthreads();                                           // (bins are reused by the next slice)
    }
}

template <int NQ, class Src>
static int kubo_fermi_launch(tbk_ctx* ctx, const Src& src, const PlaneArgs& P, int n, const double* mu_dev, int nmu, int gx, double* part) {
    const unsigned nwin = (unsigned)((nmu + kFermiBins / NQ - 1) / (kFermiBins / NQ));
    hipLaunchKernelGGL((k_kubo_fermi<Src, NQ>), dim3(gx, (unsigned)std::min(P.nslice, 65535), nwin), dim3(256), 0, ctx->stream, src, P, n,
                       mu_dev, nmu, part);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

// out[r] = sum_g part[r][g] in a fixed order (one workgroup per row)
static __global__ __launch_bounds__(256) void k_kubo_rows(const double* __restrict__ part, const int gx, double* __restrict__ out) {
    __shared__ double red[4];
    const double* p = part + (int64_t)blockIdx.x * gx;
    double acc = 0.0;
    for (int g = threadIdx.x; g < gx; g += 256) acc += p[g];
    const double t = block_sum(acc, red);
    if (threadIdx.x == 0) out[blockIdx.x] = t;
}

// The same sum over the other layout, part[g][row] (the frequency sweeps of tbk_pairs.h, tbk_chi.hip, tbk_occ.hip):
// acc[row] (+)= inv sum_g part[g][row], the groups in index order.  k_group_rows is one workgroup per row, for many groups and few
// rows (G up to 1024, rows = sums x frequencies); k_group_rows_lanes is one LANE per row, for the density matrix's up to 2^23 rows of
// at most 512 groups, where a workgroup per row would be nearly idle.  Its rows may be scattered: row r of part goes to
// acc[(r / run) stride + r % run] -- runs of `run` rows that lie `stride` apart in acc (the Green's function's launch tiles of a few
// frequencies times a part of the lattice vectors); run = nrows is the contiguous case, with no division.
static __global__ __launch_bounds__(256) void k_group_rows(const double* __restrict__ part, const int G, const int64_t nrows, const double inv,
                                                           const int accumulate, double* __restrict__ acc) {
    __shared__ double red[4];
    double s = 0.0;
    for (int g = threadIdx.x; g < G; g += 256) s += part[(int64_t)g * nrows + blockIdx.x];
    const double t = block_sum(s, red);
    if (threadIdx.x == 0) acc[blockIdx.x] = accumulate ? acc[blockIdx.x] + t * inv : t * inv;
}
static __global__ __launch_bounds__(256) void k_group_rows_lanes(const double* __restrict__ part, const int G, const int64_t nrows,
                                                                 const int64_t run, const int64_t stride, const int accumulate,
                                                                 double* __restrict__ acc) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= nrows) return;
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += part[(int64_t)g * nrows + row];
    const int64_t blk = run == nrows ? 0 : row / run;              // (uniform over the launch)
    double* a = acc + blk * stride + (row - blk * run);
    *a = accumulate ? *a + s : s;
}

static int kubo_rows_launch(tbk_ctx* ctx, const double* part, int gx, int64_t nrows, double* rows) {
    hipLaunchKernelGGL(k_kubo_rows, dim3((unsigned)nrows), dim3(256), 0, ctx->stream, part, gx, rows);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}
// sums = the nrows doubles at rows, on the host
static int kubo_to_host(tbk_ctx* ctx, const double* rows, int64_t nrows, std::vector<double>& sums) {
    sums.resize((size_t)nrows);
    TBK_HIP(hipMemcpyAsync(sums.data(), rows, (size_t)nrows * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    return TBK_OK;
}
// the tail of every mesh call: rows[r] = sum_g part[r][g] under the caller's label, then sums = rows on the host
static int kubo_rows_to_host(tbk_ctx* ctx, const char* label, const double* part, int gx, int64_t nrows, double* rows,
                             std::vector<double>& sums) {
    {
        ProfScope ps(ctx, label);
        int rc = kubo_rows_launch(ctx, part, gx, nrows, rows);
        if (rc) return rc;
    }
    return kubo_to_host(ctx, rows, nrows, sums);
}

// Plane sums: src.plane(P, s, p, ch, w) gives the NQ values of channel ch at plane point p of slice s; row = s * nch + ch
// (blockIdx.y and every gridDim.y after it), blockIdx.x = g of gx (points g 256 + t, then every gx 256 after it), one block_sum
// per quantity.  part[row][NQ][gx]
template <class Src, int NQ>
__global__ __launch_bounds__(256) void k_kubo_plane(const Src src, const PlaneArgs P, const int nch, const int64_t nrows,
                                                    double* __restrict__ part) {
    __shared__ double red[NQ][4];
    for (int64_t row = blockIdx.y; row < nrows; row += gridDim.y) {   // (rows beyond the grid's y limit: the next pass)
        const int s = (int)(row / nch), ch = (int)(row - (int64_t)s * nch);
        double acc[NQ];
#pragma unroll
        for (int c = 0; c < NQ; ++c) acc[c] = 0.0;
        for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < P.nplane; p += (int64_t)gridDim.x * 256) {
            double w[NQ];
            src.plane(P, s, p, ch, w);
#pragma unroll
            for (int c = 0; c < NQ; ++c) acc[c] += w[c];
        }
#pragma unroll
        for (int c = 0; c < NQ; ++c) {
            const double t = block_sum(acc[c], red[c]);
            if (threadIdx.x == 0) part[(row * NQ + c) * gridDim.x + blockIdx.x] = t;
        }
        __syncthreads();                                              // (red is reused by the next row)
    }
}
template <int NQ, class Src>
static int kubo_plane_launch(tbk_ctx* ctx, const Src& src, const PlaneArgs& P, int nch, int64_t nrows, int gx, double* part) {
    hipLaunchKernelGGL((k_kubo_plane<Src, NQ>), dim3(gx, (unsigned)std::min<int64_t>(nrows, 65535)), dim3(256), 0, ctx->stream, src, P,
                       nch, nrows, part);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

// Thermal scan (kT > 0) over the per-band records rec[1 + NR][nb][npts]: E, then the policy's NR records.  Workgroup (tile of
// kThermalTile levels, k-group g, slice s): lane t takes level j = tile + t and walks the records of the plane points
// [g nplane / G, (g + 1) nplane / G) of slice s (Pol::kWhole: the plane is the whole mesh in k_uniform_mesh order), every band of
// a point in order; a record's address depends on the workgroup and the loop alone, so it is read as a wave-uniform value.  The
// policy's add(e, r, u, kT, ikT, acc) is the arithmetic of one (record, level) on its NQ sums.  part[s][j][NQ][G]
static const int kThermalTile = 256;                     // levels per workgroup (one per lane)
template <class Pol>
__global__ __launch_bounds__(256) void k_kubo_thermal(const PlaneArgs P, const int nb, const double* __restrict__ rec,
                                                      const double* __restrict__ mu, const int nmu, const double kT, const int G,
                                                      double* __restrict__ part) {
    constexpr int NR = Pol::NR, NQ = Pol::NQ;
    const int base = blockIdx.x * kThermalTile;
    if (base + (int)(threadIdx.x & ~63u) >= nmu) return;            // a wavefront without a level (uniform)
    const int j = base + threadIdx.x, g = blockIdx.y;
    const double u = j < nmu ? mu[j] : 0.0;
    const double ikT = 1.0 / kT;
    const int64_t stride = (int64_t)nb * P.npts;
    const int64_t p0 = (int64_t)g * P.nplane / G, p1 = (int64_t)(g + 1) * P.nplane / G;
    for (int s = blockIdx.z; s < P.nslice; s += gridDim.z) {
        double acc[NQ];
#pragma unroll
        for (int c = 0; c < NQ; ++c) acc[c] = 0.0;
        for (int64_t p = p0; p < p1; ++p) {
            int ii[3];
            const int64_t idx = Pol::kWhole ? p : plane_point(P, s, p, ii);
            for (int b = 0; b < nb; ++b) {
                const int64_t i = (int64_t)b * P.npts + idx;
                const double e = rec[i];
                double r[NR];
#pragma unroll
                for (int c = 0; c < NR; ++c) r[c] = rec[(1 + c) * stride + i];
                Pol::add(e, r, u, kT, ikT, acc);
            }
        }
        if (j < nmu)
#pragma unroll
            for (int c = 0; c < NQ; ++c) part[(((int64_t)s * nmu + j) * NQ + c) * G + g] = acc[c];
    }
}
template <class Pol>
static int kubo_thermal_launch(tbk_ctx* ctx, const PlaneArgs& P, int n, const double* rec, const double* mu_dev, int nmu, double kT,
                               int G, double* part) {
    const unsigned ntile = (unsigned)((nmu + kThermalTile - 1) / kThermalTile);
    hipLaunchKernelGGL(k_kubo_thermal<Pol>, dim3(ntile, (unsigned)G, (unsigned)std::min(P.nslice, 65535)), dim3(256), 0, ctx->stream, P, n,
                       rec, mu_dev, nmu, kT, G, part);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

// ---------------------------------------------------------------- n != 2: contraction of the solver's eigenvectors
// A policy Q is what a (point, band b) lane keeps of its pairs (b, m), P_bm = Im V^a_bm V^b_mb and Delta = E_b - E_m:
//   pair()    adds one pair (set: the call sums a band set -- b in occ, m outside, no degeneracy rule)
//   band()    stores the lane's per-band result at i = b nfull + first + ik
//   share()   stores the lane's NSET doubles of a band set's sums; set() stores a point's sums over b of them at i = first + ik
//   kLabel    the ProfScope labels of k_kubo_lds, k_kubo_wsp, k_kubo_contract, k_kubo_occ_sum
// CurvQ (below; tbk_curv.hip and tbk_transport.hip): Omega.  OrbQ (tbk_orbmag.hip): m and Omega, or (LC, IC, Omega_occ).
// A policy with kSpin = true (SpinQ, tbk_curv.hip; section 15) replaces the first operator d_{d0} H by the spin current
// J = (Sigma_s d_{d0} H + d_{d0} H Sigma_s) / 2: its Out carries the SpinVec `spin`, and its member type Contract names the policy
// whose k_kubo_contract / k_kubo_occ_sum serve it (they see matrix elements only).  The choice is made at compile time
// (kubo_spin<Q>): a policy without the member compiles to what it was.
struct CurvQ {
    static constexpr int NSET = 1;
    static constexpr const char* kLabel[4] = {"curv_lds", "curv_wsp", "curv_contract", "curv_occ_sum"};
    struct Out {
        double* om;   // per band [n][nfull], manifold [nfull]
        double* ev;   // per band [n][nfull], nullable
    };
    double acc = 0.0;
    __device__ __forceinline__ void pair(const double pr, const double de, double, double, bool) { acc += pr / (de * de); }
    __device__ __forceinline__ void band(const Out& o, const int64_t i, const double eb) const {
        o.om[i] = -2.0 * acc;
        if (o.ev) o.ev[i] = eb;
    }
    __device__ __forceinline__ void share(double* s, double) const { s[0] = -2.0 * acc; }
    static __device__ __forceinline__ void set(const Out& o, const int64_t i, int64_t, const double (&s)[1]) { o.om[i] = s[0]; }
};

template <class Q, class = void>
struct kubo_spin : std::false_type {};
template <class Q>
struct kubo_spin<Q, std::void_t<decltype(Q::kSpin)>> : std::bool_constant<Q::kSpin> {};
template <class Q, class = void>
struct kubo_contract_policy {
    using type = Q;
};
template <class Q>
struct kubo_contract_policy<Q, std::void_t<typename Q::Contract>> {
    using type = typename Q::Contract;
};

// ---------------------------------------------------------------- the rotation into the eigenbasis in LDS (up to 32 states)
// What every kernel that holds U and d H of np points in LDS shares (k_kubo_lds; k_qgt_lds; tbk_pairs.h's pair_lds_ops for k_opt_pairs
// and k_sh_pairs): matrices of n^2 per point, point p at offset p n^2, one element per lane and step of 256.  Each kernel keeps its
// own buffer layout and says which buffers D, T and U are, and passes nn = n^2 beside n (formed once, in the kernel: k_kubo_lds
// compiles to 16 VGPRs more where these functions form it again).
// U[p][b][i] = component i of eigenvector b of point ik0 + p, from evec[b][nk][n]; also(e) runs for every element e the lane loads
template <class Also>
__device__ __forceinline__ void kubo_lds_load(cd* U, const cd* __restrict__ evec, const int64_t nk, const int64_t ik0, const int np,
                                              const int n, const int nn, const Also& also) {
    for (int e = threadIdx.x; e < np * nn; e += 256) {
        const int p = e / nn, r = e - p * nn, b = r / n, i = r - b * n;
        U[e] = evec[((int64_t)b * nk + ik0 + p) * n + i];
        also(e);
    }
}
// T = D U^T
__device__ __forceinline__ void kubo_lds_dut(cd* T, const cd* D, const cd* U, const int np, const int n, const int nn) {
    for (int e = threadIdx.x; e < np * nn; e += 256) {
        const int p = e / nn, r = e - p * nn, i = r / n, mm = r - i * n;
        const cd* dr = D + p * nn + i * n;
        const cd* um = U + p * nn + mm * n;
        cd acc{0.0, 0.0};
        for (int j = 0; j < n; ++j) cfma(acc, dr[j], um[j]);
        T[e] = acc;
    }
}
// D := conj(U) T   (reads U, T only)
__device__ __forceinline__ void kubo_lds_ut(cd* D, const cd* U, const cd* T, const int np, const int n, const int nn) {
    for (int e = threadIdx.x; e < np * nn; e += 256) {
        const int p = e / nn, r = e - p * nn, b = r / n, mm = r - b * n;
        const cd* ub = U + p * nn + b * n;
        const cd* tc = T + p * nn + mm;
        cd acc{0.0, 0.0};
        for (int i = 0; i < n; ++i) cfmac(acc, ub[i], tc[i * n]);
        D[e] = acc;
    }
}
// D := conj(U) D U^T through T, behind a barrier of the caller's; D is ready for every lane on return
__device__ __forceinline__ void kubo_lds_rotate(cd* D, cd* T, const cd* U, const int np, const int n, const int nn) {
    kubo_lds_dut(T, D, U, np, n, nn);
    __syncthreads();
    kubo_lds_ut(D, U, T, np, n, nn);
    __syncthreads();
}

// Up to 32 states: ONE kernel, P = min(64, 4096 / (4 n^2)) points per workgroup, everything of a point in LDS (64 KiB):
// U (its eigenvectors, read once from HBM), D = d_{d0} H and X = d_{d1} H (built from the non-empty slots), T = D U^T, then
// D := V^{d0} = conj(U) T, T := X U^T, and one lane per (point, band) forms V^{d1} from T on the fly and feeds Q.
// Nothing but Q's results is written.
#define KUBO_LDS_CD 4096
static inline int kubo_lds_points(int n) { return std::max(1, std::min(64, KUBO_LDS_CD / (4 * n * n))); }
template <class Q>
__global__ __launch_bounds__(256) void k_kubo_lds(const ModelView mv, const double* __restrict__ k, const cd* __restrict__ evec,
                                                  const double* __restrict__ eval, const int64_t nk, const int d0, const int d1,
                                                  const int P, const int* __restrict__ occ, const int64_t first, const int64_t nfull,
                                                  const typename Q::Out out) {
    __shared__ cd L[KUBO_LDS_CD];
    const int n = mv.nsta, nn = n * n;
    const int64_t ik0 = (int64_t)blockIdx.x * P;
    const int np = (int)std::min<int64_t>(P, nk - ik0);
    cd* U = L;
    cd* D = L + P * nn;
    cd* T = L + 2 * P * nn;
    cd* X = L + 3 * P * nn;
    kubo_lds_load(U, evec, nk, ik0, np, n, nn, [&](const int e) {
        D[e] = cd{0.0, 0.0};
        X[e] = cd{0.0, 0.0};
    });
    __syncthreads();
    for (int e = threadIdx.x; e < np * mv.nnz; e += 256) {
        const int p = e / mv.nnz;
        const int4 z4 = mv.nz[e - p * mv.nnz];
        const int a = z4.x & 0xffff, b = z4.x >> 16;
        double kk[4];
        cd z[4];
        k_phases(mv, k, ik0 + p, kk, z);
        cd h, v0, v1;
        dham_terms(mv, a, b, z4.y, z4.z, kk, z, d0, d1, h, v0, v1);
        D[p * nn + a * n + b] = v0;
        D[p * nn + b * n + a] = cconj(v0);
        X[p * nn + a * n + b] = v1;
        X[p * nn + b * n + a] = cconj(v1);
    }
    __syncthreads();
    if constexpr (kubo_spin<Q>::value) {                           // J = (Sigma_s D + D Sigma_s) / 2 into the still-free T; the two
        for (int e = threadIdx.x; e < np * nn; e += 256) {         // regions then swap roles: one barrier, no copy back
            const int p = e / nn, r = e - p * nn, i = r / n, j = r - i * n;
            const cd* dp = D + p * nn;
            T[e] = spin_apply(out.spin, i, j, dp[r], dp[(i ^ 1) * n + j], dp[i * n + (j ^ 1)]);
        }
        cd* t = D;
        D = T;
        T = t;
        __syncthreads();
    }
    kubo_lds_rotate(D, T, U, np, n, nn);                            // D := V^{d0}
    kubo_lds_dut(T, X, U, np, n, nn);                               // T := X U^T
    __syncthreads();
    double* share = (double*)X;                                    // (X is dead: the band shares, NSET np n <= 2 P n^2 doubles)
    for (int e = threadIdx.x; e < np * n; e += 256) {
        const int p = e / n, b = e - p * n;
        const int64_t ik = ik0 + p;
        const double eb = eval[(int64_t)b * nk + ik];
        const cd* ub = U + p * nn + b * n;
        const cd* va = D + p * nn + b * n;
        const cd* tp = T + p * nn;
        Q q;
        if (!occ || occ[b]) {
            for (int mm = 0; mm < n; ++mm) {
                if (mm == b) continue;
                const double em = eval[(int64_t)mm * nk + ik];
                const double de = eb - em;
                if (occ ? occ[mm] != 0 : kubo_degenerate(de, eb, em)) continue;
                cd vb{0.0, 0.0};
                for (int i = 0; i < n; ++i) cfmac(vb, ub[i], tp[i * n + mm]);
                const cd a = va[mm];
                q.pair(a.y * vb.x - a.x * vb.y, de, eb, em, occ != nullptr);   // Im V^a_bm V^b_mb = Im V^a_bm conj(V^b_bm)
            }
        }
        if (occ) q.share(share + Q::NSET * e, eb);
        else q.band(out, (int64_t)b * nfull + first + ik, eb);
    }
    if (occ) {
        __syncthreads();
        for (int p = threadIdx.x; p < np; p += 256) {
            double s[Q::NSET];
#pragma unroll
            for (int c = 0; c < Q::NSET; ++c) s[c] = 0.0;
            for (int b = 0; b < n; ++b)
#pragma unroll
                for (int c = 0; c < Q::NSET; ++c) s[c] += share[Q::NSET * (p * n + b) + c];
            Q::set(out, first + ik0 + p, nfull, s);
        }
    }
}

// 33..2048 states: W^d[ik][i][m] = sum_j d_d H_ij u_m[j] from the non-empty slots only (ModelView.nz; no dense d_d H), wt[ik][2][n][n].
// Workgroup (point, block of 256 columns); lane m owns column m of both W^d -- every slot adds to two entries of each, and no other
// lane touches them: no atomics, a fixed order.  The slot values (both directions) are computed once per point and staged in LDS.
//
// SPIN (section 15): the first direction's matrix is W^J = (Sigma_s (d_{d0} H U^T) + d_{d0} H (Sigma_s U^T)) / 2.  Sigma_s mixes only rows
// 2o and 2o + 1 of the lane's own column, so a slot (a, b) adds v0 ((Sigma_s u)[b] + Sigma_aa u[b]) / 2 to row a and
// Sigma_{a^1,a} v0 u[b] / 2 to row a^1 (and likewise for its conjugate half): still one lane per column, one read-modify-write after
// the other in slot order -- no third buffer, no atomics, the same bits every call.
template <bool SPIN>
__device__ __forceinline__ void kubo_wsp_body(const ModelView& mv, const double* __restrict__ k, const cd* __restrict__ evec,
                                              const int64_t nk, const int d0, const int d1, cd* __restrict__ wt, const SpinVec& sv) {
    __shared__ int sab[256];
    __shared__ cd sv0[256], sv1[256];
    const int n = mv.nsta;
    const int64_t ik = blockIdx.x, nn = (int64_t)n * n;
    const int m = blockIdx.y * 256 + threadIdx.x;
    const bool live = m < n;
    cd* w0 = wt + 2 * ik * nn;
    cd* w1 = w0 + nn;
    if (live)
        for (int i = 0; i < n; ++i) {
            w0[(int64_t)i * n + m] = cd{0.0, 0.0};
            w1[(int64_t)i * n + m] = cd{0.0, 0.0};
        }
    double kk[4];
    cd z[4];
    k_phases(mv, k, ik, kk, z);
    const cd* u = evec + ((int64_t)(live ? m : 0) * nk + ik) * n;
    for (int q0 = 0; q0 < mv.nnz; q0 += 256) {
        __syncthreads();
        if (q0 + (int)threadIdx.x < mv.nnz) {
            const int4 z4 = mv.nz[q0 + threadIdx.x];
            cd h;
            dham_terms(mv, z4.x & 0xffff, z4.x >> 16, z4.y, z4.z, kk, z, d0, d1, h, sv0[threadIdx.x], sv1[threadIdx.x]);
            sab[threadIdx.x] = z4.x;
        }
        __syncthreads();
        const int cnt = min(256, mv.nnz - q0);
        if (!live) continue;
        for (int q = 0; q < cnt; ++q) {
            const int a = sab[q] & 0xffff, b = sab[q] >> 16;
            const cd v0 = sv0[q], v1 = sv1[q], ub = u[b];
            cd* pa0 = w0 + (int64_t)a * n + m;
            cd* pa1 = w1 + (int64_t)a * n + m;
            cd t0 = *pa0, t1 = *pa1;
            if constexpr (SPIN) cfma(t0, v0, cscale(cadd(spin_vec(sv, u, b), cmul(spin_elem(sv, a & 1, a & 1), ub)), 0.5));
            else cfma(t0, v0, ub);
            cfma(t1, v1, ub);
            *pa0 = t0;
            *pa1 = t1;
            if constexpr (SPIN) {
                cd* px = w0 + (int64_t)(a ^ 1) * n + m;
                cd x = *px;
                cfma(x, cmul(spin_elem(sv, (a & 1) ^ 1, a & 1), v0), cscale(ub, 0.5));
                *px = x;
            }
            if (a != b) {
                const cd ua = u[a];
                cd* pb0 = w0 + (int64_t)b * n + m;
                cd* pb1 = w1 + (int64_t)b * n + m;
                cd s0 = *pb0, s1 = *pb1;
                if constexpr (SPIN) cfma(s0, cconj(v0), cscale(cadd(spin_vec(sv, u, a), cmul(spin_elem(sv, b & 1, b & 1), ua)), 0.5));
                else cfma(s0, cconj(v0), ua);
                cfma(s1, cconj(v1), ua);
                *pb0 = s0;
                *pb1 = s1;
                if constexpr (SPIN) {
                    cd* px = w0 + (int64_t)(b ^ 1) * n + m;
                    cd x = *px;
                    cfma(x, cmul(spin_elem(sv, (b & 1) ^ 1, b & 1), cconj(v0)), cscale(ua, 0.5));
                    *px = x;
                }
            }
        }
    }
}
static __global__ __launch_bounds__(256) void k_kubo_wsp(const ModelView mv, const double* __restrict__ k, const cd* __restrict__ evec,
                                                         const int64_t nk, const int d0, const int d1, cd* __restrict__ wt) {
    kubo_wsp_body<false>(mv, k, evec, nk, d0, d1, wt, SpinVec{});
}
// (a template so that only a unit that launches it holds a copy)
template <class Q>
__global__ __launch_bounds__(256) void k_kubo_wsp_spin(const ModelView mv, const double* __restrict__ k, const cd* __restrict__ evec,
                                                       const int64_t nk, const int d0, const int d1, cd* __restrict__ wt,
                                                       const SpinVec sv) {
    kubo_wsp_body<true>(mv, k, evec, nk, d0, d1, wt, sv);
}

// 33..2048 states, one lane per (ik, band b) on k_kubo_wsp's W^d: V^d_{b,m} = sum_i conj(u_b[i]) W^d[i][m], fed to Q as in k_kubo_lds.
// A band set's shares go to tmp[ik][b][NSET], summed per point by k_kubo_occ_sum.
template <class Q>
__global__ __launch_bounds__(256) void k_kubo_contract(const cd* __restrict__ evec, const double* __restrict__ eval,
                                                       const cd* __restrict__ wt, const int64_t nk, const int n,
                                                       const int* __restrict__ occ, const int64_t first, const int64_t nfull,
                                                       const typename Q::Out out, double* __restrict__ tmp) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nk * n) return;
    const int64_t ik = idx / n;
    const int b = (int)(idx - ik * n);
    const int64_t nn = (int64_t)n * n;
    const cd* u = evec + ((int64_t)b * nk + ik) * n;
    const cd* w0 = wt + (2 * ik) * nn;
    const cd* w1 = w0 + nn;
    const double eb = eval[(int64_t)b * nk + ik];
    Q q;
    if (!occ || occ[b]) {
        for (int m = 0; m < n; ++m) {
            if (m == b) continue;
            const double em = eval[(int64_t)m * nk + ik];
            const double de = eb - em;
            if (occ ? occ[m] != 0 : kubo_degenerate(de, eb, em)) continue;
            cd va{0.0, 0.0}, vb{0.0, 0.0};
            for (int i = 0; i < n; ++i) {
                cfmac(va, u[i], w0[(int64_t)i * n + m]);
                cfmac(vb, u[i], w1[(int64_t)i * n + m]);
            }
            q.pair(va.y * vb.x - va.x * vb.y, de, eb, em, occ != nullptr);   // Im V^a_bm V^b_mb = Im V^a_bm conj(V^b_bm)
        }
    }
    if (occ) q.share(tmp + Q::NSET * idx, eb);
    else q.band(out, (int64_t)b * nfull + first + ik, eb);
}

template <class Q>
__global__ __launch_bounds__(256) void k_kubo_occ_sum(const double* __restrict__ tmp, const int64_t nk, const int n, const int64_t first,
                                                      const int64_t nfull, const typename Q::Out out) {
    const int64_t ik = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (ik >= nk) return;
    double s[Q::NSET];
#pragma unroll
    for (int c = 0; c < Q::NSET; ++c) s[c] = 0.0;
    for (int b = 0; b < n; ++b)
#pragma unroll
        for (int c = 0; c < Q::NSET; ++c) s[c] += tmp[Q::NSET * (ik * n + b) + c];
    Q::set(out, first + ik, nfull, s);
}

// ---------------------------------------------------------------- host side: checks and mesh set-up
// the argument checks of a (dir0, dir1) quantity `what`; mask (n entries) = 1 for the bands of occ, empty without occ
static int kubo_occ_mask(const char* fn, tbk_model* m, const int32_t* occ, int nocc, std::vector<int>& mask) {
    const int n = m->nsta;
    mask.clear();
    if (occ) {
        TBK_REQUIRE(nocc >= 1 && nocc <= n, TBK_EINVAL, "%s: nocc=%d (1..%d)", fn, nocc, n);
        mask.assign(n, 0);
        for (int i = 0; i < nocc; ++i) {
            TBK_REQUIRE(occ[i] >= 0 && occ[i] < n, TBK_EINVAL, "%s: occ[%d]=%d outside [0, %d)", fn, i, occ[i], n);
            TBK_REQUIRE(!mask[occ[i]], TBK_EINVAL, "%s: band %d appears twice in occ", fn, occ[i]);
            mask[occ[i]] = 1;
        }
    } else {
        TBK_REQUIRE(nocc == 0, TBK_EINVAL, "%s: nocc=%d without occ", fn, nocc);
    }
    return TBK_OK;
}
static int kubo_check(const char* fn, const char* what, tbk_model* m, int dir0, int dir1, const int32_t* occ, int nocc,
                      std::vector<int>& mask) {
    TBK_REQUIRE(m, TBK_EINVAL, "%s: null model", fn);
    TBK_REQUIRE(m->dim_k >= 2, TBK_EINVAL, "%s: the %s needs dim_k >= 2 (the model has %d)", fn, what, m->dim_k);
    TBK_REQUIRE(dir0 >= 0 && dir0 < m->dim_k && dir1 >= 0 && dir1 < m->dim_k && dir0 != dir1, TBK_EINVAL,
                "%s: dirs (%d, %d) must be two different axes in [0, %d)", fn, dir0, dir1, m->dim_k);
    return kubo_occ_mask(fn, m, occ, nocc, mask);
}
// the checks of the Fermi levels of a mesh call, in the order its other checks fall between them: their number (min_levels..8192),
// the temperature (positive: kT > 0, else kT >= 0), every level finite
static int kubo_levels_check(const char* fn, int nmu, const double* mu, int min_levels) {
    TBK_REQUIRE(nmu >= min_levels && nmu <= 8192 && (nmu == 0 || mu), TBK_EINVAL, "%s: nmu=%d (%d..8192 levels)", fn, nmu, min_levels);
    return TBK_OK;
}
static int kubo_kt_check(const char* fn, double kT, bool positive) {
    TBK_REQUIRE(std::isfinite(kT) && (positive ? kT > 0.0 : kT >= 0.0), TBK_EINVAL, "%s: kT must be finite and %s 0", fn,
                positive ? ">" : ">=");
    return TBK_OK;
}
static int kubo_levels_finite(const char* fn, int nmu, const double* mu) {
    for (int j = 0; j < nmu; ++j) TBK_REQUIRE(std::isfinite(mu[j]), TBK_EINVAL, "%s: Fermi level %d is not finite", fn, j);
    return TBK_OK;
}

// the checks that the mesh sweeps share, each where the caller's order of checks has it: the dimension of the mesh; npts = its
// points; the frequencies (1..kKuboOmegaMax, finite) and eta; kT and the Fermi level
static const int kKuboOmegaMax = 65536;
static int kubo_mesh_dim(const char* fn, int dk) {
    TBK_REQUIRE(dk >= 1 && dk <= 3, TBK_EINVAL, "%s: dim_k=%d (meshes of 1, 2 or 3 dimensions)", fn, dk);
    return TBK_OK;
}
static int kubo_mesh_points(const char* fn, int dk, const int32_t* mesh, int64_t& npts) {
    npts = 1;
    for (int d = 0; d < dk; ++d) {
        TBK_REQUIRE(mesh[d] >= 1, TBK_EINVAL, "%s: mesh[%d]=%d", fn, d, mesh[d]);
        npts *= mesh[d];
    }
    return TBK_OK;
}
static int kubo_omega_check(const char* fn, int nomega, const double* omega, double eta) {
    TBK_REQUIRE(nomega >= 1 && nomega <= kKuboOmegaMax, TBK_EINVAL, "%s: nomega=%d (1..%d frequencies)", fn, nomega, kKuboOmegaMax);
    for (int j = 0; j < nomega; ++j) TBK_REQUIRE(std::isfinite(omega[j]), TBK_EINVAL, "%s: frequency %d is not finite", fn, j);
    TBK_REQUIRE(std::isfinite(eta) && eta > 0.0, TBK_EINVAL, "%s: eta must be finite and > 0", fn);
    return TBK_OK;
}
static int kubo_occupation_check(const char* fn, double kT, double mu) {
    int rc = kubo_kt_check(fn, kT, false);
    if (rc) return rc;
    TBK_REQUIRE(std::isfinite(mu), TBK_EINVAL, "%s: the Fermi level must be finite", fn);
    return TBK_OK;
}

// a mesh of dk = 1, 2 or 3 dimensions as one "plane": every point, in k_uniform_mesh order
static int kubo_whole_mesh(const char* fn, const int32_t* mesh, int dk, PlaneArgs& P) {
    P = PlaneArgs{};
    int rc = kubo_mesh_points(fn, std::min(dk, 3), mesh, P.npts);
    if (rc) return rc;
    for (int d = 0; d < 3; ++d) P.N[d] = d < dk ? mesh[d] : 1;
    P.da = 0;
    P.db = dk > 1 ? 1 : 0;
    P.dc = -1;
    P.nplane = P.npts;
    P.nslice = 1;
    return TBK_OK;
}
// the (dir0, dir1) planes of a mesh of dim_k = 2 or 3 dimensions (checked by the caller)
static int kubo_planes(const char* fn, const int32_t* mesh, int dir0, int dir1, int dk, PlaneArgs& P) {
    int rc = kubo_whole_mesh(fn, mesh, dk, P);
    if (rc) return rc;
    P.da = dir0;
    P.db = dir1;
    P.dc = dk == 3 ? 3 - dir0 - dir1 : -1;
    P.nplane = (int64_t)P.N[dir0] * P.N[dir1];
    P.nslice = P.dc >= 0 ? P.N[P.dc] : 1;
    return TBK_OK;
}

// mus = the levels in the order ord: ascending (ties by index) when `sorted`, else as given
static void kubo_levels(const double* mu, int nmu, bool sorted, std::vector<int>& ord, std::vector<double>& mus) {
    ord.resize(nmu);
    std::iota(ord.begin(), ord.end(), 0);
    if (sorted) std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return mu[x] < mu[y]; });
    mus.resize(nmu);
    for (int j = 0; j < nmu; ++j) mus[j] = mu[ord[j]];
}

// workgroups per row of the plane sums and per (slice, level, quantity) of the Fermi scan, k-groups of the thermal scan: functions of
// the mesh shape, n, nmu, nq alone
static inline int kubo_plane_gx(const PlaneArgs& P) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((P.nplane + 2047) / 2048, 1024));
}
static inline int kubo_fermi_gx(const PlaneArgs& P, int n, int nmu, int nq) {
    const int64_t tiles = (P.nplane * n + 255) / 256;
    const int64_t cap = std::max<int64_t>(1, ((int64_t)1 << 22) / ((int64_t)P.nslice * nmu * nq));
    return (int)std::max<int64_t>(1, std::min<int64_t>({(tiles + 7) / 8, 512, cap}));
}
static inline int kubo_thermal_groups(const PlaneArgs& P, int n, int nmu, int nq) {
    const int64_t cap = std::max<int64_t>(1, ((int64_t)1 << 22) / ((int64_t)P.nslice * nmu * nq));
    return (int)std::max<int64_t>(1, std::min<int64_t>({(P.nplane * n + 1023) / 1024, 1024, cap}));
}

// ---------------------------------------------------------------- host side: a call's workspace
// The device buffers of one call, carved from the context's scratch block: add(p, bytes) registers the buffer of pointer p once
// (0 bytes: not wanted), kubo_carve() asks for the total (256 leading bytes, every buffer at a multiple of 256) and place() sets
// the pointers (null for a buffer not wanted).  No HIP types: check/kubo_carve_check.cpp drives the arithmetic on the host alone.
struct KuboCarve {
    static const int kMax = 8;
    void* ptr[kMax];                       // where each buffer's pointer lives
    size_t off[kMax], total = 256;
    int cnt = 0;
    bool full = false;                     // a buffer beyond kMax was registered: kubo_carve fails
    template <class T>
    void add(T*& p, size_t bytes) {
        if (cnt == kMax) {
            full = true;
            return;
        }
        ptr[cnt] = &p;
        off[cnt++] = bytes ? total : 0;
        total += al256(bytes);
    }
    void place(void* base) const {
        for (int i = 0; i < cnt; ++i) {
            void* p = off[i] ? (unsigned char*)base + off[i] : nullptr;
            memcpy(ptr[i], &p, sizeof p);
        }
    }
};
static int kubo_carve(tbk_ctx* ctx, const KuboCarve& c) {
    TBK_REQUIRE(!c.full, TBK_EINVAL, "kubo_carve: more than %d buffers", KuboCarve::kMax);
    void* base = nullptr;
    int rc = tbk_ctx_scratch(ctx, c.total, &base);
    if (!rc) c.place(base);
    return rc;
}

// ---------------------------------------------------------------- host side: the chunk pipeline
// The points [0, nk) of a k list or a mesh go through the solver in chunks of a fixed length, so that the chunking -- and with it
// every result -- does not depend on the machine: at most kKuboChunkBytes of eigenvectors (a caller may shorten it further).
// KuboChunks describes a chunk's workspace: k, eigenvalues and eigenvectors of `chunk` points (vectors = false: eigenvalues only -- no
// bytes for eigenvectors, and the solver and the body get a null vector pointer), then up to three buffers of the caller (x0, x1, x2
// bytes); bytes() of scratch at `base`.
static const size_t kKuboChunkBytes = (size_t)32 << 20;
static inline int64_t kubo_chunk_len(int n, int64_t nk) {
    const int64_t chunk = std::max<int64_t>(1, (int64_t)(kKuboChunkBytes / ((size_t)n * n * sizeof(cd))));
    return std::min<int64_t>(chunk, std::max<int64_t>(nk, 1));
}
struct KuboChunks {
    int64_t chunk = 0;
    size_t off[7] = {0, 0, 0, 0, 0, 0, 0};   // of k, eigenvalues, eigenvectors, the three extra buffers, the end
    unsigned char* base = nullptr;
    KuboChunks() {}
    KuboChunks(int n, int dk, int64_t chunk_, size_t x0, size_t x1, size_t x2, bool vectors = true) : chunk(chunk_) {
        const size_t b[6] = {(size_t)chunk * dk * sizeof(double), (size_t)chunk * n * sizeof(double),
                             vectors ? (size_t)chunk * n * n * sizeof(cd) : 0, x0, x1, x2};
        for (int i = 0; i < 6; ++i) off[i + 1] = off[i] + al256(b[i]);
    }
    size_t bytes() const { return off[6]; }
    template <class T>
    T* extra(int i) const { return (T*)(base + off[3 + i]); }
};

// body(first, cnt, k, eval, evec) for every chunk [first, first + cnt): k from k_all_dev (list) or generated from `mesh`, eval[n][cnt]
// and evec[n][cnt][n] from tbk_solve_list_dev_checked, all on the device and valid until the next chunk
template <class Body>
static int kubo_for_chunks(tbk_model* m, const KuboChunks& w, const double* k_all_dev, const int32_t* mesh, int64_t nk, Body&& body) {
    double* kc = (double*)(w.base + w.off[0]);
    double* ec = (double*)(w.base + w.off[1]);
    cd* vc = w.off[3] > w.off[2] ? (cd*)(w.base + w.off[2]) : nullptr;
    for (int64_t first = 0; first < nk; first += w.chunk) {
        const int64_t cnt = std::min<int64_t>(w.chunk, nk - first);
        const double* kp = kc;
        if (mesh) {
            int rc = tbk_k_uniform_mesh_range_dev(m->ctx, m->dim_k, mesh, first, cnt, kc);
            if (rc) return rc;
        } else {
            kp = k_all_dev + first * m->dim_k;
        }
        int rc = tbk_solve_list_dev_checked(m, kp, cnt, ec, (double*)vc);
        if (rc) return rc;
        rc = body(first, cnt, kp, (const double*)ec, (const cd*)vc);
        if (rc) return rc;
    }
    return TBK_OK;
}

// The n != 2 contraction over points [0, nk) with policy Q: its workspace (W^d from 33 states, the occ mask, the band-set shares of
// the wide form) and the pipeline.  Per band Q::band's arrays at stride nk, band set (mask not empty) Q::set's.
static KuboChunks kubo_contract_chunks(int n, int dk, int64_t nk, bool manifold, int nset) {
    const int64_t chunk = kubo_chunk_len(n, nk);
    const bool wide = n > 32;
    return KuboChunks(n, dk, chunk, wide ? 2 * (size_t)chunk * n * n * sizeof(cd) : 0, (size_t)n * sizeof(int),
                      wide && manifold ? (size_t)nset * chunk * n * sizeof(double) : 0);
}
// `after(first, cnt, k, eval, evec)` runs in the same chunk body, behind the contraction, while the chunk's eigenpairs are valid.
template <class Q, class After>
static int kubo_contract(tbk_model* m, const double* k_all_dev, const int32_t* mesh, int64_t nk, int d0, int d1,
                         const std::vector<int>& mask, const KuboChunks& w, const typename Q::Out out, After&& after) {
    tbk_ctx* ctx = m->ctx;
    const int n = m->nsta;
    cd* wt = w.extra<cd>(0);
    int* occ_dev = w.extra<int>(1);
    double* tmp = w.extra<double>(2);
    const bool manifold = !mask.empty();
    const int* occ = manifold ? (const int*)occ_dev : (const int*)nullptr;
    if (manifold) TBK_HIP(hipMemcpyAsync(occ_dev, mask.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    return kubo_for_chunks(m, w, k_all_dev, mesh, nk, [&](int64_t first, int64_t cnt, const double* kp, const double* ec, const cd* vc) -> int {
        if (n <= 32) {
            const int P = kubo_lds_points(n);
            {
                ProfScope ps(ctx, Q::kLabel[0]);
                hipLaunchKernelGGL(k_kubo_lds<Q>, dim3((unsigned)((cnt + P - 1) / P)), dim3(256), 0, ctx->stream, m->view, kp, vc, ec, cnt,
                                   d0, d1, P, occ, first, nk, out);
                TBK_HIP(hipGetLastError());
            }
            return after(first, cnt, kp, ec, vc);
        }
        {
            ProfScope ps(ctx, Q::kLabel[1]);
            const dim3 grid((unsigned)cnt, (unsigned)((n + 255) / 256));
            if constexpr (kubo_spin<Q>::value)
                hipLaunchKernelGGL(k_kubo_wsp_spin<Q>, grid, dim3(256), 0, ctx->stream, m->view, kp, vc, cnt, d0, d1, wt, out.spin);
            else
                hipLaunchKernelGGL(k_kubo_wsp, grid, dim3(256), 0, ctx->stream, m->view, kp, vc, cnt, d0, d1, wt);
            TBK_HIP(hipGetLastError());
        }
        using C = typename kubo_contract_policy<Q>::type;   // (Q itself unless Q names another policy's kernels)
        const typename C::Out cout = out;
        {
            ProfScope ps(ctx, Q::kLabel[2]);
            hipLaunchKernelGGL(k_kubo_contract<C>, dim3(nblk(cnt * n)), dim3(256), 0, ctx->stream, vc, ec, (const cd*)wt, cnt, n, occ, first,
                               nk, cout, tmp);
            TBK_HIP(hipGetLastError());
        }
        if (manifold) {
            ProfScope ps(ctx, Q::kLabel[3]);
            hipLaunchKernelGGL(k_kubo_occ_sum<C>, dim3(nblk(cnt)), dim3(256), 0, ctx->stream, (const double*)tmp, cnt, n, first, nk, cout);
            TBK_HIP(hipGetLastError());
        }
        return after(first, cnt, kp, ec, vc);
    });
}
template <class Q>
static int kubo_contract(tbk_model* m, const double* k_all_dev, const int32_t* mesh, int64_t nk, int d0, int d1,
                         const std::vector<int>& mask, const KuboChunks& w, const typename Q::Out out) {
    return kubo_contract<Q>(m, k_all_dev, mesh, nk, d0, d1, mask, w, out,
                            [](int64_t, int64_t, const double*, const double*, const cd*) -> int { return TBK_OK; });
}
