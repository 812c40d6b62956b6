// tbk_kpm.h -- what the translation units of the kernel polynomial method share (tbk_kpm.hip: the operator and the single moments;
// tbk_kpm_cond.hip: the double moments of the Kubo-Bastin conductivity; tbk_kpm_series.hip: operator functions and the local Chern
// marker; tbk_kpm_eigs.hip: eigenpairs in an energy window): the operator's handle, the random-phase generator, the fixed-order
// sums, the values of the operator at a k-point, the row mapping, the sparse row product and the one Chebyshev step kernel; on the
// host the argument checks, the launch plan, the workspace carving, the start vectors and the driver of the steps; and the series
// f(H) v of tbk_kpm_series.hip, which tbk_kpm_eigs.hip filters with: its epilogue, guard and gather kernels and its driver.
// Templates and static functions: the library has no relocatable device code.  DESIGN.md sections 21 to 25.
#pragma once
#include <algorithm>
#include <cmath>
#include "tbk_internal.h"

#define KPM_NV 8            // vectors per block
#define KPM_MAX_WG 2048     // workgroups of a step (grid-stride over the row tiles beyond that)
#define KPM_MAX_SLOTS 128   // steps between two reductions of the partial sums
#define KPM_PART_BYTES ((size_t)32 << 20)   // ... and the workspace they may take

struct tbk_sparse {
    tbk_ctx* ctx = nullptr;
    int dim_k = 0, nsta = 0;
    int64_t nnz = 0;
    double gmin = 0.0, gmax = 0.0;   // Gershgorin interval
    double vbound[4] = {0.0, 0.0, 0.0, 0.0};   // >= ||dH/dk_d||_2 at every k: the largest row sum of 2 pi |amp| |(R + orb_col - orb_row)_d|
    void* blob = nullptr;            // one device allocation holding all tables
    const int64_t* row_ptr = nullptr;
    const int32_t* col = nullptr;
    const int32_t* row_of = nullptr;
    const cd* amp = nullptr;
    const int4* R = nullptr;
    const double4* orb = nullptr;
};

// val[nnz] = the values of the operator at the k-point k_dev[dim_k] (device memory), on the context's stream (tbk_kpm.hip); a model
// with dim_k = 0 needs none: its values are sp->amp
int kpm_values_at(const tbk_sparse* sp, const double* k_dev, cd* val);

static inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
static inline unsigned kpm_stream_grid(int64_t items) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + 255) / 256, 2048)); }

// element i of random-phase vector number g: a pure function of (seed, g, i)
__host__ __device__ inline uint64_t kpm_mix(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ cd kpm_random_phase(const uint64_t seed, const uint64_t g, const uint64_t i) {
    const uint64_t h = kpm_mix(kpm_mix(kpm_mix(seed) ^ g) ^ i);
    const double u = (double)(h >> 11) * 0x1.0p-53;      // [0, 1)
    double s, c;
    sincospi(2.0 * u, &s, &c);
    return cd{c, s};
}

// The sums of a workgroup's (A, B) over its rows, per vector: across the 64 / NV rows of a wavefront by shuffles, across the four
// wavefronts through LDS in a fixed order -> part[workgroup][2][NV].
template <int NV>
__device__ __forceinline__ void kpm_block_sums(double dA, double dB, double* __restrict__ part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = NV; o < 64; o <<= 1) {
        dA += __shfl_xor(dA, o);
        dB += __shfl_xor(dB, o);
    }
    __shared__ double red[4][2][NV];
    if (lane < NV) {
        red[wave][0][lane] = dA;
        red[wave][1][lane] = dB;
    }
    __syncthreads();
    if (threadIdx.x < 2 * NV) {
        const int s = threadIdx.x / NV, v = threadIdx.x % NV;
        part[(int64_t)blockIdx.x * 2 * NV + threadIdx.x] = ((red[0][s][v] + red[1][s][v]) + red[2][s][v]) + red[3][s][v];
    }
}

// body(row, v) for every row of this workgroup's tiles: a wavefront covers 64 / NV rows x NV vectors (the vector index fastest, so
// the NV lanes of a row read the same matrix entry and one contiguous 16 NV-byte segment of a vector block), a workgroup 4 x 64 / NV
// rows, and the workgroups stride over the row tiles beyond KPM_MAX_WG of them.
template <int NV, class Body>
__device__ __forceinline__ void kpm_for_rows(const int nsta, Body body) {
    constexpr int RPW = 64 / NV, RPB = 4 * RPW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, v = lane % NV, rw = lane / NV;
    const int64_t ntiles = ((int64_t)nsta + RPB - 1) / RPB;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row = tile * RPB + wave * RPW + rw;
        if (row < nsta) body(row, v);
    }
}

// sum over the entries e of the CSR row of val[e] in[col[e]][v]; each lane walks the entries of its row
template <int NV>
__device__ __forceinline__ cd kpm_row_product(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                              const cd* __restrict__ val, const cd* __restrict__ in, const int64_t row, const int v) {
    const int64_t e0 = row_ptr[row], e1 = row_ptr[row + 1];
    cd acc{0.0, 0.0};
    for (int64_t e = e0; e < e1; ++e) cfma(acc, val[e], in[(int64_t)col[e] * NV + v]);
    return acc;
}

// alpha_0 of one block of NV vectors, alpha[row][NV], and the partial sums of <alpha_0|alpha_0> (the slot of step 0).
// mode 0: random phases, vector numbers g0 + v; 1: unit vectors at states[v]; 2: src[v][nsta].  Vectors v >= nv are zero.
template <int NV>
__global__ __launch_bounds__(256) void k_kpm_init(const int nsta, const int nv, const int mode, const uint64_t seed, const uint64_t g0,
                                                  const int32_t* __restrict__ states, const cd* __restrict__ src,
                                                  cd* __restrict__ cur, double* __restrict__ part) {
    double dA = 0.0;
    kpm_for_rows<NV>(nsta, [&](const int64_t row, const int v) {
        cd x{0.0, 0.0};
        if (v < nv) {
            if (mode == 0) x = kpm_random_phase(seed, g0 + (uint64_t)v, (uint64_t)row);
            else if (mode == 1) x = cd{states[v] == row ? 1.0 : 0.0, 0.0};
            else x = src[(int64_t)v * nsta + row];
        }
        cur[row * NV + v] = x;
        dA += cabs2(x);
    });
    kpm_block_sums<NV>(dA, 0.0, part);
}

// dots[step][2][NV] = the sum over the workgroups of part[slot][workgroup][2][NV], one workgroup per step of the chunk: 256 / (2 NV)
// strided partial sums per column, each in ascending workgroup order, then added in ascending order -- a fixed shape.
template <int NV>
__global__ __launch_bounds__(256) void k_kpm_reduce(const int nwg, const double* __restrict__ part, double* __restrict__ dots) {
    constexpr int NC = 2 * NV, G = 256 / NC;
    const int c = threadIdx.x % NC, g = threadIdx.x / NC;
    const double* p = part + (int64_t)blockIdx.x * nwg * NC;
    double s = 0.0;
    for (int w = g; w < nwg; w += G) s += p[(int64_t)w * NC + c];
    __shared__ double red[G][NC];
    red[g][c] = s;
    __syncthreads();
    if (threadIdx.x < NC) {
        double t = red[0][c];
#pragma unroll
        for (int i = 1; i < G; ++i) t += red[i][c];
        dots[(int64_t)blockIdx.x * NC + c] = t;
    }
}

// val[e] = amp[e] exp(2 pi i k.(R_e + orb_col - orb_row)) for one k; VEL: also the two velocity operators,
// va[e] = 2 pi i (R_e + orb_col - orb_row)_da val[e] and vb the same along db.  A lane per entry.
__device__ __forceinline__ double kpm_pick(const double4 a, const int d) { return d == 0 ? a.x : (d == 1 ? a.y : (d == 2 ? a.z : a.w)); }
__device__ __forceinline__ int kpm_pick(const int4 a, const int d) { return d == 0 ? a.x : (d == 1 ? a.y : (d == 2 ? a.z : a.w)); }
template <bool VEL>
__global__ __launch_bounds__(256) void k_kpm_values(const int64_t nnz, const int dim_k, const int da, const int db,
                                                    const double* __restrict__ k, const int32_t* __restrict__ col,
                                                    const int32_t* __restrict__ row_of, const cd* __restrict__ amp,
                                                    const int4* __restrict__ R, const double4* __restrict__ orb, cd* __restrict__ val,
                                                    cd* __restrict__ va, cd* __restrict__ vb) {
    double kk[4] = {0.0, 0.0, 0.0, 0.0};
    for (int d = 0; d < dim_k; ++d) kk[d] = k[d];
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * 256) {
        const int4 r = R[e];
        const double4 oc = orb[col[e]], orw = orb[row_of[e]];
        double x = kk[0] * ((double)r.x + oc.x - orw.x);
        x = fma(kk[1], (double)r.y + oc.y - orw.y, x);
        x = fma(kk[2], (double)r.z + oc.z - orw.z, x);
        x = fma(kk[3], (double)r.w + oc.w - orw.w, x);
        double s, c;
        sincospi(2.0 * x, &s, &c);
        const cd h = cmul(amp[e], cd{c, s});
        if (VEL) {
            const double ta = 2.0 * M_PI * ((double)kpm_pick(r, da) + kpm_pick(oc, da) - kpm_pick(orw, da));
            const double tb = 2.0 * M_PI * ((double)kpm_pick(r, db) + kpm_pick(oc, db) - kpm_pick(orw, db));
            va[e] = cd{-ta * h.y, ta * h.x};
            vb[e] = cd{-tb * h.y, tb * h.x};
        }
        val[e] = h;
    }
}

// What a step does with the new value nw of (row, v) besides storing it (x0 is cur's element): row<NV, FIRST>() may add to the
// row-local sums (dA, dB), which go to `part` through kpm_block_sums where SUMS is set.  KpmSeriesTerm (below) and KpmResid
// (tbk_kpm_eigs.hip) are two more.
struct KpmDots {   // A = <nw|nw>, B = Re <nw|cur>
    static constexpr bool SUMS = true;
    double* part;
    template <int NV, bool FIRST>
    __device__ __forceinline__ void row(int, int64_t, int, const cd x0, const cd nw, double& dA, double& dB) const {
        dA += cabs2(nw);
        dB += nw.x * x0.x + nw.y * x0.y;
    }
};
struct KpmNoSums {   // the vector alone: no sums, no LDS, no barrier
    static constexpr bool SUMS = false;
    template <int NV, bool FIRST>
    __device__ __forceinline__ void row(int, int64_t, int, cd, cd, double&, double&) const {}
};

// One Chebyshev step for a block of NV vectors: out = nw = 2 H~ cur - prev (FIRST: nw = H~ cur, prev unused), H~ = (A - b) / a
// with A the CSR operator of the values `val`, then the epilogue.  IN_PLACE: prev is out (the argument is not read): the element
// of prev is read from out before nw goes there -- row i reads only its own element, so two buffers are enough for a recursion.
// Said at compile time, not as "out may be prev", so that out can be __restrict__: without it every store to out stands between
// the epilogue and what it reads (the coefficients of a series would come through vector instead of scalar loads).  out is never
// cur.  An empty row gives nw = -(2 b / a) cur - prev.  With (b, inv_a) = (0, 1) and FIRST it is the plain product A cur (a
// velocity operator).
template <int NV, bool FIRST, class Epi, bool IN_PLACE = true>
__global__ __launch_bounds__(256) void k_kpm_step(const int nsta, const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                  const cd* __restrict__ val, const cd* __restrict__ cur, const cd* prev,
                                                  cd* __restrict__ out, const double b, const double inv_a, const Epi epi) {
    const cd* pv = IN_PLACE ? out : prev;
    double dA = 0.0, dB = 0.0;
    kpm_for_rows<NV>(nsta, [&](const int64_t row, const int v) {
        const cd acc = kpm_row_product<NV>(row_ptr, col, val, cur, row, v);
        const cd x0 = cur[row * NV + v];
        const cd h{(acc.x - b * x0.x) * inv_a, (acc.y - b * x0.y) * inv_a};
        cd nw = h;
        if (!FIRST) {
            const cd p = pv[row * NV + v];
            nw = cd{2.0 * h.x - p.x, 2.0 * h.y - p.y};
        }
        out[row * NV + v] = nw;
        epi.template row<NV, FIRST>(nsta, row, v, x0, nw, dA, dB);
    });
    if constexpr (Epi::SUMS) kpm_block_sums<NV>(dA, dB, epi.part);
}

// ------------------------------------------------------------------ series (tbk_kpm_series.hip, tbk_kpm_eigs.hip)
#define KPMS_GUARD 5                         // doubles of the guard record: flag, <T_j v|T_j v>, <v|v>, sample, vector

// The epilogue of k_kpm_step that adds the term of step j to every series: acc[s][row][NV] += coef[s][j] nw, s ascending; FIRST
// (j = 1) writes acc[s] = coef[s][0] cur + coef[s][1] nw instead.  part: the row-local sums of <nw|nw> (the second slot stays zero).
struct KpmSeriesTerm {
    static constexpr bool SUMS = true;
    int nset, ncoef, j;
    const cd* coef;
    cd* acc;
    double* part;
    template <int NV, bool FIRST>
    __device__ __forceinline__ void row(const int nsta, const int64_t row, const int v, const cd x0, const cd nw, double& dA, double&) const {
        add<NV, FIRST>(nset, ncoef, j, coef, acc, nsta, row, v, x0, nw);
        dA += cabs2(nw);
    }
    // a function of its own for the __restrict__ of its arguments, which a member cannot carry: with it the coefficients come
    // through scalar loads
    template <int NV, bool FIRST>
    static __device__ __forceinline__ void add(const int nset, const int ncoef, const int j, const cd* __restrict__ coef,
                                               cd* __restrict__ acc, const int nsta, const int64_t row, const int v, const cd x0,
                                               const cd nw) {
        for (int s = 0; s < nset; ++s) {
            cd* dst = acc + ((int64_t)s * nsta + row) * NV + v;
            cd t = FIRST ? cmul_x(coef[(int64_t)s * ncoef], x0) : *dst;
            cfma_x(t, coef[(int64_t)s * ncoef + j], nw);
            *dst = t;
        }
    }
};

// ncoef = 1: acc[s][row][NV] = coef[s][0] cur, no sparse product; a lane per element
static __global__ __launch_bounds__(256) void k_kpm_series_const(const int64_t len, const int nset, const int ncoef, const cd* __restrict__ coef,
                                                          const cd* __restrict__ cur, cd* __restrict__ acc) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < len; i += (int64_t)gridDim.x * 256) {
        const cd x = cur[i];
        for (int s = 0; s < nset; ++s) acc[(int64_t)s * len + i] = cmul_x(coef[(int64_t)s * ncoef], x);
    }
}

// The guard of one series: dots[step][2][NV] holds A_step = <T_step v|T_step v> per vector, A_0 = <v|v>.  The largest A per vector
// (a NaN counts as infinite) against (1 + 1e-6) A_0; the first violation of a call is recorded in rec = (1, A, A_0, sample, vector).
// One workgroup; the launches of a call are ordered on the stream, so "first" is the same in every run.
template <int NV>
__global__ __launch_bounds__(256) void k_kpm_series_guard(const int nstep, const double* __restrict__ dots, const double sample,
                                                          double* __restrict__ rec) {
    constexpr int NC = 2 * NV, G = 256 / NV;
    const int v = threadIdx.x % NV, g = threadIdx.x / NV;
    double mx = 0.0;
    for (int s = g; s < nstep; s += G) {
        const double A = dots[(int64_t)s * NC + v];
        mx = fmax(mx, A == A ? A : INFINITY);
    }
    __shared__ double red[G][NV];
    red[g][v] = mx;
    __syncthreads();
    if (threadIdx.x == 0 && rec[0] == 0.0)
        for (int u = 0; u < NV; ++u) {
            double t = red[0][u];
            for (int i = 1; i < G; ++i) t = fmax(t, red[i][u]);
            const double a0 = dots[u];
            if (!(t <= (1.0 + 1e-6) * a0)) {
                rec[0] = 1.0;
                rec[1] = t;
                rec[2] = a0;
                rec[3] = sample;
                rec[4] = (double)u;
                break;
            }
        }
}

// out[s][v][nsta] = acc[s][row][v], v < nv: a tile of 32 rows x NV vectors through LDS, so that both sides move whole segments.
// grid (row tiles, sets); out is the slice of this block of vectors, set_stride elements between two sets.
template <int NV>
__global__ __launch_bounds__(256) void k_kpm_series_gather(const int nsta, const int nv, const int64_t set_stride,
                                                           const cd* __restrict__ acc, cd* __restrict__ out) {
    constexpr int RPB = 256 / NV;
    __shared__ cd t[NV][RPB + 1];
    const int64_t ntiles = ((int64_t)nsta + RPB - 1) / RPB;
    const int s = blockIdx.y;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row0 = tile * RPB;
        {
            const int r = threadIdx.x / NV, v = threadIdx.x % NV;
            if (row0 + r < nsta) t[v][r] = acc[((int64_t)s * nsta + row0 + r) * NV + v];
        }
        __syncthreads();
        {
            const int v = threadIdx.x / RPB, r = threadIdx.x % RPB;
            if (v < nv && row0 + r < nsta) out[(int64_t)s * set_stride + (int64_t)v * nsta + row0 + r] = t[v][r];
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ host
// The arguments the entry points share; `who` is the entry point and `order_name` its name for the number of terms.  A model with
// dim_k = 0 has one (empty) k-point.
static int kpm_check_args(const char* who, const tbk_sparse* sp, const char* order_name, int order, int nvec, const double* vectors,
                          const int32_t* states, double emin, double emax, const double* k, int64_t* nk) {
    TBK_REQUIRE(order >= 1, TBK_EINVAL, "%s: %s=%d", who, order_name, order);
    TBK_REQUIRE(nvec >= 1, TBK_EINVAL, "%s: nvec=%d", who, nvec);
    TBK_REQUIRE(!(vectors && states), TBK_EINVAL, "%s: both vectors and states given", who);
    TBK_REQUIRE(std::isfinite(emin) && std::isfinite(emax) && emax > emin, TBK_EINVAL, "%s: bounds (%g, %g)", who, emin, emax);
    if (sp->dim_k == 0) *nk = 1;
    TBK_REQUIRE(*nk >= 0 && (sp->dim_k == 0 || k || *nk == 0), TBK_EINVAL, "%s: null k list", who);
    if (states)
        for (int v = 0; v < nvec; ++v)
            TBK_REQUIRE(states[v] >= 0 && states[v] < sp->nsta, TBK_EINVAL, "%s: state %d out of range [0, %d)", who, states[v], sp->nsta);
    return TBK_OK;
}

// The launch plan of a call: the workgroups of every kernel on the row mapping, and the slots of `part`, one per step between two
// reductions (steps 0 .. nsteps; step 0 is the norm of the start vectors).
struct KpmPlan {
    int nwg, nslots;
    size_t slot_len() const { return (size_t)nwg * 2 * KPM_NV; }      // doubles of one slot
    size_t part_len() const { return (size_t)nslots * slot_len(); }
};
static inline KpmPlan kpm_plan(int nsta, int nsteps) {
    constexpr int RPB = 4 * (64 / KPM_NV);
    const int64_t ntiles = ((int64_t)nsta + RPB - 1) / RPB;
    KpmPlan P{(int)std::min<int64_t>(ntiles, KPM_MAX_WG), 1};
    P.nslots = (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(KPM_MAX_SLOTS, (size_t)nsteps + 1),
                                                         KPM_PART_BYTES / (P.slot_len() * sizeof(double))));
    return P;
}

// A device workspace carved by one list: layout(c) names every buffer once, c.take(pointer, elements); it runs once to add the
// sizes up and once more on the allocation.
struct KpmCarve {
    unsigned char* base = nullptr;
    size_t off = 0;
    template <class T>
    void take(T*& p, size_t count) {
        p = base ? (T*)(base + off) : nullptr;
        off += up256(count * sizeof(T));
    }
};
template <class Layout>
static int kpm_workspace(tbk_ctx* ctx, Layout&& layout, size_t* total) {
    KpmCarve c;
    layout(c);
    *total = c.off;
    void* ws = nullptr;
    int rc = tbk_ctx_scratch(ctx, c.off, &ws);
    if (rc) return rc;
    c = KpmCarve{(unsigned char*)ws, 0};
    layout(c);
    return TBK_OK;
}

// The k list and the start vectors of a call: random phases (mode 0), unit vectors at `states` (1) or supplied `vectors` (2).
struct KpmStart {
    int dim_k, nsta, nvec, mode;
    int64_t nk;
    uint64_t seed;
    const double* k;
    const void* src;
    double* k_dev = nullptr;
    unsigned char* src_dev = nullptr;
    KpmStart(const tbk_sparse* sp, const double* k_, int64_t nk_, int nvec_, const double* vectors, const int32_t* states, uint64_t seed_)
        : dim_k(sp->dim_k), nsta(sp->nsta), nvec(nvec_), mode(vectors ? 2 : (states ? 1 : 0)), nk(nk_), seed(seed_), k(k_),
          src(vectors ? (const void*)vectors : (const void*)states) {}
    size_t src_bytes() const { return mode == 2 ? (size_t)nvec * nsta * sizeof(cd) : (mode == 1 ? (size_t)nvec * sizeof(int32_t) : 0); }
    void carve(KpmCarve& c) {
        c.take(k_dev, (size_t)nk * std::max(dim_k, 1));
        c.take(src_dev, src_bytes());
    }
    int upload(tbk_ctx* ctx) const {
        if (dim_k > 0) TBK_HIP(hipMemcpyAsync(k_dev, k, (size_t)nk * dim_k * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        if (mode != 0) TBK_HIP(hipMemcpyAsync(src_dev, src, src_bytes(), hipMemcpyHostToDevice, ctx->stream));
        return TBK_OK;
    }
    const double* k_at(int64_t q) const { return k_dev + q * dim_k; }
    // vectors v0 .. v0 + nv - 1 of k-point q -> cur, the partial sums of their norms -> part (one slot)
    int launch(tbk_ctx* ctx, int nwg, int64_t q, int v0, int nv, cd* cur, double* part) const {
        ProfScope ps(ctx, "kpm_init");
        hipLaunchKernelGGL((k_kpm_init<KPM_NV>), dim3(nwg), dim3(256), 0, ctx->stream, nsta, nv, mode, seed, (uint64_t)(q * nvec + v0),
                           mode == 1 ? (const int32_t*)src_dev + v0 : nullptr, mode == 2 ? (const cd*)src_dev + (size_t)v0 * nsta : nullptr,
                           cur, part);
        TBK_HIP(hipGetLastError());
        return TBK_OK;
    }
};

// dots[i] = the sums of slot i of part, i < count
static int kpm_reduce(tbk_ctx* ctx, int nwg, int count, const double* part, double* dots) {
    ProfScope ps(ctx, "kpm_reduce");
    hipLaunchKernelGGL((k_kpm_reduce<KPM_NV>), dim3(count), dim3(256), 0, ctx->stream, nwg, part, dots);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

// The order of a series of steps whose partial sums share nslots slots.  Step 0 (the start vectors) is in slot 0 on entry; steps
// 1 .. nsteps follow, step(j, slot), and reduce(first, count) empties the slots 0 .. count - 1, which hold the steps first ..
// first + count - 1, when all nslots are full and once more at the end.  No device call of its own.
template <class Step, class Reduce>
static int kpm_slot_schedule(int nsteps, int nslots, Step&& step, Reduce&& reduce) {
    int chunk0 = 0;    // first step of the partial sums not yet reduced; step j sits in slot j - chunk0
    for (int j = 1; j <= nsteps; ++j) {
        if (j - chunk0 == nslots) {
            int rc = reduce(chunk0, nslots);
            if (rc) return rc;
            chunk0 = j;
        }
        int rc = step(j, j - chunk0);
        if (rc) return rc;
    }
    return reduce(chunk0, nsteps + 1 - chunk0);
}

// Steps 1 .. nsteps of a recursion on the buffers (cur, prev): launch(j, cur, prev, part_j) starts step j, which writes alpha_j
// over prev (in place) and its partial sums into part_j; the buffers swap after every step.  -> dots[step][2][NV], steps 0 .. nsteps
template <class Launch>
static int kpm_run_steps(tbk_ctx* ctx, const KpmPlan& P, int nsteps, cd* cur, cd* prev, double* part, double* dots, Launch&& launch) {
    return kpm_slot_schedule(
        nsteps, P.nslots,
        [&](int j, int slot) {
            int rc = launch(j, (const cd*)cur, prev, part + (size_t)slot * P.slot_len());
            std::swap(cur, prev);
            return rc;
        },
        [&](int first, int count) { return kpm_reduce(ctx, P.nwg, count, part, dots + (size_t)first * 2 * KPM_NV); });
}

// ------------------------------------------------------------------ series, host
// One series for a block of NV vectors.  On entry `cur` holds the start vectors and slot 0 of `part` the partial sums of their
// norms; on return (of the launches) acc[s][row][NV] holds sum_m coef[s][m] T_m(H~) cur and the guard has seen every norm.
struct KpmSeries {
    tbk_ctx* ctx;
    const tbk_sparse* sp;
    KpmPlan plan;
    int nset, ncoef;
    double b, inv_a;
    const cd* coef;      // device, [nset][ncoef]
    cd *cur, *prev;
    double *part, *dots, *rec;
};

static int kpm_series_run(const KpmSeries& S, const cd* val, cd* acc, double sample) {
    constexpr int NV = KPM_NV;
    tbk_ctx* ctx = S.ctx;
    const int n = S.sp->nsta, nsteps = S.ncoef - 1, nwg = S.plan.nwg;
    if (nsteps == 0) {
        ProfScope ps(ctx, "kpm_series_const");
        hipLaunchKernelGGL(k_kpm_series_const, dim3(kpm_stream_grid((int64_t)n * NV)), dim3(256), 0, ctx->stream, (int64_t)n * NV, S.nset,
                           S.ncoef, S.coef, S.cur, acc);
        TBK_HIP(hipGetLastError());
    }
    int rc = kpm_run_steps(ctx, S.plan, nsteps, S.cur, S.prev, S.part, S.dots, [&](int j, const cd* x, cd* y, double* pj) {
        const KpmSeriesTerm term{S.nset, S.ncoef, j, S.coef, acc, pj};
        ProfScope ps(ctx, "kpm_series_step");
        if (j == 1)
            hipLaunchKernelGGL((k_kpm_step<NV, true, KpmSeriesTerm>), dim3(nwg), dim3(256), 0, ctx->stream, n, S.sp->row_ptr, S.sp->col, val,
                               x, nullptr, y, S.b, S.inv_a, term);
        else
            hipLaunchKernelGGL((k_kpm_step<NV, false, KpmSeriesTerm>), dim3(nwg), dim3(256), 0, ctx->stream, n, S.sp->row_ptr, S.sp->col, val,
                               x, nullptr, y, S.b, S.inv_a, term);
        TBK_HIP(hipGetLastError());
        return TBK_OK;
    });
    if (rc) return rc;
    ProfScope ps(ctx, "kpm_series_guard");
    hipLaunchKernelGGL((k_kpm_series_guard<NV>), dim3(1), dim3(256), 0, ctx->stream, nsteps + 1, S.dots, sample, S.rec);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

// the verdict of the guard record after the call's synchronisation
static int kpm_series_verdict(const char* who, const double* rec, const tbk_sparse* sp, double emin, double emax) {
    if (rec[0] == 0.0) return TBK_OK;
    tbk_set_error("%s: <T_j v|T_j v> reaches %g for vector %lld of sample %lld, beyond <v|v> = %g: the bounds (%.17g, %.17g) do not "
                  "contain the spectrum (Gershgorin interval of this operator: (%.17g, %.17g))",
                  who, rec[1], (long long)rec[4], (long long)rec[3], rec[2], emin, emax, sp->gmin, sp->gmax);
    return TBK_EINVAL;
}

template <class Layout>
static int kpm_series_workspace(const char* who, tbk_ctx* ctx, Layout&& layout) {
    size_t total;
    int rc = kpm_workspace(ctx, layout, &total);
    if (rc == TBK_ENOMEM) {
        (void)hipGetLastError();
        tbk_set_error("%s: no device workspace of %zu bytes", who, total);
    }
    return rc;
}
