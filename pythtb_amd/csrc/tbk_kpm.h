// tbk_kpm.h -- what the translation units of the kernel polynomial method share (tbk_kpm.hip: the operator and the single moments;
// tbk_kpm_cond.hip: the double moments of the Kubo-Bastin conductivity; tbk_kpm_series.hip: operator functions and the local Chern
// marker): the operator's handle, the random-phase generator, the start vectors and the fixed-order sums.  DESIGN.md sections 21 to 23.
#pragma once
#include <algorithm>
#include "tbk_internal.h"

#define KPM_NV 8            // vectors per block
#define KPM_MAX_WG 2048     // workgroups of a step (grid-stride over the row tiles beyond that)

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

// alpha_0 of one block of NV vectors, alpha[row][NV], and the partial sums of <alpha_0|alpha_0> (the slot of step 0).
// mode 0: random phases, vector numbers g0 + v; 1: unit vectors at states[v]; 2: src[v][nsta].  Vectors v >= nv are zero.
template <int NV>
__global__ __launch_bounds__(256) void k_kpm_init(const int nsta, const int nv, const int mode, const uint64_t seed, const uint64_t g0,
                                                  const int32_t* __restrict__ states, const cd* __restrict__ src,
                                                  cd* __restrict__ cur, double* __restrict__ part) {
    constexpr int RPW = 64 / NV, RPB = 4 * RPW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, v = lane % NV, rw = lane / NV;
    const int64_t ntiles = ((int64_t)nsta + RPB - 1) / RPB;
    double dA = 0.0;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row = tile * RPB + wave * RPW + rw;
        if (row < nsta) {
            cd x{0.0, 0.0};
            if (v < nv) {
                if (mode == 0) x = kpm_random_phase(seed, g0 + (uint64_t)v, (uint64_t)row);
                else if (mode == 1) x = cd{states[v] == row ? 1.0 : 0.0, 0.0};
                else x = src[(int64_t)v * nsta + row];
            }
            cur[row * NV + v] = x;
            dA += cabs2(x);
        }
    }
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
