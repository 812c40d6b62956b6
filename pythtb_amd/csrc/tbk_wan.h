// tbk_wan.h -- the host-only part of tbk_wan.hip (projected and maximally localised Wannier functions on uniform k meshes, DESIGN.md
// section 34): the argument checks and caps of tbk_wannier_mesh, the neighbour of a mesh point under a b-vector step with the exact
// integer reciprocal vector G it wraps by, the partition of every kernel and the layout of the driver's private workspace.  No device
// call: check/wan_plan_check.cpp drives it on the host alone (make wan-check).
//
// Caps:  nsta <= 2048 (the dense solver);  1 <= nw <= 16 functions from nw <= nb <= 32 bands;  every N_a >= 3 (a step +b and its
// mirror -b must reach different points);  at most 6 b-vectors with step components in {-1, 0, 1};  the rotated states
// u~[N_k][nw][nsta] stay resident: N_k nsta nw <= kTdStateCap = 2^26 c128 (tbk_td.h);  0 <= max_iter <= 65536;  at most 4096 lattice
// vectors from the caller, or the N_k of the torus set;  nR nsta nw <= 2^26 with the functions, nR nw^2 <= 2^26 always.
//
// Partition, a function of (mesh, nsta, nb, nw, the number of b-vectors) alone -- NOT of max_iter, tol or check_every:
//   chunk   points per solve: kubo_chunk_len(nsta, N_k)
//   P       points per workgroup of k_wan_rotate: their Loewdin factors (nb nw c128 each) share 1024 c128 of LDS
//   Q       (point, b-vector) items per workgroup of k_wan_overlap: nw^2 lanes each, 256 lanes and WAN_OV_ROWS rows of LDS at most
//   G       k-groups of the spread sums: group g takes the points [g N_k / G, (g + 1) N_k / G), in 128 / (nw nbv) interleaved slices
//   GF      k-groups of a Fourier sum, from N_k and the number of its outputs (wan_fourier_groups)
#pragma once
#include "tbk_td.h"
#include "tbk_occ.h"
#include "tbk_small_eig.h"

#define WAN_NW_MAX 16
#define WAN_NB_MAX 32
#define WAN_BV_MAX 6
#define WAN_OV_TJ 32                                      // components per LDS tile of the overlap kernel
#define WAN_OV_ROWS 80                                    // rows of WAN_OV_TJ + 1 c128 in that tile (two per function and item)
#define WAN_ROT_LDS 1024                                  // c128 of Loewdin factors per workgroup of the rotation
static const int kWanIterMax = 65536;
static const int kWanRMax = 4096;                         // lattice vectors of a caller's list
static const int64_t kWanTermMax = (int64_t)1 << 20;      // terms of all trial functions together
static const int64_t kWanOutCap = (int64_t)1 << 26;       // c128 of one output table
static const int kWanGroupsMax = 1024;
static const double kWanSvMin = 1e-8;                     // below it the trial functions count as singular on the bands

struct WanArgs {
    int nb = 0, nw = 0;
    const int32_t* bands = nullptr;      // [nb]
    int64_t nterm = 0;
    const int32_t* term_ptr = nullptr;   // [nw + 1]: the terms of function n
    const int32_t* term_state = nullptr; // [nterm]
    const int32_t* term_R = nullptr;     // [nterm][dim_k]
    const double* term_amp = nullptr;    // [nterm][2]
    int nbv = 0;
    const int32_t* bstep = nullptr;      // [nbv][dim_k], components in {-1, 0, 1}: b = sum_a step_a beta_a / N_a
    const double* bw = nullptr;          // [nbv] weights
    const double* bgram = nullptr;       // [nbv][nbv]: b . b' (Cartesian)
    int max_iter = 0, check_every = 10;
    double tol = 0.0;
    int nR = 0, r_user = 0;              // r_user: the caller's own list (<= 4096) instead of the torus set
    const int32_t* R = nullptr;          // [nR][dim_k]
    int want_fn = 0;
};

static int wan_check(const char* fn, int dk, int n, const int32_t* mesh, const WanArgs& A, int64_t& npts) {
    TBK_REQUIRE(dk >= 1 && dk <= 3, TBK_EINVAL, "%s: dim_k=%d (a k mesh needs 1, 2 or 3 periodic dimensions)", fn, dk);
    TBK_REQUIRE(n >= 1 && n <= kTdStatesMax, TBK_EINVAL, "%s: nsta=%d (1..%d states, the dense solver's limit)", fn, n, kTdStatesMax);
    TBK_REQUIRE(mesh, TBK_EINVAL, "%s: null mesh", fn);
    int rc = kubo_mesh_points(fn, dk, mesh, npts);
    if (rc) return rc;
    for (int d = 0; d < dk; ++d) TBK_REQUIRE(mesh[d] >= 3, TBK_EINVAL, "%s: mesh[%d]=%d (at least 3: +b and -b must differ)", fn, d, mesh[d]);
    TBK_REQUIRE(npts < ((int64_t)1 << 31), TBK_EINVAL, "%s: a mesh of %lld points (fewer than 2^31)", fn, (long long)npts);
    TBK_REQUIRE(A.nw >= 1 && A.nw <= WAN_NW_MAX, TBK_EINVAL, "%s: nw=%d (1..%d trial functions)", fn, A.nw, WAN_NW_MAX);
    TBK_REQUIRE(A.nb >= A.nw && A.nb <= WAN_NB_MAX && A.nb <= n && A.bands, TBK_EINVAL, "%s: nb=%d (nw = %d .. min(%d, nsta = %d) bands)", fn,
                A.nb, A.nw, WAN_NB_MAX, n);
    {
        std::vector<char> seen((size_t)n, 0);
        for (int i = 0; i < A.nb; ++i) {
            TBK_REQUIRE(A.bands[i] >= 0 && A.bands[i] < n, TBK_EINVAL, "%s: bands[%d]=%d outside [0, %d)", fn, i, A.bands[i], n);
            TBK_REQUIRE(!seen[(size_t)A.bands[i]], TBK_EINVAL, "%s: band %d appears twice", fn, A.bands[i]);
            seen[(size_t)A.bands[i]] = 1;
        }
    }
    TBK_REQUIRE(npts * n * A.nw <= kTdStateCap, TBK_EINVAL,
                "%s: %lld points x %d functions x %d components = %lld c128 stay resident (at most %lld): coarsen the mesh", fn,
                (long long)npts, A.nw, n, (long long)(npts * n * A.nw), (long long)kTdStateCap);
    TBK_REQUIRE(A.term_ptr && A.term_state && A.term_R && A.term_amp && A.nterm >= A.nw && A.nterm <= kWanTermMax, TBK_EINVAL,
                "%s: %lld trial terms (at least one per function, at most 2^20)", fn, (long long)A.nterm);
    TBK_REQUIRE(A.term_ptr[0] == 0 && A.term_ptr[A.nw] == A.nterm, TBK_EINVAL, "%s: the term ranges do not cover the term list", fn);
    for (int w = 0; w < A.nw; ++w)
        TBK_REQUIRE(A.term_ptr[w + 1] > A.term_ptr[w], TBK_EINVAL, "%s: trial function %d has no term", fn, w);
    for (int64_t t = 0; t < A.nterm; ++t) {
        TBK_REQUIRE(A.term_state[t] >= 0 && A.term_state[t] < n, TBK_EINVAL, "%s: trial term %lld has a state index out of range", fn, (long long)t);
        TBK_REQUIRE(std::isfinite(A.term_amp[2 * t]) && std::isfinite(A.term_amp[2 * t + 1]), TBK_EINVAL, "%s: trial term %lld is not finite", fn,
                    (long long)t);
        for (int d = 0; d < dk; ++d) {
            const int32_t r = A.term_R[t * dk + d];
            TBK_REQUIRE(r > -kOccRAbsMax && r < kOccRAbsMax, TBK_EINVAL, "%s: trial term %lld has a lattice component of 2^30 or more", fn, (long long)t);
        }
    }
    TBK_REQUIRE(A.nbv >= 1 && A.nbv <= WAN_BV_MAX && A.bstep && A.bw && A.bgram, TBK_EINVAL, "%s: %d b-vectors (1..%d)", fn, A.nbv, WAN_BV_MAX);
    for (int i = 0; i < A.nbv; ++i) {
        bool zero = true;
        for (int d = 0; d < dk; ++d) {
            const int s = A.bstep[i * dk + d];
            TBK_REQUIRE(s >= -1 && s <= 1, TBK_EINVAL, "%s: b-vector %d has a step of %d (-1, 0 or 1)", fn, i, s);
            zero = zero && s == 0;
        }
        TBK_REQUIRE(!zero, TBK_EINVAL, "%s: b-vector %d is zero", fn, i);
        TBK_REQUIRE(std::isfinite(A.bw[i]) && A.bw[i] > 0.0, TBK_EINVAL, "%s: the weight of b-vector %d is not positive (a mesh too skewed for this star)",
                    fn, i);
        for (int j = 0; j < A.nbv; ++j) TBK_REQUIRE(std::isfinite(A.bgram[i * A.nbv + j]), TBK_EINVAL, "%s: b . b' is not finite", fn);
    }
    TBK_REQUIRE(A.max_iter >= 0 && A.max_iter <= kWanIterMax, TBK_EINVAL, "%s: max_iter=%d (0..%d)", fn, A.max_iter, kWanIterMax);
    TBK_REQUIRE(A.check_every >= 1, TBK_EINVAL, "%s: check_every=%d (at least 1)", fn, A.check_every);
    TBK_REQUIRE(A.tol >= 0.0 && std::isfinite(A.tol), TBK_EINVAL, "%s: tol=%.17g (finite, >= 0)", fn, A.tol);
    TBK_REQUIRE(A.R && A.nR >= 1 && (int64_t)A.nR <= (A.r_user ? (int64_t)kWanRMax : npts), TBK_EINVAL,
                "%s: %d lattice vectors (1..%d in a list of the caller's, the %lld of the torus otherwise)", fn, A.nR, kWanRMax, (long long)npts);
    for (int64_t i = 0; i < (int64_t)A.nR * dk; ++i)
        TBK_REQUIRE(A.R[i] > -kOccRAbsMax && A.R[i] < kOccRAbsMax, TBK_EINVAL, "%s: lattice vector %lld has a component of 2^30 or more", fn,
                    (long long)(i / dk));
    TBK_REQUIRE((int64_t)A.nR * A.nw * A.nw <= kWanOutCap, TBK_EINVAL, "%s: nR * nw^2 = %lld (at most 2^26)", fn, (long long)A.nR * A.nw * A.nw);
    if (A.want_fn)
        TBK_REQUIRE((int64_t)A.nR * n * A.nw <= kWanOutCap, TBK_EINVAL, "%s: the functions take nR * nsta * nw = %lld c128 (at most 2^26)", fn,
                    (long long)A.nR * n * A.nw);
    return TBK_OK;
}

// ---------------------------------------------------------------- the mesh
struct WanMesh {
    int N[3];
    int dk;
};
// The point k + b of point idx (row-major, last axis fastest, as k_uniform_mesh) for the step s[dk], and the integer G with
// k + b = k' + G, k' inside the zone: +1 where the step wraps past N_a - 1, -1 where it wraps below 0.
__host__ __device__ inline int64_t wan_neighbour(const WanMesh& M, int64_t idx, const int* s, int* G) {
    int i[3] = {0, 0, 0};
    for (int d = M.dk - 1; d >= 0; --d) {
        i[d] = (int)(idx % M.N[d]);
        idx /= M.N[d];
    }
    int64_t out = 0;
    for (int d = 0; d < M.dk; ++d) {
        int j = i[d] + s[d];
        G[d] = 0;
        if (j >= M.N[d]) j -= M.N[d], G[d] = 1;
        if (j < 0) j += M.N[d], G[d] = -1;
        out = out * M.N[d] + j;
    }
    return out;
}

// ---------------------------------------------------------------- the plan
static inline int wan_rot_points(int n, int nb, int nw) { return std::max(1, std::min({16, 256 / n, WAN_ROT_LDS / (nb * nw)})); }
static inline int wan_ov_items(int nw) { return std::max(1, std::min({8, 256 / (nw * nw), WAN_OV_ROWS / (2 * nw)})); }
// k-groups of a Fourier sum with `tot` outputs: as many as bring the lanes to kWanFourierLanes, at most wan_groups(npts); the partial
// sums G tot fit the kWanFourierLanes c128 of FPART (G = 1 writes no partial sums)
static const int64_t kWanFourierLanes = (int64_t)1 << 16;
static inline int wan_groups(int64_t npts);
static inline int wan_fourier_groups(int64_t npts, int64_t tot) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(kWanFourierLanes / std::max<int64_t>(tot, 1), wan_groups(npts)));
}
static inline int wan_groups(int64_t npts) { return (int)std::max<int64_t>(1, std::min<int64_t>((npts + 63) / 64, kWanGroupsMax)); }

struct WanPlan {
    int n = 0, dk = 0, nb = 0, nw = 0, nbv = 0;
    int64_t npts = 0, chunk = 0, nchunks = 0;
    int P = 0, Q = 0, G = 0, nq = 0;      // nq = nw nbv: the (function, b-vector) pairs of the spread sums
    enum { BANDS, TPTR, TSTATE, TRV, TAMP, PHASE, BSTEP, BW, BGRAM, UT, EB, U0, UACC, EXPW, MOV, SVK, PART, S1, CB, FIN, HIST, DHIST, HW, TW, RDEV,
           HOP, FN, FPART, CHUNKS, NBUF };
    size_t off[NBUF + 1];
    size_t total = 0;
    KuboChunks cw;
};
static WanPlan wan_plan(int n, int dk, int64_t npts, const int32_t* mesh, int nb, int nw, int nbv, int64_t nterm, int max_iter, int nR, int want_fn) {
    WanPlan p;
    const size_t D = sizeof(double), C = sizeof(cd);
    p.n = n, p.dk = dk, p.nb = nb, p.nw = nw, p.nbv = nbv, p.npts = npts;
    p.chunk = kubo_chunk_len(n, npts);
    p.nchunks = (npts + p.chunk - 1) / p.chunk;
    p.P = wan_rot_points(n, nb, nw);
    p.Q = wan_ov_items(nw);
    p.G = wan_groups(npts);
    p.nq = nw * nbv;
    p.cw = KuboChunks(n, dk, p.chunk, 0, 0, 0);
    int64_t ntw = 0;
    for (int d = 0; d < dk; ++d) ntw += mesh[d];
    size_t b[WanPlan::NBUF];
    b[WanPlan::BANDS] = (size_t)nb * sizeof(int32_t);
    b[WanPlan::TPTR] = (size_t)(nw + 1) * sizeof(int32_t);
    b[WanPlan::TSTATE] = (size_t)nterm * sizeof(int32_t);
    b[WanPlan::TRV] = (size_t)nterm * 3 * sizeof(int32_t);
    b[WanPlan::TAMP] = (size_t)nterm * C;
    b[WanPlan::PHASE] = (size_t)3 * n * C;
    b[WanPlan::BSTEP] = (size_t)WAN_BV_MAX * 3 * sizeof(int32_t);
    b[WanPlan::BW] = (size_t)WAN_BV_MAX * D;
    b[WanPlan::BGRAM] = (size_t)WAN_BV_MAX * WAN_BV_MAX * D;
    b[WanPlan::UT] = (size_t)npts * nw * n * C;
    b[WanPlan::EB] = (size_t)npts * nb * D;
    b[WanPlan::U0] = (size_t)npts * nb * nw * C;
    b[WanPlan::UACC] = (size_t)npts * nw * nw * C;
    b[WanPlan::EXPW] = (size_t)npts * nw * nw * C;
    b[WanPlan::MOV] = (size_t)npts * nbv * nw * nw * C;
    b[WanPlan::SVK] = (size_t)npts * D;
    b[WanPlan::PART] = (size_t)p.G * 4 * p.nq * D;
    b[WanPlan::S1] = (size_t)p.nq * D;
    b[WanPlan::CB] = (size_t)p.nq * D;
    b[WanPlan::FIN] = (size_t)(4 + nw) * D;
    b[WanPlan::HIST] = (size_t)(max_iter + 1) * D;
    b[WanPlan::DHIST] = (size_t)(max_iter + 1) * D;
    b[WanPlan::HW] = (size_t)npts * nw * nw * C;
    b[WanPlan::TW] = (size_t)ntw * C;
    b[WanPlan::RDEV] = (size_t)nR * 3 * sizeof(int32_t);
    b[WanPlan::HOP] = (size_t)nR * nw * nw * C;
    b[WanPlan::FN] = want_fn ? (size_t)nR * n * nw * C : 0;
    b[WanPlan::FPART] = (size_t)kWanFourierLanes * C;
    b[WanPlan::CHUNKS] = p.cw.bytes();
    p.off[0] = 256;
    for (int i = 0; i < WanPlan::NBUF; ++i) p.off[i + 1] = p.off[i] + al256(b[i]);
    p.total = p.off[WanPlan::NBUF];
    return p;
}
