// tbk_lat.h -- the host-only part of the lattice sum of weighted projectors (tbk_lat_dev.h), shared by the
// density matrix (tbk_occ.h) and the lattice Green's function (tbk_gf.h): the LDS budget of the frame, its lane map -- the functions
// the kernel itself runs, so that check/occ_plan_check.cpp replays the same code on the host -- the partition of a chunk into batches,
// entries per lane, tiles and k-groups, and the check of a list of lattice vectors.  No device call.
#pragma once
#include "tbk_kubo.h"

#define OCC_LDS_CD 1408                                  // c128 of eigenvectors in LDS per workgroup of k_lat_lds (22 KiB)
#define OCC_LDS_PN 256                                   // (point, state) pairs of a batch at most: their weights and orbital phases
static const int kOccRMax = 4096;                        // lattice vectors of one call
static const int32_t kOccRAbsMax = (int32_t)1 << 30;     // |R_a| below this

// ---------------------------------------------------------------- the lane map of k_lat_lds
// nab entries (i, j) on 256 lanes.  ES = 1 (nab <= 256): lane t = q nab + entry takes the points q, q + Q, ... of a batch (Q = 256 / nab
// shares; a lane beyond the last share idles).  ES = 2 or 4: lane t takes the entries t, t + 256, ... and every point.
struct LatLane {
    int Q, q, el0;
    bool live;
};
__host__ __device__ inline LatLane lat_lane(const int ES, const int nab, const int t) {
    LatLane l;
    l.Q = ES == 1 && nab < 256 ? 256 / nab : 1;
    l.q = ES == 1 ? t / nab : 0;
    l.el0 = ES == 1 ? t - l.q * nab : t;
    l.live = ES > 1 || l.q < l.Q;
    return l;
}
__host__ __device__ inline void lat_entry(const int el, const int na, int& i, int& j) {
    i = el / na;
    j = el - i * na;
}
static inline int lat_entries_per_lane(int64_t nab) { return nab <= 256 ? 1 : (nab <= 512 ? 2 : 4); }
// points per batch: their eigenvectors in LDS, and at most OCC_LDS_PN (point, state) pairs
static inline int lat_points(int n) { return std::max(1, std::min({64, OCC_LDS_CD / (n * n), OCC_LDS_PN / n})); }

// ---------------------------------------------------------------- the partition
struct LatPart {
    bool lds = false;       // up to 32 states: k_lat_lds, else k_lat_tile
    int64_t npts = 0, chunk = 0, nchunks = 0;
    int P = 0;              // points per batch (lds)
    int ES = 0;             // entries per lane (lds): 1 up to 256 entries, 2 up to 512, 4 up to 1024
    int T = 0;              // 16 x 16 tiles per side of the tiled form
    int G = 0;              // k-groups of a chunk: group g takes the points [g cnt / G, (g + 1) cnt / G) of a chunk of cnt
};
// n states of which na are kept, workgroups of `block` (frequency, lattice vector) pairs.  A group walks about four batches (lds) or
// eight points (tiled); never more groups than points, nor than the cap on part allows for one block of the full matrix.
static LatPart lat_partition(int n, int na, int64_t npts, int block, int64_t part_cap, int groups_max) {
    LatPart p;
    p.lds = n <= 32;
    p.npts = npts;
    p.chunk = kubo_chunk_len(n, npts);
    p.nchunks = (npts + p.chunk - 1) / p.chunk;
    p.P = lat_points(n);
    p.ES = lat_entries_per_lane((int64_t)na * na);
    p.T = (na + 15) / 16;
    const int64_t per = p.lds ? 4 * (int64_t)p.P : 8;
    p.G = (int)std::max<int64_t>(1, std::min<int64_t>({(p.chunk + per - 1) / per, (int64_t)groups_max, part_cap / ((int64_t)n * n * block)}));
    return p;
}

// ---------------------------------------------------------------- checks
static int lat_R_check(const char* fn, int dk, int nR, const int32_t* R) {
    TBK_REQUIRE(nR >= 1 && nR <= kOccRMax && R, TBK_EINVAL, "%s: nR=%d (1..%d lattice vectors)", fn, nR, kOccRMax);
    for (int64_t j = 0; j < (int64_t)nR * dk; ++j)
        TBK_REQUIRE(R[j] > -kOccRAbsMax && R[j] < kOccRAbsMax, TBK_EINVAL, "%s: lattice vector %lld has a component of 2^30 or more", fn,
                    (long long)(j / dk));
    return TBK_OK;
}
