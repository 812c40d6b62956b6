// tbk_chi.h -- the host-only part of tbk_chi.hip (the Lindhard susceptibility on k meshes): the argument checks
// of tbk_susceptibility_mesh and the plan of one call -- the chunk of mesh points, the k-groups and tiles of the frequency stage, the
// groups of the static sums, the points per workgroup of the LDS pair kernel and the layout of the scratch block.  No device call:
// check/chi_plan_check.cpp drives it on the host alone (make chi-check).
//
// Everything here is a function of (mesh, n, dim_k, nw, flags) alone -- NOT of nq: a q of the list is worked through with the same
// chunks, groups and tiles whatever stands beside it, so it gives the same bits alone and inside a longer list.
#pragma once
#include "tbk_pairs.h"

#define TBK_CHI_FLAGS_ALL TBK_CHI_MATRIX_ELEMENTS
#define CHI_LDS_CD 2048                                  // c128 of LDS per workgroup of k_chi_pairs (32 KiB: five workgroups per CU)
static const int64_t kChiOutCap = (int64_t)1 << 22;      // nq nw at most
static const int kChiListMax = 65536;                    // q points at most (frequencies: kKuboOmegaMax)

// points per workgroup of k_chi_pairs: U(k) and U(k+q) of every point in LDS
static inline int chi_lds_points(int n) { return std::max(1, std::min(64, CHI_LDS_CD / (2 * n * n))); }

struct ChiPlan {
    bool dynamic = false, me = false, lds = false, wide = false;
    int64_t npts = 0, chunk = 0, nchunks = 0;
    int P = 0;             // points per workgroup of k_chi_pairs (lds)
    int G = 0;             // k-groups of a chunk: of the frequency stage, and of the lane-per-pair kernel
    int64_t gmax = 0;      // groups that one (chunk, q) writes at most
    unsigned ntile = 0;    // frequency tiles
    int64_t nrows = 0;     // rows per q: 2 nw (x, y per frequency) or 1
    int64_t part_doubles = 0, acc_doubles = 0;
    // the chunk's first extra buffer holds k + q, E(k+q) and U(k+q) at these offsets; the second the records, the third |M|^2
    size_t off_e2 = 0, off_v2 = 0, x0 = 0, x1 = 0, x2 = 0;
    // the scratch block: 256 leading bytes, omega, the q list, acc[nq][nrows], part[gmax][nrows], then the chunk workspace
    size_t off_om = 0, off_q = 0, off_acc = 0, off_part = 0, off_chunks = 0, total = 0;
    KuboChunks cw;
};

// the checks of tbk_susceptibility_mesh behind its pointers; npts = the points of the mesh
static int chi_check(const char* fn, int dk, int n, const int32_t* mesh, int nq, const double* q, int nomega, const double* omega,
                     double eta, double mu, double kT, int flags, int64_t& npts) {
    int rc = kubo_mesh_dim(fn, dk);
    if (rc) return rc;
    TBK_REQUIRE(n >= 1 && n <= 2048, TBK_EINVAL, "%s: nsta=%d (1..2048 states)", fn, n);
    TBK_REQUIRE((flags & ~TBK_CHI_FLAGS_ALL) == 0, TBK_EINVAL, "%s: flags=%d (TBK_CHI_MATRIX_ELEMENTS or 0)", fn, flags);
    TBK_REQUIRE(nq >= 1 && nq <= kChiListMax, TBK_EINVAL, "%s: nq=%d (1..%d q points)", fn, nq, kChiListMax);
    for (int64_t j = 0; j < (int64_t)nq * dk; ++j)
        TBK_REQUIRE(std::isfinite(q[j]), TBK_EINVAL, "%s: q point %lld is not finite", fn, (long long)(j / dk));
    if (omega) {
        rc = kubo_omega_check(fn, nomega, omega, eta);
        if (rc) return rc;
        TBK_REQUIRE((int64_t)nq * nomega <= kChiOutCap, TBK_EINVAL, "%s: nq * nomega = %lld (at most %lld)", fn,
                    (long long)nq * nomega, (long long)kChiOutCap);
    } else {
        TBK_REQUIRE(nomega == 0, TBK_EINVAL, "%s: nomega=%d without omega (the static mode takes 0)", fn, nomega);
        TBK_REQUIRE(eta == 0.0, TBK_EINVAL, "%s: the static mode is the eta -> 0 limit: eta must be 0", fn);
    }
    rc = kubo_occupation_check(fn, kT, mu);
    return rc ? rc : kubo_mesh_points(fn, dk, mesh, npts);
}

// the plan of a checked call
static ChiPlan chi_plan(int n, int dk, int64_t npts, int nq, int nw, int flags) {
    ChiPlan p;
    const size_t nn = (size_t)n * n;
    p.dynamic = nw > 0;
    p.me = (flags & TBK_CHI_MATRIX_ELEMENTS) != 0;
    p.lds = p.me && n <= 32;
    p.wide = p.me && n > 32;
    p.npts = npts;
    p.chunk = kubo_chunk_len(n, npts);                   // at most kKuboChunkBytes of eigenvectors -- and as many bytes of records
    p.nchunks = (npts + p.chunk - 1) / p.chunk;
    p.P = chi_lds_points(n);
    p.nrows = p.dynamic ? 2 * (int64_t)nw : 1;
    p.G = (int)std::max<int64_t>(1, std::min<int64_t>({kPairPartCap / p.nrows, (int64_t)kPairGroupsMax, p.chunk}));
    p.gmax = !p.dynamic && p.lds ? (p.chunk + p.P - 1) / p.P : p.G;
    p.ntile = (unsigned)((nw + kPairTile - 1) / kPairTile);
    p.part_doubles = p.gmax * p.nrows;
    p.acc_doubles = (int64_t)nq * p.nrows;
    p.off_e2 = al256((size_t)p.chunk * dk * sizeof(double));
    p.off_v2 = p.off_e2 + al256((size_t)p.chunk * n * sizeof(double));
    p.x0 = p.off_v2 + (p.me ? al256((size_t)p.chunk * nn * sizeof(cd)) : 0);
    p.x1 = p.dynamic ? (size_t)p.chunk * nn * 2 * sizeof(double) : 0;
    p.x2 = p.wide ? (size_t)p.chunk * nn * sizeof(double) : 0;
    p.cw = KuboChunks(n, dk, p.chunk, p.x0, p.x1, p.x2, p.me);
    p.off_om = 256;
    p.off_q = p.off_om + al256((size_t)nw * sizeof(double));
    p.off_acc = p.off_q + al256((size_t)nq * dk * sizeof(double));
    p.off_part = p.off_acc + al256((size_t)p.acc_doubles * sizeof(double));
    p.off_chunks = p.off_part + al256((size_t)p.part_doubles * sizeof(double));
    p.total = p.off_chunks + p.cw.bytes();
    return p;
}
