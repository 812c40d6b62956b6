// tbk_pairs_dm.h -- the host-only part of tbk_pairs_dm.hip (selected entries of the density matrix on k meshes):
// the argument checks of tbk_density_matrix_pairs_mesh, the stage buffer of the kernel -- how many points or bands of a point it holds
// at a time, replayed on the host by check/bdg_plan_check.cpp -- the partition of a chunk into k-groups and of the triple list into
// tiles and launch ranges, and the layout of the scratch block.  No device call.
//
// Every partition here is a function of (mesh, n, dim_k) alone -- NOT of the number of triples, nor of what they are: a triple is
// worked through with the same groups, the same stages and the same order of bands whatever stands beside it, so it gives the same
// bits alone and inside any list.
#pragma once
#include "tbk_occ.h"

#define PDM_LDS_CD 2048                                  // c128 of eigenvectors in LDS per workgroup of k_pairs_dm (32 KiB)
#define PDM_ROWS 512                                     // (point, band) rows of a stage at most: their weights
#define PDM_TILE 64                                      // triples per workgroup: one per lane of a wavefront
static const int64_t kPdmTripleMax = (int64_t)1 << 20;   // triples of one call
static const int kPdmGroupsMax = 512;                    // k-groups of a chunk
static const int64_t kPdmPartCap = (int64_t)1 << 22;     // c128 of group partials per launch (64 MiB)

// ---------------------------------------------------------------- the stage
// What k_pairs_dm holds in LDS at a time.  n^2 <= PDM_LDS_CD: every band of P points (at most 64).  Beyond: NB bands of one point,
// the bands of a point in ceil(n / NB) stages.  n <= 2048 = PDM_LDS_CD: a band always fits.
struct PdmStage {
    int P, NB;
};
__host__ __device__ inline PdmStage pdm_stage(const int n) {
    PdmStage s;
    if ((int64_t)n * n <= PDM_LDS_CD) {
        s.P = PDM_LDS_CD / (n * n) < 64 ? PDM_LDS_CD / (n * n) : 64;
        s.NB = n;
    } else {
        s.P = 1;
        s.NB = PDM_LDS_CD / n;
    }
    return s;
}

// ---------------------------------------------------------------- checks
static int pdm_check(const char* fn, int dk, int n, const int32_t* mesh, double mu, double kT, int64_t nt, const int32_t* ij, const int32_t* R,
                     int64_t& npts) {
    int rc = occ_mesh_check(fn, dk, n, mesh, npts);
    if (rc) return rc;
    TBK_REQUIRE(std::isfinite(mu), TBK_EINVAL, "%s: the Fermi level must be finite", fn);
    rc = kubo_kt_check(fn, kT, false);
    if (rc) return rc;
    TBK_REQUIRE(nt >= 1 && nt <= kPdmTripleMax && ij && R, TBK_EINVAL, "%s: %lld triples (1..2^20)", fn, (long long)nt);
    for (int64_t p = 0; p < nt; ++p) {
        TBK_REQUIRE(ij[2 * p] >= 0 && ij[2 * p] < n && ij[2 * p + 1] >= 0 && ij[2 * p + 1] < n, TBK_EINVAL,
                    "%s: triple %lld has a state index out of range", fn, (long long)p);
        for (int d = 0; d < dk; ++d)
            TBK_REQUIRE(R[p * dk + d] > -kOccRAbsMax && R[p * dk + d] < kOccRAbsMax, TBK_EINVAL,
                        "%s: triple %lld has a lattice component of 2^30 or more", fn, (long long)p);
    }
    return TBK_OK;
}

// ---------------------------------------------------------------- the partition
// Group g of G takes the points [g cnt / G, (g + 1) cnt / G) of a chunk of cnt: about four stages of P points, or eight points.
// A launch takes TL triples (whole tiles): part[G][TL] stays under kPdmPartCap.
struct PdmPart {
    int64_t npts = 0, chunk = 0, nchunks = 0;
    int P = 0, NB = 0, G = 0;
    int64_t TL = 0;
};
static PdmPart pdm_partition(int n, int64_t npts) {
    PdmPart p;
    const PdmStage s = pdm_stage(n);
    p.npts = npts;
    p.chunk = kubo_chunk_len(n, npts);
    p.nchunks = (npts + p.chunk - 1) / p.chunk;
    p.P = s.P, p.NB = s.NB;
    const int64_t per = std::max<int64_t>(4 * (int64_t)p.P, 8);
    p.G = (int)std::max<int64_t>(1, std::min<int64_t>((p.chunk + per - 1) / per, kPdmGroupsMax));
    p.TL = kPdmPartCap / p.G / PDM_TILE * PDM_TILE;
    return p;
}

// ---------------------------------------------------------------- the workspace of the stage
// The device buffers occ_pairs_stage works in, beside the chunk's eigenpairs: the triples (ij[nt][2], R[nt][dk] int32), part[G][min(TL, nt)]
// c128 and acc[nt] c128.  PdmPlan lays them out in one block behind 256 leading bytes, with the chunk workspace of a stand-alone call.
struct PdmPlan : PdmPart {
    int64_t nt = 0, part_cd = 0;
    size_t off_ij = 0, off_R = 0, off_acc = 0, off_part = 0, off_chunks = 0, total = 0;
    KuboChunks cw;
};
static PdmPlan pdm_plan(int n, int dk, int64_t npts, int64_t nt, bool with_chunks) {
    PdmPlan p;
    static_cast<PdmPart&>(p) = pdm_partition(n, npts);
    p.nt = nt;
    p.part_cd = (int64_t)p.G * std::min<int64_t>(p.TL, nt);
    p.off_ij = 256;
    p.off_R = p.off_ij + al256((size_t)nt * 2 * sizeof(int32_t));
    p.off_acc = p.off_R + al256((size_t)nt * dk * sizeof(int32_t));
    p.off_part = p.off_acc + al256((size_t)nt * sizeof(cd));
    p.off_chunks = p.off_part + al256((size_t)p.part_cd * sizeof(cd));
    if (with_chunks) p.cw = KuboChunks(n, dk, p.chunk, 0, 0, 0);
    p.total = p.off_chunks + (with_chunks ? p.cw.bytes() : 0);
    return p;
}
