// tbk_chim.h -- the host-only part of tbk_chim.hip (the orbital-resolved susceptibility matrix and its RPA on k meshes, DESIGN.md
// section 28): the argument checks of tbk_susceptibility_matrix_mesh behind those of tbk_chi.h and the plan of one call -- the chunk of
// mesh points, the k-groups, the frequency tiles and entry blocks of the frequency stage, the points per batch of the LDS kernel and
// the layout of the scratch block.  No device call: check/chim_plan_check.cpp drives it on the host alone (make chim-check).
//
// Everything here but acc, the interaction and the result is a function of (mesh, n, dim_k, nw, na) alone -- NOT of nq: a q of the
// list is worked through with the same chunks, groups, tiles and blocks whatever stands beside it.
#pragma once
#include "tbk_chi.h"

#define CHIM_LDS_D 4032                                  // doubles of LDS per workgroup of k_chim_static (31.5 KiB: five workgroups per CU)
static const int kChimSelMax = 16;                       // selected states at most (na^2 <= 256: one workgroup's lanes)
static const int64_t kChimOutCap = (int64_t)1 << 22;     // nq max(nw, 1) na^2 at most
static const int kChimBlock = 4;                         // entries (a, b) per workgroup of k_chim_omega
// rows per q from which the group sum takes one lane per row (k_group_rows_lanes: 64 workgroups and more, coalesced, the groups one
// after the other) instead of one workgroup per row (k_group_rows: strided reads)
static const int64_t kChimLaneRows = 16384;

// doubles per point of k_chim_static's batch: the na selected components of U(k) and U(k+q) (complex) and the n^2 weights
static inline int chim_point_doubles(int n, int na) { return 4 * n * na + n * n; }
static inline int chim_lds_points(int n, int na) { return std::max(1, std::min(64, CHIM_LDS_D / chim_point_doubles(n, na))); }

struct ChimPlan {
    bool dynamic = false, lds = false, tables = false, rpa = false, lane_rows = false;
    int na = 0, nab = 0;   // selected states, entries (a, b)
    int64_t npts = 0, chunk = 0, nchunks = 0;
    int P = 0;             // points per batch of k_chim_static (lds)
    int G = 0;             // k-groups of a chunk
    int EB = 0;            // entries per workgroup of k_chim_omega (1 for a single entry)
    unsigned ntile = 0, neb = 0;   // frequency tiles, entry blocks
    int64_t nrows = 0;     // doubles per q: 2 na^2 max(nw, 1)
    int64_t nmat = 0;      // matrices of the result: nq max(nw, 1)
    int64_t part_doubles = 0, acc_doubles = 0, out_cd = 0;
    // the chunk's first extra buffer holds k + q, E(k+q) and U(k+q) at these offsets; the second the records (d, c) or the static
    // weights L; the third the tables X (at 0) and Y (at off_y)
    size_t off_e2 = 0, off_v2 = 0, x0 = 0, x1 = 0, x2 = 0, off_y = 0;
    // the scratch block: 256 leading bytes, omega, the q list, the selection, V, acc[nq][nrows], part[G][nrows], the result
    // (chi0[nmat][na^2], then chi[nmat][na^2] and det[nmat] with an interaction), then the chunk workspace
    size_t off_om = 0, off_q = 0, off_sel = 0, off_v = 0, off_acc = 0, off_part = 0, off_out = 0, off_chunks = 0, total = 0;
    KuboChunks cw;
};

// the checks of tbk_susceptibility_matrix_mesh behind its pointers (v null: no interaction); npts = the points of the mesh
static int chim_check(const char* fn, int dk, int n, const int32_t* mesh, int nq, const double* q, int nomega, const double* omega,
                      double eta, double mu, double kT, int nsel, const int32_t* sel, const double* v, int nvq, bool want_rpa,
                      bool want_det, int64_t& npts) {
    int rc = chi_check(fn, dk, n, mesh, nq, q, nomega, omega, eta, mu, kT, TBK_CHI_MATRIX_ELEMENTS, npts);
    if (rc) return rc;
    TBK_REQUIRE(nsel >= 1 && nsel <= kChimSelMax, TBK_EINVAL, "%s: nsel=%d (1..%d selected states)", fn, nsel, kChimSelMax);
    for (int i = 0; i < nsel; ++i) {
        TBK_REQUIRE(sel[i] >= 0 && sel[i] < n, TBK_EINVAL, "%s: selected state %d is %d (0..%d)", fn, i, sel[i], n - 1);
        for (int j = 0; j < i; ++j) TBK_REQUIRE(sel[j] != sel[i], TBK_EINVAL, "%s: state %d is selected twice", fn, sel[i]);
    }
    const int64_t per = (int64_t)std::max(nomega, 1) * nsel * nsel;
    TBK_REQUIRE((int64_t)nq * per <= kChimOutCap, TBK_EINVAL, "%s: nq * max(nomega, 1) * nsel^2 = %lld (at most %lld)", fn,
                (long long)nq * per, (long long)kChimOutCap);
    if (!v) {
        TBK_REQUIRE(nvq == 0, TBK_EINVAL, "%s: nvq=%d without an interaction (0)", fn, nvq);
        TBK_REQUIRE(!want_rpa && !want_det, TBK_EINVAL, "%s: chi_rpa and det need an interaction", fn);
        return TBK_OK;
    }
    TBK_REQUIRE(nvq == 1 || nvq == nq, TBK_EINVAL, "%s: nvq=%d (1 matrix, or one per q: %d)", fn, nvq, nq);
    TBK_REQUIRE(want_rpa, TBK_EINVAL, "%s: an interaction needs chi_rpa", fn);
    for (int64_t j = 0; j < (int64_t)nvq * nsel * nsel * 2; ++j)
        TBK_REQUIRE(std::isfinite(v[j]), TBK_EINVAL, "%s: the interaction is not finite (matrix %lld)", fn,
                    (long long)(j / (2 * nsel * nsel)));
    return TBK_OK;
}

// the plan of a checked call
static ChimPlan chim_plan(int n, int dk, int64_t npts, int nq, int nw, int na, int nvq) {
    ChimPlan p;
    const size_t nn = (size_t)n * n, D = sizeof(double);
    p.dynamic = nw > 0;
    p.lds = !p.dynamic && n <= 32;
    p.tables = !p.lds;
    p.rpa = nvq > 0;
    p.na = na;
    p.nab = na * na;
    p.npts = npts;
    // at most kKuboChunkBytes of eigenvectors (and of records), and as many of the two tables X, Y where they are formed
    p.chunk = kubo_chunk_len(n, npts);
    if (p.tables) p.chunk = std::min<int64_t>(p.chunk, std::max<int64_t>(1, (int64_t)(kKuboChunkBytes / ((size_t)2 * n * p.nab * sizeof(cd)))));
    p.nchunks = (npts + p.chunk - 1) / p.chunk;
    p.P = chim_lds_points(n, na);
    p.nrows = 2 * (int64_t)p.nab * std::max(nw, 1);
    p.nmat = (int64_t)nq * std::max(nw, 1);
    p.G = (int)std::max<int64_t>(1, std::min<int64_t>({kPairPartCap / p.nrows, (int64_t)kPairGroupsMax, p.chunk}));
    p.lane_rows = p.nrows >= kChimLaneRows;
    p.EB = p.nab == 1 ? 1 : kChimBlock;
    p.neb = (unsigned)((p.nab + p.EB - 1) / p.EB);
    p.ntile = (unsigned)((nw + kPairTile - 1) / kPairTile);
    p.part_doubles = p.G * p.nrows;
    p.acc_doubles = (int64_t)nq * p.nrows;
    p.out_cd = p.nmat * p.nab + (p.rpa ? p.nmat * p.nab + p.nmat : 0);
    p.off_e2 = al256((size_t)p.chunk * dk * D);
    p.off_v2 = p.off_e2 + al256((size_t)p.chunk * n * D);
    p.x0 = p.off_v2 + al256((size_t)p.chunk * nn * sizeof(cd));
    p.x1 = p.tables ? (size_t)p.chunk * nn * (p.dynamic ? 2 : 1) * D : 0;
    p.off_y = p.tables ? al256((size_t)p.chunk * n * p.nab * sizeof(cd)) : 0;
    p.x2 = p.tables ? p.off_y + (size_t)p.chunk * n * p.nab * sizeof(cd) : 0;
    p.cw = KuboChunks(n, dk, p.chunk, p.x0, p.x1, p.x2);
    p.off_om = 256;
    p.off_q = p.off_om + al256((size_t)nw * D);
    p.off_sel = p.off_q + al256((size_t)nq * dk * D);
    p.off_v = p.off_sel + al256((size_t)na * sizeof(int32_t));
    p.off_acc = p.off_v + al256((size_t)nvq * p.nab * sizeof(cd));
    p.off_part = p.off_acc + al256((size_t)p.acc_doubles * D);
    p.off_out = p.off_part + al256((size_t)p.part_doubles * D);
    p.off_chunks = p.off_out + al256((size_t)p.out_cd * sizeof(cd));
    p.total = p.off_chunks + p.cw.bytes();
    return p;
}
