// tbk_td.h -- the host-only part of tbk_td.hip (real-time propagation under a uniform time-dependent field in the velocity gauge,
// k -> k + kappa(t): the current and the energy on k meshes and the propagator of a driven period on k lists):
// the argument checks of tbk_propagate_mesh and tbk_propagator_list, the caps, and the plan of a call -- the chunk, the points per
// workgroup and the padded row of the LDS step, the tiles of the wide step, the k-groups of the measurement -- with the layout of the
// scratch block.  No device call: check/td_plan_check.cpp drives it on the host alone (make td-check).
//
// Caps:  nsta <= 2048 (the dense solver);  1 <= nt <= kTdStepsMax = 65536 steps;  the carried states -- N_k nprop nsta c128 on a mesh
// (nprop = nocc bands, or nsta with Fermi weights), nk nsta^2 on a list -- at most kTdStateCap = 2^26 c128 (1 GiB): they stay resident
// for the whole call.
//
// Partition, a function of (mesh or nk, nsta, dim_k, nprop) alone -- NOT of nt, dt or the shifts:
//   chunk   points per solve: kubo_chunk_len(nsta, N_k)
//   P, LD   nsta <= 32: points per workgroup of k_td_step_lds and the row length of its eigenvectors in LDS (nsta | 1: odd, so that the
//           16 lanes of one ds_read_b128 group, each on another eigenvector, fall on different banks)
//   T, TM   nsta > 32: 16 x 16 tiles per nsta and per nprop of k_td_tile
//   G       k-groups of the measurement: group g takes the points [g cnt / G, (g + 1) cnt / G) of a chunk of cnt
// A time step does the same work on the same partition whatever stands behind it, so a run of nt' < nt steps gives the bits of the
// first nt' + 1 entries of the longer run.
#pragma once
#include "tbk_kubo.h"

#define TD_LDS_U 1056                                     // c128 of eigenvectors in LDS per workgroup of k_td_step_lds (32 rows of 33)
#define TD_LDS_C 1024                                     // c128 of carried states / coefficients beside them
#define TD_LDS_PN 256                                     // (point, state) pairs of a workgroup at most: their phases
#define TD_ES 4                                           // coefficients per lane at most (TD_LDS_C / 256)
#define TD_OB_PB 16                                       // points per batch of k_td_observe_rvec
#define TD_OB_SLOTS 136                                   // slots of 16 states: its sigma[TD_OB_PB][136] is 34 KiB of LDS
#define TD_NR 4                                           // measured sums per time at most: E and dim_k components of J
static const int kTdStatesMax = 2048;                     // the dense solver's limit
static const int kTdStepsMax = 65536;                     // time steps of one call
static const int64_t kTdStateCap = (int64_t)1 << 26;      // c128 of carried states (1 GiB)
static const int kTdGroupsMax = 512;                      // k-groups of the measurement

struct TdKappa {
    double v[3];
};
// kappa at time j and at the midpoint of step j -> j + 1: plain double arithmetic on the host, 0.5 (a + b) as the reference forms it
static inline TdKappa td_kappa(const double* shift, int dk, int64_t j) {
    TdKappa k{{0.0, 0.0, 0.0}};
    for (int d = 0; d < dk; ++d) k.v[d] = shift[j * dk + d];
    return k;
}
static inline TdKappa td_kappa_mid(const double* shift, int dk, int64_t j) {
    TdKappa k{{0.0, 0.0, 0.0}};
    for (int d = 0; d < dk; ++d) k.v[d] = 0.5 * (shift[j * dk + d] + shift[(j + 1) * dk + d]);
    return k;
}

// ---------------------------------------------------------------- checks
static int td_common_check(const char* fn, int dk, int n, int nt, const double* shift, double dt) {
    TBK_REQUIRE(dk >= 1 && dk <= 3, TBK_EINVAL, "%s: dim_k=%d (a uniform field needs 1, 2 or 3 periodic dimensions)", fn, dk);
    TBK_REQUIRE(n >= 1 && n <= kTdStatesMax, TBK_EINVAL, "%s: nsta=%d (1..%d states, the dense solver's limit)", fn, n, kTdStatesMax);
    TBK_REQUIRE(nt >= 1 && nt <= kTdStepsMax, TBK_EINVAL, "%s: nt=%d (1..%d time steps)", fn, nt, kTdStepsMax);
    TBK_REQUIRE(std::isfinite(dt) && dt > 0.0, TBK_EINVAL, "%s: dt must be finite and > 0", fn);
    TBK_REQUIRE(shift, TBK_EINVAL, "%s: null shift", fn);
    for (int64_t j = 0; j < ((int64_t)nt + 1) * dk; ++j)
        TBK_REQUIRE(std::isfinite(shift[j]), TBK_EINVAL, "%s: the shift at time %lld is not finite", fn, (long long)(j / dk));
    return TBK_OK;
}
// tbk_propagate_mesh; npts = the mesh points, nprop = the carried states per point (nocc bands, or all nsta with Fermi weights)
static int td_mesh_check(const char* fn, int dk, int n, const int32_t* mesh, int nt, const double* shift, double dt, int nocc,
                         const int32_t* occ, double mu, double kT, int64_t& npts, int& nprop) {
    int rc = td_common_check(fn, dk, n, nt, shift, dt);
    if (rc) return rc;
    TBK_REQUIRE(mesh, TBK_EINVAL, "%s: null mesh", fn);
    rc = kubo_mesh_points(fn, dk, mesh, npts);
    if (rc) return rc;
    TBK_REQUIRE(npts < ((int64_t)1 << 31), TBK_EINVAL, "%s: a mesh of %lld points (fewer than 2^31)", fn, (long long)npts);
    if (occ) {
        TBK_REQUIRE(nocc >= 1 && nocc <= n, TBK_EINVAL, "%s: nocc=%d (1..%d)", fn, nocc, n);
        std::vector<char> seen((size_t)n, 0);
        for (int i = 0; i < nocc; ++i) {
            TBK_REQUIRE(occ[i] >= 0 && occ[i] < n, TBK_EINVAL, "%s: occ[%d]=%d outside [0, %d)", fn, i, occ[i], n);
            TBK_REQUIRE(!seen[(size_t)occ[i]], TBK_EINVAL, "%s: band %d appears twice in occ", fn, occ[i]);
            seen[(size_t)occ[i]] = 1;
        }
        nprop = nocc;
    } else {
        TBK_REQUIRE(nocc == 0, TBK_EINVAL, "%s: nocc=%d without occ", fn, nocc);
        rc = kubo_occupation_check(fn, kT, mu);
        if (rc) return rc;
        nprop = n;
    }
    TBK_REQUIRE(npts * nprop * n <= kTdStateCap, TBK_EINVAL,
                "%s: %lld points x %d carried states x %d components = %lld c128 stay resident (at most %lld): coarsen the mesh or select fewer bands",
                fn, (long long)npts, nprop, n, (long long)(npts * nprop * n), (long long)kTdStateCap);
    return TBK_OK;
}
// tbk_propagator_list
static int td_list_check(const char* fn, int dk, int n, int64_t nk, const double* k, int nt, const double* shift, double dt) {
    int rc = td_common_check(fn, dk, n, nt, shift, dt);
    if (rc) return rc;
    TBK_REQUIRE(nk >= 1 && k, TBK_EINVAL, "%s: nk=%lld (at least one k-point)", fn, (long long)nk);
    TBK_REQUIRE(nk <= kTdStateCap && nk * n * n <= kTdStateCap, TBK_EINVAL, "%s: nk * nsta^2 = %lld c128 stay resident (at most %lld): split k_list", fn,
                (long long)(nk * n * n), (long long)kTdStateCap);
    for (int64_t j = 0; j < nk * dk; ++j) TBK_REQUIRE(std::isfinite(k[j]), TBK_EINVAL, "%s: k-point %lld is not finite", fn, (long long)(j / dk));
    return TBK_OK;
}

// ---------------------------------------------------------------- the plan
// the measurement walks the terms by lattice vector (k_td_observe_rvec) for 5 .. 16 states when the model keeps them so (nR > 0, at most
// 256 vectors): a property of the model alone.  Below 5 states a slot has too few terms for the batches to pay.
static inline bool td_observe_by_vector(int n, int nR) { return n >= 5 && n <= 16 && nR > 0; }
// points per workgroup of k_td_step_lds: their eigenvectors in rows of LD, their carried states and their phases in LDS
static inline int td_lds_row(int n) { return n | 1; }
static inline int td_lds_points(int n) {
    return std::max(1, std::min({64, TD_LDS_U / (n * td_lds_row(n)), TD_LDS_C / (n * n), TD_LDS_PN / n}));
}

struct TdPlan {
    bool lds = false, mesh = false;
    int n = 0, dk = 0, nprop = 0, nr = 0;   // states, dimensions, carried states per point, measured sums per time (1 + dim_k; list: 0)
    int64_t npts = 0, chunk = 0, nchunks = 0;
    int P = 0, LD = 0;      // lds: points per workgroup, row length of the eigenvectors
    int T = 0, TM = 0;      // not lds: 16 x 16 tiles per nsta and per nprop
    int G = 0;              // k-groups of the measurement (mesh)
    int64_t psi_cd = 0;     // npts nprop nsta
    // the scratch block: 256 leading bytes, the k list (list call), the band selection (int32), psi[nprop][npts][nsta], the weights
    // fw[nprop][npts], kpop[nsta][npts], pop[nsta], obs[nt + 1][nr], part[G][nr], then the chunk workspace, whose first extra buffer
    // holds the unshifted k of the chunk (mesh) and whose second holds the coefficients X[chunk][nprop][nsta] of the wide step
    size_t off_k = 0, off_sel = 0, off_psi = 0, off_fw = 0, off_kpop = 0, off_pop = 0, off_obs = 0, off_part = 0, off_chunks = 0, total = 0;
    KuboChunks cw;
};
static TdPlan td_plan(int n, int dk, int64_t npts, int nprop, int nt, bool mesh) {
    TdPlan p;
    const size_t D = sizeof(double);
    p.lds = n <= 32;
    p.mesh = mesh;
    p.n = n, p.dk = dk, p.nprop = nprop, p.npts = npts;
    p.nr = mesh ? 1 + dk : 0;
    p.chunk = kubo_chunk_len(n, npts);
    p.nchunks = (npts + p.chunk - 1) / p.chunk;
    p.LD = td_lds_row(n);
    p.P = p.lds ? td_lds_points(n) : 0;
    p.T = (n + 15) / 16;
    p.TM = (nprop + 15) / 16;
    p.G = mesh ? (int)std::max<int64_t>(1, std::min<int64_t>((p.chunk + 7) / 8, kTdGroupsMax)) : 0;
    p.psi_cd = npts * nprop * n;
    p.cw = KuboChunks(n, dk, p.chunk, mesh ? (size_t)p.chunk * dk * D : 0, p.lds ? 0 : (size_t)p.chunk * nprop * n * sizeof(cd), 0);
    p.off_k = 256;
    p.off_sel = p.off_k + al256(mesh ? 0 : (size_t)npts * dk * D);
    p.off_psi = p.off_sel + al256((size_t)nprop * sizeof(int32_t));
    p.off_fw = p.off_psi + al256((size_t)p.psi_cd * sizeof(cd));
    p.off_kpop = p.off_fw + al256(mesh ? (size_t)nprop * npts * D : 0);
    p.off_pop = p.off_kpop + al256(mesh ? (size_t)n * npts * D : 0);
    p.off_obs = p.off_pop + al256(mesh ? (size_t)n * D : 0);
    p.off_part = p.off_obs + al256(mesh ? ((size_t)nt + 1) * p.nr * D : 0);
    p.off_chunks = p.off_part + al256(mesh ? (size_t)p.G * p.nr * D : 0);
    p.total = p.off_chunks + p.cw.bytes();
    return p;
}
