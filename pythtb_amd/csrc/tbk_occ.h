// tbk_occ.h -- the host-only part of tbk_occ.hip (the Fermi level from the filling, the thermodynamic sums and the density matrix
// on k meshes): the argument checks of tbk_thermodynamics_mesh, tbk_fermi_level_mesh and
// tbk_density_matrix_mesh, the order-preserving integer key of a double that the Fermi selection bisects on, and the plan of a call --
// the groups of the level scans, the chunk, groups, points per workgroup and R tiles of the density matrix, and the layout of the
// scratch block.  No device call: check/occ_plan_check.cpp drives it on the host alone (make occ-check).
//
// Every partition here is a function of (mesh, n, dim_k) alone -- NOT of the number of Fermi levels, fillings or lattice vectors: a
// level, a filling or an R is worked through with the same groups whatever stands beside it, so it gives the same bits alone and
// inside a longer list.
#pragma once
#include <cfloat>
#include "tbk_lat.h"

#define OCC_RB 4                                         // lattice vectors per workgroup of the density-matrix kernels
static const int kOccFillMax = 64;                       // fillings of one tbk_fermi_level_mesh call
static const int64_t kOccOutCap = (int64_t)1 << 22;      // nR nsta^2 at most (64 MiB of c128)
static const int64_t kOccPartCap = (int64_t)1 << 22;     // c128 of group partials per launch (64 MiB)
static const int kOccGroupsMax = 512;                    // k-groups of a chunk of the density matrix
static const int kOccScanGroupsMax = 1024;               // groups of a level scan
static const int kOccSteps = 64;                         // bisection steps on the 64-bit key: the bracket ends on neighbouring doubles

// ---------------------------------------------------------------- the ordered key of a double
// key(a) < key(b) exactly when a < b for finite doubles (-0 sorts just below +0): the bit pattern with the sign bit flipped for
// positive values and every bit flipped for negative ones
__host__ __device__ inline uint64_t occ_key(const double x) {
    uint64_t b;
    memcpy(&b, &x, sizeof b);
    return (b >> 63) ? ~b : (b | ((uint64_t)1 << 63));
}
__host__ __device__ inline double occ_unkey(const uint64_t k) {
    const uint64_t b = (k >> 63) ? (k & ~((uint64_t)1 << 63)) : ~k;
    double x;
    memcpy(&x, &b, sizeof x);
    return x;
}

// ---------------------------------------------------------------- checks
// the mesh of a model with dim_k 1..3 and 1..2048 states; npts = its points
static int occ_mesh_check(const char* fn, int dk, int n, const int32_t* mesh, int64_t& npts) {
    int rc = kubo_mesh_dim(fn, dk);
    if (rc) return rc;
    TBK_REQUIRE(n >= 1 && n <= 2048, TBK_EINVAL, "%s: nsta=%d (1..2048 states)", fn, n);
    rc = kubo_mesh_points(fn, dk, mesh, npts);
    if (rc) return rc;
    TBK_REQUIRE(npts < ((int64_t)1 << 31), TBK_EINVAL, "%s: a mesh of %lld points (fewer than 2^31)", fn, (long long)npts);
    return TBK_OK;
}
static int occ_thermo_check(const char* fn, int dk, int n, const int32_t* mesh, int nmu, const double* mu, double kT, int64_t& npts) {
    int rc = occ_mesh_check(fn, dk, n, mesh, npts);
    if (!rc) rc = kubo_levels_check(fn, nmu, mu, 1);
    if (!rc) rc = kubo_kt_check(fn, kT, false);
    return rc ? rc : kubo_levels_finite(fn, nmu, mu);
}
// the fillings of tbk_fermi_level_mesh; target[j] = n_electrons[j] N_k, at kT = 0 the integer count c within 1e-6 of it
static int occ_fermi_check(const char* fn, int dk, int n, const int32_t* mesh, int nfill, const double* nel, double kT, int want_edges,
                           int64_t& npts, std::vector<double>& target) {
    int rc = occ_mesh_check(fn, dk, n, mesh, npts);
    if (rc) return rc;
    TBK_REQUIRE(nfill >= 1 && nfill <= kOccFillMax && nel, TBK_EINVAL, "%s: %d values of n_electrons (1..%d)", fn, nfill, kOccFillMax);
    rc = kubo_kt_check(fn, kT, false);
    if (rc) return rc;
    TBK_REQUIRE(!(want_edges && kT > 0.0), TBK_EINVAL, "%s: the band edges exist at kT = 0 only", fn);
    target.resize((size_t)nfill);
    const double total = (double)n * (double)npts;
    for (int j = 0; j < nfill; ++j) {
        TBK_REQUIRE(std::isfinite(nel[j]), TBK_EINVAL, "%s: n_electrons[%d] is not finite", fn, j);
        if (kT > 0.0) {
            TBK_REQUIRE(nel[j] > 0.0 && nel[j] < (double)n, TBK_EINVAL, "%s: n_electrons[%d]=%.17g outside (0, %d)", fn, j, nel[j], n);
            target[j] = nel[j] * (double)npts;
            continue;
        }
        const double c = nel[j] * (double)npts, r = std::nearbyint(c);
        TBK_REQUIRE(fabs(c - r) <= 1e-6, TBK_EINVAL, "%s: n_electrons[%d] times the %lld mesh points is %.17g, not an integer", fn, j,
                    (long long)npts, c);
        TBK_REQUIRE(r >= 1.0 && r <= total - 1.0, TBK_EINVAL, "%s: n_electrons[%d] gives %.0f of %.0f levels (1..%.0f)", fn, j, r, total,
                    total - 1.0);
        target[j] = r;
    }
    return TBK_OK;
}
static int occ_dm_check(const char* fn, int dk, int n, const int32_t* mesh, double mu, double kT, int nR, const int32_t* R, int64_t& npts) {
    int rc = occ_mesh_check(fn, dk, n, mesh, npts);
    if (rc) return rc;
    TBK_REQUIRE(std::isfinite(mu), TBK_EINVAL, "%s: the Fermi level must be finite", fn);
    rc = kubo_kt_check(fn, kT, false);
    if (rc) return rc;
    rc = lat_R_check(fn, dk, nR, R);
    if (rc) return rc;
    TBK_REQUIRE((int64_t)nR * n * n <= kOccOutCap, TBK_EINVAL, "%s: nR * nsta^2 = %lld (at most %lld)", fn, (long long)nR * n * n,
                (long long)kOccOutCap);
    return TBK_OK;
}

// ---------------------------------------------------------------- the level scans (thermodynamics, Fermi selection)
// The L = n N_k levels of the mesh stay on the device as one flat array.  Group g of G walks the levels [g L / G, (g + 1) L / G).
static inline int occ_scan_groups(int64_t nlev) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((nlev + 1023) / 1024, kOccScanGroupsMax));
}
struct OccScanPlan {
    int64_t npts = 0, nlev = 0;
    int G = 0;              // groups of the thermal scan / of a bisection pass
    int gx = 0;             // workgroups of the kT = 0 Fermi scan (tbk_kubo.h's k_kubo_fermi; thermodynamics only)
    int nq = 0;             // sums per level: thermodynamics 2 (kT = 0: N, E) or 3 (N, E, S); Fermi selection 1
    int64_t nrows = 0, part_doubles = 0;
    // behind the k list and the eigenvalues of the whole mesh: part, rows, the levels; the Fermi selection also its brackets
    // (lo, hi keys), the targets and the edges
    size_t off_k = 0, off_e = 0, off_part = 0, off_rows = 0, off_mu = 0, off_lo = 0, off_hi = 0, off_target = 0, off_edges = 0, total = 0;
};
static OccScanPlan occ_scan_plan(int n, int dk, int64_t npts, int nmu, bool thermal, bool fermi) {
    OccScanPlan p;
    const size_t D = sizeof(double);
    p.npts = npts;
    p.nlev = npts * n;
    p.G = occ_scan_groups(p.nlev);
    PlaneArgs P{};
    P.nplane = P.npts = npts;
    P.nslice = 1;
    p.nq = fermi ? 1 : (thermal ? 3 : 2);
    p.gx = !fermi && !thermal ? kubo_fermi_gx(P, n, nmu, 2) : 0;
    p.nrows = (int64_t)nmu * p.nq;
    // the Fermi selection's last pass keeps two values per (filling, group): the count up to the lower edge and the next level above
    p.part_doubles = fermi ? (int64_t)2 * nmu * p.G : p.nrows * (p.gx ? p.gx : p.G);
    p.off_k = 256;
    p.off_e = p.off_k + al256((size_t)npts * dk * D);
    p.off_part = p.off_e + al256((size_t)p.nlev * D);
    p.off_rows = p.off_part + al256((size_t)p.part_doubles * D);
    p.off_mu = p.off_rows + al256((size_t)p.nrows * D);
    p.off_lo = p.off_mu + al256((size_t)nmu * D);
    p.off_hi = p.off_lo + (fermi ? al256((size_t)nmu * D) : 0);
    p.off_target = p.off_hi + (fermi ? al256((size_t)nmu * D) : 0);
    p.off_edges = p.off_target + (fermi ? al256((size_t)nmu * D) : 0);
    p.total = p.off_edges + (fermi ? al256((size_t)2 * nmu * D) : 0);
    return p;
}

// ---------------------------------------------------------------- the density matrix
// the partition of tbk_lat.h with every state kept and OCC_RB lattice vectors per workgroup, and
struct OccDmPlan : LatPart {
    int RT = 0;             // lattice vectors per launch: part[G][RT][n^2] stays under kOccPartCap
    int64_t part_cd = 0, acc_cd = 0;
    // the scratch block: 256 leading bytes, the R list (int32), acc[nR][n^2], part[G][RT][n^2], then the chunk workspace, whose first
    // extra buffer holds the weights f[n][chunk]
    size_t off_R = 0, off_acc = 0, off_part = 0, off_chunks = 0, total = 0;
    KuboChunks cw;
};
static OccDmPlan occ_dm_plan(int n, int dk, int64_t npts, int nR) {
    OccDmPlan p;
    const int64_t nn = (int64_t)n * n;
    static_cast<LatPart&>(p) = lat_partition(n, n, npts, OCC_RB, kOccPartCap, kOccGroupsMax);
    int64_t rt = std::max<int64_t>(1, kOccPartCap / (p.G * nn));
    if (rt >= OCC_RB) rt -= rt % OCC_RB;
    p.RT = (int)std::min<int64_t>(rt, kOccRMax);
    p.part_cd = (int64_t)p.G * std::min(p.RT, nR) * nn;
    p.acc_cd = (int64_t)nR * nn;
    p.cw = KuboChunks(n, dk, p.chunk, (size_t)p.chunk * n * sizeof(double), 0, 0);
    p.off_R = 256;
    p.off_acc = p.off_R + al256((size_t)nR * dk * sizeof(int32_t));
    p.off_part = p.off_acc + al256((size_t)p.acc_cd * sizeof(cd));
    p.off_chunks = p.off_part + al256((size_t)p.part_cd * sizeof(cd));
    p.total = p.off_chunks + p.cw.bytes();
    return p;
}
