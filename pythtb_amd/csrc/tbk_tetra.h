// tbk_tetra.h -- the host-only part of tbk_tetra.hip (the linear tetrahedron method on k meshes): the
// arithmetic of one simplex (host and device: the ordering of its corners, the occupation weights w_i(E) and, carried along as the
// derivative part of a dual number, the DOS weights d_i(E) = dw_i/dE), the argument checks of tbk_tetrahedron_dos_mesh,
// tbk_tetrahedron_weights_mesh and tbk_tetrahedron_fermi_level_mesh, the plans of their launches and the layout of their scratch
// blocks.  No device call: check/tetra_plan_check.cpp drives it on the host alone (make tetra-check).
//
// The simplices: the cell with origin o is cut along the diagonal o -> o + (1, .., 1) into dim! simplices, one per permutation
// (a, b, c) of the axes, with corner slots 0..dim = o, o + e_a, o + e_a + e_b, o + e_a + e_b + e_c (periodic).  Every simplex is
// worked with volume 1; the callers divide by the simplices of the mesh at the end.
//
// Every partition here is a function of (mesh, n, dim_k) alone -- NOT of the number of energies, bands per launch or selected
// states: an energy, a band or a state is worked through with the same groups whatever stands beside it.
#pragma once
#include "tbk_occ.h"

static const int kTetEnergyMax = 65536;                  // energies of one tbk_tetrahedron_dos_mesh call
static const int64_t kTetOutCap = (int64_t)1 << 22;      // doubles per result array at most
static const int64_t kTetPartCap = (int64_t)1 << 23;     // doubles of group partials per launch (64 MiB)
static const int kTetSelMax = 16;                        // selected states of the projected DOS
static const int64_t kTetWeightsMax = (int64_t)1 << 31;  // weights of one tbk_tetrahedron_weights_mesh call
static const int kTetTile = 1024;                       // energies per launch (four blocks of 256 lanes)
static const int kTetCellGroupsMax = 1024;               // k-groups of the cell form
static const int kTetPdosGroupsMax = 512;                // k-groups of a chunk of the projected DOS
static const int kTetTrials = 256;                       // trial energies per round of the Fermi search
static const int kTetRoundsMax = 16;                     // rounds at most (257^8 > 2^64: eight or nine are taken)

// ---------------------------------------------------------------- the simplices of a cell
// axis of step i (0 .. dim - 1) of simplex p (0 .. dim! - 1): the permutations of the axes in lexicographic order
__host__ __device__ constexpr int tet_axis(const int dim, const int p, const int i) {
    if (dim == 1) return 0;
    if (dim == 2) return p == 0 ? i : 1 - i;
    const int a = p / 2, lo = a == 0 ? 1 : 0, hi = a == 2 ? 1 : 2;
    return i == 0 ? a : (((i == 1) == (p % 2 == 0)) ? lo : hi);
}
// corner slot s of simplex p as a bit mask of unit steps from the origin (bit a: + e_a)
__host__ __device__ constexpr int tet_corner(const int dim, const int p, const int s) {
    int m = 0;
    for (int i = 0; i < s; ++i) m |= 1 << tet_axis(dim, p, i);
    return m;
}
__host__ __device__ constexpr int tet_simplices(const int dim) { return dim == 3 ? 6 : dim; }

// ---------------------------------------------------------------- one simplex
// a value and its derivative with respect to E
struct Du {
    double v, d;
};
__host__ __device__ inline Du operator+(const Du a, const Du b) { return Du{a.v + b.v, a.d + b.d}; }
__host__ __device__ inline Du operator-(const Du a, const Du b) { return Du{a.v - b.v, a.d - b.d}; }
__host__ __device__ inline Du operator*(const Du a, const Du b) { return Du{a.v * b.v, a.v * b.d + a.d * b.v}; }
__host__ __device__ inline Du operator*(const double c, const Du a) { return Du{c * a.v, c * a.d}; }
__host__ __device__ inline Du operator-(const double c, const Du a) { return Du{c - a.v, -a.d}; }
// (x - lo) / (hi - lo) and (hi - x) / (hi - lo) for lo <= x <= hi, lo < hi: ratios bounded by 1
__host__ __device__ inline Du tet_up(const double x, const double lo, const double r) { return Du{(x - lo) * r, r}; }
__host__ __device__ inline Du tet_dn(const double x, const double hi, const double r) { return Du{(hi - x) * r, -r}; }

// the corners in ascending order of energy, ties by slot (a stable insertion sort: a swap only where strictly greater); s[i] = the
// slot that ends at position i
template <int NV>
__host__ __device__ inline void tet_sort(double (&e)[NV], int (&s)[NV]) {
#pragma unroll
    for (int i = 0; i < NV; ++i) s[i] = i;
#pragma unroll
    for (int i = 1; i < NV; ++i)
#pragma unroll
        for (int j = i; j > 0; --j)
            if (e[j - 1] > e[j]) {
                const double te = e[j];
                e[j] = e[j - 1];
                e[j - 1] = te;
                const int ts = s[j];
                s[j] = s[j - 1];
                s[j - 1] = ts;
            }
}

// w[i] = (w_i(E), d_i(E)) of the corner at sorted position i, for a simplex of volume 1 with sorted corner energies e.  The level at
// E is occupied (f = [e <= E]): E >= e_max gives 1 / (dim + 1) each and no DOS, E <= e_min nothing; in between the branch whose
// half-open interval holds E, so that every difference divided by is positive.
template <int DIM>
__host__ __device__ inline void tet_eval(const double (&e)[DIM + 1], const double E, Du (&w)[DIM + 1]) {
    if (E >= e[DIM]) {
#pragma unroll
        for (int i = 0; i <= DIM; ++i) w[i] = Du{1.0 / (DIM + 1), 0.0};
        return;
    }
    if (E <= e[0]) {
#pragma unroll
        for (int i = 0; i <= DIM; ++i) w[i] = Du{0.0, 0.0};
        return;
    }
    if constexpr (DIM == 1) {
        const Du t = tet_up(E, e[0], 1.0 / (e[1] - e[0]));
        w[1] = 0.5 * (t * t);
        w[0] = t - w[1];
    } else if constexpr (DIM == 2) {
        const double third = 1.0 / 3.0;
        if (E < e[1]) {
            const Du t2 = tet_up(E, e[0], 1.0 / (e[1] - e[0])), t3 = tet_up(E, e[0], 1.0 / (e[2] - e[0]));
            const Du c = third * (t2 * t3);
            w[0] = c * (3.0 - (t2 + t3));
            w[1] = c * t2;
            w[2] = c * t3;
        } else {
            const Du s1 = tet_dn(E, e[2], 1.0 / (e[2] - e[0])), s2 = tet_dn(E, e[2], 1.0 / (e[2] - e[1]));
            const Du c = third * (s1 * s2);
            w[0] = third - c * s1;
            w[1] = third - c * s2;
            w[2] = third - c * (3.0 - (s1 + s2));
        }
    } else {
        if (E < e[1]) {
            const Du t2 = tet_up(E, e[0], 1.0 / (e[1] - e[0])), t3 = tet_up(E, e[0], 1.0 / (e[2] - e[0])),
                     t4 = tet_up(E, e[0], 1.0 / (e[3] - e[0]));
            const Du c = 0.25 * (t2 * t3 * t4);
            w[0] = c * (4.0 - (t2 + t3 + t4));
            w[1] = c * t2;
            w[2] = c * t3;
            w[3] = c * t4;
        } else if (E < e[2]) {
            const double r31 = 1.0 / (e[2] - e[0]), r41 = 1.0 / (e[3] - e[0]), r32 = 1.0 / (e[2] - e[1]), r42 = 1.0 / (e[3] - e[1]);
            const Du a31 = tet_up(E, e[0], r31), a41 = tet_up(E, e[0], r41), a32 = tet_up(E, e[1], r32), a42 = tet_up(E, e[1], r42);
            const Du b31 = tet_dn(E, e[2], r31), b41 = tet_dn(E, e[3], r41), b32 = tet_dn(E, e[2], r32), b42 = tet_dn(E, e[3], r42);
            const Du c1 = 0.25 * (a31 * a41), c2 = 0.25 * (a41 * a32 * b31), c3 = 0.25 * (a42 * a32 * b41);
            const Du c12 = c1 + c2, c23 = c2 + c3, c123 = c12 + c3;
            w[0] = c1 + c12 * b31 + c123 * b41;
            w[1] = c123 + c23 * b32 + c3 * b42;
            w[2] = c12 * a31 + c23 * a32;
            w[3] = c123 * a41 + c3 * a42;
        } else {
            const Du s1 = tet_dn(E, e[3], 1.0 / (e[3] - e[0])), s2 = tet_dn(E, e[3], 1.0 / (e[3] - e[1])),
                     s3 = tet_dn(E, e[3], 1.0 / (e[3] - e[2]));
            const Du c = 0.25 * (s1 * s2 * s3);
            w[0] = 0.25 - c * s1;
            w[1] = 0.25 - c * s2;
            w[2] = 0.25 - c * s3;
            w[3] = 0.25 - c * (4.0 - (s1 + s2 + s3));
        }
    }
}

// Bloechl's curvature correction of the corner at sorted position i (3-D): g_T / 40 * sum_j (e_j - e_i), g_T = sum_j d_j
__host__ __device__ inline double tet_correction(const double (&e)[4], const Du (&w)[4], const int i) {
    const double g = (w[0].d + w[1].d) + (w[2].d + w[3].d);
    return g * (1.0 / 40.0) * (((e[0] - e[i]) + (e[1] - e[i])) + ((e[2] - e[i]) + (e[3] - e[i])));
}

// ---------------------------------------------------------------- checks
static int tet_energies_check(const char* fn, int nE, const double* en) {
    TBK_REQUIRE(nE >= 1 && nE <= kTetEnergyMax && en, TBK_EINVAL, "%s: nE=%d (1..%d energies)", fn, nE, kTetEnergyMax);
    for (int j = 0; j < nE; ++j) TBK_REQUIRE(std::isfinite(en[j]), TBK_EINVAL, "%s: energy %d is not finite", fn, j);
    return TBK_OK;
}
// nsel = 0 and no list: no projected DOS
static int tet_dos_check(const char* fn, int dk, int n, const int32_t* mesh, int nE, const double* en, int per_band, int nsel,
                         const int32_t* sel, int64_t& npts) {
    int rc = occ_mesh_check(fn, dk, n, mesh, npts);
    if (!rc) rc = tet_energies_check(fn, nE, en);
    if (rc) return rc;
    const int64_t nb = per_band ? n : 1;
    TBK_REQUIRE(nb * nE <= kTetOutCap, TBK_EINVAL, "%s: nsta * nE = %lld (at most %lld)", fn, (long long)(nb * nE), (long long)kTetOutCap);
    if (nsel == 0 && !sel) return TBK_OK;
    TBK_REQUIRE(nsel >= 1 && nsel <= kTetSelMax && sel, TBK_EINVAL, "%s: nsel=%d (1..%d selected states)", fn, nsel, kTetSelMax);
    for (int i = 0; i < nsel; ++i) {
        TBK_REQUIRE(sel[i] >= 0 && sel[i] < n, TBK_EINVAL, "%s: selected state %d is %d (0..%d)", fn, i, sel[i], n - 1);
        for (int j = 0; j < i; ++j) TBK_REQUIRE(sel[j] != sel[i], TBK_EINVAL, "%s: state %d is selected twice", fn, sel[i]);
    }
    TBK_REQUIRE((int64_t)nsel * nb * nE <= kTetOutCap, TBK_EINVAL, "%s: nsel * %snE = %lld (at most %lld)", fn, per_band ? "nsta * " : "",
                (long long)((int64_t)nsel * nb * nE), (long long)kTetOutCap);
    return TBK_OK;
}
static int tet_weights_check(const char* fn, int dk, int n, const int32_t* mesh, double mu, int correction, int derivative, int64_t& npts) {
    int rc = occ_mesh_check(fn, dk, n, mesh, npts);
    if (rc) return rc;
    TBK_REQUIRE(std::isfinite(mu), TBK_EINVAL, "%s: the Fermi level must be finite", fn);
    TBK_REQUIRE(!(correction && dk != 3), TBK_EINVAL, "%s: the curvature correction exists for dim_k = 3 only (dim_k=%d)", fn, dk);
    TBK_REQUIRE(!(correction && derivative), TBK_EINVAL, "%s: the curvature correction applies to the occupation weights, not to their derivative", fn);
    TBK_REQUIRE((int64_t)n * npts <= kTetWeightsMax, TBK_EINVAL, "%s: nsta * N_k = %lld weights (at most 2^31)", fn, (long long)((int64_t)n * npts));
    return TBK_OK;
}
static int tet_fermi_check(const char* fn, int dk, int n, const int32_t* mesh, double nel, int64_t& npts) {
    int rc = occ_mesh_check(fn, dk, n, mesh, npts);
    if (rc) return rc;
    TBK_REQUIRE(std::isfinite(nel) && nel > 0.0 && nel < (double)n, TBK_EINVAL, "%s: n_electrons=%.17g outside (0, %d)", fn, nel, n);
    return TBK_OK;
}
// the band m whose top is the lower edge where n_electrons is within 1e-9 of an integer m in [1, n - 1] (else 0)
static inline int tet_integer_filling(double nel, int n) {
    const double r = std::nearbyint(nel);
    return (fabs(nel - r) <= 1e-9 && r >= 1.0 && r <= (double)(n - 1)) ? (int)r : 0;
}

// ---------------------------------------------------------------- a round of the Fermi search
// The trial keys inside the bracket (lo, hi) of ordered keys (occ_key): every key where at most kTetTrials lie inside, else
// kTetTrials of them at even steps.  Ascending, strictly inside.
static inline int tet_trial_keys(uint64_t lo, uint64_t hi, uint64_t* keys) {
    const uint64_t width = hi - lo;
    if (width <= 1) return 0;
    if (width - 1 <= (uint64_t)kTetTrials) {
        for (uint64_t j = 1; j < width; ++j) keys[j - 1] = lo + j;
        return (int)(width - 1);
    }
    for (int j = 0; j < kTetTrials; ++j)
        keys[j] = lo + (uint64_t)(((unsigned __int128)width * (unsigned)(j + 1)) / (unsigned)(kTetTrials + 1));
    return kTetTrials;
}

// ---------------------------------------------------------------- launches of a sweep over energies (and bands)
// The energies go in tiles of ET = min(nE, kTetTile), a launch's lanes; per band, the bands in tiles of BT (one per blockIdx.z), so
// that part[G][bt][Q][et] stays under kTetPartCap.  Launch (ie, ib) adds its rows [bt][Q][et] at acc + (ie * nbt + ib) * stride.
struct TetSweep {
    int G = 0, Q = 0, ET = 0, BT = 0, net = 0, nbt = 0;
    int64_t stride = 0, acc_doubles = 0, part_doubles = 0;
    bool per_band = false;
    int et(int ie, int nE) const { return std::min(ET, nE - ie * ET); }          // energies of tile ie
    int bt(int ib, int n) const { return per_band ? std::min(BT, n - ib * BT) : 1; }   // blockIdx.z of band tile ib
    int b0(int ib) const { return per_band ? ib * BT : 0; }                      // its first band
    int bpz(int n) const { return per_band ? 1 : n; }                            // bands per blockIdx.z
};
static TetSweep tet_sweep(int G, int Q, int n, int nE, bool per_band) {
    TetSweep s;
    s.per_band = per_band;
    s.G = G;
    s.Q = Q;
    s.ET = std::min(nE, kTetTile);
    s.net = (nE + s.ET - 1) / s.ET;
    const int64_t per = (int64_t)G * Q * s.ET;
    s.BT = per_band ? (int)std::max<int64_t>(1, std::min<int64_t>({kTetPartCap / per, (int64_t)n, 65535})) : 1;
    s.nbt = per_band ? (n + s.BT - 1) / s.BT : 1;
    s.stride = (int64_t)s.BT * Q * s.ET;
    s.acc_doubles = s.stride * s.net * s.nbt;
    s.part_doubles = per * s.BT;
    return s;
}

static inline int tet_cell_groups(int64_t npts) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((npts + 15) / 16, kTetCellGroupsMax));
}
static inline int tet_pdos_groups(int64_t chunk) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((chunk + 15) / 16, kTetPdosGroupsMax));
}
static inline int tet_minmax_gx(int64_t npts) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((npts + 2047) / 2048, 1024));
}

// ---------------------------------------------------------------- the scratch blocks
// tbk_tetrahedron_dos_mesh: 256 leading bytes, the k list and the eigenvalues of the whole mesh, the energies, the selection, the
// cell form's acc, part (the larger of the two forms'), the projected DOS's acc, then the chunk workspace (with a selection)
struct TetDosPlan {
    bool per_band = false, pdos = false;
    int64_t npts = 0, chunk = 0;
    TetSweep cell, vert;
    size_t off_k = 0, off_e = 0, off_en = 0, off_sel = 0, off_acc = 0, off_part = 0, off_pacc = 0, off_chunks = 0, total = 0;
    KuboChunks cw;
};
static TetDosPlan tet_dos_plan(int n, int dk, int64_t npts, int nE, bool per_band, int nsel) {
    TetDosPlan p;
    const size_t D = sizeof(double);
    p.per_band = per_band;
    p.pdos = nsel > 0;
    p.npts = npts;
    p.cell = tet_sweep(tet_cell_groups(npts), 2, n, nE, per_band);
    int64_t part = p.cell.part_doubles;
    if (p.pdos) {
        p.chunk = kubo_chunk_len(n, npts);
        p.vert = tet_sweep(tet_pdos_groups(p.chunk), nsel, n, nE, per_band);
        part = std::max(part, p.vert.part_doubles);
        p.cw = KuboChunks(n, dk, p.chunk, 0, 0, 0);
    }
    p.off_k = 256;
    p.off_e = p.off_k + al256((size_t)npts * dk * D);
    p.off_en = p.off_e + al256((size_t)npts * n * D);
    p.off_sel = p.off_en + al256((size_t)nE * D);
    p.off_acc = p.off_sel + al256((size_t)nsel * sizeof(int32_t));
    p.off_part = p.off_acc + al256((size_t)p.cell.acc_doubles * D);
    p.off_pacc = p.off_part + al256((size_t)part * D);
    p.off_chunks = p.off_pacc + al256((size_t)p.vert.acc_doubles * D);
    p.total = p.off_chunks + (p.pdos ? p.cw.bytes() : 0);
    return p;
}
// tbk_tetrahedron_fermi_level_mesh: the k list, the eigenvalues, the trial energies, the rows (N, g)[trials], part, the band extrema
struct TetFermiPlan {
    int64_t npts = 0;
    int gx = 0;
    TetSweep cell;
    size_t off_k = 0, off_e = 0, off_en = 0, off_acc = 0, off_part = 0, off_mm = 0, total = 0;
};
static TetFermiPlan tet_fermi_plan(int n, int dk, int64_t npts) {
    TetFermiPlan p;
    const size_t D = sizeof(double);
    p.npts = npts;
    p.gx = tet_minmax_gx(npts);
    p.cell = tet_sweep(tet_cell_groups(npts), 2, n, kTetTrials, false);
    p.off_k = 256;
    p.off_e = p.off_k + al256((size_t)npts * dk * D);
    p.off_en = p.off_e + al256((size_t)npts * n * D);
    p.off_acc = p.off_en + al256((size_t)kTetTrials * D);
    p.off_part = p.off_acc + al256((size_t)p.cell.acc_doubles * D);
    p.off_mm = p.off_part + al256((size_t)p.cell.part_doubles * D);
    p.total = p.off_mm + al256((size_t)n * p.gx * 2 * D);
    return p;
}
// tbk_tetrahedron_weights_mesh: the k list, the eigenvalues, the weights [n][N_k]
struct TetWeightsPlan {
    size_t off_k = 0, off_e = 0, off_w = 0, total = 0;
};
static TetWeightsPlan tet_weights_plan(int n, int dk, int64_t npts) {
    TetWeightsPlan p;
    const size_t D = sizeof(double);
    p.off_k = 256;
    p.off_e = p.off_k + al256((size_t)npts * dk * D);
    p.off_w = p.off_e + al256((size_t)npts * n * D);
    p.total = p.off_w + al256((size_t)npts * n * D);
    return p;
}
