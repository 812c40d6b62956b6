// tbk_bse.h -- the host-only part of tbk_bse.hip (excitons: the Tamm-Dancoff Bethe-Salpeter operator, its dense states and its Haydock
// spectrum on k meshes): the argument checks and caps of tbk_exciton_apply_mesh, tbk_exciton_states_mesh and
// tbk_exciton_spectrum_mesh, the selection of the valence and conduction bands, the expansion of a state-indexed bond list into the
// ordered set E of directed entries with the index map of the Hartree field h, the partition of the mesh into tiles and k-groups, the
// layout of the workspace, the Lanczos runs of a polarizability tensor with the algebra that turns them into the tensor, and the
// continued fraction.  No device call: check/bse_plan_check.cpp drives it on the host alone (make bse-check).
//
// Every partition is a function of (mesh, nv, nc) alone -- NOT of the block width nor of the interaction list: a vector is worked
// through with the same tiles, the same groups and the same order of operations whatever stands beside it.
#pragma once
#include <complex>
#include "tbk_mf.h"

static const int kBseBandMax = 16;                          // selected valence bands, and conduction bands
static const int kBseBlockMax = 16;                         // vectors of one application
static const int64_t kBseDenseMax = 2048;                   // transitions of the dense path (the dense solver's limit)
static const int64_t kBseTransMax = (int64_t)1 << 24;       // transitions of the operator and of the Haydock path
static const int64_t kBseVecCap = (int64_t)1 << 26;         // c128 of selected eigenvectors kept resident (1 GiB)
static const int kBseEntryMax = 1024;                       // directed entries plus touched states
static const int kBseGroupsMax = 1024;                      // k-groups of the pair and project stages
static const int kBseNormGroupsMax = 1024;                  // groups of a vector norm
static const int kBseStepsMax = 65536;                      // Lanczos steps of one call
static const double kBseBreakdown = 1e-10;                  // beta below this times the largest |alpha| so far ends a run
#define BSE_EC 8                                            // entries per workgroup of the pair stage, per pass of the project stage

// ---------------------------------------------------------------- checks
struct BseArgs {
    int nint = 0;
    const int32_t* ab = nullptr;     // [nint][2] states (a, b)
    const int32_t* R = nullptr;      // [nint][dim_k]
    const double* V = nullptr;       // [nint]
    double mu = 0.0;
    int nv = 0, nc = 0;              // with a list: its length; without: the top nv occupied / bottom nc empty bands, 0 = all
    const int32_t* vsel = nullptr;   // band indices, or null
    const int32_t* csel = nullptr;
    int direct = 1, exchange = 1;
};
// the mesh, the Fermi level and the interaction list by the rules of tbk_mean_field_mesh; the band arguments as far as they can be
// judged before the bands are known
static int bse_check(const char* fn, int dk, int n, const int32_t* mesh, const BseArgs& A, int64_t& npts) {
    MfArgs M;
    M.nint = A.nint, M.ab = A.ab, M.R = A.R, M.V = A.V, M.have_nel = 0, M.mu = A.mu;
    double target;
    int rc = mf_check(fn, dk, n, mesh, M, npts, target);
    if (rc) return rc;
    TBK_REQUIRE(n >= 2, TBK_EINVAL, "%s: a model of one state has no transitions", fn);
    for (int s = 0; s < 2; ++s) {
        const int cnt = s ? A.nc : A.nv;
        const int32_t* sel = s ? A.csel : A.vsel;
        const char* what = s ? "conduction" : "valence";
        TBK_REQUIRE(cnt >= 0 && !(sel && cnt < 1), TBK_EINVAL, "%s: no %s band selected", fn, s ? "empty" : "occupied");
        TBK_REQUIRE(cnt <= kBseBandMax, TBK_EINVAL, "%s: %d %s bands (at most %d)", fn, cnt, what, kBseBandMax);
        for (int i = 0; sel && i < cnt; ++i) {
            TBK_REQUIRE(sel[i] >= 0 && sel[i] < n, TBK_EINVAL, "%s: %s band %d out of range", fn, what, sel[i]);
            for (int j = 0; j < i; ++j) TBK_REQUIRE(sel[j] != sel[i], TBK_EINVAL, "%s: %s band %d is selected twice", fn, what, sel[i]);
        }
    }
    return TBK_OK;
}

// The selected bands once the number nocc of occupied levels is known: bands[0..nv) the valence bands, bands[nv..nv + nc) the
// conduction bands, both ascending.  A count m means the top m occupied / the bottom m empty bands, 0 all of them.
static int bse_select(const char* fn, int n, int nocc, const BseArgs& A, int32_t* bands, int& nv, int& nc) {
    TBK_REQUIRE(nocc >= 1, TBK_EINVAL, "%s: no occupied band selected (no level at or below the Fermi level)", fn);
    TBK_REQUIRE(nocc < n, TBK_EINVAL, "%s: no empty band selected (every level is at or below the Fermi level)", fn);
    std::vector<int32_t> v, c;
    if (A.vsel) {
        v.assign(A.vsel, A.vsel + A.nv);
        for (int32_t b : v) TBK_REQUIRE(b < nocc, TBK_EINVAL, "%s: valence band %d is not occupied (%d occupied bands)", fn, b, nocc);
    } else {
        const int m = A.nv ? A.nv : nocc;
        TBK_REQUIRE(m <= nocc, TBK_EINVAL, "%s: %d valence bands of %d occupied ones", fn, m, nocc);
        for (int b = nocc - m; b < nocc; ++b) v.push_back(b);
    }
    if (A.csel) {
        c.assign(A.csel, A.csel + A.nc);
        for (int32_t b : c) TBK_REQUIRE(b >= nocc, TBK_EINVAL, "%s: conduction band %d is occupied (%d occupied bands)", fn, b, nocc);
    } else {
        const int m = A.nc ? A.nc : n - nocc;
        TBK_REQUIRE(m <= n - nocc, TBK_EINVAL, "%s: %d conduction bands of %d empty ones", fn, m, n - nocc);
        for (int b = nocc; b < nocc + m; ++b) c.push_back(b);
    }
    TBK_REQUIRE((int)v.size() <= kBseBandMax, TBK_EINVAL, "%s: %d valence bands (at most %d)", fn, (int)v.size(), kBseBandMax);
    TBK_REQUIRE((int)c.size() <= kBseBandMax, TBK_EINVAL, "%s: %d conduction bands (at most %d)", fn, (int)c.size(), kBseBandMax);
    std::sort(v.begin(), v.end());
    std::sort(c.begin(), c.end());
    nv = (int)v.size(), nc = (int)c.size();
    for (int i = 0; i < nv; ++i) bands[i] = v[i];
    for (int i = 0; i < nc; ++i) bands[nv + i] = c[i];
    return TBK_OK;
}
// the caps that need the band counts: transitions of the path (dense: mode 1), resident eigenvectors
static int bse_caps(const char* fn, int mode, int n, int64_t npts, int nv, int nc) {
    const int64_t nt = npts * nv * nc, cap = mode == 1 ? kBseDenseMax : kBseTransMax;
    TBK_REQUIRE(nt <= cap, TBK_EINVAL, "%s: %lld transitions (at most %lld on this path)", fn, (long long)nt, (long long)cap);
    TBK_REQUIRE(npts * n * (nv + nc) <= kBseVecCap, TBK_EINVAL, "%s: N_k nsta (nv + nc) = %lld resident eigenvector components (at most 2^26)",
                fn, (long long)(npts * n * (nv + nc)));
    return TBK_OK;
}

// ---------------------------------------------------------------- the interaction
// E holds, for bond e of the list, the directed entries 2 e = (a, b, R) and 2 e + 1 = (b, a, -R), both with V_e.  The touched states
// st (ascending) carry rho and h; h_a = sum over the entries with a_e = a, in the order of E, of V_e rho_{b_e}: the CSR map
// (hptr over st, hent the entry, hslot the place of b_e in st).  The pair stage forms, per vector, the np = ned + nst sums
//   p < ned:   F_p   = sum_k e^{-2 pi i k.(R + tau_b - tau_a)} T_ab(k)      (direct; ned = 2 nint, or 0 with direct off)
//   p >= ned:  rho_s = sum_k T_ss(k), s = st[p - ned]                        (exchange; nst = 0 with exchange off)
struct BseProblem {
    int dk = 0, nint = 0, ne = 0, ned = 0, nst = 0, np = 0;
    std::vector<int32_t> ea, eb, eR;     // [ne], [ne], [ne][3]: the set E
    std::vector<double> eV;              // [ne]
    std::vector<int32_t> st;             // [nst]
    std::vector<int32_t> hptr, hent, hslot;
    std::vector<int32_t> pa, pb, pR;     // [np], [np], [np][3]: what the pair stage sums
};
static int bse_problem(const char* fn, int dk, int n, const BseArgs& A, BseProblem& P) {
    P = BseProblem();
    P.dk = dk, P.nint = A.nint, P.ne = 2 * A.nint;
    IntBonds W;                                               // the walk of tbk_int.h: the repeated bond, the touched states
    int rc = int_bonds(fn, dk, n, A.nint, A.ab, A.R, A.V, W);
    if (rc) return rc;
    for (int e = 0; e < A.nint; ++e) {
        const int a = A.ab[2 * e], b = A.ab[2 * e + 1];
        int R[3] = {0, 0, 0};
        for (int d = 0; d < dk; ++d) R[d] = A.R[(int64_t)e * dk + d];
        P.ea.push_back(a), P.eb.push_back(b);
        P.ea.push_back(b), P.eb.push_back(a);
        for (int d = 0; d < 3; ++d) P.eR.push_back(R[d]);
        for (int d = 0; d < 3; ++d) P.eR.push_back(-R[d]);
        P.eV.push_back(A.V[e]), P.eV.push_back(A.V[e]);
    }
    P.ned = A.direct ? P.ne : 0;
    for (int a = 0; A.exchange && a < n; ++a)
        if (W.occ_par[a] >= 0) P.st.push_back(a);
    P.nst = (int)P.st.size();
    P.np = P.ned + P.nst;
    TBK_REQUIRE(P.np <= kBseEntryMax, TBK_EINVAL, "%s: %d directed entries and touched states (at most %d)", fn, P.np, kBseEntryMax);
    P.hptr.assign((size_t)P.nst + 1, 0);
    for (int i = 0; i < P.nst; ++i) {
        for (int e = 0; e < P.ne; ++e)
            if (P.ea[e] == P.st[i]) {
                P.hent.push_back(e);
                P.hslot.push_back((int32_t)(std::lower_bound(P.st.begin(), P.st.end(), P.eb[e]) - P.st.begin()));
            }
        P.hptr[i + 1] = (int32_t)P.hent.size();
    }
    for (int p = 0; p < P.ned; ++p) {
        P.pa.push_back(P.ea[p]), P.pb.push_back(P.eb[p]);
        for (int d = 0; d < 3; ++d) P.pR.push_back(P.eR[3 * (size_t)p + d]);
    }
    for (int i = 0; i < P.nst; ++i) {
        P.pa.push_back(P.st[i]), P.pb.push_back(P.st[i]);
        for (int d = 0; d < 3; ++d) P.pR.push_back(0);
    }
    return TBK_OK;
}

// ---------------------------------------------------------------- the partition
// The 256 lanes of a workgroup of the pair and project stages take (point q of a tile, v, c): P = 256 / (nv nc) points per tile.
// Group g of G takes the tiles [g ntiles / G, (g + 1) ntiles / G): about two.  A vector norm is formed by GN groups of strided lanes.
struct BsePart {
    int nvc = 0, P = 0, G = 0, GN = 0;
    int64_t npts = 0, ntiles = 0, nt = 0;
};
__host__ __device__ inline void bse_lane(const int t, const int nvc, const int nc, int& q, int& r, int& v, int& c) {
    q = t / nvc;
    r = t - q * nvc;
    v = r / nc;
    c = r - v * nc;
}
static BsePart bse_partition(int64_t npts, int nv, int nc) {
    BsePart p;
    p.npts = npts;
    p.nvc = nv * nc;
    p.P = 256 / p.nvc;
    p.ntiles = (npts + p.P - 1) / p.P;
    p.G = (int)std::max<int64_t>(1, std::min<int64_t>((p.ntiles + 1) / 2, kBseGroupsMax));
    p.nt = npts * p.nvc;
    p.GN = (int)std::max<int64_t>(1, std::min<int64_t>((p.nt + 1023) / 1024, kBseNormGroupsMax));
    return p;
}

// ---------------------------------------------------------------- the Lanczos runs of a polarizability
// Full tensor (da < 0): runs 0..dk-1 start from D^a; then, for every pair a < b in order, one from D^a + D^b and one from D^a + i D^b:
// dk^2 runs.  One component (da, db): da == db one run; else D^da, D^db, D^da + D^db, D^da + i D^db.
struct BseRun {
    int a, b, kind;    // 0: D^a; 1: D^a + D^b; 2: D^a + i D^b
};
static std::vector<BseRun> bse_runs(int dk, int da, int db) {
    std::vector<BseRun> r;
    if (da < 0) {
        for (int a = 0; a < dk; ++a) r.push_back(BseRun{a, a, 0});
        for (int a = 0; a < dk; ++a)
            for (int b = a + 1; b < dk; ++b) r.push_back(BseRun{a, b, 1}), r.push_back(BseRun{a, b, 2});
    } else if (da == db) {
        r.push_back(BseRun{da, da, 0});
    } else {
        r.push_back(BseRun{da, da, 0}), r.push_back(BseRun{db, db, 0});
        r.push_back(BseRun{da, db, 1}), r.push_back(BseRun{da, db, 2});
    }
    return r;
}
// <v| (H - z)^-1 |v> = norm2 / (alpha_0 - z - beta_0^2 / (alpha_1 - z - ...)), the levels 0..m-1 of a run of m steps, from the bottom
typedef std::complex<double> bse_c;
static inline bse_c bse_cfrac(int m, const double* alpha, const double* beta, double norm2, bse_c z) {
    if (m < 1) return bse_c(0.0, 0.0);
    bse_c d = alpha[m - 1] - z;
    for (int j = m - 2; j >= 0; --j) d = alpha[j] - z - beta[j] * beta[j] / d;
    return norm2 / d;
}
// With g(v) = <v|G|v> bilinear in (bra conjugated, ket): g(a + b) = g_a + g_b + G_ab + G_ba, g(a + i b) = g_a + g_b + i G_ab - i G_ba,
// so with S = g(a + b) - g_a - g_b and T = g(a + i b) - g_a - g_b:  G_ab = (S - i T) / 2,  G_ba = (S + i T) / 2.
static inline void bse_polarize(bse_c ga, bse_c gb, bse_c gs, bse_c gi, bse_c& gab, bse_c& gba) {
    const bse_c S = gs - ga - gb, T = gi - ga - gb, iT = bse_c(-T.imag(), T.real());
    gab = 0.5 * (S - iT);
    gba = 0.5 * (S + iT);
}
// chi(omega) from the runs of bse_runs(dk, da, db): out[dk][dk] (da < 0) or out[1]; g[r] the continued fraction of run r
static inline void bse_tensor(int dk, int da, int db, const bse_c* g, double inv_nk, bse_c* out) {
    if (da < 0) {
        for (int a = 0; a < dk; ++a) out[a * dk + a] = g[a] * inv_nk;
        int r = dk;
        for (int a = 0; a < dk; ++a)
            for (int b = a + 1; b < dk; ++b, r += 2) {
                bse_c gab, gba;
                bse_polarize(g[a], g[b], g[r], g[r + 1], gab, gba);
                out[a * dk + b] = gab * inv_nk;
                out[b * dk + a] = gba * inv_nk;
            }
    } else if (da == db) {
        out[0] = g[0] * inv_nk;
    } else {
        bse_c gab, gba;
        bse_polarize(g[0], g[1], g[2], g[3], gab, gba);
        out[0] = gab * inv_nk;
    }
}
static int bse_reconstruct_check(const char* fn, int dk, int da, int db, int nsteps, int nw, const double* omega, double eta) {
    TBK_REQUIRE(dk >= 1 && dk <= 3, TBK_EINVAL, "%s: dim_k=%d (1..3)", fn, dk);
    TBK_REQUIRE((da < 0 && db < 0) || (da >= 0 && da < dk && db >= 0 && db < dk), TBK_EINVAL, "%s: directions (%d, %d) of %d", fn, da, db, dk);
    TBK_REQUIRE(nsteps >= 1 && nsteps <= kBseStepsMax, TBK_EINVAL, "%s: n_steps=%d (1..%d)", fn, nsteps, kBseStepsMax);
    TBK_REQUIRE(nw >= 1 && nw <= 65536 && omega, TBK_EINVAL, "%s: nomega=%d (1..65536 frequencies)", fn, nw);
    for (int j = 0; j < nw; ++j) TBK_REQUIRE(std::isfinite(omega[j]), TBK_EINVAL, "%s: frequency %d is not finite", fn, j);
    TBK_REQUIRE(std::isfinite(eta) && eta > 0.0, TBK_EINVAL, "%s: eta must be finite and > 0", fn);
    return TBK_OK;
}

// ---------------------------------------------------------------- the workspace
// One block of the context's scratch (the device-buffer grower), behind 256 leading bytes.  mode 0: apply, 1: states, 2: spectrum.
// nb: vectors carried at once (the block of an application; 16 on the dense path; the runs of the spectrum).
struct BsePlan : BsePart {
    int mode = 0, n = 0, dk = 0, nv = 0, nc = 0, ns = 0, nb = 0, np = 0, nsteps = 0;
    enum { K_ALL, CNT, SCAL, BANDS, U, EV, GAPS, DIP, PA, PB, PR, EVV, ST, HPTR, HENT, HSLOT, PART, FSUM, FS, HF, X, Y, Z, DPART, NPART, ALPHA, BETA,
           LZ, RUNS, HMAT, EVAL, EVEC, DL, SAB, NBUF };
    size_t off[NBUF + 1];
    size_t off_chunks = 0, total = 0;
    KuboChunks cw;
};
static BsePlan bse_plan(int mode, int n, int dk, int64_t npts, int nv, int nc, int nb, const BseProblem& Q, int nsteps) {
    BsePlan p;
    static_cast<BsePart&>(p) = bse_partition(npts, nv, nc);
    p.mode = mode, p.n = n, p.dk = dk, p.nv = nv, p.nc = nc, p.ns = nv + nc, p.nb = nb, p.np = Q.np, p.nsteps = nsteps;
    const size_t D = sizeof(double), Z = sizeof(cd), I = sizeof(int32_t);
    const size_t nt = (size_t)p.nt;
    size_t b[BsePlan::NBUF];
    for (size_t& x : b) x = 0;
    b[BsePlan::K_ALL] = (size_t)npts * dk * D;
    b[BsePlan::CNT] = (size_t)npts * I;
    b[BsePlan::SCAL] = 256;                                   // gap, max Delta, max |E|, first k with another count, that count
    b[BsePlan::BANDS] = 2 * kBseBandMax * I;
    b[BsePlan::U] = (size_t)npts * p.ns * n * Z;
    b[BsePlan::EV] = (size_t)npts * p.ns * D;
    b[BsePlan::GAPS] = nt * D;
    b[BsePlan::DIP] = mode ? (size_t)dk * nt * Z : 0;
    b[BsePlan::PA] = b[BsePlan::PB] = (size_t)Q.np * I;
    b[BsePlan::PR] = (size_t)Q.np * 3 * I;
    b[BsePlan::EVV] = (size_t)Q.ne * D;
    b[BsePlan::ST] = (size_t)Q.nst * I;
    b[BsePlan::HPTR] = (size_t)(Q.nst + 1) * I;
    b[BsePlan::HENT] = b[BsePlan::HSLOT] = Q.hent.size() * I;
    b[BsePlan::PART] = (size_t)p.G * nb * Q.np * Z;
    b[BsePlan::FSUM] = (size_t)nb * Q.np * Z;
    b[BsePlan::FS] = (size_t)nb * Q.ned * Z;
    b[BsePlan::HF] = (size_t)nb * Q.nst * Z;
    b[BsePlan::X] = b[BsePlan::Y] = (size_t)nb * nt * Z;
    b[BsePlan::DPART] = (size_t)nb * p.G * D;
    if (mode == 2) {
        b[BsePlan::Z] = (size_t)nb * nt * Z;
        b[BsePlan::NPART] = (size_t)nb * p.GN * D;
        b[BsePlan::ALPHA] = b[BsePlan::BETA] = (size_t)nb * nsteps * D;
        b[BsePlan::LZ] = (size_t)nb * 8 * D;                  // per run: alpha of the step, beta of the step, norm, largest |alpha|, done, n_used
        b[BsePlan::RUNS] = (size_t)nb * 3 * I;
    }
    if (mode == 1) {
        b[BsePlan::HMAT] = b[BsePlan::EVEC] = nt * nt * Z;
        b[BsePlan::EVAL] = nt * D;
        b[BsePlan::DL] = nt * dk * Z;
    }
    if (mode) b[BsePlan::SAB] = (size_t)dk * dk * Z;
    p.off[0] = 256;
    for (int i = 0; i < BsePlan::NBUF; ++i) p.off[i + 1] = p.off[i] + al256(b[i]);
    p.off_chunks = p.off[BsePlan::NBUF];
    p.cw = KuboChunks(n, dk, kubo_chunk_len(n, npts), 0, 0, 0);
    p.total = p.off_chunks + p.cw.bytes();
    return p;
}
