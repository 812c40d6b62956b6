// tbk_mf.h -- the host-only part of tbk_mf.hip (the self-consistent Hartree-Fock driver on k meshes): the
// argument checks and caps of tbk_mean_field_mesh, the expansion of a state-indexed interaction list into the real parameter vector
// x, the pinned keys of the private model, the term -> (coefficient, parameter, part) map that k_mf_apply gathers over, the small
// Anderson solve (host and device: k_mf_mix calls the same routine) and the layout of the driver's private workspace.  No device
// call: check/mf_plan_check.cpp drives it on the host alone (make mf-check).
//
// Every partition is a function of (mesh, nsta, dim_k, the interaction's structure) alone.
#pragma once
#include "tbk_int.h"

static const int64_t kMfParamMax = (int64_t)1 << 20;    // real parameters of the field
static const int kMfHistMax = 8;                        // Anderson pairs kept
static const int kMfIterMax = 65536;                    // iterations of one call
static const int64_t kMfResidentMax = (int64_t)1 << 26; // c128 of eigenvectors kept resident (1 GiB; tbk_td.hip's cap on carried states)
static const double kMfReg = 1e-12;                     // added to the unit diagonal of the scaled Gram matrix
static const double kMfCoefMax = 1e6;                   // an Anderson coefficient beyond this: the linear step

// ---------------------------------------------------------------- checks
struct MfArgs {
    int nint = 0;
    const int32_t* ab = nullptr;     // [nint][2] states (a, b)
    const int32_t* R = nullptr;      // [nint][dim_k]
    const double* V = nullptr;       // [nint]
    int fock = 1;
    int have_nel = 1;                // 1: n_electrons, 0: fermi_level
    double nel = 0.0, mu = 0.0, kT = 0.0, mixing = 0.5, tol = 1e-10;
    int history = 4, max_iter = 200, check_every = 1;
};
static int mf_check(const char* fn, int dk, int n, const int32_t* mesh, const MfArgs& A, int64_t& npts, double& target) {
    int rc = occ_mesh_check(fn, dk, n, mesh, npts);
    if (rc) return rc;
    rc = kubo_kt_check(fn, A.kT, false);
    if (rc) return rc;
    TBK_REQUIRE(A.nint >= 1 && A.ab && A.V && A.R, TBK_EINVAL, "%s: the interaction list is empty", fn);
    TBK_REQUIRE(A.nint <= kMfParamMax, TBK_EINVAL, "%s: %d interaction entries (at most 2^20 parameters)", fn, A.nint);
    TBK_REQUIRE(A.history >= 0 && A.history <= kMfHistMax, TBK_EINVAL, "%s: history=%d (0..%d)", fn, A.history, kMfHistMax);
    TBK_REQUIRE(A.max_iter >= 1 && A.max_iter <= kMfIterMax, TBK_EINVAL, "%s: max_iter=%d (1..%d)", fn, A.max_iter, kMfIterMax);
    TBK_REQUIRE(A.check_every >= 1, TBK_EINVAL, "%s: check_every=%d (at least 1)", fn, A.check_every);
    TBK_REQUIRE(A.mixing > 0.0 && A.mixing <= 1.0, TBK_EINVAL, "%s: mixing=%.17g (0 < mixing <= 1)", fn, A.mixing);
    TBK_REQUIRE(A.tol >= 0.0 && std::isfinite(A.tol), TBK_EINVAL, "%s: tol=%.17g (finite, >= 0)", fn, A.tol);
    if (A.have_nel) {
        std::vector<double> t;
        rc = occ_fermi_check(fn, dk, n, mesh, 1, &A.nel, A.kT, 0, npts, t);
        if (rc) return rc;
        target = t[0];
    } else {
        TBK_REQUIRE(std::isfinite(A.mu), TBK_EINVAL, "%s: the Fermi level must be finite", fn);
        target = 0.0;
    }
    for (int e = 0; e < A.nint; ++e)
        if ((rc = int_entry_check(fn, dk, n, e, A.ab, A.R, A.V))) return rc;
    return TBK_OK;
}

// ---------------------------------------------------------------- the parameters
// x = (n_a of every state some V touches, ascending a; then, with Fock, Re and Im of D_ab(R) of every entry, in list order).
// The walk over the list is tbk_int.h's: occ_par[a] is the parameter of n_a.
struct MfField {           // one contribution to a term of the private model: amp(key) += coef x[par] in its real (part 0) or imaginary part
    int a, b, R[4];        // the key in flatten order: a <= b (a > b is stored as (b, a, -R), conjugated: the sign of an imaginary coef)
    double coef;
    int par, part;
};
// The field entries of one (entry, channel, block); `off` shifts both states into the block (0: the particles; n: the holes of a
// Nambu model, tbk_bdg.h).
// Hartree: the on-site energy of a gets s V n_b and that of b gets s V n_a (a == b, R != 0: 2 V n_a, the bonds to R and to -R)
static void mf_field_hartree(std::vector<MfField>& F, int a, int b, double V, int par_a, int par_b, int off, double s) {
    F.push_back(MfField{off + a, off + a, {0, 0, 0, 0}, s * V, par_b, 0});
    F.push_back(MfField{off + b, off + b, {0, 0, 0, 0}, s * V, par_a, 0});
}
// Fock: the entry (a, b, R) of the table gets (s_re Re + i s_im Im) V D_ab(R), D = x[pr] + i x[pr + 1]: -1, -1 on the particles
// (-V D), +1, -1 on the holes (V conj(D)).  One stored direction per call: the slot (a, b, R) itself where a <= b, or (mirror) the
// slot (b, a, -R) with the conjugate where a >= b -- on the diagonal (a == b) both, the slot also holds the mirror term at -R.
static void mf_field_fock(std::vector<MfField>& F, int a, int b, const int* R, double V, int pr, int off, double s_re, double s_im, bool mirror) {
    const int m = mirror ? -1 : 1;
    const MfField f{off + (mirror ? b : a), off + (mirror ? a : b), {m * R[0], m * R[1], m * R[2], m * R[3]}, s_re * V, pr, 0};
    F.push_back(f);
    F.push_back(f);
    F.back().coef = m * s_im * V, F.back().par = pr + 1, F.back().part = 1;
}
struct MfProblem : IntBonds {
    int n = 0, dk = 0, nint = 0, fock = 0;
    int64_t np = 0;
    std::vector<int64_t> gidx;           // [np]: where x_out[p] sits in acc[nR][n][n] seen as doubles
    std::vector<int32_t> pin;            // [npin][6]
    std::vector<MfField> field;
};
static int mf_problem(const char* fn, int dk, int n, const MfArgs& A, MfProblem& P) {
    P = MfProblem();
    int rc = int_bonds(fn, dk, n, A.nint, A.ab, A.R, A.V, P);
    if (rc) return rc;
    P.n = n, P.dk = dk, P.nint = A.nint, P.fock = A.fock ? 1 : 0;
    TBK_REQUIRE(P.nR <= kOccRMax, TBK_EINVAL, "%s: %d distinct lattice vectors (at most %d)", fn, P.nR, kOccRMax);
    TBK_REQUIRE((int64_t)P.nR * n * n <= kOccOutCap, TBK_EINVAL, "%s: nR * nsta^2 = %lld (at most %lld)", fn, (long long)P.nR * n * n,
                (long long)kOccOutCap);
    P.np = (int64_t)P.nocc + (P.fock ? 2 * (int64_t)A.nint : 0);
    TBK_REQUIRE(P.np <= kMfParamMax, TBK_EINVAL, "%s: %lld parameters (at most 2^20)", fn, (long long)P.np);
    P.gidx.resize((size_t)P.np);
    const int64_t nn = (int64_t)n * n;
    for (int a = 0; a < n; ++a)
        if (P.occ_par[a] >= 0) {
            P.gidx[P.occ_par[a]] = 2 * ((int64_t)a * n + a);
            const int32_t q[6] = {a, a, 0, 0, 0, 0};
            P.pin.insert(P.pin.end(), q, q + 6);
        }
    for (int e = 0; e < A.nint; ++e) {
        const int a = A.ab[2 * e], b = A.ab[2 * e + 1];
        const double V = A.V[e];
        int R[4] = {0, 0, 0, 0};
        for (int d = 0; d < dk; ++d) R[d] = A.R[(int64_t)e * dk + d];
        mf_field_hartree(P.field, a, b, V, P.occ_par[a], P.occ_par[b], 0, 1.0);
        if (!P.fock) continue;
        const int pr = P.nocc + 2 * e, pi = pr + 1;
        P.gidx[pr] = 2 * ((int64_t)P.ent_r[e] * nn + (int64_t)a * n + b);
        P.gidx[pi] = P.gidx[pr] + 1;
        const int32_t q[6] = {a, b, R[0], R[1], R[2], R[3]};
        P.pin.insert(P.pin.end(), q, q + 6);
        if (a <= b) mf_field_fock(P.field, a, b, R, V, pr, 0, -1.0, -1.0, false);
        if (a >= b) mf_field_fock(P.field, a, b, R, V, pr, 0, -1.0, -1.0, true);
    }
    return TBK_OK;
}

// ---------------------------------------------------------------- the term -> parameter map
// CSR over the terms of the flattened private model that carry a field, in ascending term index; the contributions of a term in the
// order of P.field (the order of the interaction list): k_mf_apply adds them in that order, one lane per term.
struct MfMap {
    std::vector<int32_t> term, ptr, par, part;    // [nft], [nft + 1], [nnz], [nnz]
    std::vector<int64_t> rblk;                    // [nft]: the term's cell of rblock, -1 without that table
    std::vector<double> coef;                     // [nnz]
    std::vector<double> base;                     // [nft][2]: the amplitude of the bare model
};
static int mf_map(const char* fn, const MfProblem& P, int nslot, const std::vector<int32_t>& slot_ptr, const std::vector<int32_t>& R4,
                  const std::vector<double>& amp2, int nRb, const std::vector<int32_t>& rvec, MfMap& M) {
    M = MfMap();
    const int n = P.n;
    std::map<int64_t, std::vector<int>> by_term;
    for (size_t f = 0; f < P.field.size(); ++f) {
        const MfField& F = P.field[f];
        const int s = F.a * n - F.a * (F.a - 1) / 2 + (F.b - F.a);
        int64_t found = -1;
        for (int t = slot_ptr[s]; t < slot_ptr[s + 1]; ++t)
            if (R4[4 * (size_t)t] == F.R[0] && R4[4 * (size_t)t + 1] == F.R[1] && R4[4 * (size_t)t + 2] == F.R[2] && R4[4 * (size_t)t + 3] == F.R[3])
                found = t;
        TBK_REQUIRE(found >= 0, TBK_EINVAL, "%s: the pinned term (%d, %d) is missing from the flattened model", fn, F.a, F.b);
        by_term[found].push_back((int)f);
    }
    M.ptr.push_back(0);
    for (auto& kv : by_term) {
        const int64_t t = kv.first;
        M.term.push_back((int32_t)t);
        M.base.push_back(amp2[2 * (size_t)t]);
        M.base.push_back(amp2[2 * (size_t)t + 1]);
        int64_t cell = -1;
        if (nRb > 0) {
            int s = 0;
            while (slot_ptr[s + 1] <= t) ++s;
            for (int r = 0; r < nRb; ++r)
                if (rvec[4 * (size_t)r] == R4[4 * (size_t)t] && rvec[4 * (size_t)r + 1] == R4[4 * (size_t)t + 1] &&
                    rvec[4 * (size_t)r + 2] == R4[4 * (size_t)t + 2] && rvec[4 * (size_t)r + 3] == R4[4 * (size_t)t + 3])
                    cell = (int64_t)r * nslot + s;
            TBK_REQUIRE(cell >= 0, TBK_EINVAL, "%s: term %lld has no cell in the lattice-vector table", fn, (long long)t);
        }
        M.rblk.push_back(cell);
        for (int f : kv.second) {
            M.coef.push_back(P.field[f].coef);
            M.par.push_back(P.field[f].par);
            M.part.push_back(P.field[f].part);
        }
        M.ptr.push_back((int32_t)M.coef.size());
    }
    return TBK_OK;
}

// ---------------------------------------------------------------- the Anderson (Pulay) step
// Given the Gram matrix B[j][k] = <r_j, r_k> of the cnt residuals in the ring (row length kMfHistMax), the coefficients c with
// sum c = 1 that minimise |sum c_j r_j|^2: with d_j = sqrt(B_jj), solve (D^-1 B D^-1 + kMfReg I) z = D^-1 1 by Gaussian elimination
// with partial pivoting, y = D^-1 z, c = y / sum y.  False -- the caller takes the linear step -- when a d_j is zero or not finite,
// a pivot is not above 1e-14, the sum is zero or not finite, or a |c_j| exceeds kMfCoefMax.
#define MF_AND_WORK (kMfHistMax * (kMfHistMax + 1) + kMfHistMax)   // doubles of work space (LDS on the device: no private arrays)
inline __host__ __device__ bool mf_anderson(const int cnt, const double* B, double* c, double* W) {
    const int LD = kMfHistMax + 1;
    double* A = W;
    double* d = W + kMfHistMax * LD;
    if (cnt < 1 || cnt > kMfHistMax) return false;
    for (int j = 0; j < cnt; ++j) {
        d[j] = sqrt(B[j * kMfHistMax + j]);
        if (!(d[j] > 0.0) || !(d[j] < 1.7e308)) return false;
    }
    for (int j = 0; j < cnt; ++j) {
        for (int k = 0; k < cnt; ++k) A[j * LD + k] = B[j * kMfHistMax + k] / (d[j] * d[k]) + (j == k ? kMfReg : 0.0);
        A[j * LD + cnt] = 1.0 / d[j];
    }
    for (int p = 0; p < cnt; ++p) {
        int best = p;
        for (int j = p + 1; j < cnt; ++j)
            if (fabs(A[j * LD + p]) > fabs(A[best * LD + p])) best = j;
        if (!(fabs(A[best * LD + p]) > 1e-14)) return false;
        if (best != p)
            for (int k = p; k <= cnt; ++k) {
                const double t = A[p * LD + k];
                A[p * LD + k] = A[best * LD + k];
                A[best * LD + k] = t;
            }
        for (int j = p + 1; j < cnt; ++j) {
            const double f = A[j * LD + p] / A[p * LD + p];
            for (int k = p; k <= cnt; ++k) A[j * LD + k] -= f * A[p * LD + k];
        }
    }
    double sum = 0.0;
    for (int p = cnt - 1; p >= 0; --p) {
        double s = A[p * LD + cnt];
        for (int k = p + 1; k < cnt; ++k) s -= A[p * LD + k] * c[k];
        c[p] = s / A[p * LD + p];
    }
    for (int j = 0; j < cnt; ++j) {
        c[j] /= d[j];
        sum += c[j];
    }
    if (!(fabs(sum) > 0.0) || !(fabs(sum) < 1.7e308)) return false;
    for (int j = 0; j < cnt; ++j) {
        c[j] /= sum;
        if (!(fabs(c[j]) <= kMfCoefMax)) return false;
    }
    return true;
}

// ---------------------------------------------------------------- the workspace
// The loop's share of a driver's private device block, behind the driver's own buffers: the vectors and the ring of the mixing, the
// gather indices, the term -> parameter map and the two history arrays (occ_cols occupations per iteration).  Returns its end.
struct MfLoopBufs {
    enum { XIN, XOUT, XPREV, RINGX, RINGR, SMALL, GIDX, TBASE, TPTR, TTERM, TRBLK, CCOEF, CPAR, CPART, RESH, OCCH, NBUF };
    size_t off[NBUF + 1];
};
static size_t mf_loop_bufs(MfLoopBufs& L, size_t at, int64_t np, int history, int max_iter, int64_t nft, int64_t nnz, int occ_cols) {
    const size_t D = sizeof(double);
    const int m = std::max(history, 1);
    size_t b[MfLoopBufs::NBUF];
    b[MfLoopBufs::XIN] = b[MfLoopBufs::XOUT] = b[MfLoopBufs::XPREV] = (size_t)np * D;
    b[MfLoopBufs::RINGX] = b[MfLoopBufs::RINGR] = (size_t)m * np * D;
    b[MfLoopBufs::SMALL] = 1024;                        // the Gram matrix [8][8]
    b[MfLoopBufs::GIDX] = (size_t)np * sizeof(int64_t);
    b[MfLoopBufs::TBASE] = (size_t)nft * 2 * D;
    b[MfLoopBufs::TPTR] = (size_t)(nft + 1) * sizeof(int32_t);
    b[MfLoopBufs::TTERM] = (size_t)nft * sizeof(int32_t);
    b[MfLoopBufs::TRBLK] = (size_t)nft * sizeof(int64_t);
    b[MfLoopBufs::CCOEF] = (size_t)nnz * D;
    b[MfLoopBufs::CPAR] = b[MfLoopBufs::CPART] = (size_t)nnz * sizeof(int32_t);
    b[MfLoopBufs::RESH] = (size_t)max_iter * D;
    b[MfLoopBufs::OCCH] = (size_t)max_iter * occ_cols * D;
    L.off[0] = al256(at);
    for (int i = 0; i < MfLoopBufs::NBUF; ++i) L.off[i + 1] = L.off[i] + al256(b[i]);
    return L.off[MfLoopBufs::NBUF];
}

// One private device block.  resident: every chunk's eigenvectors stay (chunk c at c * vstride c128); else one chunk's worth.
struct MfPlan {
    bool resident = false;
    int64_t npts = 0, chunk = 0, nchunks = 0, nlev = 0, vstride = 0;
    int G = 0;                 // groups of the level scans (occ_scan_groups)
    OccDmPlan dm;
    enum { K_ALL, LEV, EC, VEC, FW, DPART, ACC, RDEV, FPART, FSMALL, SPART, NBUF };
    size_t off[NBUF + 1];
    MfLoopBufs loop;
    size_t total = 0;
};
static inline int64_t mf_resident_cap(long long knob) {
    return knob > 0 && knob < kMfResidentMax ? (int64_t)knob : kMfResidentMax;
}
static MfPlan mf_plan(int n, int dk, int64_t npts, int nR, int64_t np, int history, int max_iter, int64_t nft, int64_t nnz, int64_t resident_cap) {
    MfPlan p;
    const size_t D = sizeof(double);
    const int64_t nn = (int64_t)n * n;
    p.npts = npts;
    p.nlev = npts * n;
    p.G = occ_scan_groups(p.nlev);
    p.dm = occ_dm_plan(n, dk, npts, nR);
    p.chunk = p.dm.chunk;
    p.nchunks = p.dm.nchunks;
    p.resident = npts * nn <= resident_cap;
    p.vstride = (int64_t)(al256((size_t)p.chunk * nn * sizeof(cd)) / sizeof(cd));
    size_t b[MfPlan::NBUF];
    b[MfPlan::K_ALL] = (size_t)npts * dk * D;
    b[MfPlan::LEV] = (size_t)p.nlev * D;
    b[MfPlan::EC] = (size_t)p.chunk * n * D;
    b[MfPlan::VEC] = (size_t)(p.resident ? p.nchunks : 1) * p.vstride * sizeof(cd);
    b[MfPlan::FW] = (size_t)p.chunk * n * D;
    b[MfPlan::DPART] = (size_t)p.dm.part_cd * sizeof(cd);
    b[MfPlan::ACC] = (size_t)p.dm.acc_cd * sizeof(cd);
    b[MfPlan::RDEV] = (size_t)nR * dk * sizeof(int32_t);
    b[MfPlan::FPART] = (size_t)2 * p.G * D;
    b[MfPlan::FSMALL] = 2048;                           // mu, lo, hi, target, edges[2] of the one filling, 256 bytes apart
    b[MfPlan::SPART] = (size_t)3 * p.G * D + 256;       // the final scan's partials and its three sums
    p.off[0] = 256;
    for (int i = 0; i < MfPlan::NBUF; ++i) p.off[i + 1] = p.off[i] + al256(b[i]);
    p.total = mf_loop_bufs(p.loop, p.off[MfPlan::NBUF], np, history, max_iter, nft, nnz, n);
    return p;
}

