// tbk_mf.h -- the host-only part of tbk_mf.hip (the self-consistent Hartree-Fock driver on k meshes): the
// argument checks and caps of tbk_mean_field_mesh, the expansion of a state-indexed interaction list into the real parameter vector
// x, the pinned keys of the private model, the term -> (coefficient, parameter, part) map that k_mf_apply gathers over, the small
// Anderson solve (host and device: k_mf_mix calls the same routine) and the layout of the driver's private workspace.  No device
// call: check/mf_plan_check.cpp drives it on the host alone (make mf-check).
//
// Every partition is a function of (mesh, nsta, dim_k, the interaction's structure) alone.
#pragma once
#include <map>
#include <array>
#include "tbk_occ.h"

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
    for (int e = 0; e < A.nint; ++e) {
        const int a = A.ab[2 * e], b = A.ab[2 * e + 1];
        TBK_REQUIRE(a >= 0 && a < n && b >= 0 && b < n, TBK_EINVAL, "%s: interaction %d has a state index out of range", fn, e);
        TBK_REQUIRE(std::isfinite(A.V[e]), TBK_EINVAL, "%s: interaction %d is not finite", fn, e);
        bool zero = true;
        for (int d = 0; d < dk; ++d) {
            const int32_t r = A.R[(int64_t)e * dk + d];
            TBK_REQUIRE(r > -kOccRAbsMax && r < kOccRAbsMax, TBK_EINVAL, "%s: interaction %d has a lattice component of 2^30 or more", fn, e);
            zero = zero && r == 0;
        }
        TBK_REQUIRE(!(a == b && zero), TBK_EINVAL, "%s: interaction %d couples state %d to itself (a self-interaction)", fn, e, a);
    }
    return TBK_OK;
}

// ---------------------------------------------------------------- the parameters
// x = (n_a of every state some V touches, ascending a; then, with Fock, Re and Im of D_ab(R) of every entry, in list order).
// An entry (a, b, R) stands for the bond and its mirror (b, a, -R): given twice in either form it is refused.
struct MfField {           // one contribution to a term of the private model: amp(key) += coef x[par] in its real (part 0) or imaginary part
    int a, b, R[4];        // the key in flatten order: a <= b (a > b is stored as (b, a, -R), conjugated: the sign of an imaginary coef)
    double coef;
    int par, part;
};
struct MfProblem {
    int n = 0, dk = 0, nint = 0, nocc = 0, fock = 0, nR = 0;
    int64_t np = 0;
    std::vector<int> occ_par;            // [n]: the parameter of n_a, -1 where no V touches a
    std::vector<int32_t> Rl;             // [nR][dk]: R = 0 first, then the entries' vectors in order of first appearance
    std::vector<int> ent_r;              // [nint]: the index of an entry's R in Rl
    std::vector<int64_t> gidx;           // [np]: where x_out[p] sits in acc[nR][n][n] seen as doubles
    std::vector<int32_t> pin;            // [npin][6]
    std::vector<MfField> field;
    std::vector<double> rowsum;          // [n]: sum_b,R |V_ab(R)| (both directions of every bond)
};
static int mf_problem(const char* fn, int dk, int n, const MfArgs& A, MfProblem& P) {
    P = MfProblem();
    P.n = n, P.dk = dk, P.nint = A.nint, P.fock = A.fock ? 1 : 0;
    P.occ_par.assign((size_t)n, -1);
    P.rowsum.assign((size_t)n, 0.0);
    std::map<std::array<int, 6>, int> seen;
    std::map<std::array<int, 4>, int> rid;
    rid[{0, 0, 0, 0}] = 0;
    P.Rl.assign((size_t)dk, 0);
    P.ent_r.resize((size_t)A.nint);
    for (int e = 0; e < A.nint; ++e) {
        const int a = A.ab[2 * e], b = A.ab[2 * e + 1];
        std::array<int, 4> R{0, 0, 0, 0};
        for (int d = 0; d < dk; ++d) R[d] = A.R[(int64_t)e * dk + d];
        const std::array<int, 6> k1{a, b, R[0], R[1], R[2], R[3]}, k2{b, a, -R[0], -R[1], -R[2], -R[3]};
        TBK_REQUIRE(!seen.count(k1) && !seen.count(k2), TBK_EINVAL, "%s: interaction %d repeats the bond of interaction %d (a bond is given once)",
                    fn, e, seen.count(k1) ? seen[k1] : seen[k2]);
        seen[k1] = e;
        P.occ_par[a] = P.occ_par[b] = 0;
        auto it = rid.find(R);
        if (it == rid.end()) {
            it = rid.emplace(R, (int)rid.size()).first;
            for (int d = 0; d < dk; ++d) P.Rl.push_back(R[d]);
        }
        P.ent_r[e] = it->second;
        P.rowsum[a] += fabs(A.V[e]);
        P.rowsum[b] += fabs(A.V[e]);
    }
    P.nR = (int)rid.size();
    TBK_REQUIRE(P.nR <= kOccRMax, TBK_EINVAL, "%s: %d distinct lattice vectors (at most %d)", fn, P.nR, kOccRMax);
    TBK_REQUIRE((int64_t)P.nR * n * n <= kOccOutCap, TBK_EINVAL, "%s: nR * nsta^2 = %lld (at most %lld)", fn, (long long)P.nR * n * n,
                (long long)kOccOutCap);
    for (int a = 0; a < n; ++a)
        if (P.occ_par[a] == 0) P.occ_par[a] = P.nocc++;
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
        // Hartree: the on-site energy of a gets V n_b and that of b gets V n_a (a == b, R != 0: 2 V n_a, the bonds to R and to -R)
        P.field.push_back(MfField{a, a, {0, 0, 0, 0}, V, P.occ_par[b], 0});
        P.field.push_back(MfField{b, b, {0, 0, 0, 0}, V, P.occ_par[a], 0});
        if (!P.fock) continue;
        const int pr = P.nocc + 2 * e, pi = pr + 1;
        P.gidx[pr] = 2 * ((int64_t)P.ent_r[e] * nn + (int64_t)a * n + b);
        P.gidx[pi] = P.gidx[pr] + 1;
        const int32_t q[6] = {a, b, R[0], R[1], R[2], R[3]};
        P.pin.insert(P.pin.end(), q, q + 6);
        // Fock: the entry (a, b, R) of the table gets -V D_ab(R); stored above the diagonal, so (a > b) as (b, a, -R) conjugated;
        // on the diagonal (a == b) the slot also holds the mirror term at -R with the conjugate
        if (a <= b) {
            P.field.push_back(MfField{a, b, {R[0], R[1], R[2], R[3]}, -V, pr, 0});
            P.field.push_back(MfField{a, b, {R[0], R[1], R[2], R[3]}, -V, pi, 1});
        }
        if (a >= b) {
            P.field.push_back(MfField{b, a, {-R[0], -R[1], -R[2], -R[3]}, -V, pr, 0});
            P.field.push_back(MfField{b, a, {-R[0], -R[1], -R[2], -R[3]}, V, pi, 1});
        }
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
// One private device block.  resident: every chunk's eigenvectors stay (chunk c at c * vstride c128); else one chunk's worth.
struct MfPlan {
    bool resident = false;
    int64_t npts = 0, chunk = 0, nchunks = 0, nlev = 0, vstride = 0;
    int G = 0;                 // groups of the level scans (occ_scan_groups)
    OccDmPlan dm;
    enum { K_ALL, LEV, EC, VEC, FW, DPART, ACC, RDEV, FPART, FSMALL, SPART, XIN, XOUT, XPREV, RINGX, RINGR, SMALL, GIDX, TBASE, TPTR, TTERM, TRBLK,
           CCOEF, CPAR, CPART, RESH, OCCH, NBUF };
    size_t off[NBUF + 1];
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
    const int m = std::max(history, 1);
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
    b[MfPlan::XIN] = b[MfPlan::XOUT] = b[MfPlan::XPREV] = (size_t)np * D;
    b[MfPlan::RINGX] = b[MfPlan::RINGR] = (size_t)m * np * D;
    b[MfPlan::SMALL] = 1024;                            // the Gram matrix [8][8]
    b[MfPlan::GIDX] = (size_t)np * sizeof(int64_t);
    b[MfPlan::TBASE] = (size_t)nft * 2 * D;
    b[MfPlan::TPTR] = (size_t)(nft + 1) * sizeof(int32_t);
    b[MfPlan::TTERM] = (size_t)nft * sizeof(int32_t);
    b[MfPlan::TRBLK] = (size_t)nft * sizeof(int64_t);
    b[MfPlan::CCOEF] = (size_t)nnz * D;
    b[MfPlan::CPAR] = b[MfPlan::CPART] = (size_t)nnz * sizeof(int32_t);
    b[MfPlan::RESH] = (size_t)max_iter * D;
    b[MfPlan::OCCH] = (size_t)max_iter * n * D;
    p.off[0] = 256;
    for (int i = 0; i < MfPlan::NBUF; ++i) p.off[i + 1] = p.off[i] + al256(b[i]);
    p.total = p.off[MfPlan::NBUF];
    return p;
}
