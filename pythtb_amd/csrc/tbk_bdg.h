// tbk_bdg.h -- the host-only part of tbk_bdg.hip (self-consistent Bogoliubov-de Gennes superconductivity on k meshes, DESIGN.md section
// 36): the argument checks and caps of tbk_bdg_mesh, the expansion of a state-indexed interaction list into the real parameter vector
// x, the triples of the Nambu density matrix the loop consumes, the pinned keys and the field of the private Nambu model (fed to
// tbk_mf.h's term -> parameter map) and the layout of the driver's private workspace.  No device call: check/bdg_plan_check.cpp drives
// it on the host alone (make bdg-check).
//
// n = nsta of the normal model; the Nambu model has N = 2 n states, particle a and hole n + a.  With D the density matrix of the Nambu
// model at Fermi level 0: n_a = D_aa(0), <c+_{b,R} c_{a,0}> = D_ab(R), F_ab(R) = <c_{b,R} c_{a,0}> = D_{a,n+b}(R).
#pragma once
#include "tbk_mf.h"
#include "tbk_pairs_dm.h"

static const int kBdgStatesMax = 1024;                  // states of the normal model

struct BdgArgs : MfArgs {
    int hartree = 1, pairing = 1;
    double mu_step = 1.0;
};
// mf_check's rules for the mesh, kT, the list and the loop; then: nsta <= 1024, any 0 < n_electrons < nsta (N is continuous in a paired
// state: no integrality rule), mu_step
static int bdg_check(const char* fn, int dk, int n, const int32_t* mesh, const BdgArgs& A, int64_t& npts) {
    TBK_REQUIRE(n >= 1 && n <= kBdgStatesMax, TBK_EINVAL, "%s: nsta=%d (1..%d states)", fn, n, kBdgStatesMax);
    MfArgs B = A;
    B.have_nel = 0, B.mu = A.have_nel ? 0.0 : A.mu;
    double target;
    int rc = mf_check(fn, dk, n, mesh, B, npts, target);
    if (rc) return rc;
    if (A.have_nel)
        TBK_REQUIRE(std::isfinite(A.nel) && A.nel > 0.0 && A.nel < (double)n, TBK_EINVAL, "%s: n_electrons=%.17g outside (0, %d)", fn, A.nel, n);
    TBK_REQUIRE(std::isfinite(A.mu_step) && A.mu_step > 0.0, TBK_EINVAL, "%s: mu_step=%.17g (finite, > 0)", fn, A.mu_step);
    return TBK_OK;
}

// ---------------------------------------------------------------- the parameters
// x = (n_a of every state some V touches, ascending a; with fock Re, Im of D_ab(R) per entry; with pairing Re, Im of F_ab(R) per entry;
// with n_electrons given, mu last).  The triples of the Nambu density matrix: (a, a, 0) of EVERY state (N_out needs them all), then
// (a, b, R) per entry with fock, then (a, n + b, R) per entry with pairing.  P is tbk_mf.h's problem of the NAMBU model (P.n = 2 n): its
// pins and its field, through which mf_map builds the gather of k_mf_apply.
struct BdgProblem : IntBonds {                   // (the walk of tbk_int.h over the NORMAL model's states: occ_par[n], Rl)
    int n = 0, dk = 0, nint = 0, hartree = 0, fock = 0, pairing = 0, have_nel = 0;
    int64_t np = 0, nt = 0;
    int par_d = -1, par_f = -1, par_mu = -1;     // the first parameter of the D block and of the F block, and mu (-1: absent)
    std::vector<int32_t> tij, tR;                // [nt][2], [nt][dk]
    std::vector<int64_t> gidx;                   // [np - have_nel]: where x_out[p] sits in acc[nt] seen as doubles
    MfProblem P;
};
static int bdg_problem(const char* fn, int dk, int n, const BdgArgs& A, BdgProblem& B) {
    B = BdgProblem();
    B.n = n, B.dk = dk, B.nint = A.nint, B.hartree = A.hartree ? 1 : 0, B.fock = A.fock ? 1 : 0, B.pairing = A.pairing ? 1 : 0;
    B.have_nel = A.have_nel ? 1 : 0;
    TBK_REQUIRE(B.hartree || B.fock || B.pairing, TBK_EINVAL, "%s: every channel is switched off", fn);
    MfProblem& P = B.P;
    P.n = 2 * n, P.dk = dk, P.nint = A.nint, P.fock = B.fock;
    int rc = int_bonds(fn, dk, n, A.nint, A.ab, A.R, A.V, B);
    if (rc) return rc;
    TBK_REQUIRE(B.nR <= kOccRMax, TBK_EINVAL, "%s: %d distinct lattice vectors (at most %d)", fn, B.nR, kOccRMax);
    B.np = B.nocc;
    if (B.fock) B.par_d = (int)B.np, B.np += 2 * (int64_t)A.nint;
    if (B.pairing) B.par_f = (int)B.np, B.np += 2 * (int64_t)A.nint;
    if (B.have_nel) B.par_mu = (int)B.np, B.np += 1;
    TBK_REQUIRE(B.np <= kMfParamMax, TBK_EINVAL, "%s: %lld parameters (at most 2^20)", fn, (long long)B.np);
    B.nt = (int64_t)n + (int64_t)(B.fock + B.pairing) * A.nint;
    B.tij.reserve((size_t)B.nt * 2), B.tR.reserve((size_t)B.nt * dk);
    B.gidx.assign((size_t)(B.np - B.have_nel), 0);
    auto triple = [&](int i, int j, const int* R) {
        B.tij.push_back(i), B.tij.push_back(j);
        for (int d = 0; d < dk; ++d) B.tR.push_back(R ? R[d] : 0);
        return (int64_t)B.tij.size() / 2 - 1;
    };
    auto pin = [&](int a, int b, const int* R, int sign) {
        const int32_t q[6] = {a, b, sign * R[0], sign * R[1], sign * R[2], sign * R[3]};
        P.pin.insert(P.pin.end(), q, q + 6);
    };
    const int zero[4] = {0, 0, 0, 0};
    for (int a = 0; a < n; ++a) {
        const int64_t t = triple(a, a, nullptr);
        if (B.occ_par[a] >= 0) B.gidx[B.occ_par[a]] = 2 * t;
        if (B.have_nel || (B.hartree && B.occ_par[a] >= 0)) pin(a, a, zero, 1), pin(n + a, n + a, zero, 1);
        if (B.have_nel) {                                          // mu: -1 on the particle diagonal, +1 on the hole diagonal
            P.field.push_back(MfField{a, a, {0, 0, 0, 0}, -1.0, B.par_mu, 0});
            P.field.push_back(MfField{n + a, n + a, {0, 0, 0, 0}, 1.0, B.par_mu, 0});
        }
    }
    for (int ch = 0; ch < 3; ++ch)                                 // the channels one after the other: the order of x and of the triples
        for (int e = 0; e < A.nint; ++e) {
            const int a = A.ab[2 * e], b = A.ab[2 * e + 1];
            const double V = A.V[e];
            int R[4] = {0, 0, 0, 0};
            for (int d = 0; d < dk; ++d) R[d] = A.R[(int64_t)e * dk + d];
            const int mR[4] = {-R[0], -R[1], -R[2], -R[3]};
            if (ch == 0 && B.hartree) {
                // the on-site energy of a gets V n_b and that of b gets V n_a; the hole block the negative
                mf_field_hartree(P.field, a, b, V, B.occ_par[a], B.occ_par[b], 0, 1.0);
                mf_field_hartree(P.field, a, b, V, B.occ_par[a], B.occ_par[b], n, -1.0);
            }
            if (ch == 1 && B.fock) {
                const int pr = B.par_d + 2 * e, pi = pr + 1;
                const int64_t t = triple(a, b, R);
                B.gidx[pr] = 2 * t, B.gidx[pi] = 2 * t + 1;
                pin(a, b, R, 1), pin(n + a, n + b, R, 1);
                // particle: (a, b, R) gets -V D; hole: (n + a, n + b, R) gets +V conj(D); per stored direction (tbk_mf.h), particle
                // before hole
                for (int mirror = 0; mirror < 2; ++mirror)
                    if (mirror ? a >= b : a <= b) {
                        mf_field_fock(P.field, a, b, R, V, pr, 0, -1.0, -1.0, mirror);
                        mf_field_fock(P.field, a, b, R, V, pr, n, 1.0, -1.0, mirror);
                    }
            }
            if (ch == 2 && B.pairing) {
                const int pr = B.par_f + 2 * e, pi = pr + 1;
                const int64_t t = triple(a, n + b, R);
                B.gidx[pr] = 2 * t, B.gidx[pi] = 2 * t + 1;
                pin(a, n + b, R, 1), pin(b, n + a, R, -1);
                // Delta = V F on the hop (a -> n + b, R), -Delta on its antisymmetric mirror (b -> n + a, -R); both above the diagonal
                P.field.push_back(MfField{a, n + b, {R[0], R[1], R[2], R[3]}, V, pr, 0});
                P.field.push_back(MfField{a, n + b, {R[0], R[1], R[2], R[3]}, V, pi, 1});
                P.field.push_back(MfField{b, n + a, {mR[0], mR[1], mR[2], mR[3]}, -V, pr, 0});
                P.field.push_back(MfField{b, n + a, {mR[0], mR[1], mR[2], mR[3]}, -V, pi, 1});
            }
        }
    return TBK_OK;
}

// ---------------------------------------------------------------- the workspace
// One private device block.  The eigenvectors of ONE chunk: there is no resident and no two-pass form, the pair stage runs behind
// every chunk's solve at the Fermi level 0.
struct BdgPlan {
    int64_t npts = 0, nlev = 0;
    int G = 0;                 // groups of the level scans (occ_scan_groups)
    PdmPart pd;
    enum { K_ALL, LEV, EC, VEC, PART, ACC, TIJ, TR, SPART, GAPP, NBUF };
    size_t off[NBUF + 1];
    MfLoopBufs loop;
    size_t total = 0;
};
static BdgPlan bdg_plan(int n, int dk, int64_t npts, int64_t nt, int64_t np, int history, int max_iter, int64_t nft, int64_t nnz) {
    BdgPlan p;
    const size_t D = sizeof(double);
    const int N = 2 * n;
    p.npts = npts;
    p.nlev = npts * N;
    p.G = occ_scan_groups(p.nlev);
    p.pd = pdm_partition(N, npts);
    size_t b[BdgPlan::NBUF];
    b[BdgPlan::K_ALL] = (size_t)npts * dk * D;
    b[BdgPlan::LEV] = (size_t)p.nlev * D;
    b[BdgPlan::EC] = (size_t)p.pd.chunk * N * D;
    b[BdgPlan::VEC] = (size_t)p.pd.chunk * N * N * sizeof(cd);
    b[BdgPlan::PART] = (size_t)p.pd.G * std::min<int64_t>(p.pd.TL, nt) * sizeof(cd);
    b[BdgPlan::ACC] = (size_t)nt * sizeof(cd);
    b[BdgPlan::TIJ] = (size_t)nt * 2 * sizeof(int32_t);
    b[BdgPlan::TR] = (size_t)nt * dk * sizeof(int32_t);
    b[BdgPlan::SPART] = (size_t)3 * p.G * D + 512;      // the final scan's partials, its three sums, and the level 0 it scans at
    b[BdgPlan::GAPP] = (size_t)p.G * D + 256;           // the partial minima of |E| and their minimum
    p.off[0] = 256;
    for (int i = 0; i < BdgPlan::NBUF; ++i) p.off[i + 1] = p.off[i] + al256(b[i]);
    p.total = mf_loop_bufs(p.loop, p.off[BdgPlan::NBUF], np, history, max_iter, nft, nnz, n);
    return p;
}
