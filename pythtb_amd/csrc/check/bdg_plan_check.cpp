// Stand-alone host check of tbk_bdg.h and tbk_pairs_dm.h (no device call): built under AddressSanitizer + UBSan by
// `make -C pythtb_amd/csrc bdg-check` and run as an ordinary program.  It covers every argument rule of tbk_bdg_mesh and
// tbk_density_matrix_pairs_mesh and the edge of every cap; the parameter layout, the triples, the pins and the term -> parameter map
// for hand-worked cases (a Hubbard pair with the three channels and mu; a spinless bond with a = b; a Fock + pairing bond given from
// the upper orbital, a > b); the stage of the pair kernel for every size, its lane shares replayed on the host, the k-groups and the
// launch ranges of the triple list; and the workspace layouts, filled and read back under the sanitizer.
#include <cmath>
#include <limits>
#include <vector>
#include "../tbk_bdg.h"
#include "check_common.h"

#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) return printf("line %d: %s (%s)\n", __LINE__, #cond, g_err), 1;  \
    } while (0)

struct Inter {
    std::vector<int32_t> ab, R;
    std::vector<double> V;
    void add(int a, int b, std::vector<int> r, double v) {
        ab.push_back(a), ab.push_back(b);
        for (int x : r) R.push_back(x);
        V.push_back(v);
    }
    BdgArgs args() const {
        BdgArgs A;
        A.nint = (int)V.size(), A.ab = ab.data(), A.R = R.data(), A.V = V.data();
        A.nel = 0.8, A.fock = 0;
        return A;
    }
};

static int check_arguments() {
    const int32_t mesh[3] = {4, 4, 4};
    Inter I;
    I.add(0, 1, {0, 0}, -1.0);
    int64_t npts;
    BdgArgs A = I.args();
    EXPECT(bdg_check("t", 2, 2, mesh, A, npts) == TBK_OK && npts == 16);
    EXPECT(bdg_check("t", 0, 2, mesh, A, npts) == TBK_EINVAL);                     // dim_k 1..3
    EXPECT(bdg_check("t", 4, 2, mesh, A, npts) == TBK_EINVAL);
    EXPECT(bdg_check("t", 2, 1025, mesh, A, npts) == TBK_EINVAL && strstr(g_err, "1024"));
    {
        BdgArgs B = A;
        B.nel = 512.0;
        EXPECT(bdg_check("t", 2, 1024, mesh, B, npts) == TBK_OK);
    }
#define BAD(stmt)                                                 \
    do {                                                          \
        BdgArgs B = A;                                            \
        stmt;                                                     \
        EXPECT(bdg_check("t", 2, 2, mesh, B, npts) == TBK_EINVAL); \
    } while (0)
#define GOOD(stmt)                                                \
    do {                                                          \
        BdgArgs B = A;                                            \
        stmt;                                                     \
        EXPECT(bdg_check("t", 2, 2, mesh, B, npts) == TBK_OK);    \
    } while (0)
    BAD(B.nint = 0);
    BAD(B.history = -1);
    BAD(B.history = 9);
    GOOD(B.history = 0);
    GOOD(B.history = 8);
    BAD(B.max_iter = 0);
    BAD(B.max_iter = 65537);
    GOOD(B.max_iter = 65536);
    BAD(B.check_every = 0);
    GOOD(B.check_every = 1 << 20);
    BAD(B.mixing = 0.0);
    BAD(B.mixing = 1.0000001);
    GOOD(B.mixing = 1.0);
    BAD(B.tol = -1e-300);
    BAD(B.tol = std::numeric_limits<double>::infinity());
    GOOD(B.tol = 0.0);
    BAD(B.kT = -1.0);
    GOOD(B.nel = 0.53);                                                            // no integrality rule, at kT = 0 either
    GOOD(B.nel = 1.9999);
    BAD(B.nel = 2.0);
    BAD(B.nel = 0.0);
    BAD(B.nel = std::numeric_limits<double>::quiet_NaN());
    BAD(B.mu_step = 0.0);
    BAD(B.mu_step = std::numeric_limits<double>::infinity());
    GOOD(B.mu_step = 1e-3);
    BAD((B.have_nel = 0, B.mu = std::numeric_limits<double>::infinity()));
    GOOD((B.have_nel = 0, B.mu = -3.0, B.nel = 0.0));
    Inter S;
    S.add(1, 1, {0, 0}, 1.0);
    BdgArgs As = S.args();
    EXPECT(bdg_check("t", 2, 2, mesh, As, npts) == TBK_EINVAL && strstr(g_err, "self-interaction"));
    Inter O;
    O.add(0, 2, {0, 0}, 1.0);
    BdgArgs Ao = O.args();
    EXPECT(bdg_check("t", 2, 2, mesh, Ao, npts) == TBK_EINVAL);
    Inter L;
    L.add(0, 1, {1 << 30, 0}, 1.0);
    BdgArgs Al = L.args();
    EXPECT(bdg_check("t", 2, 2, mesh, Al, npts) == TBK_EINVAL);
    // the caps of the expansion: 4096 lattice vectors; every channel off
    Inter M;
    for (int r = 1; r <= 4096; ++r) M.add(0, 1, {r, 0}, 1.0);
    BdgProblem P;
    EXPECT(bdg_problem("t", 2, 2, M.args(), P) == TBK_EINVAL && strstr(g_err, "distinct lattice vectors"));
    M.ab.resize(2 * 4095), M.R.resize(2 * 4095), M.V.resize(4095);
    EXPECT(bdg_problem("t", 2, 2, M.args(), P) == TBK_OK && P.nR == 4096);
    BdgArgs Off = I.args();
    Off.hartree = Off.fock = Off.pairing = 0;
    EXPECT(bdg_problem("t", 2, 2, Off, P) == TBK_EINVAL && strstr(g_err, "switched off"));
    // the triples of tbk_density_matrix_pairs_mesh
    const int32_t ij[4] = {0, 1, 1, 1}, R2[4] = {0, 0, -3, 5};
    EXPECT(pdm_check("t", 2, 2, mesh, 0.0, 0.0, 2, ij, R2, npts) == TBK_OK);
    EXPECT(pdm_check("t", 2, 2, mesh, 0.0, 0.0, 0, ij, R2, npts) == TBK_EINVAL);
    EXPECT(pdm_check("t", 2, 2, mesh, 0.0, 0.0, kPdmTripleMax + 1, ij, R2, npts) == TBK_EINVAL);
    EXPECT(pdm_check("t", 2, 2, mesh, std::numeric_limits<double>::quiet_NaN(), 0.0, 2, ij, R2, npts) == TBK_EINVAL);
    EXPECT(pdm_check("t", 2, 2, mesh, 0.0, -1.0, 2, ij, R2, npts) == TBK_EINVAL);
    const int32_t ijb[4] = {0, 1, 2, 1}, Rb[4] = {0, 0, 1 << 30, 0};
    EXPECT(pdm_check("t", 2, 2, mesh, 0.0, 0.0, 2, ijb, R2, npts) == TBK_EINVAL && strstr(g_err, "triple 1"));
    EXPECT(pdm_check("t", 2, 2, mesh, 0.0, 0.0, 2, ij, Rb, npts) == TBK_EINVAL && strstr(g_err, "2^30"));
    return 0;
}

// the fields of a key, in list order
static std::vector<MfField> fields_of(const MfProblem& P, int a, int b, std::vector<int> R) {
    R.resize(4, 0);
    std::vector<MfField> out;
    for (const MfField& F : P.field)
        if (F.a == a && F.b == b && F.R[0] == R[0] && F.R[1] == R[1] && F.R[2] == R[2] && F.R[3] == R[3]) out.push_back(F);
    return out;
}
static bool has_pin(const MfProblem& P, int a, int b, std::vector<int> R) {
    R.resize(4, 0);
    for (size_t p = 0; p + 6 <= P.pin.size(); p += 6)
        if (P.pin[p] == a && P.pin[p + 1] == b && P.pin[p + 2] == R[0] && P.pin[p + 3] == R[1] && P.pin[p + 4] == R[2] && P.pin[p + 5] == R[3])
            return true;
    return false;
}

static int check_expansion() {
    BdgProblem B;
    {   // a Hubbard pair: one spinful orbital, states (up, down), U = -4 at R = 0; Hartree + Fock + pairing + mu.  n = 2, Nambu 4
        Inter I;
        I.add(0, 1, {0, 0}, -4.0);
        BdgArgs A = I.args();
        A.fock = 1;
        EXPECT(bdg_problem("t", 2, 2, A, B) == TBK_OK);
        // x = (n_0, n_1, Re D, Im D, Re F, Im F, mu); triples (0,0,0) (1,1,0) (0,1,0) (0,3,0)
        EXPECT(B.nocc == 2 && B.np == 7 && B.par_d == 2 && B.par_f == 4 && B.par_mu == 6 && B.nt == 4 && B.nR == 1);
        EXPECT(B.tij[4] == 0 && B.tij[5] == 1 && B.tij[6] == 0 && B.tij[7] == 3);
        EXPECT(B.gidx.size() == 6 && B.gidx[0] == 0 && B.gidx[1] == 2 && B.gidx[2] == 4 && B.gidx[3] == 5 && B.gidx[4] == 6 && B.gidx[5] == 7);
        const MfProblem& P = B.P;
        EXPECT(P.n == 4);
        // the particle on-site term of state 0: -mu, then -4 n_1; its hole: +mu, +4 n_1
        std::vector<MfField> f = fields_of(P, 0, 0, {0, 0});
        EXPECT(f.size() == 2 && f[0].coef == -1.0 && f[0].par == 6 && f[1].coef == -4.0 && f[1].par == 1 && f[1].part == 0);
        f = fields_of(P, 2, 2, {0, 0});
        EXPECT(f.size() == 2 && f[0].coef == 1.0 && f[0].par == 6 && f[1].coef == 4.0 && f[1].par == 1);
        // Fock on (0, 1): -V D = +4 D; on the hole (2, 3): V conj(D) = -4 Re + 4 i Im
        f = fields_of(P, 0, 1, {0, 0});
        EXPECT(f.size() == 2 && f[0].coef == 4.0 && f[0].par == 2 && f[0].part == 0 && f[1].coef == 4.0 && f[1].par == 3 && f[1].part == 1);
        f = fields_of(P, 2, 3, {0, 0});
        EXPECT(f.size() == 2 && f[0].coef == -4.0 && f[0].par == 2 && f[1].coef == 4.0 && f[1].par == 3 && f[1].part == 1);
        // pairing: Delta = V F on (0 -> 2 + 1), -Delta on (1 -> 2 + 0)
        f = fields_of(P, 0, 3, {0, 0});
        EXPECT(f.size() == 2 && f[0].coef == -4.0 && f[0].par == 4 && f[0].part == 0 && f[1].coef == -4.0 && f[1].par == 5 && f[1].part == 1);
        f = fields_of(P, 1, 2, {0, 0});
        EXPECT(f.size() == 2 && f[0].coef == 4.0 && f[0].par == 4 && f[1].coef == 4.0 && f[1].par == 5 && f[1].part == 1);
        for (int a = 0; a < 4; ++a) EXPECT(has_pin(P, a, a, {0, 0}));
        EXPECT(has_pin(P, 0, 1, {0, 0}) && has_pin(P, 2, 3, {0, 0}) && has_pin(P, 0, 3, {0, 0}) && has_pin(P, 1, 2, {0, 0}));
        // the map over a flattened 4-state model that holds exactly the pinned terms: slots (0,0)=0 (0,1)=1 (0,3)=3 (1,1)=4 (1,2)=5
        // (2,2)=7 (2,3)=8 (3,3)=9, one term each
        std::vector<int32_t> slot_ptr = {0, 1, 2, 2, 3, 4, 5, 5, 6, 7, 8};
        std::vector<int32_t> R4(8 * 4, 0), rvec;
        std::vector<double> amp2(16, 0.0);
        amp2[0] = 0.5, amp2[2 * 5] = -0.5;                                         // eps_0 and its hole
        MfMap M;
        EXPECT(mf_map("t", P, 10, slot_ptr, R4, amp2, 0, rvec, M) == TBK_OK);
        EXPECT(M.term.size() == 8 && M.ptr.back() == (int)P.field.size() && M.base[0] == 0.5 && M.base[2 * 5] == -0.5);
        EXPECT(M.ptr[1] == 2 && M.par[0] == 6 && M.coef[0] == -1.0 && M.par[1] == 1 && M.coef[1] == -4.0);
        // given the Fermi level: no mu, no pins on untouched diagonals beyond the Hartree ones
        A.have_nel = 0, A.mu = -2.0;
        EXPECT(bdg_problem("t", 2, 2, A, B) == TBK_OK && B.np == 6 && B.par_mu == -1 && fields_of(B.P, 0, 0, {0, 0}).size() == 1);
        // pairing alone
        A.hartree = 0, A.fock = 0;
        EXPECT(bdg_problem("t", 2, 2, A, B) == TBK_OK && B.np == 4 && B.par_f == 2 && B.par_d == -1 && B.nt == 3 && B.P.field.size() == 4);
    }
    {   // a spinless bond with a = b: (0, 0, R = +1), V = -3, no Fock.  n = 1, Nambu 2
        Inter I;
        I.add(0, 0, {1}, -3.0);
        BdgArgs A = I.args();
        EXPECT(bdg_problem("t", 1, 1, A, B) == TBK_OK);
        EXPECT(B.nocc == 1 && B.np == 4 && B.par_f == 1 && B.par_mu == 3 && B.nt == 2 && B.nR == 2 && B.Rl[1] == 1);
        EXPECT(B.tij[2] == 0 && B.tij[3] == 1 && B.tR[1] == 1 && B.gidx[1] == 2 && B.gidx[2] == 3);
        // Hartree: 2 V n_0 in two halves, the hole the negative
        std::vector<MfField> f = fields_of(B.P, 0, 0, {0});
        EXPECT(f.size() == 3 && f[1].coef == -3.0 && f[2].coef == -3.0 && f[1].par == 0);
        f = fields_of(B.P, 1, 1, {0});
        EXPECT(f.size() == 3 && f[0].coef == 1.0 && f[1].coef == 3.0 && f[2].coef == 3.0);
        // pairing: (0 -> 1, R = 1) gets Delta, (0 -> 1, R = -1) gets -Delta: two terms of the same slot
        f = fields_of(B.P, 0, 1, {1});
        EXPECT(f.size() == 2 && f[0].coef == -3.0 && f[1].part == 1);
        f = fields_of(B.P, 0, 1, {-1});
        EXPECT(f.size() == 2 && f[0].coef == 3.0 && f[1].coef == 3.0);
        EXPECT(has_pin(B.P, 0, 1, {1}) && has_pin(B.P, 0, 1, {-1}));
        // with Fock the diagonal slot holds both directions, particle and hole
        A.fock = 1;
        EXPECT(bdg_problem("t", 1, 1, A, B) == TBK_OK && B.np == 6 && B.par_d == 1 && B.par_f == 3 && B.nt == 3);
        f = fields_of(B.P, 0, 0, {-1});
        EXPECT(f.size() == 2 && f[0].coef == 3.0 && f[1].coef == -3.0 && f[1].part == 1);   // conj(-V D)
        f = fields_of(B.P, 1, 1, {1});
        EXPECT(f.size() == 2 && f[0].coef == -3.0 && f[1].coef == 3.0);                     // V conj(D)
    }
    {   // Fock + pairing on a bond given from the upper orbital: (1, 0, R = +1), V = 0.5, two spinless orbitals.  n = 2, Nambu 4
        Inter I;
        I.add(1, 0, {1}, 0.5);
        BdgArgs A = I.args();
        A.fock = 1, A.hartree = 0;
        EXPECT(bdg_problem("t", 1, 2, A, B) == TBK_OK);
        EXPECT(B.np == 7 && B.par_d == 2 && B.par_f == 4 && B.nt == 4);
        EXPECT(B.tij[4] == 1 && B.tij[5] == 0 && B.tR[2] == 1 && B.tij[6] == 1 && B.tij[7] == 2 && B.tR[3] == 1);
        // particle: stored as (0, 1, -1) conjugated: -V Re, +V Im; hole (2, 3, -1): +V Re, +V Im
        std::vector<MfField> f = fields_of(B.P, 0, 1, {-1});
        EXPECT(f.size() == 2 && f[0].coef == -0.5 && f[0].par == 2 && f[1].coef == 0.5 && f[1].par == 3 && f[1].part == 1);
        f = fields_of(B.P, 2, 3, {-1});
        EXPECT(f.size() == 2 && f[0].coef == 0.5 && f[1].coef == 0.5 && f[1].part == 1);
        // pairing: (1 -> 2 + 0, R = 1) gets Delta, (0 -> 2 + 1, R = -1) gets -Delta
        f = fields_of(B.P, 1, 2, {1});
        EXPECT(f.size() == 2 && f[0].coef == 0.5 && f[0].par == 4 && f[1].coef == 0.5 && f[1].par == 5);
        f = fields_of(B.P, 0, 3, {-1});
        EXPECT(f.size() == 2 && f[0].coef == -0.5 && f[1].coef == -0.5);
        EXPECT(fields_of(B.P, 0, 0, {0}).size() == 1 && fields_of(B.P, 1, 1, {0}).size() == 1);   // mu alone: no Hartree
        // the bond and its mirror: refused
        I.add(0, 1, {-1}, 0.5);
        EXPECT(bdg_problem("t", 1, 2, I.args(), B) == TBK_EINVAL && strstr(g_err, "given once"));
    }
    return 0;
}

// the stage of k_pairs_dm for every size; its loops replayed for a few: every (point, band) of a group is visited once, by one wavefront
static int check_stage() {
    for (int n = 1; n <= 2048; ++n) {
        const PdmStage s = pdm_stage(n);
        EXPECT(s.P >= 1 && s.P <= 64 && s.NB >= 1 && s.NB <= n);
        EXPECT((int64_t)s.P * s.NB * n <= PDM_LDS_CD);                            // the vectors of a stage
        EXPECT(s.P * s.NB <= PDM_ROWS);                                           // its weights
        EXPECT(s.P == 1 || s.NB == n);                                            // several points: every band of each
    }
    EXPECT(pdm_stage(45).P == 1 && pdm_stage(45).NB == 45 && pdm_stage(46).NB == 44 && pdm_stage(4).P == 64 && pdm_stage(8).P == 32);
    for (int n : {1, 3, 4, 18, 34, 40, 46, 64, 100, 2048}) {
        const PdmStage st = pdm_stage(n);
        const bool pts = st.P > 1;
        const int64_t p0 = 7, p1 = 7 + 2 * st.P + 1;
        std::vector<int> seen((size_t)(p1 - p0) * n, 0);
        for (int w = 0; w < 4; ++w)
            for (int64_t b0 = p0; b0 < p1; b0 += st.P) {
                const int np = (int)std::min<int64_t>(st.P, p1 - b0);
                for (int bb0 = 0; bb0 < n; bb0 += st.NB) {
                    const int nb = std::min(st.NB, n - bb0);
                    const int bs = pts ? 0 : ((w - bb0) & 3), bstep = pts ? 1 : 4;
                    for (int p = pts ? w : 0; p < np; p += pts ? 4 : 1)
                        for (int b = bs; b < nb; b += bstep) {
                            EXPECT((int64_t)(b * np + p) * n + n <= PDM_LDS_CD);
                            seen[(size_t)(b0 + p - p0) * n + bb0 + b]++;
                        }
                }
            }
        for (int v : seen) EXPECT(v == 1);
    }
    return 0;
}

static int check_plans() {
    // 40 states on 1369 points: chunks of 1310 + 59; 164 groups of eight points; launch ranges of whole tiles under the cap
    PdmPart a = pdm_partition(40, 1369);
    EXPECT(a.chunk == 1310 && a.nchunks == 2 && a.P == 1 && a.NB == 40 && a.G == 164);
    EXPECT(a.TL % PDM_TILE == 0 && a.TL >= PDM_TILE && (int64_t)a.G * a.TL <= kPdmPartCap);
    EXPECT(check_groups("pairs", a.G, 1369, a.chunk, a.nchunks) == 0);
    // the Nambu model of Haldane on 256 x 256: one chunk, 64 points per stage, 256 groups
    PdmPart h = pdm_partition(4, 65536);
    EXPECT(h.nchunks == 1 && h.P == 64 && h.G == 256 && (int64_t)h.G * h.TL <= kPdmPartCap);
    for (int n : {1, 2, 4, 16, 45, 46, 64, 1024, 2048})
        for (int64_t npts : {(int64_t)1, (int64_t)7, (int64_t)4096, (int64_t)1 << 24}) {
            const PdmPart p = pdm_partition(n, npts);
            EXPECT(p.G >= 1 && p.G <= kPdmGroupsMax && p.G <= p.chunk && p.TL >= PDM_TILE && (int64_t)p.G * p.TL <= kPdmPartCap);
            EXPECT(check_groups("pairs", p.G, npts, p.chunk, p.nchunks) == 0);
        }
    // the launch ranges of 2^20 triples cover the list once
    {
        const PdmPart p = pdm_partition(64, 4096);
        int64_t at = 0, launches = 0;
        for (int64_t t0 = 0; t0 < kPdmTripleMax; t0 += p.TL) at += std::min<int64_t>(p.TL, kPdmTripleMax - t0), ++launches;
        EXPECT(at == kPdmTripleMax && launches == (kPdmTripleMax + p.TL - 1) / p.TL);
    }
    // the scratch block of the stand-alone call: nothing in the partition depends on the number of triples
    const PdmPlan s1 = pdm_plan(40, 2, 1369, 1, true), s2 = pdm_plan(40, 2, 1369, 100000, true);
    EXPECT(s1.G == s2.G && s1.chunk == s2.chunk && s1.TL == s2.TL && s1.P == s2.P);
    for (const PdmPlan* s : {&s1, &s2}) {
        const size_t buf[5][2] = {{s->off_ij, (size_t)s->nt * 8}, {s->off_R, (size_t)s->nt * 2 * 4}, {s->off_acc, (size_t)s->nt * 16},
                                  {s->off_part, (size_t)s->part_cd * 16}, {s->off_chunks, s->cw.bytes()}};
        EXPECT(check_buffers("pairs", buf, 5, s->total) == 0);
    }
    EXPECT(s2.part_cd == (int64_t)s2.G * std::min<int64_t>(s2.TL, 100000));
    // the driver's workspace: 20 states (Nambu 40) on 1369 points, 23 triples, 11 parameters
    const BdgPlan b = bdg_plan(20, 2, 1369, 23, 11, 4, 6, 50, 90);
    EXPECT(b.pd.chunk == 1310 && b.pd.nchunks == 2 && b.nlev == 40 * 1369 && b.G == occ_scan_groups(40 * 1369));
    size_t buf[BdgPlan::NBUF + MfLoopBufs::NBUF][2];                                // the driver's own buffers, then the loop block
    for (int i = 0; i < BdgPlan::NBUF; ++i) buf[i][0] = b.off[i], buf[i][1] = b.off[i + 1] - b.off[i];
    for (int i = 0; i < MfLoopBufs::NBUF; ++i) buf[BdgPlan::NBUF + i][0] = b.loop.off[i], buf[BdgPlan::NBUF + i][1] = b.loop.off[i + 1] - b.loop.off[i];
    EXPECT(check_buffers("bdg", buf, BdgPlan::NBUF + MfLoopBufs::NBUF, b.total) == 0);
    EXPECT(b.off[BdgPlan::VEC + 1] - b.off[BdgPlan::VEC] == al256((size_t)1310 * 1600 * 16));   // ONE chunk of eigenvectors
    EXPECT(b.loop.off[MfLoopBufs::OCCH + 1] - b.loop.off[MfLoopBufs::OCCH] == al256((size_t)6 * 20 * 8));
    // no partition depends on history, max_iter or the parameters
    const BdgPlan c = bdg_plan(20, 2, 1369, 2000, 900, 0, 500, 3, 5);
    EXPECT(c.pd.G == b.pd.G && c.pd.chunk == b.pd.chunk && c.G == b.G && c.pd.TL == b.pd.TL);
    return 0;
}

int main() {
    int bad = check_arguments();
    if (!bad) bad = check_expansion();
    if (!bad) bad = check_stage();
    if (!bad) bad = check_plans();
    printf(bad ? "bdg_plan_check: FAILED\n" : "bdg_plan_check: ok\n");
    return bad ? 1 : 0;
}
