// Stand-alone host check of tbk_mf.h (no device call): built under AddressSanitizer + UBSan by `make -C pythtb_amd/csrc mf-check` and run
// as an ordinary program.  It covers every argument rule of tbk_mean_field_mesh and the edge of every cap; the expansion of an
// interaction list into parameters, pins, gather indices and the term -> parameter map for hand-worked cases (Hubbard U on a spinful
// two-orbital cell; one nearest-neighbour V on a spinless cell with and without a hop on that bond; a bond and its mirror given
// twice); the walk over the interaction list that the three drivers share (tbk_int.h: the repeated bond with the earlier index, the
// lattice vectors in order of first appearance, the ascending touched states, dim_k = 1, 2, 3, 4096 and 4097 vectors); the small
// Anderson solve against values worked out by hand (m = 1, 2, 8, a zero residual, a non-finite entry); and the loop block and the
// resident and two-pass workspace layouts, filled and read back under the sanitizer.  The pinned flatten itself lives in
// tbk_core.hip, beside the flatten it extends, and is held by tests/test_mean_field.py through tbk_model_flatten_host_pinned.
#include <cmath>
#include <limits>
#include <vector>
#include "../tbk_mf.h"
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
    MfArgs args() const {
        MfArgs A;
        A.nint = (int)V.size(), A.ab = ab.data(), A.R = R.data(), A.V = V.data();
        A.nel = 1.0;
        return A;
    }
};

static int check_arguments() {
    const int32_t mesh[3] = {4, 4, 4};
    Inter I;
    I.add(0, 1, {0, 0}, 1.0);
    int64_t npts;
    double target;
    MfArgs A = I.args();
    EXPECT(mf_check("t", 2, 2, mesh, A, npts, target) == TBK_OK && npts == 16 && target == 16.0);
    EXPECT(mf_check("t", 0, 2, mesh, A, npts, target) == TBK_EINVAL);              // dim_k 1..3
    EXPECT(mf_check("t", 4, 2, mesh, A, npts, target) == TBK_EINVAL);
    EXPECT(mf_check("t", 2, 2049, mesh, A, npts, target) == TBK_EINVAL);           // nsta <= 2048
#define BAD(stmt)                                                         \
    do {                                                                  \
        MfArgs B = A;                                                     \
        stmt;                                                             \
        EXPECT(mf_check("t", 2, 2, mesh, B, npts, target) == TBK_EINVAL); \
    } while (0)
#define GOOD(stmt)                                                        \
    do {                                                                  \
        MfArgs B = A;                                                     \
        stmt;                                                             \
        EXPECT(mf_check("t", 2, 2, mesh, B, npts, target) == TBK_OK);     \
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
    BAD(B.mixing = std::numeric_limits<double>::quiet_NaN());
    GOOD(B.mixing = 1.0);
    BAD(B.tol = -1e-300);
    BAD(B.tol = std::numeric_limits<double>::infinity());
    GOOD(B.tol = 0.0);
    BAD(B.kT = -1.0);
    BAD(B.nel = 0.53);                                                             // 0.53 x 16 points: not an integer at kT = 0
    BAD(B.nel = 2.0);                                                              // every level: nothing to select
    GOOD((B.nel = 0.53, B.kT = 0.1));
    BAD((B.nel = 2.0, B.kT = 0.1));
    BAD((B.have_nel = 0, B.mu = std::numeric_limits<double>::infinity()));
    GOOD((B.have_nel = 0, B.mu = -3.0));
    Inter S;                                                                       // a self-interaction, an index, a long vector
    S.add(1, 1, {0, 0}, 1.0);
    MfArgs As = S.args();
    EXPECT(mf_check("t", 2, 2, mesh, As, npts, target) == TBK_EINVAL && strstr(g_err, "self-interaction"));
    Inter O;
    O.add(0, 2, {0, 0}, 1.0);
    MfArgs Ao = O.args();
    EXPECT(mf_check("t", 2, 2, mesh, Ao, npts, target) == TBK_EINVAL);
    Inter L;
    L.add(0, 1, {1 << 30, 0}, 1.0);
    MfArgs Al = L.args();
    EXPECT(mf_check("t", 2, 2, mesh, Al, npts, target) == TBK_EINVAL);
    Inter N;
    N.add(0, 1, {0, 0}, std::numeric_limits<double>::quiet_NaN());
    MfArgs An = N.args();
    EXPECT(mf_check("t", 2, 2, mesh, An, npts, target) == TBK_EINVAL);
    // the caps of the expansion: 4096 lattice vectors, nR nsta^2 <= 2^22
    Inter M;
    for (int r = 1; r <= 4096; ++r) M.add(0, 1, {r, 0}, 1.0);                      // with R = 0: 4097 vectors
    MfProblem P;
    EXPECT(mf_problem("t", 2, 2, M.args(), P) == TBK_EINVAL && strstr(g_err, "distinct lattice vectors"));
    M.ab.resize(2 * 4095), M.R.resize(2 * 4095), M.V.resize(4095);
    EXPECT(mf_problem("t", 2, 2, M.args(), P) == TBK_OK && P.nR == 4096);
    Inter W;
    W.add(0, 1, {1}, 1.0);
    EXPECT(mf_problem("t", 1, 1449, W.args(), P) == TBK_EINVAL && strstr(g_err, "nR * nsta^2"));   // 2 x 1449^2 > 2^22
    EXPECT(mf_problem("t", 1, 1448, W.args(), P) == TBK_OK);
    return 0;
}

static int check_expansion() {
    MfProblem P;
    {   // Hubbard U on a spinful two-orbital cell: states (0 up, 0 down, 1 up, 1 down), entries (0, 1) and (2, 3) at R = 0
        Inter I;
        I.add(0, 1, {0, 0}, 3.0);
        I.add(2, 3, {0, 0}, 2.0);
        MfArgs A = I.args();
        EXPECT(mf_problem("t", 2, 4, A, P) == TBK_OK);
        EXPECT(P.nocc == 4 && P.np == 8 && P.nR == 1 && P.pin.size() == 6 * 6);
        EXPECT(P.gidx[0] == 0 && P.gidx[1] == 2 * 5 && P.gidx[3] == 2 * 15 && P.gidx[4] == 2 * 1 && P.gidx[5] == 2 * 1 + 1 &&
               P.gidx[6] == 2 * 11);
        EXPECT(P.rowsum[0] == 3.0 && P.rowsum[3] == 2.0);
        // the flattened model: on-site terms of the four states and the two spin-flip terms, slots of a 4-state model
        // (0,0)=0 (0,1)=1 (1,1)=4 (2,2)=7 (2,3)=8 (3,3)=9; terms in slot order, one each
        const int nslot = 10;
        std::vector<int32_t> slot_ptr = {0, 1, 2, 2, 2, 3, 3, 3, 4, 5, 6};
        std::vector<int32_t> R4(6 * 4, 0);
        std::vector<double> amp2 = {0.1, 0, 0, 0, 0.1, 0, -0.1, 0, 0, 0, -0.1, 0};
        std::vector<int32_t> rvec(4, 0);
        MfMap M;
        EXPECT(mf_map("t", P, nslot, slot_ptr, R4, amp2, 1, rvec, M) == TBK_OK);
        EXPECT(M.term.size() == 6 && M.ptr.back() == 8);
        // term 0 = eps of state 0: + 3 n_1 (parameter 1); term 1 = (0, 1): -3 Re (parameter 4), -3 Im (parameter 5)
        EXPECT(M.ptr[1] == 1 && M.coef[0] == 3.0 && M.par[0] == 1 && M.part[0] == 0 && M.base[0] == 0.1);
        EXPECT(M.ptr[2] == 3 && M.coef[1] == -3.0 && M.par[1] == 4 && M.part[1] == 0 && M.coef[2] == -3.0 && M.par[2] == 5 && M.part[2] == 1);
        EXPECT(M.rblk[1] == 1 && M.rblk[4] == 8 && M.rblk[5] == 9);
        EXPECT(M.coef[3] == 3.0 && M.par[3] == 0);                                 // eps of state 1: + 3 n_0
    }
    {   // one nearest-neighbour V on a spinless two-orbital cell, given from the upper orbital: (1, 0, R = +1) is stored as (0, 1, -1)
        Inter I;
        I.add(1, 0, {1}, 0.5);
        EXPECT(mf_problem("t", 1, 2, I.args(), P) == TBK_OK);
        EXPECT(P.nocc == 2 && P.np == 4 && P.nR == 2 && P.Rl[0] == 0 && P.Rl[1] == 1);
        EXPECT(P.gidx[2] == 2 * (4 + 2) && P.gidx[3] == 2 * (4 + 2) + 1);          // D_10(R = 1): acc[1][1][0]
        // (a) the model has a hop on that bond: terms eps_0 | (0,1,R=-1) | eps_1
        std::vector<int32_t> slot_ptr = {0, 1, 2, 3};
        std::vector<int32_t> R4 = {0, 0, 0, 0, -1, 0, 0, 0, 0, 0, 0, 0};
        std::vector<double> amp2 = {0, 0, -1.0, 0, 0, 0};
        std::vector<int32_t> rvec;
        MfMap M;
        EXPECT(mf_map("t", P, 3, slot_ptr, R4, amp2, 0, rvec, M) == TBK_OK);
        EXPECT(M.term.size() == 3 && M.term[1] == 1 && M.base[2] == -1.0 && M.rblk[1] == -1);
        // the stored term is the conjugate: -V Re, +V Im
        EXPECT(M.coef[1] == -0.5 && M.par[1] == 2 && M.part[1] == 0 && M.coef[2] == 0.5 && M.par[2] == 3 && M.part[2] == 1);
        // (b) without the pinned term the map refuses
        std::vector<int32_t> sp2 = {0, 1, 1, 2};
        std::vector<int32_t> R42(8, 0);
        std::vector<double> a2(4, 0.0);
        EXPECT(mf_map("t", P, 3, sp2, R42, a2, 0, rvec, M) == TBK_EINVAL);
        // Hartree only: no bond parameters and no bond pin
        MfArgs A = I.args();
        A.fock = 0;
        EXPECT(mf_problem("t", 1, 2, A, P) == TBK_OK && P.np == 2 && P.pin.size() == 12 && P.field.size() == 2);
    }
    {   // a bond and its mirror: refused; a bond on the diagonal gets both directions
        Inter I;
        I.add(0, 1, {1}, 0.5);
        I.add(1, 0, {-1}, 0.5);
        EXPECT(mf_problem("t", 1, 2, I.args(), P) == TBK_EINVAL && strstr(g_err, "given once"));
        Inter J;
        J.add(0, 0, {1}, 0.5);
        J.add(0, 0, {-1}, 0.5);
        EXPECT(mf_problem("t", 1, 1, J.args(), P) == TBK_EINVAL);
        Inter K;
        K.add(0, 0, {1}, 0.5);
        EXPECT(mf_problem("t", 1, 1, K.args(), P) == TBK_OK && P.np == 3);
        int nfock = 0;
        for (const MfField& F : P.field) nfock += F.par >= 1;
        EXPECT(nfock == 4 && P.field[0].coef == 0.5 && P.field[1].coef == 0.5);    // Hartree: 2 V n_0 in two halves
    }
    return 0;
}

static int check_anderson() {
    double B[64], c[8], W[MF_AND_WORK];
    memset(B, 0, sizeof B);
    B[0] = 4.0;
    EXPECT(mf_anderson(1, B, c, W) && fabs(c[0] - 1.0) < 1e-15);
    B[0] = 1.0, B[9] = 4.0;                                                        // orthogonal residuals: c_j ~ 1 / |r_j|^2
    EXPECT(mf_anderson(2, B, c, W) && fabs(c[0] - 0.8) < 1e-11 && fabs(c[1] - 0.2) < 1e-11);
    B[0] = 1.0, B[1] = B[8] = -0.5, B[9] = 1.0;                                    // symmetric: halves
    EXPECT(mf_anderson(2, B, c, W) && fabs(c[0] - 0.5) < 1e-12 && fabs(c[1] - 0.5) < 1e-12);
    B[0] = 1.0, B[1] = B[8] = 1.0, B[9] = 1.0;                                     // the same residual twice: singular but for the
    EXPECT(mf_anderson(2, B, c, W) && fabs(c[0] + c[1] - 1.0) < 1e-12);            // regularisation, which splits it evenly
    EXPECT(fabs(c[0] - 0.5) < 1e-3);
    B[0] = 0.0, B[1] = B[8] = 0.0, B[9] = 1.0;                                     // a zero residual: the linear step
    EXPECT(!mf_anderson(2, B, c, W));
    B[0] = std::numeric_limits<double>::quiet_NaN();
    EXPECT(!mf_anderson(2, B, c, W));
    memset(B, 0, sizeof B);
    for (int j = 0; j < 8; ++j) B[9 * j] = 1.0;
    EXPECT(mf_anderson(8, B, c, W));
    for (int j = 0; j < 8; ++j) EXPECT(fabs(c[j] - 0.125) < 1e-12);
    EXPECT(!mf_anderson(0, B, c, W) && !mf_anderson(9, B, c, W));
    return 0;
}

// buffers [off[i], off[i + 1]) from `first` on: every one 256-aligned and behind the one before, the last ending at `total`; then filled
// and read back under the sanitizer
static int check_offsets(const char* tag, const std::vector<size_t>& off, size_t first, size_t total) {
    const int nb = (int)off.size() - 1;
    size_t end = first;
    for (int i = 0; i < nb; ++i) {
        if (off[i] % 256 || off[i] < end) return printf("%s: buffer %d at %zu (the previous one ends at %zu)\n", tag, i, off[i], end);
        end = off[i + 1];
    }
    if (end != total) return printf("%s: the total\n", tag);
    if (total > ((size_t)256 << 20)) return 0;
    unsigned char* base = (unsigned char*)aligned_alloc(256, al256(total));
    if (!base) return printf("%s: no host block\n", tag);
    int bad = 0;
    for (int i = 0; i < nb; ++i) memset(base + off[i], i + 1, off[i + 1] - off[i]);
    for (int i = 0; i < nb && !bad; ++i)
        for (size_t j = off[i]; j < off[i + 1]; j += 61)
            if (base[j] != (unsigned char)(i + 1)) {
                bad = printf("%s: buffer %d is overwritten\n", tag, i);
                break;
            }
    free(base);
    return bad;
}
// the driver's own buffers, then the loop block behind them
static int check_layout(const char* tag, const MfPlan& p) {
    std::vector<size_t> off(p.off, p.off + MfPlan::NBUF);
    off.insert(off.end(), p.loop.off, p.loop.off + MfLoopBufs::NBUF + 1);
    if (p.loop.off[0] != p.off[MfPlan::NBUF]) return printf("%s: the loop block does not follow the driver's buffers\n", tag);
    return check_offsets(tag, off, 256, p.total);
}
// the walk of tbk_int.h itself, as the three drivers call it
static int check_walk() {
    IntBonds B;
    auto walk = [&](int dk, int n, const Inter& I) { return int_bonds("t", dk, n, (int)I.V.size(), I.ab.data(), I.R.data(), I.V.data(), B); };
    for (int dk = 1; dk <= 3; ++dk) {
        auto vec = [&](int r) {                                                    // r in the LAST component: a key cut short would miss it
            std::vector<int> v((size_t)dk, 0);
            v[dk - 1] = r;
            return v;
        };
        // a bond and its mirror, in both orders, behind another bond: the refusal names the earlier entry
        for (int order = 0; order < 2; ++order) {
            Inter I;
            I.add(0, 2, vec(0), 1.0);
            I.add(order ? 1 : 0, order ? 0 : 1, vec(order ? -1 : 1), 0.5);
            I.add(order ? 0 : 1, order ? 1 : 0, vec(order ? 1 : -1), 0.5);
            EXPECT(walk(dk, 3, I) == TBK_EINVAL && strstr(g_err, "interaction 2 repeats the bond of interaction 1") && strstr(g_err, "given once"));
            I.ab[4] = I.ab[2], I.ab[5] = I.ab[3], I.R[2 * dk + dk - 1] = I.R[dk + dk - 1];   // the same entry again
            EXPECT(walk(dk, 3, I) == TBK_EINVAL && strstr(g_err, "interaction 2 repeats the bond of interaction 1"));
            I.R[2 * dk + dk - 1] = 7;                                              // another vector: another bond
            EXPECT(walk(dk, 3, I) == TBK_OK && B.nR == 3);
        }
        // the lattice vectors: R = 0 first, then in order of first appearance -- with R = 0 given first, in the middle, not at all
        const int given[3][3] = {{0, 1, 2}, {2, 0, 1}, {3, -1, 3}}, Rl[3][3] = {{0, 1, 2}, {0, 2, 1}, {0, 3, -1}}, er[3][3] = {{0, 1, 2}, {1, 0, 2}, {1, 2, 1}};
        for (int c = 0; c < 3; ++c) {
            Inter I;
            for (int e = 0; e < 3; ++e) I.add(e, e + 1, vec(given[c][e]), 1.0 + e);
            EXPECT(walk(dk, 4, I) == TBK_OK && B.nR == 3 && B.Rl.size() == (size_t)3 * dk && B.ent_r.size() == 3);
            for (int r = 0; r < 3; ++r) {
                EXPECT(B.Rl[(size_t)r * dk + dk - 1] == Rl[c][r] && B.ent_r[r] == er[c][r]);
                for (int d = 0; d + 1 < dk; ++d) EXPECT(B.Rl[(size_t)r * dk + d] == 0);
            }
            EXPECT(B.nocc == 4 && B.rowsum[0] == 1.0 && B.rowsum[1] == 3.0 && B.rowsum[2] == 5.0 && B.rowsum[3] == 3.0);
        }
        // the touched states, ascending, with gaps
        Inter G;
        G.add(7, 2, vec(0), 1.0);
        G.add(5, 7, vec(1), -2.0);
        EXPECT(walk(dk, 9, G) == TBK_OK && B.nocc == 3 && B.occ_par.size() == 9 && B.occ_par[2] == 0 && B.occ_par[5] == 1 && B.occ_par[7] == 2);
        for (int a : {0, 1, 3, 4, 6, 8}) EXPECT(B.occ_par[a] == -1 && B.rowsum[a] == 0.0);
        EXPECT(B.rowsum[7] == 3.0 && B.rowsum[2] == 1.0 && B.rowsum[5] == 2.0);
        // one state, one entry: the bond to its own image, both directions in the row sum
        Inter O;
        O.add(0, 0, vec(1), -0.75);
        EXPECT(walk(dk, 1, O) == TBK_OK && B.nocc == 1 && B.occ_par[0] == 0 && B.nR == 2 && B.ent_r[0] == 1 && B.rowsum[0] == 1.5);
        // 4096 vectors and 4097: the walk counts them, the cap is the driver's (check_arguments)
        Inter M;
        for (int r = 1; r <= 4096; ++r) M.add(0, 1, vec(r), 1.0);
        EXPECT(walk(dk, 2, M) == TBK_OK && B.nR == 4097 && B.ent_r[4095] == 4096 && B.Rl.size() == (size_t)4097 * dk);
        MfProblem P;
        EXPECT(mf_problem("t", dk, 2, M.args(), P) == TBK_EINVAL && strstr(g_err, "4097 distinct lattice vectors"));
        M.ab.resize(2 * 4095), M.R.resize((size_t)dk * 4095), M.V.resize(4095);
        EXPECT(walk(dk, 2, M) == TBK_OK && B.nR == 4096 && B.Rl[(size_t)4095 * dk + dk - 1] == 4095);
        EXPECT(mf_problem("t", dk, 2, M.args(), P) == TBK_OK && P.nR == 4096);
    }
    return 0;
}

// the loop block alone: np = 1, no map (nft = 0), without and with the longest ring, behind an unaligned end
static int check_loop_block() {
    for (int history : {0, 8}) {
        MfLoopBufs L;
        const size_t end = mf_loop_bufs(L, 256 + 40, 1, history, 3, 0, 0, 5);
        EXPECT(L.off[0] == 512);
        EXPECT(check_offsets("loop", std::vector<size_t>(L.off, L.off + MfLoopBufs::NBUF + 1), 512, end) == 0);
        auto size = [&](int i) { return L.off[i + 1] - L.off[i]; };
        EXPECT(size(MfLoopBufs::XIN) == 256 && size(MfLoopBufs::XOUT) == 256 && size(MfLoopBufs::XPREV) == 256 && size(MfLoopBufs::GIDX) == 256);
        EXPECT(size(MfLoopBufs::RINGX) == 256 && size(MfLoopBufs::RINGR) == 256 && size(MfLoopBufs::SMALL) == 1024);
        EXPECT(size(MfLoopBufs::TBASE) == 0 && size(MfLoopBufs::TTERM) == 0 && size(MfLoopBufs::TRBLK) == 0 && size(MfLoopBufs::TPTR) == 256);
        EXPECT(size(MfLoopBufs::CCOEF) == 0 && size(MfLoopBufs::CPAR) == 0 && size(MfLoopBufs::CPART) == 0);
        EXPECT(size(MfLoopBufs::RESH) == 256 && size(MfLoopBufs::OCCH) == 256);
    }
    // the sizes of a larger one: 100 parameters, a ring of 8, 7 terms with 19 contributions, 11 iterations of 6 occupations
    MfLoopBufs L;
    const size_t end = mf_loop_bufs(L, 256, 100, 8, 11, 7, 19, 6);
    EXPECT(check_offsets("loop", std::vector<size_t>(L.off, L.off + MfLoopBufs::NBUF + 1), 256, end) == 0);
    auto size = [&](int i) { return L.off[i + 1] - L.off[i]; };
    EXPECT(size(MfLoopBufs::XIN) == al256(800) && size(MfLoopBufs::RINGX) == al256(6400) && size(MfLoopBufs::RINGR) == al256(6400));
    EXPECT(size(MfLoopBufs::GIDX) == al256(800) && size(MfLoopBufs::TBASE) == al256(112) && size(MfLoopBufs::TPTR) == al256(32));
    EXPECT(size(MfLoopBufs::TTERM) == al256(28) && size(MfLoopBufs::TRBLK) == al256(56) && size(MfLoopBufs::CCOEF) == al256(152));
    EXPECT(size(MfLoopBufs::CPAR) == al256(76) && size(MfLoopBufs::CPART) == al256(76) && size(MfLoopBufs::RESH) == al256(88));
    EXPECT(size(MfLoopBufs::OCCH) == al256(528));
    return 0;
}

static int check_plans() {
    // 40 states on 1369 points: chunks of 1310 + 59; resident, and two-pass under a lowered cap
    MfPlan a = mf_plan(40, 1, 1369, 2, 120, 4, 3, 80, 160, mf_resident_cap(-1));
    EXPECT(a.resident && a.chunk == 1310 && a.nchunks == 2 && a.nlev == 40 * 1369 && a.vstride >= 1310 * 1600 && a.vstride % 16 == 0);
    EXPECT(a.off[MfPlan::VEC + 1] - a.off[MfPlan::VEC] >= (size_t)2 * a.vstride * 16);
    EXPECT(check_layout("resident", a) == 0);
    MfPlan b = mf_plan(40, 1, 1369, 2, 120, 4, 3, 80, 160, mf_resident_cap(1));
    EXPECT(!b.resident && b.chunk == a.chunk && b.nchunks == a.nchunks && b.G == a.G && b.dm.G == a.dm.G);   // the same partition
    EXPECT(b.off[MfPlan::VEC + 1] - b.off[MfPlan::VEC] == al256((size_t)b.vstride * 16));
    EXPECT(check_layout("two-pass", b) == 0);
    // the cap itself: 2^26 c128 resident, one more point not
    EXPECT(mf_plan(32, 2, 65536, 1, 32, 0, 1, 32, 32, mf_resident_cap(-1)).resident);
    EXPECT(!mf_plan(32, 2, 65537, 1, 32, 0, 1, 32, 32, mf_resident_cap(-1)).resident);
    EXPECT(mf_resident_cap(0) == kMfResidentMax && mf_resident_cap((long long)1 << 40) == kMfResidentMax && mf_resident_cap(5) == 5);
    // no partition depends on history, max_iter or the number of parameters
    MfPlan c = mf_plan(40, 1, 1369, 2, 7, 0, 500, 3, 5, mf_resident_cap(-1));
    EXPECT(c.chunk == a.chunk && c.G == a.G && c.dm.G == a.dm.G && c.dm.P == a.dm.P && c.dm.RT == a.dm.RT);
    EXPECT(check_layout("small", mf_plan(2, 2, 144, 3, 14, 8, 65536, 8, 20, mf_resident_cap(-1))) == 0);
    return 0;
}

int main() {
    int bad = check_arguments();
    if (!bad) bad = check_expansion();
    if (!bad) bad = check_walk();
    if (!bad) bad = check_anderson();
    if (!bad) bad = check_loop_block();
    if (!bad) bad = check_plans();
    printf(bad ? "mf_plan_check: FAILED\n" : "mf_plan_check: ok\n");
    return bad ? 1 : 0;
}
