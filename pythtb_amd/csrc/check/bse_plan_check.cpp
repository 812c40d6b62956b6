// Stand-alone host check of tbk_bse.h (no device call): built under AddressSanitizer + UBSan by `make -C pythtb_amd/csrc bse-check`
// and run as an ordinary program.  It covers the argument rules and caps of the exciton calls and the band selection; the expansion
// of a bond list into the set E with the index map of h for hand-worked cases (a Hubbard pair, a spinless bond, a bond with R != 0);
// the lane map and the partitions, and their independence of block width and list; the workspace layouts, filled and read back under
// the sanitizer; the polarisation algebra that turns the Lanczos runs into the tensor; and the continued fraction against a 3 x 3
// resolvent worked by hand.
#include <cmath>
#include <limits>
#include <vector>
#include "../tbk_bse.h"
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
    BseArgs args() const {
        BseArgs A;
        A.nint = (int)V.size(), A.ab = ab.data(), A.R = R.data(), A.V = V.data();
        return A;
    }
};

static int check_arguments() {
    const int32_t mesh[3] = {4, 4, 4};
    Inter I;
    I.add(0, 1, {0, 0}, 1.0);
    int64_t npts;
    const BseArgs A = I.args();
    EXPECT(bse_check("t", 2, 2, mesh, A, npts) == TBK_OK && npts == 16);
    EXPECT(bse_check("t", 0, 2, mesh, A, npts) == TBK_EINVAL);
    EXPECT(bse_check("t", 4, 2, mesh, A, npts) == TBK_EINVAL);
    EXPECT(bse_check("t", 2, 1, mesh, A, npts) == TBK_EINVAL);
    EXPECT(bse_check("t", 2, 2049, mesh, A, npts) == TBK_EINVAL);
#define BAD(stmt)                                                  \
    do {                                                           \
        BseArgs B = A;                                             \
        stmt;                                                      \
        EXPECT(bse_check("t", 2, 4, mesh, B, npts) == TBK_EINVAL); \
    } while (0)
#define GOOD(stmt)                                              \
    do {                                                        \
        BseArgs B = A;                                          \
        stmt;                                                   \
        EXPECT(bse_check("t", 2, 4, mesh, B, npts) == TBK_OK);  \
    } while (0)
    const int32_t two[2] = {0, 1}, twice[2] = {1, 1}, far[1] = {4};
    BAD(B.nint = 0);
    BAD(B.mu = std::numeric_limits<double>::quiet_NaN());
    BAD(B.nv = -1);
    BAD(B.nv = 17);
    GOOD(B.nv = 16);
    BAD(B.vsel = two; B.nv = 0);
    EXPECT(strstr(g_err, "no occupied band"));
    BAD(B.csel = two; B.nc = 0);
    EXPECT(strstr(g_err, "no empty band"));
    GOOD(B.vsel = two; B.nv = 2);
    BAD(B.vsel = twice; B.nv = 2);
    BAD(B.csel = far; B.nc = 1);
    {
        Inter J;
        J.add(0, 0, {0, 0}, 1.0);                                                  // a self-interaction
        EXPECT(bse_check("t", 2, 4, mesh, J.args(), npts) == TBK_EINVAL);
        Inter K;
        K.add(0, 1, {0, 0}, std::numeric_limits<double>::infinity());
        EXPECT(bse_check("t", 2, 4, mesh, K.args(), npts) == TBK_EINVAL);
    }
    // the selection
    int32_t bands[2 * kBseBandMax];
    int nv, nc;
    EXPECT(bse_select("t", 8, 3, A, bands, nv, nc) == TBK_OK && nv == 3 && nc == 5 && bands[0] == 0 && bands[3] == 3 && bands[7] == 7);
    EXPECT(bse_select("t", 8, 0, A, bands, nv, nc) == TBK_EINVAL && strstr(g_err, "no occupied band"));
    EXPECT(bse_select("t", 8, 8, A, bands, nv, nc) == TBK_EINVAL && strstr(g_err, "no empty band"));
    {
        BseArgs B = A;
        B.nv = 2, B.nc = 1;
        EXPECT(bse_select("t", 8, 3, B, bands, nv, nc) == TBK_OK && nv == 2 && nc == 1 && bands[0] == 1 && bands[1] == 2 && bands[2] == 3);
        B.nv = 4;
        EXPECT(bse_select("t", 8, 3, B, bands, nv, nc) == TBK_EINVAL);
        const int32_t v[2] = {2, 0}, c[2] = {7, 4}, cbad[1] = {2};
        B.nv = 2, B.vsel = v, B.nc = 2, B.csel = c;
        EXPECT(bse_select("t", 8, 3, B, bands, nv, nc) == TBK_OK && bands[0] == 0 && bands[1] == 2 && bands[2] == 4 && bands[3] == 7);
        B.csel = cbad, B.nc = 1;
        EXPECT(bse_select("t", 8, 3, B, bands, nv, nc) == TBK_EINVAL && strstr(g_err, "is occupied"));
        B = A;
        EXPECT(bse_select("t", 40, 20, B, bands, nv, nc) == TBK_EINVAL && strstr(g_err, "at most 16"));
    }
    // the caps
    EXPECT(bse_caps("t", 1, 2, 2048, 1, 1) == TBK_OK && bse_caps("t", 1, 2, 2049, 1, 1) == TBK_EINVAL);
    EXPECT(bse_caps("t", 1, 8, 8, 16, 16) == TBK_OK && bse_caps("t", 1, 8, 9, 16, 16) == TBK_EINVAL);
    EXPECT(bse_caps("t", 0, 2, (int64_t)1 << 24, 1, 1) == TBK_OK && bse_caps("t", 2, 2, ((int64_t)1 << 24) + 1, 1, 1) == TBK_EINVAL);
    EXPECT(bse_caps("t", 2, 2048, 1024, 16, 16) == TBK_OK && bse_caps("t", 2, 2048, 1025, 16, 16) == TBK_EINVAL && strstr(g_err, "2^26"));
    return 0;
}

static int check_problem() {
    BseProblem P;
    {   // a Hubbard pair on orbital 1 of a spinful two-orbital model: states 2 and 3
        Inter I;
        I.add(2, 3, {0, 0}, 4.0);
        EXPECT(bse_problem("t", 2, 4, I.args(), P) == TBK_OK);
        EXPECT(P.ne == 2 && P.ned == 2 && P.nst == 2 && P.np == 4);
        EXPECT(P.ea[0] == 2 && P.eb[0] == 3 && P.ea[1] == 3 && P.eb[1] == 2 && P.eV[0] == 4.0 && P.eV[1] == 4.0);
        EXPECT(P.st[0] == 2 && P.st[1] == 3);
        // h_2 = V rho_3 (entry 0), h_3 = V rho_2 (entry 1)
        EXPECT(P.hptr[0] == 0 && P.hptr[1] == 1 && P.hptr[2] == 2 && P.hent[0] == 0 && P.hslot[0] == 1 && P.hent[1] == 1 && P.hslot[1] == 0);
        EXPECT(P.pa[2] == 2 && P.pb[2] == 2 && P.pa[3] == 3 && P.pb[3] == 3);
        BseArgs A = I.args();
        A.direct = 0;
        EXPECT(bse_problem("t", 2, 4, A, P) == TBK_OK && P.ned == 0 && P.nst == 2 && P.np == 2 && P.pa[0] == 2 && P.pa[1] == 3);
        A.direct = 1, A.exchange = 0;
        EXPECT(bse_problem("t", 2, 4, A, P) == TBK_OK && P.ned == 2 && P.nst == 0 && P.np == 2 && P.hptr.size() == 1);
    }
    {   // a spinless bond (1, 0) and a second bond (1, 2): h_1 sums two entries in the order of E
        Inter I;
        I.add(1, 0, {0}, 0.5);
        I.add(1, 2, {0}, 0.25);
        EXPECT(bse_problem("t", 1, 3, I.args(), P) == TBK_OK);
        EXPECT(P.ne == 4 && P.nst == 3 && P.np == 7);
        // E = (1,0) (0,1) (1,2) (2,1); st = 0 1 2; h_0: entry 1 (b = 1); h_1: entries 0 (b = 0), 2 (b = 2); h_2: entry 3 (b = 1)
        EXPECT(P.hptr[1] == 1 && P.hptr[2] == 3 && P.hptr[3] == 4);
        EXPECT(P.hent[0] == 1 && P.hslot[0] == 1 && P.hent[1] == 0 && P.hslot[1] == 0 && P.hent[2] == 2 && P.hslot[2] == 2 && P.hent[3] == 3 &&
               P.hslot[3] == 1);
        EXPECT(P.eV[2] == 0.25 && P.eV[3] == 0.25);
        I.add(0, 1, {0}, 1.0);                                                     // the first bond again, from the other side
        EXPECT(bse_problem("t", 1, 3, I.args(), P) == TBK_EINVAL && strstr(g_err, "repeats"));
    }
    {   // a bond with R != 0 between a state and itself: both directions are entries of their own
        Inter I;
        I.add(0, 0, {1, -2}, -0.75);
        EXPECT(bse_problem("t", 2, 2, I.args(), P) == TBK_OK);
        EXPECT(P.ne == 2 && P.nst == 1 && P.np == 3);
        EXPECT(P.eR[0] == 1 && P.eR[1] == -2 && P.eR[2] == 0 && P.eR[3] == -1 && P.eR[4] == 2 && P.eR[5] == 0);
        EXPECT(P.hptr[1] == 2 && P.hent[0] == 0 && P.hent[1] == 1 && P.hslot[0] == 0 && P.hslot[1] == 0);   // h_0 = 2 V rho_0
        EXPECT(P.pR[6] == 0 && P.pR[7] == 0);
    }
    return 0;
}

static int check_partition() {
    for (int nv = 1; nv <= 16; ++nv)
        for (int nc = 1; nc <= 16; ++nc)
            for (int64_t npts : {(int64_t)1, (int64_t)7, (int64_t)144, (int64_t)4096, (int64_t)65536, ((int64_t)1 << 24) / (nv * nc)}) {
                const BsePart p = bse_partition(npts, nv, nc);
                EXPECT(p.P >= 1 && p.P * p.nvc <= 256 && (p.P + 1) * p.nvc > 256);
                EXPECT(p.ntiles * p.P >= npts && (p.ntiles - 1) * p.P < npts);
                EXPECT(p.G >= 1 && p.G <= kBseGroupsMax && p.G <= p.ntiles && p.GN >= 1 && p.GN <= kBseNormGroupsMax);
                EXPECT(check_groups("tiles", p.G, p.ntiles, p.ntiles, 1) == 0);
                // the lane map: every (q, v, c) of a tile once, lanes beyond the last point idle
                std::vector<int> seen((size_t)p.P * p.nvc, 0);
                for (int t = 0; t < 256; ++t) {
                    int q, r, v, c;
                    bse_lane(t, p.nvc, nc, q, r, v, c);
                    EXPECT(v >= 0 && v < nv && c >= 0 && c < nc && r == v * nc + c);
                    if (q < p.P) seen[(size_t)q * p.nvc + r]++;
                }
                for (int s : seen) EXPECT(s == 1);
            }
    // neither the block width nor the list enters: the plan's partition is that of (mesh, nv, nc)
    Inter I, J;
    I.add(0, 1, {0, 0}, 1.0);
    for (int e = 0; e < 40; ++e) J.add(e % 4, 4 + e % 3, {e, 1}, 0.1);
    BseProblem P, Q;
    EXPECT(bse_problem("t", 2, 8, I.args(), P) == TBK_OK && bse_problem("t", 2, 8, J.args(), Q) == TBK_OK);
    const BsePlan a = bse_plan(0, 8, 2, 900, 3, 2, 1, P, 0), b = bse_plan(0, 8, 2, 900, 3, 2, 16, Q, 0), c = bse_plan(2, 8, 2, 900, 3, 2, 4, Q, 77);
    EXPECT(a.P == b.P && a.G == b.G && a.GN == b.GN && a.ntiles == b.ntiles && a.P == c.P && a.G == c.G && a.GN == c.GN);
    return 0;
}

static int check_workspace() {
    Inter J;
    for (int e = 0; e < 9; ++e) J.add(e % 4, 4 + e % 3, {e, 1}, 0.1);
    BseProblem Q;
    EXPECT(bse_problem("t", 2, 8, J.args(), Q) == TBK_OK);
    struct Row {
        int mode, n, dk, nv, nc, nb, nsteps;
        int64_t npts;
    };
    for (const Row& r : {Row{0, 8, 2, 3, 2, 16, 0, 900}, Row{1, 8, 2, 4, 4, 16, 0, 64}, Row{2, 8, 2, 2, 2, 4, 300, 4096}, Row{2, 8, 3, 1, 1, 9, 5, 27},
                         Row{0, 8, 1, 1, 1, 1, 0, 1}}) {
        const BsePlan p = bse_plan(r.mode, r.n, r.dk, r.npts, r.nv, r.nc, r.nb, Q, r.nsteps);
        size_t buf[BsePlan::NBUF + 1][2];
        for (int i = 0; i < BsePlan::NBUF; ++i) buf[i][0] = p.off[i], buf[i][1] = p.off[i + 1] - p.off[i];
        buf[BsePlan::NBUF][0] = p.off_chunks, buf[BsePlan::NBUF][1] = p.cw.bytes();
        EXPECT(check_buffers("bse", buf, BsePlan::NBUF + 1, p.total) == 0);
        EXPECT(p.off[BsePlan::X + 1] - p.off[BsePlan::X] >= (size_t)r.nb * p.nt * sizeof(cd));
        EXPECT(p.off[BsePlan::PART + 1] - p.off[BsePlan::PART] >= (size_t)p.G * r.nb * Q.np * sizeof(cd));
        if (r.mode == 1) EXPECT(p.off[BsePlan::HMAT + 1] - p.off[BsePlan::HMAT] >= (size_t)p.nt * p.nt * sizeof(cd));
        if (r.mode != 1) EXPECT(p.off[BsePlan::HMAT + 1] == p.off[BsePlan::HMAT] && p.off[BsePlan::EVEC + 1] == p.off[BsePlan::EVEC]);
        EXPECT((r.mode == 2) == (p.off[BsePlan::Z + 1] > p.off[BsePlan::Z]));
    }
    return 0;
}

static int check_algebra() {
    // the runs
    EXPECT(bse_runs(1, -1, -1).size() == 1 && bse_runs(2, -1, -1).size() == 4 && bse_runs(3, -1, -1).size() == 9);
    EXPECT(bse_runs(3, 1, 1).size() == 1 && bse_runs(3, 2, 0).size() == 4);
    const std::vector<BseRun> r3 = bse_runs(3, -1, -1);
    EXPECT(r3[3].a == 0 && r3[3].b == 1 && r3[3].kind == 1 && r3[4].kind == 2 && r3[7].a == 1 && r3[7].b == 2 && r3[8].kind == 2);
    // the polarisation identity on a random non-Hermitian "resolvent" G (3 x 3) and vectors a, b
    const bse_c G[3][3] = {{{1.0, 0.5}, {0.2, -0.1}, {0.0, 0.3}}, {{-0.4, 0.1}, {2.0, 0.7}, {0.6, 0.0}}, {{0.1, 0.1}, {-0.3, 0.2}, {0.5, 0.9}}};
    const bse_c a[3] = {{1.0, 0.0}, {0.5, -1.0}, {0.0, 2.0}}, b[3] = {{-0.5, 0.3}, {1.5, 0.0}, {0.7, 0.7}};
    auto form = [&](const bse_c* x, const bse_c* y) {
        bse_c s = 0.0;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) s += std::conj(x[i]) * G[i][j] * y[j];
        return s;
    };
    bse_c s[3], t[3];
    for (int i = 0; i < 3; ++i) s[i] = a[i] + b[i], t[i] = a[i] + bse_c(0.0, 1.0) * b[i];
    bse_c gab, gba;
    bse_polarize(form(a, a), form(b, b), form(s, s), form(t, t), gab, gba);
    EXPECT(std::abs(gab - form(a, b)) < 1e-14 && std::abs(gba - form(b, a)) < 1e-14);
    // the tensor of dk = 2 from its four runs, and the one component from its own four: the same numbers
    const bse_c g4[4] = {form(a, a), form(b, b), form(s, s), form(t, t)};
    bse_c full[4], one[1];
    bse_tensor(2, -1, -1, g4, 0.25, full);
    bse_tensor(2, 0, 1, g4, 0.25, one);
    EXPECT(full[0] == 0.25 * form(a, a) && full[3] == 0.25 * form(b, b) && one[0] == full[1]);
    EXPECT(std::abs(full[1] - 0.25 * form(a, b)) < 1e-14 && std::abs(full[2] - 0.25 * form(b, a)) < 1e-14);
    // the continued fraction: T = tridiag(alpha = 1, 2, 3; beta = 0.5, 0.25), z = 0.5 + 0.1 i.  By hand, from the bottom:
    //   d2 = 3 - z = 2.5 - 0.1 i;  d1 = 2 - z - 0.0625 / d2;  d0 = 1 - z - 0.25 / d1;  [(T - z)^-1]_00 = 1 / d0
    const double al[3] = {1.0, 2.0, 3.0}, be[3] = {0.5, 0.25, 0.0};
    const bse_c z(0.5, 0.1);
    const bse_c d2 = bse_c(2.5, -0.1), d1 = bse_c(1.5, -0.1) - 0.0625 / d2, d0 = bse_c(0.5, -0.1) - 0.25 / d1;
    EXPECT(std::abs(bse_cfrac(3, al, be, 2.0, z) - 2.0 / d0) < 1e-15);
    // ... and against the cofactor form of the 3 x 3 inverse: [(T - z)^-1]_00 = (m11 m22 - b1^2) / det
    const bse_c m00 = 1.0 - z, m11 = 2.0 - z, m22 = 3.0 - z;
    const bse_c det = m00 * (m11 * m22 - 0.0625) - 0.25 * m22;
    EXPECT(std::abs(bse_cfrac(3, al, be, 1.0, z) - (m11 * m22 - 0.0625) / det) < 1e-14);
    EXPECT(std::abs(bse_cfrac(1, al, be, 3.0, z) - 3.0 / (1.0 - z)) < 1e-15);                // a run that ended after one step
    EXPECT(bse_cfrac(0, al, be, 3.0, z) == bse_c(0.0, 0.0));                                 // a zero start vector
    const double om[2] = {0.0, 1.0};
    EXPECT(bse_reconstruct_check("t", 2, -1, -1, 3, 2, om, 0.1) == TBK_OK);
    EXPECT(bse_reconstruct_check("t", 2, 0, 2, 3, 2, om, 0.1) == TBK_EINVAL);
    EXPECT(bse_reconstruct_check("t", 2, 0, 1, 0, 2, om, 0.1) == TBK_EINVAL);
    EXPECT(bse_reconstruct_check("t", 2, 0, 1, 3, 2, om, 0.0) == TBK_EINVAL);
    return 0;
}

int main() {
    if (check_arguments() || check_problem() || check_partition() || check_workspace() || check_algebra()) return 1;
    printf("bse_plan_check: ok\n");
    return 0;
}
