// Stand-alone host check of tbk_wdis.h and tbk_small_eig32.h (no device call): built under AddressSanitizer + UBSan by
// `make -C pythtb_amd/csrc wdis-check` and run as an ordinary program.  It covers every argument rule of tbk_wannier_dis_mesh beyond
// tbk_wannier_mesh's and the edge of both residency caps; the static LDS of every kernel of tbk_wdis.hip against the budget of 64 KiB;
// the workspace layout behind section 34's for (nsta, nb, nw) across 1, 2, 16 | 17, 32 | 33 and 2048, filled and read back under the
// sanitizer; that no partition depends on dis_iter, dis_mixing or max_iter; the round-robin schedule (every pair once per sweep, the
// pairs of a round disjoint); and small_eig_jacobi32 played by one lane for n = 1 .. 32: zero, diagonal with repeated values, random,
// random scaled by 1e-9, rank one, and a projector with eigenvalues 0 and 1 only (the input of the start), each for its reconstruction
// Q diag(lam) Q+, the orthonormality of Q and its spectrum.
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>
#include "../tbk_wdis.h"
#include "check_common.h"

#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) return printf("line %d: %s (%s)\n", __LINE__, #cond, g_err), 1;  \
    } while (0)

static int check_arguments() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    WdisArgs D;
    EXPECT(wdis_check("t", 8, 60, 4, 3, D) == TBK_OK);
#define BAD(stmt)                                                \
    do {                                                         \
        WdisArgs B;                                              \
        stmt;                                                    \
        EXPECT(wdis_check("t", 8, 60, 4, 3, B) == TBK_EINVAL);   \
    } while (0)
#define GOOD(stmt)                                               \
    do {                                                         \
        WdisArgs B;                                              \
        stmt;                                                    \
        EXPECT(wdis_check("t", 8, 60, 4, 3, B) == TBK_OK);       \
    } while (0)
    BAD(B.have_window = 1; B.window[0] = 1.0; B.window[1] = 0.0);                    // an ordered pair
    BAD(B.have_window = 1; B.window[0] = -inf; B.window[1] = 0.0);                   // finite
    BAD(B.have_window = 1; B.window[0] = 0.0; B.window[1] = nan);
    BAD(B.have_frozen = 1; B.frozen[0] = 1.0; B.frozen[1] = 0.5);
    BAD(B.have_frozen = 1; B.frozen[0] = 0.0; B.frozen[1] = inf);
    BAD(B.have_frozen = 1; B.frozen[0] = nan; B.frozen[1] = 0.0);
    GOOD(B.window[0] = 1.0; B.window[1] = 0.0);                                      // (an absent window is not looked at)
    GOOD(B.have_window = 1; B.window[0] = 0.5; B.window[1] = 0.5);
    GOOD(B.have_frozen = 1; B.frozen[0] = -2.0; B.frozen[1] = 0.5);
    BAD(B.dis_iter = -1);
    BAD(B.dis_iter = kWanIterMax + 1);
    GOOD(B.dis_iter = 0);
    GOOD(B.dis_iter = kWanIterMax);
    BAD(B.dis_mixing = 0.0);
    BAD(B.dis_mixing = -0.5);
    BAD(B.dis_mixing = 1.0 + 1e-12);
    BAD(B.dis_mixing = nan);
    GOOD(B.dis_mixing = 1e-3);
    BAD(B.dis_tol = -1e-12);
    BAD(B.dis_tol = nan);
    BAD(B.dis_tol = inf);
    GOOD(B.dis_tol = 1e-9);
    BAD(B.check_every = 0);
#undef BAD
#undef GOOD
    // the candidate states: N_k nsta nb <= 2^26 (here 2^11 * 2^10 * 2^5), and one point more
    EXPECT(wdis_check("t", 1024, 2048, 32, 1, D) == TBK_OK && (int64_t)2048 * 1024 * 32 == kTdStateCap);
    EXPECT(wdis_check("t", 1024, 2049, 32, 1, D) == TBK_EINVAL && strstr(g_err, "candidate states"));
    // the overlaps: N_k nbv nb^2 <= 2^26 where the states fit (nsta = 32 = nb, nbv = 4: 2^14 * 4 * 2^10)
    EXPECT(wdis_check("t", 32, 16384, 32, 4, D) == TBK_OK && (int64_t)16384 * 4 * 1024 == kWdisOverlapCap);
    EXPECT(wdis_check("t", 32, 16385, 32, 4, D) == TBK_EINVAL && strstr(g_err, "overlaps"));
    EXPECT(wdis_check("t", 32, 16384, 32, 5, D) == TBK_EINVAL && strstr(g_err, "overlaps"));
    return 0;
}

static int check_layout(const char* tag, const WdisPlan& p) {
    size_t end = p.wan.total;
    for (int i = 0; i < WdisPlan::NBUF; ++i) {
        if (p.off[i] % 256 || p.off[i] < end) return printf("%s: buffer %d at %zu (the previous one ends at %zu)\n", tag, i, p.off[i], end);
        end = p.off[i + 1];
    }
    if (end != p.total) return printf("%s: the total\n", tag);
    if (p.total > ((size_t)256 << 20)) return 0;
    unsigned char* base = (unsigned char*)aligned_alloc(256, al256(p.total));
    if (!base) return printf("%s: no host block\n", tag);
    int bad = 0;
    memset(base, 0xff, p.wan.total);                                                  // section 34's part
    for (int i = 0; i < WdisPlan::NBUF; ++i) memset(base + p.off[i], i + 1, p.off[i + 1] - p.off[i]);
    for (size_t j = 0; j < p.wan.total && !bad; j += 61)
        if (base[j] != 0xff) bad = printf("%s: section 34's workspace is overwritten\n", tag);
    for (int i = 0; i < WdisPlan::NBUF && !bad; ++i)
        for (size_t j = p.off[i]; j < p.off[i + 1]; j += 61)
            if (base[j] != (unsigned char)(i + 1)) {
                bad = printf("%s: buffer %d is overwritten\n", tag, i);
                break;
            }
    free(base);
    return bad;
}
static int check_plans() {
    // the static LDS of the kernels, as they declare it
    EXPECT(wdis_lds_overlap() < kWdisLdsBudget && wdis_lds_select() < kWdisLdsBudget && wdis_lds_gauge() < kWdisLdsBudget &&
           wdis_lds_reduce() < kWdisLdsBudget);
    EXPECT(WDIS_OV_EPL * 256 >= WAN_NB_MAX * WAN_NB_MAX && WDIS_OV_ROWS >= 2 * WAN_NB_MAX && (WDIS_OV_TJ + 1) % 2 == 1);
    EXPECT(WDIS_LDS_C >= WDIS_LDS_A);                                                 // the compacted matrix fits the two panels
    EXPECT(3 * SE_NMAX * SE_LD <= WDIS_LDS_A);                                        // S, Q and X of the start fit the block of Z's Q
    EXPECT(SE32_LD % 2 == 1 && SE32_LD > SE32_NMAX && SE32_W >= 5 * ((SE32_NMAX + 1) / 2) && SE32_NMAX == WAN_NB_MAX);
    const int ns[] = {1, 2, 16, 17, 32, 33, 2048}, nbs[] = {1, 2, 16, 17, 32}, nws[] = {1, 2, 3, 5, 8, 11, 16};
    const int32_t mesh[2] = {7, 9};
    for (int n : ns)
        for (int nb : nbs)
            for (int nw : nws) {
                if (nb > n || nw > nb) continue;
                const WdisPlan p = wdis_plan(n, 2, 63, mesh, nb, nw, 3, nw, 20, 63, 1, 40, 0.5);
                EXPECT(p.G == p.wan.G && p.nq == 3 * nw && p.nq <= 128 && p.keep_zin == 1);
                EXPECT(p.off[0] >= p.wan.total);
                EXPECT(p.off[WdisPlan::VB + 1] - p.off[WdisPlan::VB] >= (size_t)63 * nb * n * 16);
                EXPECT(p.off[WdisPlan::M0 + 1] - p.off[WdisPlan::M0] >= (size_t)63 * 3 * nb * nb * 16);
                EXPECT(p.off[WdisPlan::UD1 + 1] - p.off[WdisPlan::UD1] >= (size_t)63 * nb * nw * 16);
                EXPECT(p.off[WdisPlan::ZIN + 1] - p.off[WdisPlan::ZIN] >= (size_t)63 * nb * nb * 16);
                EXPECT(p.off[WdisPlan::OPART + 1] - p.off[WdisPlan::OPART] >= (size_t)p.G * p.nq * 8);
                EXPECT(p.off[WdisPlan::DISH + 1] - p.off[WdisPlan::DISH] >= (size_t)41 * 8);
                EXPECT(check_layout("plan", p) == 0);
                // no partition depends on the iteration counts or the mixing; Z_in is kept only below 1
                const WdisPlan q = wdis_plan(n, 2, 63, mesh, nb, nw, 3, 5 * nw, 65536, 1, 0, 65536, 1.0);
                EXPECT(q.G == p.G && q.nq == p.nq && q.wan.P == p.wan.P && q.wan.Q == p.wan.Q && q.wan.chunk == p.wan.chunk);
                EXPECT(q.keep_zin == 0 && q.off[WdisPlan::ZIN + 1] == q.off[WdisPlan::ZIN]);
                EXPECT(check_layout("plan, no mixing", q) == 0);
            }
    return 0;
}

// ---------------------------------------------------------------- the round-robin schedule
static int check_schedule() {
    for (int n = 2; n <= SE32_NMAX; ++n) {
        const int m = (n + 1) & ~1;
        std::vector<int> seen((size_t)m * m, 0);
        for (int r = 0; r < m - 1; ++r) {
            std::vector<int> used((size_t)m, 0);
            for (int i = 0; i < m / 2; ++i) {
                int p, q;
                se32_pair(m, r, i, p, q);
                EXPECT(p >= 0 && p < q && q < m);
                EXPECT(!used[(size_t)p] && !used[(size_t)q]);                          // the pairs of a round are disjoint
                used[(size_t)p] = used[(size_t)q] = 1;
                ++seen[(size_t)p * m + q];
            }
        }
        for (int p = 0; p < m; ++p)
            for (int q = p + 1; q < m; ++q) EXPECT(seen[(size_t)p * m + q] == 1);      // every pair once per sweep
    }
    return 0;
}

// ---------------------------------------------------------------- the eigen-solver, one lane
static double g_seed = 0.5;
static double rnd() {
    g_seed = fmod(g_seed * 997.0 + 0.123456789, 1.0);
    return 2.0 * g_seed - 1.0;
}
// spectrum: the expected eigenvalues (any order), or empty
static int eig_case(const char* tag, int n, const std::vector<cd>& H, std::vector<double> spectrum = {}) {
    std::vector<cd> A((size_t)SE32_NMAX * SE32_LD), Q((size_t)SE32_NMAX * SE32_LD);
    double W[SE32_W];
    double norm = 0.0;
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) A[r * SE32_LD + c] = H[r * n + c], norm = std::max(norm, sqrt(cabs2(H[r * n + c])));
    const int sweeps = small_eig_jacobi32(A.data(), Q.data(), W, n, 0, 1);
    if (sweeps > SE32_SWEEPS) return printf("%s n=%d: %d sweeps\n", tag, n, sweeps);
    double err = 0.0, orth = 0.0, off = 0.0;
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) {
            cd rec{0.0, 0.0}, qq{0.0, 0.0};
            for (int j = 0; j < n; ++j) {
                cfma(rec, cscale(Q[r * SE32_LD + j], A[j * SE32_LD + j].x), cconj(Q[c * SE32_LD + j]));
                cfmac(qq, Q[j * SE32_LD + r], Q[j * SE32_LD + c]);
            }
            err = std::max(err, sqrt(cabs2(csub(rec, H[r * n + c]))));
            orth = std::max(orth, sqrt(cabs2(csub(qq, cd{r == c ? 1.0 : 0.0, 0.0}))));
            if (r != c) off = std::max(off, sqrt(cabs2(A[r * SE32_LD + c])));
        }
    const double tol = 64.0 * 2.3e-16 * std::max(norm, 1e-300) * n;
    if (err > tol || orth > 64.0 * 2.3e-16 * n || off > tol)
        return printf("%s n=%d: reconstruction %.3e, orthonormality %.3e, off-diagonal %.3e (norm %.3e, %d sweeps)\n", tag, n, err, orth, off, norm,
                      sweeps);
    if (!spectrum.empty()) {
        std::vector<double> lam((size_t)n);
        for (int j = 0; j < n; ++j) lam[(size_t)j] = A[j * SE32_LD + j].x;
        std::sort(lam.begin(), lam.end());
        std::sort(spectrum.begin(), spectrum.end());
        double scale = 1e-300;
        for (double x : spectrum) scale = std::max(scale, fabs(x));
        for (int j = 0; j < n; ++j)
            if (fabs(lam[(size_t)j] - spectrum[(size_t)j]) > 64.0 * 2.3e-16 * scale * n)
                return printf("%s n=%d: eigenvalue %d is %.17g, expected %.17g\n", tag, n, j, lam[(size_t)j], spectrum[(size_t)j]);
    }
    return 0;
}
static int check_eigen() {
    for (int n = 1; n <= SE32_NMAX; ++n) {
        std::vector<cd> H((size_t)n * n, cd{0.0, 0.0});
        EXPECT(eig_case("zero", n, H, std::vector<double>((size_t)n, 0.0)) == 0);
        std::vector<double> diag((size_t)n);
        for (int j = 0; j < n; ++j) H[j * n + j] = cd{diag[(size_t)j] = (double)(j % 3) - 1.0, 0.0};   // diagonal, with repeated values
        EXPECT(eig_case("diagonal", n, H, diag) == 0);
        for (int trial = 0; trial < 3; ++trial) {
            for (int r = 0; r < n; ++r)
                for (int c = r; c < n; ++c) {
                    H[r * n + c] = cd{rnd(), r == c ? 0.0 : rnd()};
                    H[c * n + r] = cconj(H[r * n + c]);
                }
            EXPECT(eig_case("random", n, H) == 0);
            for (auto& x : H) x = cscale(x, 1e-9);
            EXPECT(eig_case("small", n, H) == 0);
        }
        std::vector<cd> v((size_t)n);                                                     // rank one: n - 1 degenerate zeros
        double vv = 0.0;
        for (int j = 0; j < n; ++j) v[(size_t)j] = cd{rnd(), rnd()}, vv += cabs2(v[(size_t)j]);
        for (int r = 0; r < n; ++r)
            for (int c = 0; c < n; ++c) H[r * n + c] = cmul(v[(size_t)r], cconj(v[(size_t)c]));
        std::vector<double> one((size_t)n, 0.0);
        one[0] = vv;
        EXPECT(eig_case("rank one", n, H, one) == 0);
        // a projector of rank nw = ceil(n / 2): orthonormal columns by Gram-Schmidt, P = U U+ (the input of the start)
        const int nw = (n + 1) / 2;
        std::vector<cd> U((size_t)n * nw);
        for (int w = 0; w < nw; ++w) {
            for (int j = 0; j < n; ++j) U[(size_t)j * nw + w] = cd{rnd(), rnd()};
            for (int pass = 0; pass < 2; ++pass)
                for (int x = 0; x < w; ++x) {
                    cd d{0.0, 0.0};
                    for (int j = 0; j < n; ++j) cfmac(d, U[(size_t)j * nw + x], U[(size_t)j * nw + w]);   // conj(u_x) u_w
                    for (int j = 0; j < n; ++j) U[(size_t)j * nw + w] = csub(U[(size_t)j * nw + w], cmul(d, U[(size_t)j * nw + x]));
                }
            double nn = 0.0;
            for (int j = 0; j < n; ++j) nn += cabs2(U[(size_t)j * nw + w]);
            for (int j = 0; j < n; ++j) U[(size_t)j * nw + w] = cscale(U[(size_t)j * nw + w], 1.0 / sqrt(nn));
        }
        for (int r = 0; r < n; ++r)
            for (int c = 0; c < n; ++c) {
                cd a{0.0, 0.0};
                for (int w = 0; w < nw; ++w) cfmac(a, U[(size_t)c * nw + w], U[(size_t)r * nw + w]);   // u_r conj(u_c)
                H[r * n + c] = a;
            }
        for (int r = 0; r < n; ++r) {
            H[r * n + r].y = 0.0;
            for (int c = r + 1; c < n; ++c) H[c * n + r] = cconj(H[r * n + c]);
        }
        std::vector<double> pr((size_t)n, 0.0);
        for (int w = 0; w < nw; ++w) pr[(size_t)w] = 1.0;
        EXPECT(eig_case("projector", n, H, pr) == 0);
    }
    return 0;
}

int main() {
    int bad = check_arguments();
    if (!bad) bad = check_plans();
    if (!bad) bad = check_schedule();
    if (!bad) bad = check_eigen();
    printf(bad ? "wdis_plan_check: FAILED\n" : "wdis_plan_check: ok\n");
    return bad ? 1 : 0;
}
