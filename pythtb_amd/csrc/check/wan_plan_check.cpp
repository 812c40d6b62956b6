// Stand-alone host check of tbk_wan.h and tbk_small_eig.h (no device call): built under AddressSanitizer + UBSan by
// `make -C pythtb_amd/csrc wan-check` and run as an ordinary program.  It covers every argument rule of tbk_wannier_mesh and the edge of
// every cap; the neighbour of a mesh point with its wrap vector on 1-, 2- and 3-D meshes; the partitions of the rotation and overlap
// kernels against their LDS budgets for (nsta, nb, nw) across 1, 2, 16 | 17, 32 | 33 and 2048; the workspace layout, filled and read
// back under the sanitizer; that no partition depends on max_iter; and the small Hermitian eigen-solver played by one lane: the
// reconstruction Q diag(lam) Q+ and the orthonormality of Q for diagonal, degenerate, random and rank-one matrices of 1 .. 16 rows.
#include <cmath>
#include <limits>
#include <vector>
#include "../tbk_wan.h"
#include "check_common.h"

#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) return printf("line %d: %s (%s)\n", __LINE__, #cond, g_err), 1;  \
    } while (0)

struct Case {
    std::vector<int32_t> bands, tptr, tstate, tR, bstep, R;
    std::vector<double> tamp, bw, bgram;
    WanArgs A;
    Case(int dk, int nb, int nw) {
        for (int b = 0; b < nb; ++b) bands.push_back(b);
        for (int w = 0; w <= nw; ++w) tptr.push_back(w);
        for (int w = 0; w < nw; ++w) {
            tstate.push_back(0);
            for (int d = 0; d < dk; ++d) tR.push_back(0);
            tamp.push_back(1.0), tamp.push_back(0.0);
        }
        for (int d = 0; d < dk; ++d) {
            for (int e = 0; e < dk; ++e) bstep.push_back(d == e ? 1 : 0);
            bw.push_back(1.0);
        }
        bgram.assign((size_t)dk * dk, 0.0);
        R.assign((size_t)dk, 0);
        sync(nb, nw, dk);
    }
    void sync(int nb, int nw, int dk) {
        A.nb = nb, A.nw = nw, A.bands = bands.data(), A.nterm = (int64_t)tstate.size(), A.term_ptr = tptr.data();
        A.term_state = tstate.data(), A.term_R = tR.data(), A.term_amp = tamp.data(), A.nbv = dk, A.bstep = bstep.data();
        A.bw = bw.data(), A.bgram = bgram.data(), A.max_iter = 0, A.check_every = 10, A.tol = 0.0, A.nR = 1, A.r_user = 0, A.R = R.data();
    }
};

static int check_arguments() {
    const int32_t mesh[3] = {4, 3, 5};
    int64_t npts;
    Case c(3, 2, 2);
    EXPECT(wan_check("t", 3, 8, mesh, c.A, npts) == TBK_OK && npts == 60);
    EXPECT(wan_check("t", 0, 8, mesh, c.A, npts) == TBK_EINVAL);                   // dim_k 1..3
    EXPECT(wan_check("t", 4, 8, mesh, c.A, npts) == TBK_EINVAL);
    EXPECT(wan_check("t", 3, 2049, mesh, c.A, npts) == TBK_EINVAL);                // nsta <= 2048
    {
        const int32_t small[3] = {4, 2, 5};
        EXPECT(wan_check("t", 3, 8, small, c.A, npts) == TBK_EINVAL);              // every N_a >= 3
    }
#define BAD(stmt)                                                        \
    do {                                                                 \
        Case d(3, 2, 2);                                                 \
        WanArgs& B = d.A;                                                \
        stmt;                                                            \
        EXPECT(wan_check("t", 3, 8, mesh, B, npts) == TBK_EINVAL);       \
    } while (0)
    BAD(B.nw = 0);
    BAD(B.nw = 3);                                                                 // nw > nb
    BAD(d.bands[1] = 0);                                                           // a repeated band
    BAD(d.bands[1] = 8);
    BAD(d.bands[0] = -1);
    BAD(d.tstate[0] = 8);                                                          // a trial state out of range
    BAD(d.tstate[1] = -1);
    BAD(d.tamp[0] = std::numeric_limits<double>::infinity());
    BAD(d.tR[0] = 1 << 30);
    BAD(d.tptr[1] = 0);                                                            // a function without terms
    BAD(d.tptr[2] = 1);
    BAD(B.nbv = 0);
    BAD(B.nbv = 7);
    BAD(d.bstep[0] = 2);
    BAD(d.bstep[0] = 0);                                                           // a zero b-vector
    BAD(d.bw[1] = 0.0);                                                            // the "too skewed" weight
    BAD(d.bw[1] = -0.25);
    BAD(d.bgram[0] = std::numeric_limits<double>::quiet_NaN());
    BAD(B.max_iter = -1);
    BAD(B.max_iter = kWanIterMax + 1);
    BAD(B.check_every = 0);
    BAD(B.tol = -1e-12);
    BAD(B.tol = std::numeric_limits<double>::quiet_NaN());
    BAD(B.nR = 0);
    BAD(B.nR = 61);                                                                // more than the torus holds
    BAD(d.R[2] = -(1 << 30));
#undef BAD
    {
        Case d(3, 2, 2);                                                           // a list of the caller's: up to 4096 whatever the mesh
        d.R.assign((size_t)3 * 4097, 0);
        d.A.R = d.R.data(), d.A.r_user = 1, d.A.nR = 4096;
        EXPECT(wan_check("t", 3, 8, mesh, d.A, npts) == TBK_OK);
        d.A.nR = 4097;
        EXPECT(wan_check("t", 3, 8, mesh, d.A, npts) == TBK_EINVAL);
    }
    {
        Case d(1, 32, 16);                                                         // nb <= 32, nw <= 16, nb <= nsta
        const int32_t m1[1] = {16};
        EXPECT(wan_check("t", 1, 32, m1, d.A, npts) == TBK_OK);
        EXPECT(wan_check("t", 1, 31, m1, d.A, npts) == TBK_EINVAL);
        Case e(1, 33, 16);
        EXPECT(wan_check("t", 1, 64, m1, e.A, npts) == TBK_EINVAL);
        Case f(1, 17, 17);
        EXPECT(wan_check("t", 1, 64, m1, f.A, npts) == TBK_EINVAL);
    }
    {
        Case d(2, 16, 16);                                                         // the resident cap: N_k nsta nw <= 2^26
        const int32_t ok[2] = {64, 32}, over[2] = {64, 33};
        EXPECT(wan_check("t", 2, 2048, ok, d.A, npts) == TBK_OK && npts * 2048 * 16 == kTdStateCap);
        EXPECT(wan_check("t", 2, 2048, over, d.A, npts) == TBK_EINVAL);
        d.A.want_fn = 1;                                                           // the functions' own cap: nR nsta nw <= 2^26
        std::vector<int32_t> R((size_t)2 * 2049, 0);
        d.A.R = R.data(), d.A.nR = 2048;
        EXPECT(wan_check("t", 2, 2048, ok, d.A, npts) == TBK_OK);
        d.A.nR = 2049;
        EXPECT(wan_check("t", 2, 2048, ok, d.A, npts) == TBK_EINVAL);
    }
    return 0;
}

static int check_neighbours() {
    int G[3];
    {
        const WanMesh M{{5, 1, 1}, 1};
        const int up[3] = {1, 0, 0}, dn[3] = {-1, 0, 0};
        EXPECT(wan_neighbour(M, 2, up, G) == 3 && G[0] == 0);
        EXPECT(wan_neighbour(M, 4, up, G) == 0 && G[0] == 1);
        EXPECT(wan_neighbour(M, 0, dn, G) == 4 && G[0] == -1);
    }
    {
        const WanMesh M{{4, 3, 5}, 3};                                             // row-major, the last axis fastest
        const int s[3] = {1, -1, 1};
        EXPECT(wan_neighbour(M, (1 * 3 + 1) * 5 + 2, s, G) == (2 * 3 + 0) * 5 + 3 && !G[0] && !G[1] && !G[2]);
        EXPECT(wan_neighbour(M, (3 * 3 + 0) * 5 + 4, s, G) == (0 * 3 + 2) * 5 + 0 && G[0] == 1 && G[1] == -1 && G[2] == 1);
        // a step and its mirror undo each other everywhere, and so do their wrap vectors
        const int sm[3] = {-1, 1, -1};
        for (int64_t k = 0; k < 60; ++k) {
            int H[3];
            const int64_t k2 = wan_neighbour(M, k, s, G);
            EXPECT(k2 >= 0 && k2 < 60 && k2 != k);
            EXPECT(wan_neighbour(M, k2, sm, H) == k && H[0] == -G[0] && H[1] == -G[1] && H[2] == -G[2]);
        }
    }
    return 0;
}

static int check_layout(const char* tag, const WanPlan& p) {
    size_t end = 256;
    for (int i = 0; i < WanPlan::NBUF; ++i) {
        if (p.off[i] % 256 || p.off[i] < end) return printf("%s: buffer %d at %zu (the previous one ends at %zu)\n", tag, i, p.off[i], end);
        end = p.off[i + 1];
    }
    if (end != p.total) return printf("%s: the total\n", tag);
    if (p.total > ((size_t)256 << 20)) return 0;
    unsigned char* base = (unsigned char*)aligned_alloc(256, al256(p.total));
    if (!base) return printf("%s: no host block\n", tag);
    int bad = 0;
    for (int i = 0; i < WanPlan::NBUF; ++i) memset(base + p.off[i], i + 1, p.off[i + 1] - p.off[i]);
    for (int i = 0; i < WanPlan::NBUF && !bad; ++i)
        for (size_t j = p.off[i]; j < p.off[i + 1]; j += 61)
            if (base[j] != (unsigned char)(i + 1)) {
                bad = printf("%s: buffer %d is overwritten\n", tag, i);
                break;
            }
    free(base);
    return bad;
}
static int check_plans() {
    const int ns[] = {1, 2, 16, 17, 32, 33, 2048}, nbs[] = {1, 2, 16, 17, 32}, nws[] = {1, 2, 3, 5, 6, 7, 8, 11, 16};
    const int32_t mesh[2] = {7, 9};
    for (int n : ns)
        for (int nb : nbs)
            for (int nw : nws) {
                if (nb > n || nw > nb) continue;
                const WanPlan p = wan_plan(n, 2, 63, mesh, nb, nw, 3, nw, 20, 63, 1);
                EXPECT(p.P >= 1 && p.P * nb * nw <= WAN_ROT_LDS && p.P <= 16);                  // the rotation's LDS block
                EXPECT(p.Q >= 1 && p.Q * nw * nw <= 256 && p.Q * 2 * nw <= WAN_OV_ROWS);        // the overlap's lanes and rows
                EXPECT(p.G >= 1 && p.G <= kWanGroupsMax && p.G <= 63 && p.nq == 3 * nw && p.nq <= 128);
                EXPECT(p.chunk >= 1 && p.chunk * p.nchunks >= 63 && p.chunk == kubo_chunk_len(n, 63));
                EXPECT(p.off[WanPlan::UT + 1] - p.off[WanPlan::UT] >= (size_t)63 * nw * n * 16);
                EXPECT(p.off[WanPlan::MOV + 1] - p.off[WanPlan::MOV] >= (size_t)63 * 3 * nw * nw * 16);
                EXPECT(p.off[WanPlan::TW + 1] - p.off[WanPlan::TW] >= (size_t)16 * 16);
                EXPECT(check_layout("plan", p) == 0);
                // no partition depends on max_iter, the terms, the lattice vectors or the functions
                const WanPlan q = wan_plan(n, 2, 63, mesh, nb, nw, 3, 5 * nw, 65536, 1, 0);
                EXPECT(q.P == p.P && q.Q == p.Q && q.G == p.G && q.chunk == p.chunk && q.nchunks == p.nchunks);
                EXPECT(q.off[WanPlan::FN + 1] == q.off[WanPlan::FN]);
            }
    EXPECT(wan_groups(1) == 1 && wan_groups(64) == 1 && wan_groups(65) == 2 && wan_groups((int64_t)1 << 30) == kWanGroupsMax);
    // the k-groups of a Fourier sum: their partial sums fit FPART, or there is one group and no partial sum
    for (int64_t np : {(int64_t)9, (int64_t)144, (int64_t)65536, (int64_t)1 << 26})
        for (int64_t tot : {(int64_t)1, (int64_t)9, (int64_t)144, (int64_t)2304, (int64_t)65536, (int64_t)65537, (int64_t)1 << 26}) {
            const int g = wan_fourier_groups(np, tot);
            EXPECT(g >= 1 && g <= wan_groups(np) && (g == 1 || g * tot <= kWanFourierLanes));
        }
    EXPECT(wan_fourier_groups(65536, 9) == 1024 && wan_fourier_groups(144, 144) == 3 && wan_fourier_groups(65536, 65536) == 1);
    EXPECT(wan_ov_items(1) == 8 && wan_ov_items(5) == 8 && wan_ov_items(6) == 6 && wan_ov_items(16) == 1);
    EXPECT(wan_rot_points(2, 1, 1) == 16 && wan_rot_points(2048, 32, 16) == 1 && wan_rot_points(33, 2, 2) == 7);
    return 0;
}

// ---------------------------------------------------------------- the eigen-solver, one lane
static double g_seed = 0.5;
static double rnd() {
    g_seed = fmod(g_seed * 997.0 + 0.123456789, 1.0);
    return 2.0 * g_seed - 1.0;
}
static int eig_case(const char* tag, int n, const std::vector<cd>& H) {
    cd A[SE_NMAX * SE_LD], Q[SE_NMAX * SE_LD];
    double norm = 0.0;
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) A[r * SE_LD + c] = H[r * n + c], norm = std::max(norm, sqrt(cabs2(H[r * n + c])));
    const int sweeps = small_eig_jacobi(A, Q, n, 0, 1);
    if (sweeps > SE_SWEEPS) return printf("%s n=%d: %d sweeps\n", tag, n, sweeps);
    double err = 0.0, orth = 0.0, off = 0.0;
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) {
            cd rec{0.0, 0.0}, qq{0.0, 0.0};
            for (int j = 0; j < n; ++j) {
                cfma(rec, cscale(Q[r * SE_LD + j], A[j * SE_LD + j].x), cconj(Q[c * SE_LD + j]));
                cfmac(qq, Q[j * SE_LD + r], Q[j * SE_LD + c]);
            }
            err = std::max(err, sqrt(cabs2(csub(rec, H[r * n + c]))));
            orth = std::max(orth, sqrt(cabs2(csub(qq, cd{r == c ? 1.0 : 0.0, 0.0}))));
            if (r != c) off = std::max(off, sqrt(cabs2(A[r * SE_LD + c])));
        }
    const double tol = 64.0 * 2.3e-16 * std::max(norm, 1e-300) * n;
    if (err > tol || orth > 64.0 * 2.3e-16 * n || off > tol)
        return printf("%s n=%d: reconstruction %.3e, orthonormality %.3e, off-diagonal %.3e (norm %.3e)\n", tag, n, err, orth, off, norm);
    return 0;
}
static int check_eigen() {
    for (int n = 1; n <= SE_NMAX; ++n) {
        std::vector<cd> H((size_t)n * n, cd{0.0, 0.0});
        EXPECT(eig_case("zero", n, H) == 0);
        for (int j = 0; j < n; ++j) H[j * n + j] = cd{(double)(j % 3) - 1.0, 0.0};       // diagonal, with repeated values
        EXPECT(eig_case("diagonal", n, H) == 0);
        for (int trial = 0; trial < 4; ++trial) {
            for (int r = 0; r < n; ++r)
                for (int c = r; c < n; ++c) {
                    H[r * n + c] = cd{rnd(), r == c ? 0.0 : rnd()};
                    H[c * n + r] = cconj(H[r * n + c]);
                }
            EXPECT(eig_case("random", n, H) == 0);
            for (auto& x : H) x = cscale(x, 1e-9);                                        // the size of a late descent step
            EXPECT(eig_case("small", n, H) == 0);
        }
        std::vector<cd> v((size_t)n);                                                     // rank one: n - 1 degenerate zeros
        for (int j = 0; j < n; ++j) v[j] = cd{rnd(), rnd()};
        for (int r = 0; r < n; ++r)
            for (int c = 0; c < n; ++c) H[r * n + c] = cmul(v[r], cconj(v[c]));
        EXPECT(eig_case("rank one", n, H) == 0);
    }
    return 0;
}

int main() {
    int bad = check_arguments();
    if (!bad) bad = check_neighbours();
    if (!bad) bad = check_plans();
    if (!bad) bad = check_eigen();
    printf(bad ? "wan_plan_check: FAILED\n" : "wan_plan_check: ok\n");
    return bad ? 1 : 0;
}
