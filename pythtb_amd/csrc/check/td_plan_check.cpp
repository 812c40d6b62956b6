// Stand-alone host check of tbk_td.h (no device call): built under AddressSanitizer + UBSan by `make -C pythtb_amd/csrc td-check` and run
// as an ordinary program.  Over a table of (n, dim_k, points, nprop, nt, mesh) it checks the plan of the propagation calls -- the chunk,
// the points per workgroup and the row length of the LDS step, the tiles of the wide step and the k-groups against values worked out by
// hand, the LDS budgets, the grid limits, that the groups cover every point of a chunk once and that nothing but the sizes of the
// measured rows depends on nt -- replays the lane maps of k_td_step_lds on the host for every n up to 32 (every LDS index inside its
// array, every element of the carried states owned by exactly one lane slot, the 16 lanes of a read group on 16 different banks) and the
// layout of the scratch block (every buffer at a multiple of 256, in order, none overlapping, filled and read back under the
// sanitizer).  Then the argument checks: every rule and the edges of the caps, one bad value at a time.
#include <cmath>
#include <limits>
#include <vector>
#include "../tbk_td.h"
#include "check_common.h"

struct Case {
    int n, dk;
    int64_t npts;
    int nprop, nt, mesh;
    // expected: points per chunk, points per workgroup and row length (LDS step), tiles per nsta and nprop (wide step), k-groups
    int64_t chunk;
    int P, LD, T, TM, G;
};
static const Case kCases[] = {
    {1, 2, 36, 1, 12, 1, 36, 64, 1, 1, 1, 5},
    {2, 2, 30, 1, 12, 1, 30, 64, 3, 1, 1, 4},                         // Haldane 6 x 5, the lower band
    {2, 2, 65536, 1, 1600, 1, 65536, 64, 3, 1, 1, 512},               // Haldane 256 x 256
    {3, 1, 7, 3, 12, 1, 7, 64, 3, 1, 1, 1},
    {4, 2, 16, 4, 12, 1, 16, 52, 5, 1, 1, 2},                         // 1056 / (4 x 5) = 52: the eigenvectors' budget binds
    {5, 3, 27, 2, 3, 1, 27, 40, 5, 1, 1, 4},                          // 1024 / 25 = 40: the coefficients' budget binds
    {8, 3, 32768, 4, 64, 1, 32768, 14, 9, 1, 1, 512},                 // 8-state silicon 32^3
    {16, 2, 9, 8, 12, 1, 9, 3, 17, 1, 1, 2},
    {18, 2, 9, 18, 12, 1, 9, 3, 19, 2, 2, 2},
    {32, 2, 4096, 16, 5, 1, 2048, 1, 33, 2, 1, 256},                  // a 32-state supercell on 64 x 64: two chunks
    {33, 1, 5, 33, 12, 1, 5, 0, 33, 3, 3, 1},                         // the first size of the tiled step
    {40, 2, 22500, 20, 3, 1, 1310, 0, 41, 3, 2, 164},                 // 150 x 150: 18 chunks
    {2048, 2, 4, 2048, 1, 1, 1, 0, 2049, 128, 128, 1},                // the largest model: a point per chunk
    {2, 2, 5, 2, 32, 0, 5, 64, 3, 1, 1, 0},                           // the list call: no weights, no measurement
    {18, 2, 1, 18, 65536, 0, 1, 3, 19, 2, 2, 0},
};

static int check_case(const Case& c) {
    char tag[160];
    snprintf(tag, sizeof tag, "td n=%d dk=%d npts=%lld nprop=%d nt=%d mesh=%d", c.n, c.dk, (long long)c.npts, c.nprop, c.nt, c.mesh);
    const TdPlan p = td_plan(c.n, c.dk, c.npts, c.nprop, c.nt, c.mesh != 0);
    if (p.chunk != c.chunk || p.P != c.P || p.LD != c.LD || p.T != c.T || p.TM != c.TM || p.G != c.G)
        return printf("%s: chunk %lld P %d LD %d T %d TM %d G %d\n", tag, (long long)p.chunk, p.P, p.LD, p.T, p.TM, p.G);
    if (p.lds != (c.n <= 32) || p.nr != (c.mesh ? 1 + c.dk : 0) || p.nr > TD_NR) return printf("%s: the form\n", tag);
    if (p.chunk < 1 || p.chunk > c.npts || p.nchunks != (c.npts + p.chunk - 1) / p.chunk) return printf("%s: the chunks\n", tag);
    if ((size_t)p.chunk * c.n * c.n * sizeof(cd) > std::max(kKuboChunkBytes, (size_t)c.n * c.n * sizeof(cd)))
        return printf("%s: the chunk holds more than kKuboChunkBytes of eigenvectors\n", tag);
    if (p.psi_cd != c.npts * c.nprop * c.n) return printf("%s: the carried states\n", tag);
    // the grids: workgroups of the LDS step, (points, tiles) of the wide step, the k-groups
    if (p.lds && (p.chunk + p.P - 1) / p.P > 2147483647) return printf("%s: the grid of the LDS step\n", tag);
    if (!p.lds && (p.chunk > 2147483647 || (int64_t)p.T * p.TM > 65535 || p.T * 16 < c.n || p.TM * 16 < c.nprop || (p.T - 1) * 16 >= c.n ||
                   (p.TM - 1) * 16 >= c.nprop))
        return printf("%s: the tiles\n", tag);
    if (c.mesh) {
        if (p.G < 1 || p.G > kTdGroupsMax) return printf("%s: G=%d\n", tag, p.G);
        if (check_groups(tag, p.G, c.npts, p.chunk, p.nchunks)) return 1;
    }
    // the partition does not depend on the number of time steps
    for (int nt : {1, 7, kTdStepsMax}) {
        const TdPlan q = td_plan(c.n, c.dk, c.npts, c.nprop, nt, c.mesh != 0);
        if (q.chunk != p.chunk || q.P != p.P || q.LD != p.LD || q.T != p.T || q.TM != p.TM || q.G != p.G || q.off_psi != p.off_psi)
            return printf("%s: the partition depends on nt\n", tag);
    }
    const size_t D = sizeof(double), cb = p.off_chunks;
    const bool mesh = c.mesh != 0;
    const size_t buf[][2] = {
        {p.off_k, mesh ? 0 : (size_t)c.npts * c.dk * D},
        {p.off_sel, (size_t)c.nprop * sizeof(int32_t)},
        {p.off_psi, (size_t)p.psi_cd * sizeof(cd)},
        {p.off_fw, mesh ? (size_t)c.nprop * c.npts * D : 0},
        {p.off_kpop, mesh ? (size_t)c.n * c.npts * D : 0},
        {p.off_pop, mesh ? (size_t)c.n * D : 0},
        {p.off_obs, mesh ? ((size_t)c.nt + 1) * p.nr * D : 0},
        {p.off_part, mesh ? (size_t)p.G * p.nr * D : 0},
        {cb + p.cw.off[0], (size_t)p.chunk * c.dk * D},
        {cb + p.cw.off[1], (size_t)p.chunk * c.n * D},
        {cb + p.cw.off[2], (size_t)p.chunk * c.n * c.n * sizeof(cd)},
        {cb + p.cw.off[3], mesh ? (size_t)p.chunk * c.dk * D : 0},
        {cb + p.cw.off[4], p.lds ? 0 : (size_t)p.chunk * c.nprop * c.n * sizeof(cd)},
    };
    return check_buffers(tag, buf, (int)(sizeof buf / sizeof buf[0]), p.total);
}

// ---------------------------------------------------------------- the lane maps of k_td_step_lds, every n up to 32
static int check_lds_maps() {
    for (int n = 1; n <= 32; ++n)
        for (int nprop : {1, (n + 1) / 2, n}) {
            const int P = td_lds_points(n), LD = td_lds_row(n), nn = n * n, pn = nprop * n;
            char tag[64];
            snprintf(tag, sizeof tag, "lds n=%d nprop=%d", n, nprop);
            if (P < 1 || P > 64 || LD < n || LD > n + 1 || !(LD & 1)) return printf("%s: P=%d LD=%d\n", tag, P, LD);
            if (P * n * LD > TD_LDS_U || P * pn > TD_LDS_C || P * n > TD_LDS_PN || P * pn > 256 * TD_ES)
                return printf("%s: %d points do not fit the LDS\n", tag, P);
            const size_t lds = (size_t)(TD_LDS_U + TD_LDS_C + TD_LDS_PN) * sizeof(cd);
            if (lds > 40960) return printf("%s: %zu bytes of LDS\n", tag, lds);
            // the load of U: every (p, b, i) to its own place
            std::vector<int> uw((size_t)TD_LDS_U, 0), own((size_t)TD_LDS_C, 0);
            for (int e = 0; e < P * nn; ++e) {
                const int p = e / nn, r = e - p * nn, b = r / n, i = r - b * n;
                const int at = (p * n + b) * LD + i;
                if (at < 0 || at >= TD_LDS_U) return printf("%s: U index %d\n", tag, at);
                if (uw[(size_t)at]++) return printf("%s: U index %d written twice\n", tag, at);
            }
            for (int t = 0; t < 256; ++t)
                for (int s = 0; s < TD_ES; ++s) {
                    const int e = t + 256 * s;
                    if (e >= P * pn) continue;
                    const int p = e / pn, r = e - p * pn, m = r / n, x = r - m * n;   // x: b in the first pass, i in the second
                    if (p >= P || m >= nprop) return printf("%s: lane %d slot %d maps outside the workgroup\n", tag, t, s);
                    ++own[(size_t)e];
                    // first pass: rows of U and of S; second: a column of U
                    if ((p * n + x) * LD + n - 1 >= TD_LDS_U || (p * nprop + m) * n + n - 1 >= TD_LDS_C)
                        return printf("%s: lane %d reads beyond the LDS (first pass)\n", tag, t);
                    if (p * n * LD + x + (n - 1) * LD >= TD_LDS_U) return printf("%s: lane %d reads beyond the LDS (second pass)\n", tag, t);
                }
            for (int e = 0; e < P * pn; ++e)
                if (own[(size_t)e] != 1) return printf("%s: element %d is owned %d times\n", tag, e, own[(size_t)e]);
            // the first pass: 16 consecutive lanes on 16 rows b of one point read U at the same i -- 16-byte slots on different banks
            if (n >= 16)
                for (int b0 = 0; b0 + 16 <= n; ++b0) {
                    unsigned seen = 0;
                    for (int l = 0; l < 16; ++l) {
                        const int bank = (((b0 + l) * LD) * 4) % 64 / 4;            // the 16-byte slot of 16 in the 256-byte bank row
                        if (seen & (1u << bank)) return printf("%s: rows %d.. share a bank\n", tag, b0);
                        seen |= 1u << bank;
                    }
                }
        }
    return 0;
}

// ---------------------------------------------------------------- the argument checks
static int check_args() {
    const char* fn = "td_plan_check";
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    int bad = 0;
    auto ok = [&](int rc, const char* what) {
        if (rc != TBK_OK) bad |= printf("refused: %s\n", what);
    };
    auto no = [&](int rc, const char* what) {
        if (rc != TBK_EINVAL) bad |= printf("accepted: %s\n", what);
    };
    const int32_t mesh[3] = {4, 5, 2}, occ[2] = {1, 0};
    const double shift[8] = {0.0, 0.1, 0.05, -0.2, 1.5, 0.0, -0.3, 0.25};   // nt = 3 in two dimensions
    int64_t npts = 0;
    int nprop = 0;
    ok(td_mesh_check(fn, 2, 4, mesh, 3, shift, 0.1, 2, occ, 0.0, 0.0, npts, nprop), "a band set");
    if (npts != 20 || nprop != 2) bad |= printf("a band set: npts %lld nprop %d\n", (long long)npts, nprop);
    ok(td_mesh_check(fn, 2, 4, mesh, 3, shift, 0.1, 0, nullptr, 0.3, 0.05, npts, nprop), "Fermi weights");
    if (nprop != 4) bad |= printf("Fermi weights: nprop %d\n", nprop);
    ok(td_mesh_check(fn, 1, 4, mesh, 7, shift, 0.1, 0, nullptr, 0.3, 0.0, npts, nprop), "one dimension, kT = 0");
    no(td_mesh_check(fn, 0, 4, mesh, 3, shift, 0.1, 2, occ, 0.0, 0.0, npts, nprop), "dim_k = 0");
    no(td_mesh_check(fn, 4, 4, mesh, 1, shift, 0.1, 2, occ, 0.0, 0.0, npts, nprop), "dim_k = 4");
    no(td_mesh_check(fn, 2, 0, mesh, 3, shift, 0.1, 0, nullptr, 0.0, 0.0, npts, nprop), "no state");
    no(td_mesh_check(fn, 2, 2049, mesh, 3, shift, 0.1, 0, nullptr, 0.0, 0.0, npts, nprop), "2049 states");
    no(td_mesh_check(fn, 2, 4, mesh, 0, shift, 0.1, 2, occ, 0.0, 0.0, npts, nprop), "nt = 0");
    no(td_mesh_check(fn, 2, 4, mesh, 65537, shift, 0.1, 2, occ, 0.0, 0.0, npts, nprop), "65537 steps");
    for (double dt : {0.0, -0.1, nan, inf}) no(td_mesh_check(fn, 2, 4, mesh, 3, shift, dt, 2, occ, 0.0, 0.0, npts, nprop), "a bad dt");
    no(td_mesh_check(fn, 2, 4, mesh, 3, nullptr, 0.1, 2, occ, 0.0, 0.0, npts, nprop), "no shift");
    for (double x : {nan, inf}) {
        double sb[8];
        memcpy(sb, shift, sizeof sb);
        sb[7] = x;
        no(td_mesh_check(fn, 2, 4, mesh, 3, sb, 0.1, 2, occ, 0.0, 0.0, npts, nprop), "a shift that is not finite");
    }
    no(td_mesh_check(fn, 2, 4, nullptr, 3, shift, 0.1, 2, occ, 0.0, 0.0, npts, nprop), "no mesh");
    {
        const int32_t zero[2] = {4, 0};
        no(td_mesh_check(fn, 2, 4, zero, 3, shift, 0.1, 2, occ, 0.0, 0.0, npts, nprop), "a mesh axis of 0");
        const int32_t huge[2] = {65536, 32768};
        no(td_mesh_check(fn, 2, 1, huge, 3, shift, 0.1, 0, nullptr, 0.0, 0.0, npts, nprop), "2^31 points");
    }
    {
        const int32_t twice[2] = {1, 1}, out[2] = {0, 4}, neg[2] = {-1, 0};
        no(td_mesh_check(fn, 2, 4, mesh, 3, shift, 0.1, 2, twice, 0.0, 0.0, npts, nprop), "a band twice");
        no(td_mesh_check(fn, 2, 4, mesh, 3, shift, 0.1, 2, out, 0.0, 0.0, npts, nprop), "a band beyond the last");
        no(td_mesh_check(fn, 2, 4, mesh, 3, shift, 0.1, 2, neg, 0.0, 0.0, npts, nprop), "a negative band");
        no(td_mesh_check(fn, 2, 4, mesh, 3, shift, 0.1, 0, occ, 0.0, 0.0, npts, nprop), "occ without a band");
        no(td_mesh_check(fn, 2, 4, mesh, 3, shift, 0.1, 5, occ, 0.0, 0.0, npts, nprop), "more bands than states");
        no(td_mesh_check(fn, 2, 4, mesh, 3, shift, 0.1, 2, nullptr, 0.0, 0.0, npts, nprop), "nocc without occ");
    }
    for (double kT : {-1e-3, nan, inf}) no(td_mesh_check(fn, 2, 4, mesh, 3, shift, 0.1, 0, nullptr, 0.0, kT, npts, nprop), "a bad kT");
    for (double mu : {nan, inf}) no(td_mesh_check(fn, 2, 4, mesh, 3, shift, 0.1, 0, nullptr, mu, 0.0, npts, nprop), "a bad Fermi level");
    {   // the cap on the carried states: 2^26 c128
        const int32_t at[2] = {4096, 4096}, over[2] = {4096, 4097};
        const int32_t one[1] = {0};
        ok(td_mesh_check(fn, 2, 2, at, 3, shift, 0.1, 0, nullptr, 0.0, 0.0, npts, nprop), "2^24 points x 2 x 2 at the cap");
        no(td_mesh_check(fn, 2, 2, over, 3, shift, 0.1, 0, nullptr, 0.0, 0.0, npts, nprop), "over the cap");
        ok(td_mesh_check(fn, 2, 2, over, 3, shift, 0.1, 1, one, 0.0, 0.0, npts, nprop), "the same mesh with one band");
    }
    // the list call
    const double k[6] = {0.1, 0.2, -1.3, 0.4, 2.5, 0.0};
    ok(td_list_check(fn, 2, 4, 3, k, 3, shift, 0.1), "three points");
    no(td_list_check(fn, 0, 4, 3, k, 3, shift, 0.1), "the list: dim_k = 0");
    no(td_list_check(fn, 2, 4, 0, k, 3, shift, 0.1), "no k-point");
    no(td_list_check(fn, 2, 4, 3, nullptr, 3, shift, 0.1), "no k list");
    no(td_list_check(fn, 2, 4, 3, k, 0, shift, 0.1), "the list: nt = 0");
    no(td_list_check(fn, 2, 4, 3, k, 3, shift, -1.0), "the list: dt < 0");
    {
        double kb[6];
        memcpy(kb, k, sizeof kb);
        kb[4] = nan;
        no(td_list_check(fn, 2, 4, 3, kb, 3, shift, 0.1), "a NaN k");
        std::vector<double> kk((size_t)2 * 17, 0.125);
        ok(td_list_check(fn, 2, 2048, 16, kk.data(), 3, shift, 0.1), "16 points of 2048 states at the cap");
        no(td_list_check(fn, 2, 2048, 17, kk.data(), 3, shift, 0.1), "17 points of 2048 states");
    }
    // the form of the measurement: by lattice vector for 5 .. 16 states that keep their terms so, whose slots fit its LDS
    for (int n = 1; n <= 40; ++n)
        for (int nR : {0, 1, 256}) {
            const bool by = td_observe_by_vector(n, nR);
            if (by != (n >= 5 && n <= 16 && nR > 0)) bad |= printf("the form of the measurement at n=%d nR=%d\n", n, nR);
            if (by && (n * (n + 1) / 2 > TD_OB_SLOTS || n > 16)) bad |= printf("n=%d: the slots do not fit the LDS of k_td_observe_rvec\n", n);
        }
    if ((size_t)TD_OB_PB * TD_OB_SLOTS * sizeof(cd) + 3 * TD_OB_SLOTS * sizeof(double) + (size_t)TD_OB_PB * 20 * sizeof(cd) > 49152)
        bad |= printf("the LDS of k_td_observe_rvec\n");
    // the midpoint of a step is 0.5 (a + b), in that order
    {
        const TdKappa a = td_kappa(shift, 2, 1), mid = td_kappa_mid(shift, 2, 1);
        if (a.v[0] != 0.05 || a.v[1] != -0.2 || a.v[2] != 0.0 || mid.v[0] != 0.5 * (0.05 + 1.5) || mid.v[1] != 0.5 * (-0.2 + 0.0))
            bad |= printf("kappa\n");
    }
    return bad;
}

int main() {
    int bad = 0, cases = 0;
    for (const Case& c : kCases) {
        bad |= check_case(c) ? 1 : 0;
        ++cases;
    }
    bad |= check_lds_maps() ? 1 : 0;
    bad |= check_args() ? 1 : 0;
    if (bad) return printf("td_plan_check: FAILED\n"), 1;
    printf("td_plan_check: %d plans, the lane maps of the LDS step for 1..32 states and the argument checks ok\n", cases);
    return 0;
}
