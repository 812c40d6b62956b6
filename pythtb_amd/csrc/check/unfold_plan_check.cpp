// Stand-alone host check of tbk_unfold.h (no device call): built under AddressSanitizer + UBSan by `make -C pythtb_amd/csrc unfold-check`
// and run as an ordinary program.  Over a table of (n, dim_k, nk, ng, nw, per_state, phases) it checks the plan of the unfolding calls --
// the chunk, the band tiles, the group slots, shares and bands of a workgroup of the projection and the accumulator tile of the
// broadening against values worked out by hand, the LDS budgets, the grid limits, that the band tiles cover every band once, that the
// chunk's buffers hold what the kernels write and that nothing but the result's size depends on nk or nw -- replays the lane maps of
// k_unfold_weights on the host (every LDS index inside its array, every member of every group read exactly once per band, states of
// group -1 never) and the layout of the scratch block (every buffer at a multiple of 256, in order, none overlapping, filled and read
// back under the sanitizer).  Then the group tables and the argument checks: every rule and the edges of the caps, one bad value at a time.
#include <cmath>
#include <limits>
#include <vector>
#include "../tbk_unfold.h"
#include "check_common.h"

// the group of state j in the cases of the table: the order make_supercell produces, every 7th state an adatom where `holes`
static std::vector<int32_t> groups_of(int n, int ng, bool holes) {
    std::vector<int32_t> g((size_t)n);
    for (int j = 0; j < n; ++j) g[(size_t)j] = holes && j % 7 == 3 ? -1 : j % ng;
    return g;
}

struct Case {
    int n, dk;
    int64_t nk;
    int ng, nw, per_state, phases, holes;
    // expected: points per chunk, bands per load, band tiles, group slots, shares, bands side by side, accumulators
    int64_t chunk;
    int BT, ntile, NGP, L, BB, GT;
};
static const Case kCases[] = {
    {1, 1, 5, 1, 1, 0, 0, 0, 5, 1, 1, 1, 32, 8, 1},
    {2, 2, 7, 2, 3, 1, 0, 0, 7, 2, 1, 2, 32, 4, 4},                            // the identity supercell of a two-band model
    {2, 2, 7, 2, 0, 1, 1, 0, 7, 2, 1, 2, 32, 4, 0},                            // the bands call
    {10, 2, 7, 2, 5, 0, 1, 0, 7, 10, 1, 2, 32, 4, 1},
    {16, 2, 7, 4, 5, 1, 0, 0, 7, 16, 1, 4, 32, 2, 4},                          // spinful: four groups
    {33, 1, 7, 3, 257, 1, 0, 1, 7, 33, 1, 4, 32, 2, 4},                        // a frequency beyond the first block; adatoms
    {40, 2, 1317, 2, 3, 1, 0, 0, 1310, 40, 1, 2, 32, 4, 4},                    // two chunks
    {45, 2, 9, 5, 2, 1, 1, 0, 9, 45, 1, 8, 32, 1, 16},                         // the last size with every band in one load
    {46, 2, 9, 5, 2, 1, 1, 0, 9, 44, 2, 8, 32, 1, 16},                         // the first with two band tiles
    {64, 2, 7, 64, 5, 1, 0, 0, 7, 32, 2, 64, 4, 1, 64},                        // 64 groups: four shares, the widest accumulator tile
    {64, 2, 7, 17, 5, 1, 0, 0, 7, 32, 2, 32, 8, 1, 64},
    {64, 2, 7, 16, 5, 1, 0, 0, 7, 32, 2, 16, 16, 1, 16},
    {129, 1, 7, 3, 5, 0, 0, 0, 7, 15, 9, 4, 32, 2, 1},
    {200, 2, 300, 2, 512, 1, 0, 0, 52, 10, 20, 2, 32, 4, 4},
    {2048, 2, 64, 2, 1024, 1, 1, 1, 1, 1, 2048, 2, 32, 4, 4},                  // the largest model: a point per chunk
    {2048, 3, 3, 64, 65536, 1, 1, 0, 1, 1, 2048, 64, 4, 1, 64},                // the most frequencies
    {2, 2, 1 << 16, 2, 128, 1, 0, 0, 1 << 16, 2, 1, 2, 32, 4, 4},              // nk nw ng at the cap
    {8, 3, 1 << 18, 64, 1, 1, 0, 0, 16384, 8, 1, 64, 4, 1, 64},                // the chunk shortened by the weights' 64 MiB: 2^26 / (8 x 64 x 8 B)
};

static int check_case(const Case& c) {
    char tag[160];
    snprintf(tag, sizeof tag, "unfold n=%d dk=%d nk=%lld ng=%d nw=%d per_state=%d phases=%d", c.n, c.dk, (long long)c.nk, c.ng, c.nw, c.per_state,
             c.phases);
    const std::vector<int32_t> group = groups_of(c.n, c.ng, c.holes != 0);
    const UnfGroups gt = unf_groups(c.n, c.ng, group.data());
    const int nidx = (int)gt.idx.size();
    const int norb = c.n;
    const UnfPlan p = unf_plan(c.n, c.dk, norb, c.nk, c.ng, c.per_state, c.nw, c.phases != 0, nidx);
    if (p.chunk != c.chunk || p.BT != c.BT || p.ntile != c.ntile || p.NGP != c.NGP || p.L != c.L || p.BB != c.BB || p.GT != c.GT)
        return printf("%s: chunk %lld BT %d ntile %d NGP %d L %d BB %d GT %d\n", tag, (long long)p.chunk, p.BT, p.ntile, p.NGP, p.L, p.BB, p.GT);
    const int ngo = c.per_state ? c.ng : 1;
    if (p.ngo != ngo) return printf("%s: ngo\n", tag);
    if (p.chunk < 1 || p.chunk > c.nk || p.nchunks != (c.nk + p.chunk - 1) / p.chunk) return printf("%s: the chunks\n", tag);
    if ((size_t)p.chunk * c.n * c.n * sizeof(cd) > std::max(kKuboChunkBytes, (size_t)c.n * c.n * sizeof(cd)))
        return printf("%s: the chunk holds more than kKuboChunkBytes of eigenvectors\n", tag);
    if (c.nw && (size_t)p.chunk * c.n * ngo * sizeof(double) > std::max(kUnfWBytes, (size_t)c.n * ngo * sizeof(double)))
        return printf("%s: the chunk's weights over kUnfWBytes\n", tag);
    // the LDS of the projection: BT bands of n components, the members, the offsets, the shares, the per-group weights
    if ((int64_t)p.BT * c.n > kUnfLdsCd || p.BT < 1 || p.BT > c.n) return printf("%s: %d bands do not fit the LDS\n", tag, p.BT);
    if (nidx > kUnfStatesMax || c.ng + 1 > kUnfGroupsMax + 1) return printf("%s: the tables do not fit the LDS\n", tag);
    const size_t ldsw = (size_t)kUnfLdsCd * sizeof(cd) + 256 * sizeof(cd) + 256 * sizeof(double) + (size_t)kUnfStatesMax * sizeof(int) +
                        (size_t)(kUnfGroupsMax + 1) * sizeof(int);
    if (ldsw > 65536) return printf("%s: %zu bytes of LDS in the projection\n", tag, ldsw);
    if (p.GT && (p.GT < ngo || (size_t)UNF_SB * (p.GT + 1) * sizeof(double) > 65536)) return printf("%s: GT=%d\n", tag, p.GT);
    if (p.NGP < c.ng || (p.NGP > 1 && p.NGP / 2 >= c.ng) || p.NGP * p.L * p.BB != 256 || p.L < 1 || p.L > 32)
        return printf("%s: the lanes NGP %d L %d BB %d\n", tag, p.NGP, p.L, p.BB);
    // the band tiles cover every band once
    {
        int at = 0;
        for (int z = 0; z < p.ntile; ++z) {
            const int b0 = z * p.BT, nb = std::min(p.BT, c.n - b0);
            if (b0 != at || nb < 1) return printf("%s: band tile %d\n", tag, z);
            at += nb;
        }
        if (at != c.n) return printf("%s: the band tiles end at %d\n", tag, at);
    }
    // the grids: (points, band tiles) and (points, blocks of frequencies)
    if (p.chunk > 2147483647 || p.ntile > 65535 || p.nwb > 65535 || (c.nw && p.nwb != (c.nw + UNF_FB - 1) / UNF_FB)) return printf("%s: the grid\n", tag);
    // the lane maps of k_unfold_weights, for the first band tile and the last
    for (int z : {0, p.ntile - 1}) {
        const int b0 = z * p.BT, nb = std::min(p.BT, c.n - b0);
        const int per = p.NGP * p.L, BB = 256 / per;
        std::vector<int> reads((size_t)nb * c.n, 0), done((size_t)nb * c.ng, 0);
        for (int b1 = 0; b1 < nb; b1 += BB) {
            for (int t = 0; t < 256; ++t) {
                const int bb = t / per, r = t - bb * per, g = r / p.L, l = r - g * p.L;
                if (bb >= BB || g >= p.NGP) return printf("%s: lane %d maps outside the workgroup\n", tag, t);
                if (b1 + bb < nb && g < c.ng)
                    for (int e = gt.off[(size_t)g] + l; e < gt.off[(size_t)g + 1]; e += p.L) {
                        if (e < 0 || e >= nidx) return printf("%s: member %d outside the list\n", tag, e);
                        const int at = (b1 + bb) * c.n + gt.idx[(size_t)e];
                        if (at < 0 || at >= p.BT * c.n || at >= kUnfLdsCd) return printf("%s: LDS index %d\n", tag, at);
                        ++reads[(size_t)at];
                    }
                const int bb2 = t / p.NGP, g2 = t - bb2 * p.NGP;
                if (t < BB * p.NGP && b1 + bb2 < nb && g2 < c.ng) {
                    if (t * p.L + p.L > 256) return printf("%s: the shares of lane %d end beyond the workgroup\n", tag, t);
                    if ((bb2 * p.NGP + g2) * p.L != t * p.L) return printf("%s: the finishing lane %d\n", tag, t);
                    ++done[(size_t)(b1 + bb2) * c.ng + g2];
                }
                if (t < BB && b1 + t < nb && t * p.NGP + c.ng > 256) return printf("%s: the total of lane %d\n", tag, t);
            }
        }
        for (int b = 0; b < nb; ++b)
            for (int j = 0; j < c.n; ++j)
                if (reads[(size_t)b * c.n + j] != (group[(size_t)j] >= 0 ? 1 : 0))
                    return printf("%s: band %d reads state %d (group %d) %d times\n", tag, b0 + b, j, group[(size_t)j], reads[(size_t)b * c.n + j]);
        for (int d : done)
            if (d != 1) return printf("%s: a (band, group) is finished %d times\n", tag, d);
    }
    // the same point is worked through the same way whatever stands beside it: nothing but the chunk and the sizes depends on nk, nw
    const UnfPlan one = unf_plan(c.n, c.dk, norb, 1, c.ng, c.per_state, c.nw ? 1 : 0, c.phases != 0, nidx);
    if (one.BT != p.BT || one.ntile != p.ntile || one.NGP != p.NGP || one.L != p.L || one.BB != p.BB || one.GT != p.GT)
        return printf("%s: the lane mapping depends on nk or nw\n", tag);
    const size_t D = sizeof(double), cb = p.off_chunks;
    const size_t buf[][2] = {
        {p.off_k, (size_t)c.nk * c.dk * D},
        {p.off_pk, c.phases ? (size_t)c.nk * c.dk * D : 0},
        {p.off_delta, c.phases ? (size_t)norb * c.dk * D : 0},
        {p.off_om, (size_t)c.nw * D},
        {p.off_goff, (size_t)(c.ng + 1) * sizeof(int32_t)},
        {p.off_idx, (size_t)nidx * sizeof(int32_t)},
        {p.off_ev, c.nw ? 0 : (size_t)c.n * c.nk * D},
        {p.off_out, (size_t)c.nk * (c.nw ? c.nw : c.n) * ngo * D},
        {cb + p.cw.off[0], (size_t)p.chunk * c.dk * D},
        {cb + p.cw.off[1], (size_t)p.chunk * c.n * D},
        {cb + p.cw.off[2], (size_t)p.chunk * c.n * c.n * sizeof(cd)},
        {cb + p.cw.off[3], c.phases ? (size_t)p.chunk * c.n * sizeof(cd) : 0},
        {cb + p.cw.off[4], c.nw ? (size_t)p.chunk * c.n * ngo * D : 0},
    };
    if (p.out_d != c.nk * (c.nw ? c.nw : c.n) * ngo) return printf("%s: the result\n", tag);
    return check_buffers(tag, buf, (int)(sizeof buf / sizeof buf[0]), p.total);
}

// ---------------------------------------------------------------- the group tables
static int check_groups() {
    int bad = 0;
    const int32_t g[9] = {1, -1, 0, 1, 2, -1, 0, 1, 1};
    const UnfGroups t = unf_groups(9, 4, g);                       // group 3 is empty
    const int32_t off[5] = {0, 2, 6, 7, 7}, idx[7] = {2, 6, 0, 3, 7, 8, 4};
    if (t.off.size() != 5 || memcmp(t.off.data(), off, sizeof off)) bad |= printf("groups: the offsets\n");
    if (t.idx.size() != 7 || memcmp(t.idx.data(), idx, sizeof idx)) bad |= printf("groups: the members\n");
    const int32_t none[3] = {-1, 0, -1};
    const UnfGroups u = unf_groups(3, 1, none);
    if (u.idx.size() != 1 || u.idx[0] != 1 || u.off[1] != 1) bad |= printf("groups: one member\n");
    return bad;
}

// ---------------------------------------------------------------- the argument checks
static int check_args() {
    const char* fn = "unfold_plan_check";
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    int bad = 0;
    auto ok = [&](int rc, const char* what) {
        if (rc != TBK_OK) bad |= printf("refused: %s\n", what);
    };
    auto no = [&](int rc, const char* what) {
        if (rc != TBK_EINVAL) bad |= printf("accepted: %s\n", what);
    };
    const double k[6] = {0.1, 0.2, -1.3, 0.4, 2.5, 0.0}, om[3] = {0.5, -1.0, 0.5};
    const double delta[8] = {0.0, 0.01, -0.02, 0.0, 0.03, 0.0, 0.0, -0.04};
    const int32_t g[4] = {0, 1, -1, 1};
    ok(unf_check(fn, 2, 4, 4, 3, k, 2, g, nullptr, nullptr, 0.5, 1, 3, om, 0.05), "three points, three frequencies");
    ok(unf_check(fn, 2, 4, 4, 3, k, 2, g, k, delta, 0.5, 0, 0, nullptr, 0.0), "the bands call with phases");
    ok(unf_check(fn, 2, 4, 2, 3, k, 2, g, k, delta, 0.5, 0, 0, nullptr, 0.0), "a spinful model: two orbitals");
    no(unf_check(fn, 0, 4, 4, 3, k, 2, g, nullptr, nullptr, 0.5, 1, 3, om, 0.05), "dim_k = 0");
    no(unf_check(fn, 4, 4, 4, 1, k, 2, g, nullptr, nullptr, 0.5, 1, 3, om, 0.05), "dim_k = 4");
    no(unf_check(fn, 2, 4, 4, 0, k, 2, g, nullptr, nullptr, 0.5, 1, 3, om, 0.05), "no k-point");
    no(unf_check(fn, 2, 4, 4, 3, nullptr, 2, g, nullptr, nullptr, 0.5, 1, 3, om, 0.05), "no k list");
    no(unf_check(fn, 2, 4, 4, 3, k, 0, g, nullptr, nullptr, 0.5, 1, 3, om, 0.05), "no group");
    no(unf_check(fn, 2, 4, 4, 3, k, 65, g, nullptr, nullptr, 0.5, 1, 3, om, 0.05), "65 groups");
    no(unf_check(fn, 2, 4, 4, 3, k, 2, nullptr, nullptr, nullptr, 0.5, 1, 3, om, 0.05), "no group map");
    no(unf_check(fn, 2, 4, 4, 3, k, 1, g, nullptr, nullptr, 0.5, 1, 3, om, 0.05), "a group beyond the last");
    {
        const int32_t low[4] = {0, -2, 1, 1}, out[4] = {-1, -1, -1, -1};
        no(unf_check(fn, 2, 4, 4, 3, k, 2, low, nullptr, nullptr, 0.5, 1, 3, om, 0.05), "a group of -2");
        no(unf_check(fn, 2, 4, 4, 3, k, 2, out, nullptr, nullptr, 0.5, 1, 3, om, 0.05), "every state outside");
    }
    no(unf_check(fn, 2, 4, 4, 3, k, 2, g, k, nullptr, 0.5, 1, 3, om, 0.05), "phase_k without delta");
    no(unf_check(fn, 2, 4, 4, 3, k, 2, g, nullptr, delta, 0.5, 1, 3, om, 0.05), "delta without phase_k");
    for (double x : {0.0, -0.5, nan, inf}) no(unf_check(fn, 2, 4, 4, 3, k, 2, g, nullptr, nullptr, x, 1, 3, om, 0.05), "a bad inv_nc");
    {
        double kb[6], db[8];
        memcpy(kb, k, sizeof kb);
        kb[3] = nan;
        no(unf_check(fn, 2, 4, 4, 3, kb, 2, g, nullptr, nullptr, 0.5, 1, 3, om, 0.05), "a NaN k");
        no(unf_check(fn, 2, 4, 4, 3, k, 2, g, kb, delta, 0.5, 1, 3, om, 0.05), "a NaN phase k");
        memcpy(db, delta, sizeof db);
        db[7] = inf;
        no(unf_check(fn, 2, 4, 4, 3, k, 2, g, k, db, 0.5, 1, 3, om, 0.05), "an infinite displacement");
    }
    no(unf_check(fn, 2, 4, 4, 3, k, 2, g, nullptr, nullptr, 0.5, 1, 3, nullptr, 0.05), "no frequency array");
    {
        const double wb[3] = {0.5, nan, 0.1};
        no(unf_check(fn, 2, 4, 4, 3, k, 2, g, nullptr, nullptr, 0.5, 1, 3, wb, 0.05), "a NaN frequency");
        std::vector<double> many(65537, 0.25);
        ok(unf_check(fn, 2, 4, 4, 3, k, 2, g, nullptr, nullptr, 0.5, 1, 65536, many.data(), 0.05), "65536 frequencies");
        no(unf_check(fn, 2, 4, 4, 3, k, 2, g, nullptr, nullptr, 0.5, 1, 65537, many.data(), 0.05), "65537 frequencies");
    }
    for (double eta : {0.0, -1e-3, nan, inf}) no(unf_check(fn, 2, 4, 4, 3, k, 2, g, nullptr, nullptr, 0.5, 1, 3, om, eta), "a bad eta");
    {   // the states and the result caps
        std::vector<int32_t> gg(2049, 0);
        ok(unf_check(fn, 2, 2048, 2048, 3, k, 1, gg.data(), nullptr, nullptr, 0.5, 1, 3, om, 0.05), "2048 states");
        no(unf_check(fn, 2, 2049, 2049, 3, k, 1, gg.data(), nullptr, nullptr, 0.5, 1, 3, om, 0.05), "2049 states");
        const int64_t nk = 1 << 16;
        std::vector<double> kk((size_t)(nk + 1) * 2, 0.125), w(129, 0.1);
        ok(unf_check(fn, 2, 4, 4, nk, kk.data(), 2, g, nullptr, nullptr, 0.5, 1, 128, w.data(), 0.05), "nk nw ng at the cap");
        no(unf_check(fn, 2, 4, 4, nk, kk.data(), 2, g, nullptr, nullptr, 0.5, 1, 129, w.data(), 0.05), "nk nw ng over the cap");
        ok(unf_check(fn, 2, 4, 4, nk, kk.data(), 2, g, nullptr, nullptr, 0.5, 0, 129, w.data(), 0.05), "the total: one group of the result");
        ok(unf_check(fn, 2, 2048, 2048, 8192, kk.data(), 1, gg.data(), nullptr, nullptr, 0.5, 0, 0, nullptr, 0.0), "nsta nk at the cap");
        no(unf_check(fn, 2, 2048, 2048, 8193, kk.data(), 1, gg.data(), nullptr, nullptr, 0.5, 0, 0, nullptr, 0.0), "nsta nk over the cap");
    }
    return bad;
}

int main() {
    int bad = 0, cases = 0;
    for (const Case& c : kCases) {
        bad |= check_case(c) ? 1 : 0;
        ++cases;
    }
    bad |= check_groups() ? 1 : 0;
    bad |= check_args() ? 1 : 0;
    if (bad) return printf("unfold_plan_check: FAILED\n"), 1;
    printf("unfold_plan_check: %d plans, the group tables and the argument checks ok\n", cases);
    return 0;
}
