// Stand-alone host check of tbk_chim.h (no device call): built under AddressSanitizer + UBSan by `make -C pythtb_amd/csrc chim-check`
// and run as an ordinary program.  Over a table of (n, dim_k, mesh, nq, nw, na, interaction) it checks the plan of
// tbk_susceptibility_matrix_mesh: the chunk, the k-groups, the frequency tiles, the entry blocks and the points per batch of the LDS
// kernel against the values worked out by hand; the chunk bound (eigenvectors, records and the two tables each within
// kKuboChunkBytes); the part buffer against its cap with at least two groups wherever the chunk has two points; the LDS budget of a
// batch; that the k-groups of every chunk (the last, shorter one included) cover its points once; that nothing but acc, V, the result
// and the offsets behind them depends on nq; and the layout of the scratch block -- every buffer at a multiple of 256, in order, none
// overlapping, the last one ending at the total (each is filled with its own index over a real host block and read back, under the
// sanitizer, where the block is at most 512 MiB).  Then the argument checks: every rule of chim_check, one bad value at a time.
#include <cmath>
#include <limits>
#include <vector>
#include "../tbk_chim.h"
#include "check_common.h"

struct Case {
    int n, dk, mesh[3], nq, nw, na, nvq;
    // expected: points per chunk, k-groups, frequency tiles, entry blocks, points per LDS batch (0: not the LDS kernel)
    int64_t chunk;
    int G;
    unsigned ntile, neb;
    int P;
};

static const Case kCases[] = {
    // one state: a single entry, blocks of one
    {1, 1, {7, 1, 1}, 4, 0, 1, 0, 7, 7, 0, 1, 64},
    {1, 1, {7, 1, 1}, 4, 6, 1, 1, 7, 7, 1, 1, 0},
    {1, 2, {2048, 2048, 1}, 1, 0, 1, 1, 2097152, 1024, 0, 1, 64},
    // the tables of one state are twice its eigenvectors: half the chunk of the static call
    {1, 2, {2048, 2048, 1}, 1, 2, 1, 0, 1048576, 1024, 1, 1, 0},
    {2, 2, {6, 5, 1}, 4, 0, 2, 0, 30, 30, 0, 1, 64},
    {2, 2, {6, 5, 1}, 4, 6, 2, 4, 30, 30, 1, 1, 0},
    {2, 2, {9, 7, 1}, 1, 513, 2, 0, 63, 63, 2, 1, 0},
    {2, 2, {256, 256, 1}, 4096, 0, 2, 1, 65536, 1024, 0, 1, 64},
    {2, 2, {256, 256, 1}, 64, 256, 2, 64, 65536, 1024, 1, 1, 0},
    {4, 2, {5, 4, 1}, 4, 6, 3, 0, 20, 20, 1, 3, 0},
    {4, 2, {5, 4, 1}, 4, 0, 3, 0, 20, 20, 0, 3, 63},
    // 8 states, all selected: tables of 2 x 8 x 64 x 16 B per point, 2048 points; 2^24 / (2 x 64 x 256) = 512 groups
    {8, 3, {32, 32, 32}, 64, 256, 8, 1, 2048, 512, 1, 16, 0},
    {8, 3, {32, 32, 32}, 64, 0, 8, 1, 32768, 1024, 0, 16, 12},
    {16, 3, {3, 2, 2}, 4, 6, 16, 0, 12, 12, 1, 64, 0},
    {16, 3, {3, 2, 2}, 4, 0, 16, 0, 12, 12, 0, 64, 3},
    {16, 3, {3, 2, 2}, 4, 0, 3, 0, 12, 12, 0, 3, 9},
    {32, 2, {3, 2, 1}, 4, 0, 5, 0, 6, 6, 0, 7, 2},
    {32, 2, {3, 2, 1}, 4, 0, 16, 0, 6, 6, 0, 64, 1},
    {32, 2, {48, 48, 1}, 2, 6, 16, 2, 128, 128, 1, 64, 0},
    // the wide form: 1618 points of eigenvectors, 1820 of tables
    {36, 2, {41, 40, 1}, 1, 0, 4, 0, 1618, 1024, 0, 4, 0},
    {36, 2, {41, 40, 1}, 1, 2, 4, 1, 1618, 1024, 1, 4, 0},
    {36, 2, {41, 40, 1}, 1, 2, 16, 1, 113, 113, 1, 64, 0},
    {2048, 1, {3, 1, 1}, 1, 0, 16, 0, 1, 1, 0, 64, 0},
    // the most rows per q: 2 nw na^2 = 2^23, two groups
    {16, 2, {8, 8, 1}, 1, 16384, 16, 1, 64, 2, 32, 64, 0},
    {2, 2, {256, 256, 1}, 16, 65536, 2, 0, 65536, 32, 128, 1, 0},
};

static int check_layout(const char* tag, const ChimPlan& p, int n, int dk, int nq, int nw, int nvq) {
    const size_t nn = (size_t)n * n, D = sizeof(double), C = sizeof(cd);
    const size_t cb = p.off_chunks;
    const size_t x0 = cb + p.cw.off[3], x2 = cb + p.cw.off[5];
    const size_t tab = p.tables ? (size_t)p.chunk * n * p.nab * C : 0;
    const size_t buf[][2] = {
        {p.off_om, (size_t)nw * D},
        {p.off_q, (size_t)nq * dk * D},
        {p.off_sel, (size_t)p.na * sizeof(int32_t)},
        {p.off_v, (size_t)nvq * p.nab * C},
        {p.off_acc, (size_t)p.acc_doubles * D},
        {p.off_part, (size_t)p.part_doubles * D},
        {p.off_out, (size_t)p.out_cd * C},
        {cb + p.cw.off[0], (size_t)p.chunk * dk * D},
        {cb + p.cw.off[1], (size_t)p.chunk * n * D},
        {cb + p.cw.off[2], (size_t)p.chunk * nn * C},
        {x0, (size_t)p.chunk * dk * D},
        {x0 + p.off_e2, (size_t)p.chunk * n * D},
        {x0 + p.off_v2, (size_t)p.chunk * nn * C},
        {cb + p.cw.off[4], p.tables ? (size_t)p.chunk * nn * (p.dynamic ? 2 : 1) * D : 0},
        {x2, tab},
        {x2 + p.off_y, tab},
    };
    const int nb = (int)(sizeof buf / sizeof buf[0]);
    size_t end = 256;
    for (int i = 0; i < nb; ++i) {
        if (buf[i][0] % 256 || buf[i][0] < end)
            return printf("%s: buffer %d at offset %zu (the previous one ends at %zu)\n", tag, i, buf[i][0], end);
        end = buf[i][0] + buf[i][1];
    }
    if (end > p.total || p.total - end >= 256 + 256) return printf("%s: the last buffer ends at %zu, the total is %zu\n", tag, end, p.total);
    if (p.total > ((size_t)512 << 20)) return 0;
    unsigned char* base = (unsigned char*)aligned_alloc(256, al256(p.total));
    if (!base) return printf("%s: no host block of %zu bytes\n", tag, p.total);
    int bad = 0;
    for (int i = 0; i < nb; ++i) memset(base + buf[i][0], i + 1, buf[i][1]);
    for (int i = 0; i < nb && !bad; ++i)
        for (size_t j = 0; j < buf[i][1]; j += 61)
            if (base[buf[i][0] + j] != (unsigned char)(i + 1)) {
                bad = printf("%s: buffer %d is overwritten at byte %zu\n", tag, i, j);
                break;
            }
    free(base);
    return bad;
}

static int check_case(const Case& c) {
    char tag[160];
    snprintf(tag, sizeof tag, "n=%d dk=%d mesh=%dx%dx%d nq=%d nw=%d na=%d nvq=%d", c.n, c.dk, c.mesh[0], c.mesh[1], c.mesh[2], c.nq, c.nw,
             c.na, c.nvq);
    const int64_t npts = (int64_t)c.mesh[0] * c.mesh[1] * c.mesh[2];
    const ChimPlan p = chim_plan(c.n, c.dk, npts, c.nq, c.nw, c.na, c.nvq);
    const size_t nn = (size_t)c.n * c.n;
    if (p.chunk != c.chunk || p.G != c.G || p.ntile != c.ntile || p.neb != c.neb || (p.lds ? p.P : 0) != c.P)
        return printf("%s: chunk %lld G %d ntile %u neb %u P %d\n", tag, (long long)p.chunk, p.G, p.ntile, p.neb, p.lds ? p.P : 0);
    if (p.lds == p.tables || p.lds != (c.nw == 0 && c.n <= 32) || p.rpa != (c.nvq > 0)) return printf("%s: the form\n", tag);
    // the chunk bound: eigenvectors, records and both tables within kKuboChunkBytes each (a single point may be larger)
    if (p.chunk < 1 || p.chunk > npts) return printf("%s: the chunk\n", tag);
    if (p.chunk > 1 && ((size_t)p.chunk * nn * sizeof(cd) > kKuboChunkBytes || p.x1 > kKuboChunkBytes || p.x2 > kKuboChunkBytes + 256))
        return printf("%s: the chunk holds more than kKuboChunkBytes\n", tag);
    if (p.nchunks != (npts + p.chunk - 1) / p.chunk) return printf("%s: nchunks\n", tag);
    if (p.G < 1 || p.G > kPairGroupsMax || p.G > p.chunk) return printf("%s: G=%d\n", tag, p.G);
    if (p.nrows != 2 * (int64_t)c.na * c.na * std::max(c.nw, 1) || p.nrows > ((int64_t)1 << 23)) return printf("%s: nrows\n", tag);
    if (p.part_doubles != p.G * p.nrows || p.part_doubles > kPairPartCap) return printf("%s: part over the cap\n", tag);
    if (p.chunk >= 2 && p.G < 2) return printf("%s: one group for a chunk of %lld points\n", tag, (long long)p.chunk);
    if (p.lds && (p.P < 1 || p.P > 64 || (c.n * c.n + 4 * c.n * c.na) * p.P > CHIM_LDS_D || 2 * 256 > CHIM_LDS_D))
        return printf("%s: %d points do not fit the LDS\n", tag, p.P);
    if (p.nab > 256 || p.nab != c.na * c.na) return printf("%s: more entries than lanes\n", tag);
    if ((int64_t)p.neb * p.EB < p.nab || (int64_t)(p.neb - 1) * p.EB >= p.nab || p.neb > 65535) return printf("%s: entry blocks\n", tag);
    if ((int64_t)p.ntile * kPairTile < c.nw || (p.ntile > 0 && (int64_t)(p.ntile - 1) * kPairTile >= c.nw)) return printf("%s: tiles\n", tag);
    if (p.lane_rows != (p.nrows >= kChimLaneRows)) return printf("%s: the group sum\n", tag);
    // the launches of one lane per item stay inside a grid
    if (p.tables && ((int64_t)p.chunk * c.n * p.nab + 255) / 256 > 0x7fffffffLL) return printf("%s: the tables' grid\n", tag);
    if (check_groups(tag, p.G, npts, p.chunk, p.nchunks)) return 1;
    // a q alone is worked through like the same q inside this list
    const ChimPlan one = chim_plan(c.n, c.dk, npts, 1, c.nw, c.na, c.nvq ? 1 : 0);
    if (one.chunk != p.chunk || one.G != p.G || one.ntile != p.ntile || one.neb != p.neb || one.EB != p.EB || one.P != p.P ||
        one.nrows != p.nrows || one.part_doubles != p.part_doubles || one.lane_rows != p.lane_rows || one.x0 != p.x0 || one.x1 != p.x1 ||
        one.x2 != p.x2 || one.off_y != p.off_y)
        return printf("%s: the plan depends on nq\n", tag);
    // ... and the interaction changes nothing of how chi0 is formed
    const ChimPlan bare = chim_plan(c.n, c.dk, npts, c.nq, c.nw, c.na, 0);
    if (bare.chunk != p.chunk || bare.G != p.G || bare.ntile != p.ntile || bare.neb != p.neb || bare.P != p.P || bare.lane_rows != p.lane_rows)
        return printf("%s: the plan depends on the interaction\n", tag);
    if (p.acc_doubles != (int64_t)c.nq * p.nrows || p.nmat != (int64_t)c.nq * std::max(c.nw, 1)) return printf("%s: acc\n", tag);
    if (p.out_cd != p.nmat * p.nab * (p.rpa ? 2 : 1) + (p.rpa ? p.nmat : 0)) return printf("%s: the result\n", tag);
    return check_layout(tag, p, c.n, c.dk, c.nq, c.nw, c.nvq);
}

static int check_args() {
    const char* fn = "chim_plan_check";
    const int32_t mesh[3] = {4, 5, 6};
    const double q[4] = {0.1, 0.2, 0.3, 0.4}, w[2] = {0.5, -1.0};
    const int32_t sel[3] = {2, 0, 1};
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    std::vector<double> v(2 * 9 * 2, 0.25);
    int64_t npts = 0;
    int bad = 0;
    auto ok = [&](int rc, const char* what) {
        if (rc != TBK_OK) bad |= printf("refused: %s\n", what);
    };
    auto no = [&](int rc, const char* what) {
        if (rc != TBK_EINVAL) bad |= printf("accepted: %s\n", what);
    };
    ok(chim_check(fn, 2, 3, mesh, 2, q, 2, w, 0.05, 0.0, 0.0, 3, sel, nullptr, 0, false, false, npts), "dynamic");
    if (npts != 20) bad |= printf("npts=%lld\n", (long long)npts);
    ok(chim_check(fn, 3, 3, mesh, 1, q, 0, nullptr, 0.0, 0.3, 0.1, 2, sel, nullptr, 0, false, false, npts), "static");
    if (npts != 120) bad |= printf("npts=%lld\n", (long long)npts);
    ok(chim_check(fn, 2, 3, mesh, 2, q, 2, w, 0.05, 0.0, 0.0, 3, sel, v.data(), 1, true, false, npts), "one V");
    ok(chim_check(fn, 2, 3, mesh, 2, q, 0, nullptr, 0.0, 0.0, 0.0, 3, sel, v.data(), 2, true, true, npts), "V(q) and det");
    // the checks of the scalar call, through chi_check
    no(chim_check(fn, 0, 3, mesh, 2, q, 2, w, 0.05, 0.0, 0.0, 3, sel, nullptr, 0, false, false, npts), "dim_k = 0");
    no(chim_check(fn, 2, 2049, mesh, 2, q, 2, w, 0.05, 0.0, 0.0, 3, sel, nullptr, 0, false, false, npts), "2049 states");
    no(chim_check(fn, 2, 3, mesh, 0, q, 2, w, 0.05, 0.0, 0.0, 3, sel, nullptr, 0, false, false, npts), "nq = 0");
    {
        const double qb[4] = {0.1, nan, 0.3, 0.4};
        no(chim_check(fn, 2, 3, mesh, 2, qb, 2, w, 0.05, 0.0, 0.0, 3, sel, nullptr, 0, false, false, npts), "a NaN q");
        const double wb[2] = {0.5, inf};
        no(chim_check(fn, 2, 3, mesh, 2, q, 2, wb, 0.05, 0.0, 0.0, 3, sel, nullptr, 0, false, false, npts), "an infinite frequency");
    }
    for (double eta : {0.0, -0.1, nan, inf}) no(chim_check(fn, 2, 3, mesh, 2, q, 2, w, eta, 0.0, 0.0, 3, sel, nullptr, 0, false, false, npts), "a bad eta");
    no(chim_check(fn, 2, 3, mesh, 2, q, 0, nullptr, 0.05, 0.0, 0.0, 3, sel, nullptr, 0, false, false, npts), "eta in the static mode");
    for (double kT : {-1e-3, nan, inf}) no(chim_check(fn, 2, 3, mesh, 2, q, 0, nullptr, 0.0, 0.0, kT, 3, sel, nullptr, 0, false, false, npts), "a bad kT");
    no(chim_check(fn, 2, 3, mesh, 2, q, 2, w, 0.05, nan, 0.0, 3, sel, nullptr, 0, false, false, npts), "a bad Fermi level");
    {
        const int32_t mb[3] = {4, 0, 6};
        no(chim_check(fn, 2, 3, mb, 2, q, 2, w, 0.05, 0.0, 0.0, 3, sel, nullptr, 0, false, false, npts), "a mesh axis of 0 points");
    }
    // the selection
    no(chim_check(fn, 2, 3, mesh, 2, q, 2, w, 0.05, 0.0, 0.0, 0, sel, nullptr, 0, false, false, npts), "no selected state");
    {
        int32_t s17[17];
        for (int i = 0; i < 17; ++i) s17[i] = i;
        no(chim_check(fn, 2, 20, mesh, 2, q, 2, w, 0.05, 0.0, 0.0, 17, s17, nullptr, 0, false, false, npts), "17 selected states");
        ok(chim_check(fn, 2, 20, mesh, 2, q, 2, w, 0.05, 0.0, 0.0, 16, s17, nullptr, 0, false, false, npts), "16 selected states");
        const int32_t rep[3] = {2, 0, 2}, neg[3] = {2, -1, 1}, out[3] = {2, 3, 1};
        no(chim_check(fn, 2, 3, mesh, 2, q, 2, w, 0.05, 0.0, 0.0, 3, rep, nullptr, 0, false, false, npts), "a repeated state");
        no(chim_check(fn, 2, 3, mesh, 2, q, 2, w, 0.05, 0.0, 0.0, 3, neg, nullptr, 0, false, false, npts), "a negative state");
        no(chim_check(fn, 2, 3, mesh, 2, q, 2, w, 0.05, 0.0, 0.0, 3, out, nullptr, 0, false, false, npts), "a state beyond the last");
    }
    // the interaction
    no(chim_check(fn, 2, 3, mesh, 2, q, 2, w, 0.05, 0.0, 0.0, 3, sel, nullptr, 1, false, false, npts), "nvq without V");
    no(chim_check(fn, 2, 3, mesh, 2, q, 2, w, 0.05, 0.0, 0.0, 3, sel, nullptr, 0, true, false, npts), "chi_rpa without V");
    no(chim_check(fn, 2, 3, mesh, 2, q, 2, w, 0.05, 0.0, 0.0, 3, sel, nullptr, 0, false, true, npts), "det without V");
    no(chim_check(fn, 2, 3, mesh, 2, q, 2, w, 0.05, 0.0, 0.0, 3, sel, v.data(), 0, true, false, npts), "V with nvq = 0");
    no(chim_check(fn, 2, 3, mesh, 2, q, 2, w, 0.05, 0.0, 0.0, 3, sel, v.data(), 3, true, false, npts), "nvq = 3 for two q");
    no(chim_check(fn, 2, 3, mesh, 2, q, 2, w, 0.05, 0.0, 0.0, 3, sel, v.data(), 1, false, false, npts), "V without chi_rpa");
    for (double x : {nan, -inf}) {
        std::vector<double> vb = v;
        vb[2 * 9 + 7] = x;
        no(chim_check(fn, 2, 3, mesh, 2, q, 2, w, 0.05, 0.0, 0.0, 3, sel, vb.data(), 2, true, false, npts), "a V that is not finite");
        ok(chim_check(fn, 2, 3, mesh, 2, q, 2, w, 0.05, 0.0, 0.0, 3, sel, vb.data(), 1, true, false, npts), "(beyond the one matrix read)");
    }
    {
        // the cap nq max(nw, 1) na^2 <= 2^22: 1024 x 1024 x 2^2 is at it, 1025 q are over; static: 65536 x 8^2 at it, 9^2 over
        std::vector<double> qs(65536 * 2, 0.25), ws(1024, 0.5);
        int32_t s9[9];
        for (int i = 0; i < 9; ++i) s9[i] = i;
        ok(chim_check(fn, 2, 9, mesh, 1024, qs.data(), 1024, ws.data(), 0.05, 0.0, 0.0, 2, s9, nullptr, 0, false, false, npts), "at the cap");
        no(chim_check(fn, 2, 9, mesh, 1025, qs.data(), 1024, ws.data(), 0.05, 0.0, 0.0, 2, s9, nullptr, 0, false, false, npts), "over the cap");
        ok(chim_check(fn, 2, 9, mesh, 65536, qs.data(), 0, nullptr, 0.0, 0.0, 0.0, 8, s9, nullptr, 0, false, false, npts), "static at the cap");
        no(chim_check(fn, 2, 9, mesh, 65536, qs.data(), 0, nullptr, 0.0, 0.0, 0.0, 9, s9, nullptr, 0, false, false, npts), "static over the cap");
    }
    return bad;
}

int main() {
    int bad = 0, cases = 0;
    for (const Case& c : kCases) {
        bad |= check_case(c) ? 1 : 0;
        ++cases;
    }
    bad |= check_args() ? 1 : 0;
    if (bad) return printf("chim_plan_check: FAILED\n"), 1;
    printf("chim_plan_check: %d plans and the argument checks ok\n", cases);
    return 0;
}
