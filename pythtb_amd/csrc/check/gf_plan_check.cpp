// Stand-alone host check of tbk_gf.h (no device call): built under AddressSanitizer + UBSan by `make -C pythtb_amd/csrc gf-check` and
// run as an ordinary program.  Over a table of (n, dim_k, mesh, nw, nR, na, ns) it checks the plan of the Green's-function calls -- the
// chunk, the points per batch, the entries per lane, the tiles, the k-groups and the frequency and R tiles of a launch against the
// values worked out by hand, the part buffer against its cap, the LDS budget, the grid limits, that the launch tiles cover every
// (frequency, R) once, that the k-groups of every chunk (the last, shorter one included) cover its
// points once, and that nothing but the tiles, acc, part's size and the offsets behind them depends on nw, nR or na -- and the layout of
// the scratch block with the extra bytes of an impurity call (every buffer at a multiple of 256, in order, none overlapping; each
// is filled with its own index over a real host block and read back, under the sanitizer, where the block is at most 512 MiB).
// Then the internal problem of the impurity calls (the reduction modulo the mesh, the de-duplication, the index tables, the union
// of the states) on cases small enough to enumerate, the 64 x 64 map the caps must admit, and the argument checks: every rule, one
// bad value at a time.  It also replays the lane map of the lattice sum (tbk_lat.h: the functions k_lat_lds runs) for 1..32 states
// and every selection length, under the density matrix's and the Green's function's block sizes.
#include <cmath>
#include <limits>
#include <vector>
#include "../tbk_gf.h"
#include "check_common.h"

// ---------------------------------------------------------------- the plan
struct Case {
    int n, dk, mesh[3], nw, nR, na, ns;   // na = 0: all states
    // expected: points per chunk, points per batch (0: the tiled form), entries per lane, tiles per side, k-groups, frequencies and
    // lattice vectors per launch
    int64_t chunk;
    int P, ES, T, G, WT, RT;
};
static const Case kCases[] = {
    {1, 2, {7, 9, 1}, 1, 10, 0, 1, 63, 64, 1, 1, 1, 1, 10},                    // the ragged 63-point batch
    {1, 2, {7, 9, 1}, 5, 10, 0, 1, 63, 64, 1, 1, 1, 5, 10},                    // one frequency above the block
    {2, 2, {12, 10, 1}, 3, 9, 0, 3, 120, 64, 1, 1, 1, 3, 9},
    {2, 2, {256, 256, 1}, 256, 1, 0, 1, 65536, 64, 1, 1, 256, 256, 1},
    {2, 2, {256, 256, 1}, 16, 9, 0, 1, 65536, 64, 1, 1, 256, 16, 9},
    {2, 2, {256, 256, 1}, 16, 8191, 0, 1, 65536, 64, 1, 1, 256, 4, 1024},     // the 64 x 64 LDOS map: eight launches per block of four
    {2, 2, {256, 256, 1}, 65536, 1, 1, 1, 65536, 64, 1, 1, 256, 16384, 1},    // the most frequencies, one entry
    {8, 3, {32, 32, 32}, 256, 1, 0, 1, 32768, 22, 1, 1, 373, 172, 1},
    {8, 3, {32, 32, 32}, 16, 9, 0, 1, 32768, 22, 1, 1, 373, 16, 9},
    {16, 3, {3, 4, 5}, 5, 12, 0, 1, 60, 5, 1, 1, 3, 5, 12},
    {16, 3, {3, 4, 5}, 6, 7, 5, 1, 60, 5, 1, 1, 3, 6, 7},                      // a selection of 5: 25 entries, ten shares of the lanes
    {18, 2, {3, 2, 1}, 3, 10, 0, 1, 6, 4, 2, 2, 1, 3, 10},                     // 324 entries: two per lane
    {32, 2, {3, 2, 1}, 5, 10, 0, 1, 6, 1, 4, 2, 2, 5, 10},
    {32, 2, {46, 46, 1}, 2, 5, 0, 1, 2048, 1, 4, 2, 512, 1, 5},               // two chunks; 512 groups: a frequency per launch
    {32, 2, {64, 64, 1}, 256, 1, 0, 1, 2048, 1, 4, 2, 512, 8, 1},
    {32, 2, {48, 48, 1}, 1, 4096, 0, 1, 2048, 1, 4, 2, 512, 1, 8},            // nw nR na^2 at the cap; R tiles of 8
    {33, 1, {5, 1, 1}, 5, 10, 0, 1, 5, 0, 4, 3, 1, 5, 10},                     // the first tiled size
    {33, 1, {5, 1, 1}, 6, 7, 5, 3, 5, 0, 1, 1, 1, 6, 7},
    {40, 2, {37, 37, 1}, 2, 14, 0, 1, 1310, 0, 4, 3, 164, 1, 14},             // two chunks, a frequency per launch
    {512, 2, {2, 2, 1}, 16, 1, 0, 1, 4, 0, 4, 32, 1, 16, 1},                   // nw na^2 at the cap
    {512, 2, {2, 2, 1}, 100, 4, 32, 16, 4, 0, 4, 2, 1, 100, 4},                // one site's neighbourhood of a 512-state supercell
    {512, 2, {2, 2, 1}, 7, 40, 48, 16, 4, 0, 4, 3, 1, 7, 40},                  // the widest internal selection of an impurity call
    {2048, 1, {3, 1, 1}, 1, 1, 0, 1, 1, 0, 4, 128, 1, 1, 1},
};

static int check_case(const Case& c) {
    char tag[160];
    snprintf(tag, sizeof tag, "gf n=%d dk=%d mesh=%dx%dx%d nw=%d nR=%d na=%d ns=%d", c.n, c.dk, c.mesh[0], c.mesh[1], c.mesh[2], c.nw, c.nR,
             c.na, c.ns);
    const int64_t npts = (int64_t)c.mesh[0] * c.mesh[1] * c.mesh[2], nn = (int64_t)c.n * c.n;
    const int na = c.na ? c.na : c.n;
    const int64_t nab = (int64_t)na * na;
    const GfImpLayout lay = gf_imp_layout(c.ns, c.nw, c.nR, std::min(na, kGfSelMax));
    const GfPlan p = gf_plan(c.n, c.dk, npts, c.nw, c.nR, na, lay.total);
    if (p.chunk != c.chunk || (p.lds ? p.P : 0) != c.P || p.ES != c.ES || p.T != c.T || p.G != c.G || p.WT != c.WT || p.RT != c.RT)
        return printf("%s: chunk %lld P %d ES %d T %d G %d WT %d RT %d\n", tag, (long long)p.chunk, p.lds ? p.P : 0, p.ES, p.T, p.G, p.WT, p.RT);
    if (p.lds != (c.n <= 32) || p.na != na || p.nab != nab) return printf("%s: lds / na\n", tag);
    if (p.chunk < 1 || p.chunk > npts || (size_t)p.chunk * nn * sizeof(cd) > std::max(kKuboChunkBytes, (size_t)nn * sizeof(cd)))
        return printf("%s: the chunk holds more than kKuboChunkBytes of eigenvectors\n", tag);
    if (p.nchunks != (npts + p.chunk - 1) / p.chunk) return printf("%s: nchunks\n", tag);
    if (p.G < 1 || p.G > kGfGroupsMax || p.G > p.chunk) return printf("%s: G=%d\n", tag, p.G);
    if (p.WT < 1 || p.WT > c.nw || p.RT < 1 || p.RT > c.nR) return printf("%s: WT=%d RT=%d\n", tag, p.WT, p.RT);
    if (p.RT != c.nR && p.WT > GF_WB) return printf("%s: tiles of lattice vectors with more than a block of frequencies\n", tag);
    if (p.WT < c.nw && p.WT >= GF_WB && p.WT % GF_WB) return printf("%s: WT=%d splits a block of frequencies\n", tag, p.WT);
    if (p.RT < c.nR && p.RT >= GF_RB && p.RT % GF_RB) return printf("%s: RT=%d splits a block of lattice vectors\n", tag, p.RT);
    if (p.part_cd != (int64_t)p.G * p.WT * p.RT * nab || p.part_cd > std::max(kGfPartCap, nab)) return printf("%s: part over the cap\n", tag);
    if (p.acc_cd != (int64_t)c.nw * c.nR * nab) return printf("%s: acc\n", tag);
    if (p.lds) {
        if (na > kGfSelMax) return printf("%s: %d selected states do not fit the LDS kernel's table\n", tag, na);
        if ((int64_t)p.P * c.n * na > OCC_LDS_CD || p.P * c.n > OCC_LDS_PN || p.P > 64) return printf("%s: %d points do not fit the LDS\n", tag, p.P);
        if ((int64_t)256 * p.ES < nab) return printf("%s: %d entries per lane do not cover na^2\n", tag, p.ES);
        const size_t lds = (size_t)OCC_LDS_CD * sizeof(cd) + (size_t)OCC_LDS_PN * (GF_WB + 1) * sizeof(cd) + (size_t)64 * GF_RB * sizeof(cd) +
                           kGfSelMax * sizeof(int);
        if (lds > 65536) return printf("%s: %zu bytes of LDS\n", tag, lds);
    } else {
        if (p.T != (na + 15) / 16) return printf("%s: T=%d\n", tag, p.T);
    }
    // the grid: (blocks of frequencies and lattice vectors) x tiles in x, the k-groups in y
    const int64_t gx = (int64_t)((p.WT + GF_WB - 1) / GF_WB) * ((p.RT + GF_RB - 1) / GF_RB) * (p.lds ? 1 : (int64_t)p.T * p.T);
    if (gx > 2147483647 || p.G > 65535) return printf("%s: the grid\n", tag);
    // the launch tiles cover every (frequency, R) once
    {
        std::vector<unsigned char> seen((size_t)c.nw * c.nR, 0);
        for (int w0 = 0; w0 < c.nw; w0 += p.WT)
            for (int r0 = 0; r0 < c.nR; r0 += p.RT)
                for (int w = w0; w < std::min(c.nw, w0 + p.WT); ++w)
                    for (int r = r0; r < std::min(c.nR, r0 + p.RT); ++r) ++seen[(size_t)w * c.nR + r];
        for (unsigned char s : seen)
            if (s != 1) return printf("%s: the launch tiles do not cover every (frequency, R) once\n", tag);
    }
    // the k-groups of a full chunk and of the last one cover the points once, in order
    if (check_groups(tag, p.G, npts, p.chunk, p.nchunks)) return 1;
    // a frequency, an R, a selection of one state alone is worked through with the same chunk, batch and groups
    const GfPlan one = gf_plan(c.n, c.dk, npts, 1, 1, 1, 0);
    if (one.chunk != p.chunk || one.P != p.P || one.G != p.G || one.cw.bytes() != p.cw.bytes()) return printf("%s: the plan depends on nw, nR or na\n", tag);
    const GfPlan same = gf_plan(c.n, c.dk, npts, 1, 1, na, 0);
    if (same.ES != p.ES || same.T != p.T) return printf("%s: the lane mapping depends on nw or nR\n", tag);
    const size_t D = sizeof(double), cb = p.off_chunks, x = p.off_x;
    const int np = std::min(na, kGfSelMax);
    const size_t buf[][2] = {
        {p.off_om, (size_t)c.nw * D},
        {p.off_R, (size_t)c.nR * c.dk * sizeof(int32_t)},
        {p.off_sel, (size_t)na * sizeof(int32_t)},
        {p.off_acc, (size_t)p.acc_cd * sizeof(cd)},
        {p.off_part, (size_t)p.part_cd * sizeof(cd)},
        {x + lay.off_v, (size_t)c.ns * c.ns * sizeof(cd)},
        {x + lay.off_tab, lay.tab_ints * sizeof(int32_t)},
        {x + lay.off_t, (size_t)c.nw * c.ns * c.ns * sizeof(cd)},
        {x + lay.off_det, (size_t)c.nw * sizeof(cd)},
        {x + lay.off_flag, (size_t)c.nw * sizeof(int32_t)},
        {x + lay.off_ldos0, (size_t)c.nw * np * D},
        {x + lay.off_dldos, (size_t)c.nw * c.nR * np * D},
        {cb + p.cw.off[0], (size_t)p.chunk * c.dk * D},
        {cb + p.cw.off[1], (size_t)p.chunk * c.n * D},
        {cb + p.cw.off[2], (size_t)p.chunk * nn * sizeof(cd)},
    };
    if (lay.tab_ints != (size_t)c.ns + (size_t)c.ns * c.ns + 2 * (size_t)c.nR * c.ns) return printf("%s: the tables\n", tag);
    return check_buffers(tag, buf, (int)(sizeof buf / sizeof buf[0]), p.total);
}

// ---------------------------------------------------------------- the lane map of k_lat_lds (tbk_lat.h), replayed
// n states of which na are kept, WB x RB accumulators per entry, weights of wbytes: every share of every entry has one (lane, slot);
// the shares cover the points of a full and of a ragged batch once; every LDS index the frame forms lies inside its array -- U
// [OCC_LDS_CD], the weights [OCC_LDS_PN][WB], the orbital phases [OCC_LDS_PN], the lattice phases [64][RB], the selection -- and the
// share buffer (256 c128, over U) fits
static int check_lane_map(int n, int na, int WB, int RB, size_t wbytes, size_t lds_max) {
    char tag[96];
    snprintf(tag, sizeof tag, "lanes n=%d na=%d WB=%d RB=%d", n, na, WB, RB);
    const int nab = na * na, ns = n * na, ES = lat_entries_per_lane(nab), P = lat_points(n);
    const LatLane l0 = lat_lane(ES, nab, 0);
    if (na > kGfSelMax || 256 * ES < nab || l0.Q < 1 || (ES == 1 && l0.Q * nab > 256) || 256 > OCC_LDS_CD) return printf("%s: ES=%d Q=%d\n", tag, ES, l0.Q);
    const size_t lds = (size_t)OCC_LDS_CD * sizeof(cd) + (size_t)OCC_LDS_PN * (WB * wbytes + sizeof(cd)) + (size_t)64 * RB * sizeof(cd);
    if (lds > lds_max) return printf("%s: %zu bytes of LDS\n", tag, lds);
    if (P < 1 || P > 64 || P * ns > OCC_LDS_CD || P * n > OCC_LDS_PN || (P * n - 1) * WB + WB - 1 >= OCC_LDS_PN * WB || (P - 1) * RB + RB - 1 >= 64 * RB)
        return printf("%s: a batch of %d points does not fit the LDS\n", tag, P);
    for (int np : {P, std::max(1, P - 1), 1}) {
        std::vector<int> own((size_t)nab * np, 0);                 // (entry, point) -> the lanes that take it
        for (int t = 0; t < 256; ++t) {
            const LatLane l = lat_lane(ES, nab, t);
            if (l.Q != l0.Q || (ES == 1 && l.live && l.q * nab + l.el0 != t)) return printf("%s: lane %d\n", tag, t);
            if (!l.live) continue;
            for (int s = 0; s < ES; ++s) {
                const int el = l.el0 + 256 * s;
                if (el >= nab) continue;
                int i, j;
                lat_entry(el, na, i, j);
                if (i < 0 || i >= na || j < 0 || j >= na || i * na + j != el) return printf("%s: entry %d is (%d, %d)\n", tag, el, i, j);
                for (int p = l.q; p < np; p += l.Q) {
                    if (p * ns + (n - 1) * na + std::max(i, j) >= OCC_LDS_CD) return printf("%s: lane %d reads beyond U\n", tag, t);
                    ++own[(size_t)el * np + p];
                }
                if (l.Q > 1 && (l.q * nab + el >= 256 || t != l.q * nab + el)) return printf("%s: the share of lane %d\n", tag, t);
            }
        }
        for (int o : own)
            if (o != 1) return printf("%s: an (entry, point) of a batch of %d is taken %d times\n", tag, np, o);
    }
    return 0;
}
static int check_lane_maps() {
    for (int n = 1; n <= 32; ++n) {
        if (check_lane_map(n, n, 1, OCC_RB, sizeof(double), 32768)) return 1;     // the density matrix: a fifth of a CU's 160 KiB
        for (int na = 1; na <= n; ++na)
            if (check_lane_map(n, na, GF_WB, GF_RB, sizeof(cd), 65536 - kGfSelMax * sizeof(int))) return 1;
    }
    return 0;
}

// ---------------------------------------------------------------- the internal problem of the impurity calls
static int check_impurity() {
    int bad = 0;
    {   // two sites of a 3-state chain on a mesh of 7; probes at -1, 0, 8 (= 1 mod 7), probe states (2, 0)
        const int32_t mesh[1] = {7}, st[2] = {1, 0}, Rs[2] = {0, 3}, Rp[3] = {-1, 0, 8}, probe[2] = {2, 0};
        const GfImpurity g = gf_impurity_build(1, mesh, 2, st, Rs, 3, Rp, 2, probe);
        const int32_t sel[3] = {2, 0, 1};                          // the probes, then the site state not among them
        if (g.na != 3 || memcmp(g.sel.data(), sel, sizeof sel)) bad |= printf("impurity: the union of the states\n");
        if (g.pos_site[0] != 2 || g.pos_site[1] != 1 || g.pos_probe[0] != 0 || g.pos_probe[1] != 1) bad |= printf("impurity: the places\n");
        auto at = [&](int r) {
            r = ((r % 7) + 7) % 7;
            for (int i = 0; i < g.nR; ++i)
                if (g.R[i] == r) return i;
            return -1;
        };
        if (g.R[0] != 0) bad |= printf("impurity: index 0 is not R = 0\n");
        for (int i = 0; i < g.nR; ++i)
            for (int j = 0; j < i; ++j)
                if (g.R[i] == g.R[j]) bad |= printf("impurity: a lattice vector is kept twice\n");
        for (int i = 0; i < g.nR; ++i)
            if (g.R[i] < 0 || g.R[i] >= 7) bad |= printf("impurity: a lattice vector is not reduced\n");
        for (int a = 0; a < 2; ++a)
            for (int b = 0; b < 2; ++b)
                if (g.pair[a * 2 + b] != at(Rs[b] - Rs[a]) || g.pair[a * 2 + b] < 0) bad |= printf("impurity: pair (%d, %d)\n", a, b);
        for (int r = 0; r < 3; ++r)
            for (int b = 0; b < 2; ++b)
                if (g.out[r * 2 + b] != at(Rs[b] - Rp[r]) || g.in[r * 2 + b] != at(Rp[r] - Rs[b]) || g.out[r * 2 + b] < 0 || g.in[r * 2 + b] < 0)
                    bad |= printf("impurity: probe %d, site %d\n", r, b);
        if (g.nR > 7) bad |= printf("impurity: %d lattice vectors on a torus of 7 cells\n", g.nR);
        if (gf_impurity_caps("check", g, 65536, 65536 * 6) != TBK_OK) bad |= printf("impurity: the small case is refused\n");
    }
    {   // the map the caps must admit: 64 x 64 cells around one site of a 2-state model on 256 x 256, at 16 frequencies
        const int32_t mesh[2] = {256, 256}, st[1] = {0}, Rs[2] = {0, 0}, probe[2] = {0, 1};
        std::vector<int32_t> Rp;
        for (int a = 0; a < 64; ++a)
            for (int b = 0; b < 64; ++b) Rp.push_back(a), Rp.push_back(b);
        const GfImpurity g = gf_impurity_build(2, mesh, 1, st, Rs, 4096, Rp.data(), 2, probe);
        if (g.nR != 8191 || g.na != 2) bad |= printf("impurity: the 64 x 64 map has %d lattice vectors, %d states\n", g.nR, g.na);
        if (gf_impurity_caps("check", g, 16, (int64_t)16 * 4096 * 2) != TBK_OK) bad |= printf("impurity: the 64 x 64 map at 16 frequencies is refused\n");
        if (gf_impurity_caps("check", g, 300, (int64_t)300 * 4096 * 2) != TBK_EINVAL) bad |= printf("impurity: 300 frequencies of the map are accepted\n");
        // the same map on a mesh of 32 x 32: the differences fold onto the 1024 cells of the torus
        const int32_t small[2] = {32, 32};
        const GfImpurity f = gf_impurity_build(2, small, 1, st, Rs, 4096, Rp.data(), 2, probe);
        if (f.nR != 1024) bad |= printf("impurity: %d lattice vectors on a torus of 1024 cells\n", f.nR);
        for (int r = 0; r < 4096; ++r) {
            const int32_t* o = &f.R[(size_t)f.out[r] * 2];
            const int32_t* i = &f.R[(size_t)f.in[r] * 2];
            if (o[0] != ((-Rp[2 * r]) % 32 + 32) % 32 || o[1] != ((-Rp[2 * r + 1]) % 32 + 32) % 32 || i[0] != Rp[2 * r] % 32 || i[1] != Rp[2 * r + 1] % 32) {
                bad |= printf("impurity: probe %d of the folded map\n", r);
                break;
            }
        }
    }
    {   // more internal lattice vectors than kGfIntRMax: a line of 4096 probes against 16 sites far apart
        const int32_t mesh[1] = {1 << 20};
        std::vector<int32_t> st(16, 0), Rs(16), Rp(4096), probe(1, 0);
        for (int a = 0; a < 16; ++a) Rs[a] = a * 10000;
        for (int r = 0; r < 4096; ++r) Rp[r] = r;
        const GfImpurity g = gf_impurity_build(1, mesh, 16, st.data(), Rs.data(), 4096, Rp.data(), 1, probe.data());
        if (g.nR <= kGfIntRMax) bad |= printf("impurity: %d lattice vectors where more than %d were meant\n", g.nR, kGfIntRMax);
        if (gf_impurity_caps("check", g, 1, 4096) != TBK_EINVAL) bad |= printf("impurity: %d internal lattice vectors are accepted\n", g.nR);
    }
    return bad;
}

// ---------------------------------------------------------------- the argument checks
static int check_args() {
    const char* fn = "gf_plan_check";
    const int32_t mesh[3] = {4, 5, 6};
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    int64_t npts = 0;
    int na = 0, bad = 0;
    auto ok = [&](int rc, const char* what) {
        if (rc != TBK_OK) bad |= printf("refused: %s\n", what);
    };
    auto no = [&](int rc, const char* what) {
        if (rc != TBK_EINVAL) bad |= printf("accepted: %s\n", what);
    };
    const double om[3] = {0.5, -1.0, 0.5};
    const int32_t R[6] = {0, 0, 1, -1, 1073741823, -1073741823};
    const int32_t sel[3] = {2, 0, 1};
    ok(gf_green_check(fn, 2, 3, mesh, 3, om, 0.05, 3, R, 0, nullptr, npts, na), "three frequencies, three lattice vectors, all states");
    if (npts != 20 || na != 3) bad |= printf("npts=%lld na=%d\n", (long long)npts, na);
    ok(gf_green_check(fn, 3, 3, mesh, 3, om, 0.05, 2, R, 3, sel, npts, na), "a 3-D mesh and a selection");
    no(gf_green_check(fn, 0, 3, mesh, 3, om, 0.05, 3, R, 0, nullptr, npts, na), "dim_k = 0");
    no(gf_green_check(fn, 4, 3, mesh, 3, om, 0.05, 3, R, 0, nullptr, npts, na), "dim_k = 4");
    no(gf_green_check(fn, 2, 2049, mesh, 3, om, 0.05, 3, R, 0, nullptr, npts, na), "2049 states");
    {
        const int32_t mb[3] = {4, 0, 6}, huge[3] = {65536, 32768, 1};
        no(gf_green_check(fn, 2, 3, mb, 3, om, 0.05, 3, R, 0, nullptr, npts, na), "a mesh axis of 0 points");
        no(gf_green_check(fn, 2, 3, huge, 3, om, 0.05, 3, R, 0, nullptr, npts, na), "2^31 mesh points");
    }
    no(gf_green_check(fn, 2, 3, mesh, 0, om, 0.05, 3, R, 0, nullptr, npts, na), "no frequency");
    no(gf_green_check(fn, 2, 3, mesh, 3, nullptr, 0.05, 3, R, 0, nullptr, npts, na), "no frequency array");
    {
        std::vector<double> many(65537, 0.25);
        ok(gf_green_check(fn, 2, 1, mesh, 65536, many.data(), 0.05, 1, R, 0, nullptr, npts, na), "65536 frequencies");
        no(gf_green_check(fn, 2, 1, mesh, 65537, many.data(), 0.05, 1, R, 0, nullptr, npts, na), "65537 frequencies");
        const double wb[3] = {0.5, nan, 0.1}, wi[3] = {0.5, 0.1, -inf};
        no(gf_green_check(fn, 2, 3, mesh, 3, wb, 0.05, 3, R, 0, nullptr, npts, na), "a NaN frequency");
        no(gf_green_check(fn, 2, 3, mesh, 3, wi, 0.05, 3, R, 0, nullptr, npts, na), "an infinite frequency");
    }
    for (double eta : {0.0, -1e-3, nan, inf}) no(gf_green_check(fn, 2, 3, mesh, 3, om, eta, 3, R, 0, nullptr, npts, na), "a bad eta");
    no(gf_green_check(fn, 2, 3, mesh, 3, om, 0.05, 0, R, 0, nullptr, npts, na), "nR = 0");
    no(gf_green_check(fn, 2, 3, mesh, 3, om, 0.05, 3, nullptr, 0, nullptr, npts, na), "no R list");
    {
        const int32_t big[4] = {0, 0, 1073741824, 0}, neg[4] = {0, -1073741824, 0, 0};
        no(gf_green_check(fn, 2, 3, mesh, 3, om, 0.05, 2, big, 0, nullptr, npts, na), "a component of 2^30");
        no(gf_green_check(fn, 2, 3, mesh, 3, om, 0.05, 2, neg, 0, nullptr, npts, na), "a component of -2^30");
        std::vector<int32_t> many((size_t)4097 * 2, 1);
        ok(gf_green_check(fn, 2, 3, mesh, 1, om, 0.05, 4096, many.data(), 0, nullptr, npts, na), "4096 lattice vectors");
        no(gf_green_check(fn, 2, 3, mesh, 1, om, 0.05, 4097, many.data(), 0, nullptr, npts, na), "4097 lattice vectors");
        std::vector<double> w(257, 0.1);
        ok(gf_green_check(fn, 2, 2, mesh, 256, w.data(), 0.05, 4096, many.data(), 0, nullptr, npts, na), "nw nR na^2 at the cap");
        no(gf_green_check(fn, 2, 2, mesh, 257, w.data(), 0.05, 4096, many.data(), 0, nullptr, npts, na), "nw nR na^2 over the cap");
        ok(gf_green_check(fn, 2, 512, mesh, 16, w.data(), 0.05, 1, many.data(), 0, nullptr, npts, na), "16 matrices of 512 states");
        no(gf_green_check(fn, 2, 512, mesh, 17, w.data(), 0.05, 1, many.data(), 0, nullptr, npts, na), "17 matrices of 512 states");
        ok(gf_green_check(fn, 2, 2048, mesh, 1, w.data(), 0.05, 1, many.data(), 0, nullptr, npts, na), "one matrix of 2048 states");
        no(gf_green_check(fn, 2, 2048, mesh, 2, w.data(), 0.05, 1, many.data(), 0, nullptr, npts, na), "two matrices of 2048 states");
    }
    {   // the selection
        std::vector<int32_t> s33(33);
        for (int i = 0; i < 33; ++i) s33[i] = i;
        ok(gf_sel_check(fn, 512, 32, s33.data(), na), "32 selected states");
        if (na != 32) bad |= printf("na=%d\n", na);
        no(gf_sel_check(fn, 512, 33, s33.data(), na), "33 selected states");
        no(gf_sel_check(fn, 512, 0, s33.data(), na), "an empty selection");
        no(gf_sel_check(fn, 512, 2, nullptr, na), "a count without a selection");
        const int32_t twice[3] = {4, 1, 4}, out[2] = {0, 3}, neg[2] = {0, -1};
        no(gf_sel_check(fn, 8, 3, twice, na), "a state selected twice");
        no(gf_sel_check(fn, 3, 2, out, na), "a state beyond the last");
        no(gf_sel_check(fn, 3, 2, neg, na), "a negative state");
    }
    {   // the sites and the potential
        const int32_t st[3] = {0, 2, 0}, Rs[6] = {0, 0, 1, 0, -1, 2};
        const double V[18] = {1.0, 0.0, 0.2, 0.3, 0.0, -0.1, 0.2, -0.3, -0.5, 0.0, 0.4, 0.0, 0.0, 0.1, 0.4, 0.0, 0.7, 0.0};
        ok(gf_sites_check(fn, 2, 3, mesh, 3, st, Rs, V), "three sites, a Hermitian potential");
        no(gf_sites_check(fn, 2, 3, mesh, 0, st, Rs, V), "no site");
        no(gf_sites_check(fn, 2, 3, mesh, 3, nullptr, Rs, V), "no site states");
        no(gf_sites_check(fn, 2, 3, mesh, 3, st, nullptr, V), "no site vectors");
        no(gf_sites_check(fn, 2, 3, mesh, 3, st, Rs, nullptr), "no potential");
        no(gf_sites_check(fn, 2, 2, mesh, 3, st, Rs, V), "a site state beyond the last");
        const int32_t same[6] = {0, 0, 1, 0, 4, -5}, far[6] = {0, 0, 1, 0, 1073741824, 2};
        no(gf_sites_check(fn, 2, 3, mesh, 3, st, same, V), "two sites that coincide modulo the mesh");
        no(gf_sites_check(fn, 2, 3, mesh, 3, st, far, V), "a site vector of 2^30");
        double W[18];
        memcpy(W, V, sizeof W);
        W[3] = 0.31;
        no(gf_sites_check(fn, 2, 3, mesh, 3, st, Rs, W), "a potential that is not Hermitian");
        memcpy(W, V, sizeof W);
        W[9] = 1e-3;
        no(gf_sites_check(fn, 2, 3, mesh, 3, st, Rs, W), "a diagonal entry with an imaginary part");
        memcpy(W, V, sizeof W);
        W[0] = nan;
        no(gf_sites_check(fn, 2, 3, mesh, 3, st, Rs, W), "a NaN in the potential");
        std::vector<int32_t> s17(17, 0), r17(34, 0);
        for (int a = 0; a < 17; ++a) r17[2 * a] = a % 4, r17[2 * a + 1] = a / 4;
        std::vector<double> v17((size_t)2 * 17 * 17, 0.0);
        ok(gf_sites_check(fn, 2, 3, mesh, 16, s17.data(), r17.data(), v17.data()), "16 sites");
        no(gf_sites_check(fn, 2, 3, mesh, 17, s17.data(), r17.data(), v17.data()), "17 sites");
    }
    return bad;
}

int main() {
    int bad = 0, cases = 0;
    for (const Case& c : kCases) {
        bad |= check_case(c) ? 1 : 0;
        ++cases;
    }
    bad |= check_lane_maps() ? 1 : 0;
    bad |= check_impurity() ? 1 : 0;
    bad |= check_args() ? 1 : 0;
    if (bad) return printf("gf_plan_check: FAILED\n"), 1;
    printf("gf_plan_check: %d plans, the lane map of the lattice sum for 1..32 states, the internal problem of the impurity calls and the argument checks ok\n", cases);
    return 0;
}
