// Stand-alone host check of tbk_occ.h (no device call): built under AddressSanitizer + UBSan by `make -C pythtb_amd/csrc occ-check`
// and run as an ordinary program.  It checks the ordered key of a double (order, round trip, the 64-step bound of the bisection on
// it, replayed on the host against a sorted list); over a table of (n, dim_k, mesh, nR) the plan of tbk_density_matrix_mesh -- the
// chunk, the points per batch, the elements per lane, the k-groups and the R tiles against the values worked out by hand, the part
// buffer against its cap, the LDS budget, the grid limits, that the k-groups of every chunk (the last, shorter one included) cover
// its points once, and that nothing but acc, part's size and the offsets behind them depends on nR -- and the plans of the level scans
// (thermodynamics at kT = 0 and kT > 0, the Fermi selection); the layout of every scratch block (every buffer at a multiple of 256,
// in order, none overlapping, the last one ending at the total; each is filled with its own index over a real host block and read
// back, under the sanitizer, where the block is at most 512 MiB).  Then the argument checks: every rule, one bad value at a time.
#include <cmath>
#include <limits>
#include <vector>
#include "../tbk_occ.h"
#include "check_common.h"

// ---------------------------------------------------------------- the key and the bisection on it
static int check_key() {
    const double inf = std::numeric_limits<double>::infinity();
    const double v[] = {-DBL_MAX, -1e300, -2.5, -1.0, -DBL_MIN, -4.9e-324, -0.0, 0.0, 4.9e-324, DBL_MIN, 0.3, 1.0, 1.0 + DBL_EPSILON, 7e22, DBL_MAX};
    const int nv = (int)(sizeof v / sizeof v[0]);
    for (int i = 0; i < nv; ++i) {
        const double back = occ_unkey(occ_key(v[i]));
        if (memcmp(&back, &v[i], sizeof back)) return printf("key: %g does not come back\n", v[i]);
        if (i && !(occ_key(v[i - 1]) < occ_key(v[i]))) return printf("key: %g and %g are out of order\n", v[i - 1], v[i]);
    }
    if (!(occ_key(-inf) < occ_key(-DBL_MAX) && occ_key(DBL_MAX) < occ_key(inf))) return printf("key: the infinities\n");
    // the selection as k_occ_bisect runs it, on the host: the c-th smallest of a list with repeats, for every c
    std::vector<double> lev = {-3.0, -3.0, -1.25, -0.0, 0.0, 1e-300, 0.5, 0.5, 0.5, 2.0, 1e17};
    for (size_t c = 1; c <= lev.size(); ++c) {
        uint64_t a = occ_key(-DBL_MAX), b = occ_key(DBL_MAX);
        for (int step = 0; step < kOccSteps; ++step) {
            const uint64_t mid = a + (b - a) / 2;
            const double mu = occ_unkey(mid);
            size_t cnt = 0;
            for (double e : lev) cnt += e <= mu;
            if (b - a > 1) (cnt >= c ? b : a) = mid;
        }
        if (b - a != 1) return printf("bisection: the bracket of c=%zu is %llu keys wide after %d steps\n", c, (unsigned long long)(b - a), kOccSteps);
        if (occ_unkey(b) != lev[c - 1]) return printf("bisection: c=%zu ends on %g, not %g\n", c, occ_unkey(b), lev[c - 1]);
    }
    return 0;
}

// ---------------------------------------------------------------- the density-matrix plan
struct Case {
    int n, dk, mesh[3], nR;
    // expected: points per chunk, points per batch (0: the tiled form), elements per lane, k-groups, lattice vectors per launch
    int64_t chunk;
    int P, ES, G, RT;
};
static const Case kCases[] = {
    {1, 2, {7, 9, 1}, 10, 63, 64, 1, 1, 4096},
    {1, 2, {2048, 2048, 1}, 1, 2097152, 64, 1, 512, 4096},
    {2, 2, {12, 10, 1}, 9, 120, 64, 1, 1, 4096},
    {2, 2, {13, 5, 1}, 4096, 65, 64, 1, 1, 4096},
    {2, 2, {256, 256, 1}, 7, 65536, 64, 1, 256, 4096},
    {3, 1, {41, 1, 1}, 6, 41, 64, 1, 1, 4096},
    {4, 2, {6, 7, 1}, 10, 42, 64, 1, 1, 4096},
    {5, 2, {64, 64, 1}, 3, 4096, 51, 1, 21, 4096},
    {8, 3, {32, 32, 32}, 64, 32768, 22, 1, 373, 172},
    {16, 3, {3, 4, 5}, 12, 60, 5, 1, 3, 4096},
    {17, 1, {100, 1, 1}, 2, 100, 4, 2, 7, 2072},
    {23, 1, {100, 1, 1}, 2, 100, 2, 4, 13, 608},
    {32, 2, {3, 2, 1}, 10, 6, 1, 4, 2, 2048},
    {32, 2, {48, 48, 1}, 4096, 2048, 1, 4, 512, 8},
    {33, 1, {5, 1, 1}, 6, 5, 0, 4, 1, 3848},
    {40, 2, {37, 37, 1}, 4, 1310, 0, 4, 164, 12},
    {512, 2, {2, 2, 1}, 16, 4, 0, 4, 1, 16},
    {2048, 1, {3, 1, 1}, 1, 1, 0, 4, 1, 1},
};

static int check_dm_case(const Case& c) {
    char tag[128];
    snprintf(tag, sizeof tag, "dm n=%d dk=%d mesh=%dx%dx%d nR=%d", c.n, c.dk, c.mesh[0], c.mesh[1], c.mesh[2], c.nR);
    const int64_t npts = (int64_t)c.mesh[0] * c.mesh[1] * c.mesh[2], nn = (int64_t)c.n * c.n;
    const OccDmPlan p = occ_dm_plan(c.n, c.dk, npts, c.nR);
    if (p.chunk != c.chunk || (p.lds ? p.P : 0) != c.P || p.ES != c.ES || p.G != c.G || p.RT != c.RT)
        return printf("%s: chunk %lld P %d ES %d G %d RT %d\n", tag, (long long)p.chunk, p.lds ? p.P : 0, p.ES, p.G, p.RT);
    if (p.lds != (c.n <= 32)) return printf("%s: lds\n", tag);
    if (p.chunk < 1 || p.chunk > npts || (size_t)p.chunk * nn * sizeof(cd) > std::max(kKuboChunkBytes, (size_t)nn * sizeof(cd)))
        return printf("%s: the chunk holds more than kKuboChunkBytes of eigenvectors\n", tag);
    if (p.nchunks != (npts + p.chunk - 1) / p.chunk) return printf("%s: nchunks\n", tag);
    if (p.G < 1 || p.G > kOccGroupsMax || p.G > p.chunk) return printf("%s: G=%d\n", tag, p.G);
    if (p.RT < 1 || p.RT > kOccRMax || (p.RT >= OCC_RB && p.RT % OCC_RB)) return printf("%s: RT=%d\n", tag, p.RT);
    if ((int64_t)p.G * p.RT * nn > std::max(kOccPartCap, nn)) return printf("%s: part of a launch is over the cap\n", tag);
    if (p.part_cd != (int64_t)p.G * std::min(p.RT, c.nR) * nn || p.acc_cd != (int64_t)c.nR * nn) return printf("%s: part / acc\n", tag);
    if (p.lds) {
        if ((int64_t)p.P * nn > OCC_LDS_CD || p.P * c.n > OCC_LDS_PN || p.P > 64) return printf("%s: %d points do not fit the LDS\n", tag, p.P);
        if ((int64_t)256 * p.ES < nn) return printf("%s: %d elements per lane do not cover n^2\n", tag, p.ES);
        if (OCC_RB * 256 > OCC_LDS_CD) return printf("%s: the shares of the lanes do not fit the LDS\n", tag);
        const size_t lds = (size_t)OCC_LDS_CD * sizeof(cd) + (size_t)OCC_LDS_PN * (sizeof(cd) + sizeof(double)) + (size_t)64 * OCC_RB * sizeof(cd);
        if (lds > 32768) return printf("%s: %zu bytes of LDS\n", tag, lds);
    } else {
        if (p.T != (c.n + 15) / 16 || (int64_t)p.T * p.T > 2147483647) return printf("%s: T=%d\n", tag, p.T);
    }
    // the grid: the k-groups in x, the blocks of lattice vectors (times the tiles) in y
    if ((int64_t)((p.RT + OCC_RB - 1) / OCC_RB) * (p.lds ? 1 : p.T * p.T) > 65535 || p.G > 65535) return printf("%s: the grid\n", tag);
    // the k-groups of a full chunk and of the last one cover the points once, in order
    if (check_groups(tag, p.G, npts, p.chunk, p.nchunks)) return 1;
    // an R alone is worked through like the same R inside this list
    const OccDmPlan one = occ_dm_plan(c.n, c.dk, npts, 1);
    if (one.chunk != p.chunk || one.P != p.P || one.ES != p.ES || one.T != p.T || one.G != p.G || one.RT != p.RT || one.cw.bytes() != p.cw.bytes())
        return printf("%s: the plan depends on nR\n", tag);
    const size_t D = sizeof(double), cb = p.off_chunks;
    const size_t buf[][2] = {
        {p.off_R, (size_t)c.nR * c.dk * sizeof(int32_t)},
        {p.off_acc, (size_t)p.acc_cd * sizeof(cd)},
        {p.off_part, (size_t)p.part_cd * sizeof(cd)},
        {cb + p.cw.off[0], (size_t)p.chunk * c.dk * D},
        {cb + p.cw.off[1], (size_t)p.chunk * c.n * D},
        {cb + p.cw.off[2], (size_t)p.chunk * nn * sizeof(cd)},
        {cb + p.cw.off[3], (size_t)p.chunk * c.n * D},
    };
    return check_buffers(tag, buf, (int)(sizeof buf / sizeof buf[0]), p.total);
}

// ---------------------------------------------------------------- the plans of the level scans
static int check_scan(int n, int dk, int64_t npts, int nmu, bool thermal, bool fermi, int G, int gx) {
    char tag[128];
    snprintf(tag, sizeof tag, "scan n=%d dk=%d npts=%lld nmu=%d thermal=%d fermi=%d", n, dk, (long long)npts, nmu, thermal, fermi);
    const OccScanPlan p = occ_scan_plan(n, dk, npts, nmu, thermal, fermi);
    if (p.G != G || p.gx != gx) return printf("%s: G %d gx %d\n", tag, p.G, p.gx);
    if (p.nlev != npts * n || p.G < 1 || p.G > kOccScanGroupsMax || p.G > p.nlev) return printf("%s: G=%d\n", tag, p.G);
    if (p.nq != (fermi ? 1 : (thermal ? 3 : 2)) || p.nrows != (int64_t)nmu * p.nq) return printf("%s: rows\n", tag);
    int64_t at = 0;
    for (int g = 0; g < p.G; ++g) {
        const int64_t l0 = (int64_t)g * p.nlev / p.G, l1 = (int64_t)(g + 1) * p.nlev / p.G;
        if (l0 != at || l1 < l0) return printf("%s: group %d starts at %lld\n", tag, g, (long long)l0);
        at = l1;
    }
    if (at != p.nlev) return printf("%s: the groups end at %lld of %lld levels\n", tag, (long long)at, (long long)p.nlev);
    // the groups do not depend on the number of levels or fillings
    if (occ_scan_plan(n, dk, npts, 1, thermal, fermi).G != p.G) return printf("%s: G depends on nmu\n", tag);
    const size_t D = sizeof(double);
    const size_t want_part = fermi ? (size_t)2 * nmu * p.G : (size_t)p.nrows * (thermal ? p.G : p.gx);
    if ((size_t)p.part_doubles != want_part) return printf("%s: part\n", tag);
    if (fermi) {
        const size_t buf[][2] = {{p.off_k, (size_t)npts * dk * D}, {p.off_e, (size_t)p.nlev * D}, {p.off_part, want_part * D},
                                 {p.off_rows, (size_t)p.nrows * D}, {p.off_mu, (size_t)nmu * D}, {p.off_lo, (size_t)nmu * D},
                                 {p.off_hi, (size_t)nmu * D}, {p.off_target, (size_t)nmu * D}, {p.off_edges, (size_t)2 * nmu * D}};
        return check_buffers(tag, buf, 9, p.total);
    }
    const size_t buf[][2] = {{p.off_k, (size_t)npts * dk * D}, {p.off_e, (size_t)p.nlev * D}, {p.off_part, want_part * D},
                             {p.off_rows, (size_t)p.nrows * D}, {p.off_mu, (size_t)nmu * D}};
    if (p.off_lo != p.total || p.off_edges != p.total) return printf("%s: buffers of the Fermi selection in a thermodynamics call\n", tag);
    return check_buffers(tag, buf, 5, p.total);
}

// ---------------------------------------------------------------- the argument checks
static int check_args() {
    const char* fn = "occ_plan_check";
    const int32_t mesh[3] = {4, 5, 6};
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    int64_t npts = 0;
    int bad = 0;
    auto ok = [&](int rc, const char* what) {
        if (rc != TBK_OK) bad |= printf("refused: %s\n", what);
    };
    auto no = [&](int rc, const char* what) {
        if (rc != TBK_EINVAL) bad |= printf("accepted: %s\n", what);
    };
    // the mesh
    ok(occ_mesh_check(fn, 2, 3, mesh, npts), "a 2-D mesh");
    if (npts != 20) bad |= printf("npts=%lld\n", (long long)npts);
    ok(occ_mesh_check(fn, 3, 2048, mesh, npts), "a 3-D mesh");
    if (npts != 120) bad |= printf("npts=%lld\n", (long long)npts);
    no(occ_mesh_check(fn, 0, 3, mesh, npts), "dim_k = 0");
    no(occ_mesh_check(fn, 4, 3, mesh, npts), "dim_k = 4");
    no(occ_mesh_check(fn, 2, 0, mesh, npts), "no state");
    no(occ_mesh_check(fn, 2, 2049, mesh, npts), "2049 states");
    {
        const int32_t mb[3] = {4, 0, 6}, mneg[3] = {-4, 5, 6}, huge[3] = {65536, 32768, 1}, most[3] = {65536, 32767, 1};
        no(occ_mesh_check(fn, 2, 3, mb, npts), "a mesh axis of 0 points");
        no(occ_mesh_check(fn, 2, 3, mneg, npts), "a negative mesh axis");
        no(occ_mesh_check(fn, 2, 3, huge, npts), "2^31 mesh points");
        ok(occ_mesh_check(fn, 2, 3, most, npts), "just under 2^31 mesh points");
    }
    // the mesh check is the one of every mesh sweep (tbk_kubo.h): the same return code and point count from each caller
    {
        const int32_t mb[3] = {4, 0, 6}, mneg[3] = {4, -5, 6};
        for (const int32_t* ms : {mesh, mb, mneg}) {
            int64_t n0 = 0, n1 = 0;
            PlaneArgs P;
            const int r0 = kubo_mesh_points(fn, 2, ms, n0), r1 = occ_mesh_check(fn, 2, 3, ms, n1), r2 = kubo_whole_mesh(fn, ms, 2, P);
            if (r0 != (ms == mesh ? TBK_OK : TBK_EINVAL) || r1 != r0 || r2 != r0) bad |= printf("mesh %dx%d: %d %d %d\n", ms[0], ms[1], r0, r1, r2);
            if (!r0 && (n0 != 20 || n1 != 20 || P.npts != 20)) bad |= printf("mesh 4x5: the point count\n");
        }
    }
    // thermodynamics
    {
        const double mu[3] = {0.5, -1.0, 0.5};
        ok(occ_thermo_check(fn, 2, 3, mesh, 3, mu, 0.0, npts), "three levels at kT = 0");
        ok(occ_thermo_check(fn, 2, 3, mesh, 3, mu, 0.07, npts), "three levels at kT > 0");
        no(occ_thermo_check(fn, 2, 3, mesh, 0, mu, 0.0, npts), "no level");
        no(occ_thermo_check(fn, 2, 3, mesh, 3, nullptr, 0.0, npts), "no level array");
        no(occ_thermo_check(fn, 2, 3, mesh, 8193, mu, 0.0, npts), "8193 levels");
        for (double kT : {-1e-3, nan, inf}) no(occ_thermo_check(fn, 2, 3, mesh, 3, mu, kT, npts), "a bad kT");
        const double mb[3] = {0.5, nan, 0.1}, mi[3] = {0.5, 0.1, -inf};
        no(occ_thermo_check(fn, 2, 3, mesh, 3, mb, 0.0, npts), "a NaN level");
        no(occ_thermo_check(fn, 2, 3, mesh, 3, mi, 0.07, npts), "an infinite level");
        std::vector<double> many(8192, 0.25);
        ok(occ_thermo_check(fn, 2, 3, mesh, 8192, many.data(), 0.0, npts), "8192 levels");
    }
    // the Fermi selection: 20 points of 3 states, 60 levels
    {
        std::vector<double> t;
        const double good[3] = {1.0, 0.05, 2.95};
        ok(occ_fermi_check(fn, 2, 3, mesh, 3, good, 0.0, 1, npts, t), "counts 20, 1 and 59");
        if (t.size() != 3 || t[0] != 20.0 || t[1] != 1.0 || t[2] != 59.0) bad |= printf("targets at kT = 0\n");
        const double near[1] = {1.0 + 4e-8};
        ok(occ_fermi_check(fn, 2, 3, mesh, 1, near, 0.0, 0, npts, t), "a count within 1e-6 of an integer");
        if (t[0] != 20.0) bad |= printf("the rounded count\n");
        const double real[2] = {0.123, 2.999};
        ok(occ_fermi_check(fn, 2, 3, mesh, 2, real, 0.05, 0, npts, t), "real fillings at kT > 0");
        if (t[0] != 0.123 * 20.0) bad |= printf("targets at kT > 0\n");
        no(occ_fermi_check(fn, 2, 3, mesh, 2, real, 0.0, 0, npts, t), "a non-integer count at kT = 0");
        no(occ_fermi_check(fn, 2, 3, mesh, 1, good, 0.05, 1, npts, t), "edges at kT > 0");
        no(occ_fermi_check(fn, 2, 3, mesh, 0, good, 0.0, 0, npts, t), "no filling");
        no(occ_fermi_check(fn, 2, 3, mesh, 65, good, 0.0, 0, npts, t), "65 fillings");
        no(occ_fermi_check(fn, 2, 3, mesh, 1, nullptr, 0.0, 0, npts, t), "no filling array");
        for (double kT : {-1e-3, nan, inf}) no(occ_fermi_check(fn, 2, 3, mesh, 3, good, kT, 0, npts, t), "a bad kT");
        for (double x : {0.0, 3.0, -0.05, 3.05, nan, inf}) {
            const double b[1] = {x};
            no(occ_fermi_check(fn, 2, 3, mesh, 1, b, 0.0, 0, npts, t), "a filling outside [1, L - 1] levels at kT = 0");
            no(occ_fermi_check(fn, 2, 3, mesh, 1, b, 0.05, 0, npts, t), "a filling outside (0, nsta) at kT > 0");
        }
        std::vector<double> many(64, 1.5);
        ok(occ_fermi_check(fn, 2, 3, mesh, 64, many.data(), 0.0, 1, npts, t), "64 fillings");
    }
    // the density matrix
    {
        const int32_t R[6] = {0, 0, 1, -1, 1073741823, -1073741823};
        ok(occ_dm_check(fn, 2, 3, mesh, 0.1, 0.0, 3, R, npts), "three lattice vectors");
        ok(occ_dm_check(fn, 3, 3, mesh, -0.1, 0.07, 2, R, npts), "two 3-D lattice vectors");
        no(occ_dm_check(fn, 2, 3, mesh, 0.1, 0.0, 0, R, npts), "nR = 0");
        no(occ_dm_check(fn, 2, 3, mesh, 0.1, 0.0, 3, nullptr, npts), "no R list");
        for (double mu : {nan, inf, -inf}) no(occ_dm_check(fn, 2, 3, mesh, mu, 0.0, 3, R, npts), "a bad Fermi level");
        for (double kT : {-1e-3, nan, inf}) no(occ_dm_check(fn, 2, 3, mesh, 0.1, kT, 3, R, npts), "a bad kT");
        const int32_t big[4] = {0, 0, 1073741824, 0}, neg[4] = {0, -1073741824, 0, 0};
        no(occ_dm_check(fn, 2, 3, mesh, 0.1, 0.0, 2, big, npts), "a component of 2^30");
        no(occ_dm_check(fn, 2, 3, mesh, 0.1, 0.0, 2, neg, npts), "a component of -2^30");
        std::vector<int32_t> many((size_t)4097 * 2, 1);
        ok(occ_dm_check(fn, 2, 3, mesh, 0.1, 0.0, 4096, many.data(), npts), "4096 lattice vectors");
        no(occ_dm_check(fn, 2, 3, mesh, 0.1, 0.0, 4097, many.data(), npts), "4097 lattice vectors");
        ok(occ_dm_check(fn, 2, 512, mesh, 0.1, 0.0, 16, many.data(), npts), "nR nsta^2 at the cap");
        no(occ_dm_check(fn, 2, 512, mesh, 0.1, 0.0, 17, many.data(), npts), "nR nsta^2 over the cap");
        ok(occ_dm_check(fn, 2, 2048, mesh, 0.1, 0.0, 1, many.data(), npts), "one matrix of 2048 states");
        no(occ_dm_check(fn, 2, 2048, mesh, 0.1, 0.0, 2, many.data(), npts), "two matrices of 2048 states");
    }
    return bad;
}

int main() {
    int bad = check_key() ? 1 : 0, cases = 0;
    for (const Case& c : kCases) {
        bad |= check_dm_case(c) ? 1 : 0;
        ++cases;
    }
    // (n, dk, npts, nmu, thermal, fermi, groups, workgroups of the kT = 0 Fermi scan)
    bad |= check_scan(1, 2, 63, 1, false, false, 1, 1) ? 1 : 0;
    bad |= check_scan(2, 2, 120, 300, false, false, 1, 1) ? 1 : 0;
    bad |= check_scan(2, 2, 120, 300, true, false, 1, 0) ? 1 : 0;
    bad |= check_scan(2, 2, 120, 64, true, true, 1, 0) ? 1 : 0;
    bad |= check_scan(2, 2, 65536, 8192, false, false, 128, 64) ? 1 : 0;
    bad |= check_scan(2, 2, 65536, 8192, true, false, 128, 0) ? 1 : 0;
    bad |= check_scan(16, 3, 32768, 5, false, true, 512, 0) ? 1 : 0;
    bad |= check_scan(40, 2, 1369, 1, true, false, 54, 0) ? 1 : 0;
    bad |= check_scan(4, 2, 4194304, 64, false, true, 1024, 0) ? 1 : 0;
    cases += 9;
    bad |= check_args() ? 1 : 0;
    if (bad) return printf("occ_plan_check: FAILED\n"), 1;
    printf("occ_plan_check: the key, %d plans and the argument checks ok\n", cases);
    return 0;
}
