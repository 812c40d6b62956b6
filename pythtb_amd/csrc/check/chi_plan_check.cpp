// Stand-alone host check of tbk_chi.h (no device call): built under AddressSanitizer + UBSan by `make -C pythtb_amd/csrc chi-check`
// and run as an ordinary program.  Over a table of (n, dim_k, mesh, nq, nw, flags) it checks the plan of tbk_susceptibility_mesh:
// the chunk, the k-groups, the frequency tiles and the groups of the static sums against the values worked out by hand; the part
// buffer against its cap; that the k-groups of every chunk (the last, shorter one included) cover its points once; that nothing but
// acc and the offsets behind it depends on nq; and the layout of the scratch block -- every buffer at a multiple of 256, in order,
// none overlapping, the last one ending at the total (each is filled with its own index over a real host block and read back, under
// the sanitizer, where the block is at most 512 MiB).  Then the argument checks: every rule of chi_check, one bad value at a time; and
// what tbk_kubo.h shares between the mesh sweeps: the eigenvalue-only chunk workspace and the one mesh check.
#include <cmath>
#include <limits>
#include <vector>
#include "../tbk_chi.h"
#include "check_common.h"

struct Case {
    int n, dk, mesh[3], nq, nw, flags;
    // expected: points per chunk, k-groups, frequency tiles, groups one (chunk, q) writes at most, points per LDS workgroup (0: not LDS)
    int64_t chunk;
    int G;
    unsigned ntile;
    int64_t gmax;
    int P;
};

static const Case kCases[] = {
    // one state: 2^21 points per chunk would fit, the mesh is shorter
    {1, 2, {16, 16, 1}, 4, 0, 1, 256, 256, 0, 4, 64},
    {1, 2, {16, 16, 1}, 4, 6, 1, 256, 256, 1, 256, 64},
    {1, 2, {16, 16, 1}, 4, 0, 0, 256, 256, 0, 256, 0},
    {1, 2, {2048, 2048, 1}, 1, 0, 1, 2097152, 1024, 0, 32768, 64},
    {2, 2, {12, 10, 1}, 4, 6, 1, 120, 120, 1, 120, 64},
    {2, 2, {12, 10, 1}, 2, 1030, 1, 120, 120, 3, 120, 64},
    {2, 2, {256, 256, 1}, 4096, 0, 1, 65536, 1024, 0, 1024, 64},
    {3, 1, {41, 1, 1}, 4, 6, 1, 41, 41, 1, 41, 64},
    {4, 2, {12, 10, 1}, 4, 0, 1, 120, 120, 0, 2, 64},
    {8, 3, {32, 32, 32}, 64, 256, 1, 32768, 1024, 1, 1024, 16},
    {16, 3, {4, 3, 5}, 4, 6, 1, 60, 60, 1, 60, 4},
    {16, 3, {4, 3, 5}, 4, 0, 1, 60, 60, 0, 15, 4},
    {32, 2, {3, 4, 1}, 4, 0, 1, 12, 12, 0, 12, 1},
    {32, 2, {48, 48, 1}, 2, 6, 1, 2048, 1024, 1, 1024, 1},
    {34, 1, {7, 1, 1}, 4, 6, 1, 7, 7, 1, 7, 0},
    {34, 1, {1900, 1, 1}, 1, 2, 1, 1814, 1024, 1, 1024, 0},
    {34, 1, {1900, 1, 1}, 1, 0, 1, 1814, 1024, 0, 1024, 0},
    {34, 1, {1900, 1, 1}, 1, 0, 0, 1814, 1024, 0, 1024, 0},
    {2048, 1, {3, 1, 1}, 1, 0, 1, 1, 1, 0, 1, 0},
    // the most frequencies: G shrinks to hold part[G][2 nw] under the cap
    {2, 2, {256, 256, 1}, 64, 65536, 1, 65536, 128, 128, 128, 64},
    {2, 2, {256, 256, 1}, 65536, 64, 0, 65536, 1024, 1, 1024, 0},
};

static int check_layout(const char* tag, const ChiPlan& p, int n, int dk, int nq, int nw) {
    const size_t nn = (size_t)n * n, D = sizeof(double);
    // (offset, bytes) of every buffer of the scratch block in order; the chunk workspace: k, E, U, then the three extras, the first
    // of which holds k + q, E(k+q), U(k+q)
    const size_t cb = p.off_chunks;
    const size_t x0 = cb + p.cw.off[3];
    const size_t buf[][2] = {
        {p.off_om, (size_t)nw * D},
        {p.off_q, (size_t)nq * dk * D},
        {p.off_acc, (size_t)p.acc_doubles * D},
        {p.off_part, (size_t)p.part_doubles * D},
        {cb + p.cw.off[0], (size_t)p.chunk * dk * D},
        {cb + p.cw.off[1], (size_t)p.chunk * n * D},
        {cb + p.cw.off[2], p.me ? (size_t)p.chunk * nn * sizeof(cd) : 0},
        {x0, (size_t)p.chunk * dk * D},
        {x0 + p.off_e2, (size_t)p.chunk * n * D},
        {x0 + p.off_v2, p.me ? (size_t)p.chunk * nn * sizeof(cd) : 0},
        {cb + p.cw.off[4], p.dynamic ? (size_t)p.chunk * nn * 2 * D : 0},
        {cb + p.cw.off[5], p.wide ? (size_t)p.chunk * nn * D : 0},
    };
    const int nb = (int)(sizeof buf / sizeof buf[0]);
    size_t end = 256;
    for (int i = 0; i < nb; ++i) {
        if (buf[i][0] % 256 || buf[i][0] < end)
            return printf("%s: buffer %d at offset %zu (the previous one ends at %zu)\n", tag, i, buf[i][0], end);
        end = buf[i][0] + buf[i][1];
    }
    if (end > p.total || p.total - end >= 256 + 256) return printf("%s: the last buffer ends at %zu, the total is %zu\n", tag, end, p.total);
    if (!p.me && p.cw.off[3] != p.cw.off[2]) return printf("%s: bytes for eigenvectors in an eigenvalue-only plan\n", tag);
    if (p.x0 != p.off_v2 + (p.me ? al256((size_t)p.chunk * nn * sizeof(cd)) : 0)) return printf("%s: x0\n", tag);
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
    char tag[128];
    snprintf(tag, sizeof tag, "n=%d dk=%d mesh=%dx%dx%d nq=%d nw=%d flags=%d", c.n, c.dk, c.mesh[0], c.mesh[1], c.mesh[2], c.nq, c.nw, c.flags);
    const int64_t npts = (int64_t)c.mesh[0] * c.mesh[1] * c.mesh[2];
    const ChiPlan p = chi_plan(c.n, c.dk, npts, c.nq, c.nw, c.flags);
    if (p.chunk != c.chunk || p.G != c.G || p.ntile != c.ntile || p.gmax != c.gmax || (p.lds ? p.P : 0) != c.P)
        return printf("%s: chunk %lld G %d ntile %u gmax %lld P %d\n", tag, (long long)p.chunk, p.G, p.ntile, (long long)p.gmax,
                      p.lds ? p.P : 0);
    if (p.chunk < 1 || p.chunk > npts || (size_t)p.chunk * c.n * c.n * sizeof(cd) > std::max(kKuboChunkBytes, (size_t)c.n * c.n * sizeof(cd)))
        return printf("%s: the chunk holds more than kKuboChunkBytes of eigenvectors\n", tag);
    if (p.nchunks != (npts + p.chunk - 1) / p.chunk) return printf("%s: nchunks\n", tag);
    if (p.G < 1 || p.G > kPairGroupsMax || p.G > p.chunk) return printf("%s: G=%d\n", tag, p.G);
    if (p.dynamic && p.part_doubles > kPairPartCap) return printf("%s: part of %lld doubles is over the cap\n", tag, (long long)p.part_doubles);
    if (!p.dynamic && p.part_doubles > std::max<int64_t>(p.chunk, 1)) return printf("%s: more static groups than points\n", tag);
    if (p.lds && (size_t)2 * p.P * c.n * c.n > CHI_LDS_CD) return printf("%s: %d points do not fit the LDS\n", tag, p.P);
    if ((int64_t)p.ntile * kPairTile < c.nw || (p.ntile > 0 && (int64_t)(p.ntile - 1) * kPairTile >= c.nw)) return printf("%s: tiles\n", tag);
    if (p.wide && p.chunk > 65535) return printf("%s: the chunk is beyond the z limit of k_chi_mprod's grid\n", tag);
    // the k-groups of a full chunk and of the last one cover the points once, in order
    if (check_groups(tag, p.G, npts, p.chunk, p.nchunks)) return 1;
    for (int64_t cnt : {p.chunk, npts - (p.nchunks - 1) * p.chunk})
        if (p.lds && !p.dynamic && (cnt + p.P - 1) / p.P > p.gmax) return printf("%s: more workgroups than part holds\n", tag);
    // a q alone is worked through like the same q inside this list
    const ChiPlan one = chi_plan(c.n, c.dk, npts, 1, c.nw, c.flags);
    if (one.chunk != p.chunk || one.G != p.G || one.ntile != p.ntile || one.gmax != p.gmax || one.P != p.P || one.nrows != p.nrows ||
        one.part_doubles != p.part_doubles || one.x0 != p.x0 || one.x1 != p.x1 || one.x2 != p.x2)
        return printf("%s: the plan depends on nq\n", tag);
    if (p.acc_doubles != (int64_t)c.nq * p.nrows) return printf("%s: acc\n", tag);
    return check_layout(tag, p, c.n, c.dk, c.nq, c.nw);
}

static int check_args() {
    const char* fn = "chi_plan_check";
    const int32_t mesh[3] = {4, 5, 6};
    const double q[4] = {0.1, 0.2, 0.3, 0.4}, w[2] = {0.5, -1.0};
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    int64_t npts = 0;
    int bad = 0;
    auto ok = [&](int rc, const char* what) {
        if (rc != TBK_OK) bad |= printf("refused: %s\n", what);
    };
    auto no = [&](int rc, const char* what) {
        if (rc != TBK_EINVAL) bad |= printf("accepted: %s\n", what);
    };
    ok(chi_check(fn, 2, 3, mesh, 2, q, 2, w, 0.05, 0.0, 0.0, 1, npts), "dynamic");
    if (npts != 20) bad |= printf("npts=%lld\n", (long long)npts);
    ok(chi_check(fn, 3, 3, mesh, 1, q, 0, nullptr, 0.0, 0.3, 0.1, 0, npts), "static");
    if (npts != 120) bad |= printf("npts=%lld\n", (long long)npts);
    no(chi_check(fn, 0, 3, mesh, 2, q, 2, w, 0.05, 0.0, 0.0, 1, npts), "dim_k = 0");
    no(chi_check(fn, 4, 3, mesh, 1, q, 2, w, 0.05, 0.0, 0.0, 1, npts), "dim_k = 4");
    no(chi_check(fn, 2, 0, mesh, 2, q, 2, w, 0.05, 0.0, 0.0, 1, npts), "no state");
    no(chi_check(fn, 2, 2049, mesh, 2, q, 2, w, 0.05, 0.0, 0.0, 1, npts), "2049 states");
    no(chi_check(fn, 2, 3, mesh, 2, q, 2, w, 0.05, 0.0, 0.0, 2, npts), "an unknown flag");
    no(chi_check(fn, 2, 3, mesh, 0, q, 2, w, 0.05, 0.0, 0.0, 1, npts), "nq = 0");
    no(chi_check(fn, 2, 3, mesh, 65537, q, 2, w, 0.05, 0.0, 0.0, 1, npts), "nq = 65537");
    {
        const double qb[4] = {0.1, nan, 0.3, 0.4}, qi[4] = {0.1, 0.2, 0.3, -inf};
        no(chi_check(fn, 2, 3, mesh, 2, qb, 2, w, 0.05, 0.0, 0.0, 1, npts), "a NaN q");
        no(chi_check(fn, 2, 3, mesh, 2, qi, 0, nullptr, 0.0, 0.0, 0.0, 1, npts), "an infinite q");
    }
    no(chi_check(fn, 2, 3, mesh, 2, q, 0, w, 0.05, 0.0, 0.0, 1, npts), "omega with nomega = 0");
    no(chi_check(fn, 2, 3, mesh, 2, q, 65537, w, 0.05, 0.0, 0.0, 1, npts), "65537 frequencies");
    {
        const double wb[2] = {0.5, inf};
        no(chi_check(fn, 2, 3, mesh, 2, q, 2, wb, 0.05, 0.0, 0.0, 1, npts), "an infinite frequency");
    }
    for (double eta : {0.0, -0.1, nan, inf}) no(chi_check(fn, 2, 3, mesh, 2, q, 2, w, eta, 0.0, 0.0, 1, npts), "a bad eta");
    no(chi_check(fn, 2, 3, mesh, 2, q, 2, nullptr, 0.0, 0.0, 0.0, 1, npts), "nomega without omega");
    no(chi_check(fn, 2, 3, mesh, 2, q, 0, nullptr, 0.05, 0.0, 0.0, 1, npts), "eta in the static mode");
    no(chi_check(fn, 2, 3, mesh, 2, q, 0, nullptr, nan, 0.0, 0.0, 1, npts), "a NaN eta in the static mode");
    for (double kT : {-1e-3, nan, inf}) no(chi_check(fn, 2, 3, mesh, 2, q, 0, nullptr, 0.0, 0.0, kT, 1, npts), "a bad kT");
    for (double mu : {nan, -inf}) no(chi_check(fn, 2, 3, mesh, 2, q, 2, w, 0.05, mu, 0.0, 1, npts), "a bad Fermi level");
    {
        const int32_t mb[3] = {4, 0, 6};
        no(chi_check(fn, 2, 3, mb, 2, q, 2, w, 0.05, 0.0, 0.0, 1, npts), "a mesh axis of 0 points");
    }
    {
        // nq nomega over the cap: 65 x 65536 (the q list and the frequencies have to be real: they are read first)
        std::vector<double> qs(65 * 2, 0.25), ws(65536, 0.5);
        no(chi_check(fn, 2, 3, mesh, 65, qs.data(), 65536, ws.data(), 0.05, 0.0, 0.0, 1, npts), "nq nomega over the cap");
        ok(chi_check(fn, 2, 3, mesh, 64, qs.data(), 65536, ws.data(), 0.05, 0.0, 0.0, 1, npts), "nq nomega at the cap");
    }
    return bad;
}

// What the mesh sweeps share (tbk_kubo.h): an eigenvalue-only KuboChunks has no bytes for eigenvectors and is that much shorter; the
// one mesh check gives every caller the same return code for a bad mesh and the same point count for a good one.
static int check_shared() {
    const char* fn = "chi_plan_check";
    const size_t vb = al256((size_t)100 * 34 * 34 * sizeof(cd));
    const KuboChunks full(34, 2, 100, 512, 0, 768), ev(34, 2, 100, 512, 0, 768, false);
    if (full.off[3] - full.off[2] != vb || ev.off[3] != ev.off[2] || ev.bytes() + vb != full.bytes() || ev.off[2] != full.off[2])
        return printf("KuboChunks: an eigenvalue-only workspace holds %zu bytes of eigenvectors\n", ev.off[3] - ev.off[2]);
    const int32_t good[3] = {4, 5, 6}, zero[3] = {4, 0, 6}, neg[3] = {4, -5, 6};
    const double q[2] = {0.1, 0.2}, w[1] = {0.5};
    tbk_model mm;
    mm.dim_k = 2, mm.nsta = 3;
    for (const int32_t* mesh : {good, zero, neg}) {
        const int want = mesh == good ? TBK_OK : TBK_EINVAL;
        int64_t np[3] = {0, 0, 0};
        PlaneArgs P;
        const int rc[4] = {kubo_mesh_points(fn, 2, mesh, np[0]), pair_sweep_check(fn, &mm, mesh, 1, w, 0.05, 0.0, 0.0, np[1]),
                           chi_check(fn, 2, 3, mesh, 1, q, 1, w, 0.05, 0.0, 0.0, 1, np[2]), kubo_whole_mesh(fn, mesh, 2, P)};
        for (int i = 0; i < 4; ++i)
            if (rc[i] != want) return printf("mesh %dx%d: caller %d returns %d, not %d\n", mesh[0], mesh[1], i, rc[i], want);
        if (want == TBK_OK && (np[0] != 20 || np[1] != 20 || np[2] != 20 || P.npts != 20)) return printf("mesh 4x5: the point count\n");
    }
    mm.dim_k = 4;
    int64_t np = 0;
    if (pair_sweep_check(fn, &mm, good, 1, w, 0.05, 0.0, 0.0, np) != TBK_EINVAL || kubo_mesh_dim(fn, 0) != TBK_EINVAL || kubo_mesh_dim(fn, 3))
        return printf("the dimension of the mesh\n");
    return 0;
}

int main() {
    int bad = 0, cases = 0;
    for (const Case& c : kCases) {
        bad |= check_case(c) ? 1 : 0;
        ++cases;
    }
    bad |= check_args() ? 1 : 0;
    bad |= check_shared() ? 1 : 0;
    if (bad) return printf("chi_plan_check: FAILED\n"), 1;
    printf("chi_plan_check: %d plans and the argument checks ok\n", cases);
    return 0;
}
