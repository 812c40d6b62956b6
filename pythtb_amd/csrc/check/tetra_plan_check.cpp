// Stand-alone host check of tbk_tetra.h (no device call): built under AddressSanitizer + UBSan by `make -C pythtb_amd/csrc tetra-check`
// and run as an ordinary program.  It checks the cut of a cell (every simplex a permutation of the axes, all different, from the
// origin to the far corner); the stable sort of the corners; the simplex arithmetic tet_eval in 1, 2 and 3 dimensions on random
// simplices in every branch (the weights against the closed forms of their sums, the derivative part against a centred difference,
// continuity across the inner corners, the curvature correction summing to zero) and the tie rule on repeated corners (finite,
// equal corners alike, the steps of a flat simplex); the trial keys of the Fermi search and the search itself replayed on the
// host; the energy and band tiles of the sweeps over a table (part against its cap, every energy and band covered once, the groups
// independent of the number of energies); the layout of every scratch block (every buffer at a multiple of 256, in order, none
// overlapping, the last one ending at the total).  Then the argument checks: every rule, one bad value at a time.
#include <cmath>
#include <limits>
#include <random>
#include <vector>
#include "../tbk_tetra.h"
#include "check_common.h"

// check_common.h's check of a scratch block over a list that grows with the form of the call; blocks up to 256 MiB are filled
static int check_buffers(const char* tag, const std::vector<std::pair<size_t, size_t>>& buf, size_t total) {
    std::vector<size_t> flat;
    for (const auto& b : buf) flat.insert(flat.end(), {b.first, b.second});
    return check_buffers(tag, (const size_t(*)[2])flat.data(), (int)buf.size(), total, (size_t)256 << 20);
}

// ---------------------------------------------------------------- the cut of a cell
static int check_cut() {
    for (int dim = 1; dim <= 3; ++dim) {
        const int ns = tet_simplices(dim);
        int fact = 1;
        for (int i = 2; i <= dim; ++i) fact *= i;
        if (ns != fact) return printf("cut: %d simplices in %d dimensions\n", ns, dim);
        std::vector<int> codes;
        for (int p = 0; p < ns; ++p) {
            int seen = 0, code = 0;
            for (int i = 0; i < dim; ++i) {
                const int a = tet_axis(dim, p, i);
                if (a < 0 || a >= dim || (seen >> a & 1)) return printf("cut: simplex %d of %d dimensions is no permutation\n", p, dim);
                seen |= 1 << a;
                code = code * 4 + a;
            }
            for (int c : codes)
                if (c == code) return printf("cut: simplex %d of %d dimensions appears twice\n", p, dim);
            codes.push_back(code);
            if (tet_corner(dim, p, 0) != 0 || tet_corner(dim, p, dim) != (1 << dim) - 1) return printf("cut: the diagonal of simplex %d\n", p);
            for (int s = 1; s <= dim; ++s)
                if (__builtin_popcount(tet_corner(dim, p, s) ^ tet_corner(dim, p, s - 1)) != 1) return printf("cut: slot %d of simplex %d\n", s, p);
        }
    }
    double e[4] = {0.5, -1.0, 0.5, -1.0};
    int s[4];
    tet_sort<4>(e, s);
    if (!(e[0] == -1.0 && e[1] == -1.0 && e[2] == 0.5 && e[3] == 0.5 && s[0] == 1 && s[1] == 3 && s[2] == 0 && s[3] == 2))
        return printf("sort: ties are not kept in slot order\n");
    return 0;
}

// ---------------------------------------------------------------- the simplex arithmetic
// (N_T, g_T) of a sorted simplex of volume 1 strictly inside a branch, from the closed forms of the sums
template <int DIM>
static void closed_sums(const double (&e)[DIM + 1], double E, double& N, double& g) {
    if constexpr (DIM == 1) {
        N = (E - e[0]) / (e[1] - e[0]);
        g = 1.0 / (e[1] - e[0]);
    } else if constexpr (DIM == 2) {
        if (E < e[1]) {
            N = (E - e[0]) * (E - e[0]) / ((e[1] - e[0]) * (e[2] - e[0]));
            g = 2.0 * (E - e[0]) / ((e[1] - e[0]) * (e[2] - e[0]));
        } else {
            N = 1.0 - (e[2] - E) * (e[2] - E) / ((e[2] - e[0]) * (e[2] - e[1]));
            g = 2.0 * (e[2] - E) / ((e[2] - e[0]) * (e[2] - e[1]));
        }
    } else {
        const double e21 = e[1] - e[0], e31 = e[2] - e[0], e41 = e[3] - e[0], e32 = e[2] - e[1], e42 = e[3] - e[1], e43 = e[3] - e[2];
        if (E < e[1]) {
            const double x = E - e[0];
            N = x * x * x / (e21 * e31 * e41);
            g = 3.0 * x * x / (e21 * e31 * e41);
        } else if (E < e[2]) {
            const double x = E - e[1];
            N = (e21 * e21 + 3.0 * e21 * x + 3.0 * x * x - (e31 + e42) * x * x * x / (e32 * e42)) / (e31 * e41);
            g = (3.0 * e21 + 6.0 * x - 3.0 * (e31 + e42) * x * x / (e32 * e42)) / (e31 * e41);
        } else {
            const double y = e[3] - E;
            N = 1.0 - y * y * y / (e41 * e42 * e43);
            g = 3.0 * y * y / (e41 * e42 * e43);
        }
    }
}

template <int DIM>
static int check_eval() {
    constexpr int NV = DIM + 1;
    std::mt19937_64 rng(1234 + DIM);
    std::uniform_real_distribution<double> U(-1.0, 1.0), F(0.1, 0.9);
    for (int it = 0; it < 2000; ++it) {
        double e[NV];
        int s[NV];
        for (double& x : e) x = U(rng);
        tet_sort<NV>(e, s);
        for (int br = 0; br < DIM; ++br) {
            if (e[br + 1] - e[br] < 0.05) continue;                  // (the centred difference's own error grows with 1 / gap^3)
            const double E = e[br] + F(rng) * (e[br + 1] - e[br]), h = 1e-6;
            Du w[NV], wp[NV], wm[NV];
            tet_eval<DIM>(e, E, w);
            tet_eval<DIM>(e, E + h, wp);
            tet_eval<DIM>(e, E - h, wm);
            double N, g, sn = 0.0, sg = 0.0;
            closed_sums<DIM>(e, E, N, g);
            for (int i = 0; i < NV; ++i) {
                sn += w[i].v;
                sg += w[i].d;
                if (!(w[i].v >= -1e-15) || !std::isfinite(w[i].d)) return printf("eval %d-D: a weight of %g\n", DIM, w[i].v);
                const double num = (wp[i].v - wm[i].v) / (2.0 * h);
                if (fabs(num - w[i].d) > 1e-6 * std::max(1.0, fabs(w[i].d)))
                    return printf("eval %d-D branch %d: d_%d = %g, the centred difference %g\n", DIM, br, i, w[i].d, num);
            }
            if (fabs(sn - N) > 1e-12 || fabs(sg - g) > 1e-11 * std::max(1.0, g))
                return printf("eval %d-D branch %d: sums (%g, %g), closed forms (%g, %g)\n", DIM, br, sn, sg, N, g);
            if constexpr (DIM == 3) {
                double c = 0.0;
                for (int i = 0; i < 4; ++i) c += tet_correction(e, w, i);
                if (fabs(c) > 1e-13 * std::max(1.0, g)) return printf("eval 3-D: the correction sums to %g\n", c);
            }
        }
        for (int j = 1; j < DIM; ++j) {                             // continuity across the inner corners
            Du a[NV], b[NV];
            tet_eval<DIM>(e, std::nextafter(e[j], -2.0), a);
            tet_eval<DIM>(e, e[j], b);
            for (int i = 0; i < NV; ++i)
                if (fabs(a[i].v - b[i].v) > 1e-12) return printf("eval %d-D: w_%d jumps by %g at corner %d\n", DIM, i, a[i].v - b[i].v, j);
        }
    }
    // ties: every run of equal corners, at the corners, between them and outside
    for (int equal = 2; equal <= NV; ++equal)
        for (int start = 0; start + equal <= NV; ++start) {
            double e[NV];
            for (int i = 0; i < NV; ++i) e[i] = i;
            for (int i = start; i < start + equal; ++i) e[i] = start;
            for (int q = -4; q <= 4 * NV + 4; ++q) {
                const double E = 0.25 * q;
                Du w[NV];
                tet_eval<DIM>(e, E, w);
                double sn = 0.0;
                for (int i = 0; i < NV; ++i) {
                    if (!std::isfinite(w[i].v) || !std::isfinite(w[i].d) || w[i].v < -1e-15 || w[i].d < -1e-15)
                        return printf("ties %d-D: corner %d at E=%g is (%g, %g)\n", DIM, i, E, w[i].v, w[i].d);
                    sn += w[i].v;
                    for (int j = 0; j < i; ++j)
                        if (e[i] == e[j] && (fabs(w[i].v - w[j].v) > 1e-14 || fabs(w[i].d - w[j].d) > 1e-13))
                            return printf("ties %d-D: equal corners %d and %d differ at E=%g\n", DIM, j, i, E);
                }
                if (E >= e[NV - 1] && fabs(sn - 1.0) > 1e-15) return printf("ties %d-D: N=%g above the simplex\n", DIM, sn);
                if (E <= e[0] && E < e[NV - 1] && sn != 0.0) return printf("ties %d-D: N=%g below the simplex\n", DIM, sn);
            }
        }
    {
        double e[NV];
        for (double& x : e) x = 0.5;
        const double at[3] = {0.4999, 0.5, 0.6}, want[3] = {0.0, 1.0, 1.0};
        for (int q = 0; q < 3; ++q) {
            Du w[NV];
            tet_eval<DIM>(e, at[q], w);
            double sn = 0.0, sg = 0.0;
            for (int i = 0; i < NV; ++i) sn += w[i].v, sg += fabs(w[i].d);
            if (fabs(sn - want[q]) > 1e-15 || sg != 0.0) return printf("flat %d-D: (N, g) = (%g, %g) at E=%g\n", DIM, sn, sg, at[q]);
        }
    }
    return 0;
}

// ---------------------------------------------------------------- the Fermi search
static int check_search() {
    uint64_t keys[kTetTrials];
    const double targets[] = {-3.25, -1e-300, 0.0, 1e-17, 0.1, 0.7310585786300049, 5e7};
    for (double root : targets) {
        // N(mu) = [mu >= root]: the search must end on root itself
        uint64_t lo = occ_key(-1e9), hi = occ_key(1e9);
        int rounds = 0;
        while (hi - lo > 1) {
            if (++rounds > kTetRoundsMax) return printf("search: %d rounds are not enough for %g\n", kTetRoundsMax, root);
            const int nt = tet_trial_keys(lo, hi, keys);
            if (nt < 1 || nt > kTetTrials) return printf("search: %d trial keys\n", nt);
            for (int j = 0; j < nt; ++j)
                if (keys[j] <= (j ? keys[j - 1] : lo) || keys[j] >= hi) return printf("search: trial key %d is out of order\n", j);
            int first = nt;
            for (int j = nt - 1; j >= 0; --j)
                if (occ_unkey(keys[j]) >= root) first = j;
            if (first < nt) hi = keys[first];
            if (first > 0) lo = keys[first - 1];
        }
        if (occ_unkey(hi) != root) return printf("search: ends on %.17g, not %.17g\n", occ_unkey(hi), root);
    }
    if (tet_trial_keys(5, 6, keys) != 0 || tet_trial_keys(5, 7, keys) != 1 || keys[0] != 6) return printf("search: the narrow brackets\n");
    if (tet_trial_keys(0, 257, keys) != 256 || keys[0] != 1 || keys[255] != 256) return printf("search: a bracket of 256 inner keys\n");
    if (tet_trial_keys(0, ~(uint64_t)0, keys) != 256 || keys[255] >= ~(uint64_t)0) return printf("search: the widest bracket\n");
    if (tet_integer_filling(1.0, 2) != 1 || tet_integer_filling(1.0 + 5e-10, 3) != 1 || tet_integer_filling(1.0 + 2e-9, 3) != 0 ||
        tet_integer_filling(2.0, 2) != 0 || tet_integer_filling(0.0, 2) != 0 || tet_integer_filling(0.5, 1) != 0)
        return printf("search: the integer fillings\n");
    return 0;
}

// ---------------------------------------------------------------- the sweeps and the scratch blocks
struct Case {
    int n, dk, mesh[3], nE, per_band, nsel;
    int G, ET, BT;          // expected of the cell form: groups, energies per launch, bands per launch
    int GP;                 // expected k-groups of a chunk of the projected DOS (0: none)
};
static const Case kCases[] = {
    {1, 2, {4, 3, 1}, 3, 0, 0, 1, 3, 1, 0},
    {3, 1, {41, 1, 1}, 40, 1, 0, 3, 40, 3, 0},
    {2, 2, {12, 10, 1}, 40, 1, 2, 8, 40, 2, 8},
    {2, 2, {256, 256, 1}, 256, 0, 2, 1024, 256, 1, 512},
    {2, 2, {256, 256, 1}, 2300, 1, 0, 1024, 1024, 2, 0},
    {8, 3, {32, 32, 32}, 65536, 0, 8, 1024, 1024, 1, 512},
    {16, 3, {5, 4, 3}, 40, 1, 16, 4, 40, 16, 4},
    {40, 2, {40, 36, 1}, 13, 1, 4, 90, 13, 40, 82},
    {2048, 1, {3, 1, 1}, 2048, 1, 1, 1, 1024, 2048, 1},
    {512, 2, {64, 64, 1}, 8192, 1, 1, 256, 1024, 16, 1},
};

static int check_sweep(const char* tag, const TetSweep& s, int n, int nE, bool per_band, int Q) {
    if (s.Q != Q || s.ET < 1 || s.ET > kTetTile || s.BT < 1 || s.BT > 65535) return printf("%s: Q %d ET %d BT %d\n", tag, s.Q, s.ET, s.BT);
    if (s.part_doubles > kTetPartCap || s.part_doubles != (int64_t)s.G * s.BT * Q * s.ET) return printf("%s: part of %lld doubles\n", tag, (long long)s.part_doubles);
    int64_t rows = 0;
    std::vector<int> ecover((size_t)nE, 0), bcover((size_t)n, 0);
    for (int ie = 0; ie < s.net; ++ie)
        for (int ib = 0; ib < s.nbt; ++ib) {
            const int et = s.et(ie, nE), bt = s.bt(ib, n);
            if (et < 1 || et > s.ET || bt < 1 || bt > s.BT) return printf("%s: launch (%d, %d) of %d energies and %d bands\n", tag, ie, ib, et, bt);
            if ((int64_t)bt * Q * et > s.stride) return printf("%s: the rows of launch (%d, %d) pass the stride\n", tag, ie, ib);
            rows += (int64_t)bt * Q * et;
            if (ib == 0)
                for (int j = 0; j < et; ++j) ++ecover[(size_t)ie * s.ET + j];
            if (ie == 0)
                for (int z = 0; z < bt; ++z)
                    for (int b = s.b0(ib) + z * s.bpz(n); b < s.b0(ib) + (z + 1) * s.bpz(n); ++b) ++bcover[b];
        }
    for (int c : ecover)
        if (c != 1) return printf("%s: an energy is covered %d times\n", tag, c);
    for (int c : bcover)
        if (c != 1) return printf("%s: a band is covered %d times\n", tag, c);
    if (rows != (int64_t)(per_band ? n : 1) * Q * nE || s.acc_doubles < rows) return printf("%s: %lld rows\n", tag, (long long)rows);
    return 0;
}

static int check_case(const Case& c) {
    char tag[160];
    snprintf(tag, sizeof tag, "dos n=%d dk=%d mesh=%dx%dx%d nE=%d per_band=%d nsel=%d", c.n, c.dk, c.mesh[0], c.mesh[1], c.mesh[2], c.nE,
             c.per_band, c.nsel);
    const int64_t npts = (int64_t)c.mesh[0] * c.mesh[1] * c.mesh[2];
    const TetDosPlan p = tet_dos_plan(c.n, c.dk, npts, c.nE, c.per_band != 0, c.nsel);
    if (p.cell.G != c.G || p.cell.ET != c.ET || p.cell.BT != c.BT || (p.pdos ? p.vert.G : 0) != c.GP)
        return printf("%s: G %d ET %d BT %d GP %d\n", tag, p.cell.G, p.cell.ET, p.cell.BT, p.pdos ? p.vert.G : 0);
    if (p.cell.G > npts || p.cell.G > kTetCellGroupsMax) return printf("%s: more groups than cells\n", tag);
    int bad = check_sweep(tag, p.cell, c.n, c.nE, c.per_band != 0, 2);
    if (!bad && p.pdos) {
        if (p.vert.G > p.chunk || p.vert.G > kTetPdosGroupsMax || p.chunk != kubo_chunk_len(c.n, npts)) return printf("%s: the chunk's groups\n", tag);
        bad = check_sweep(tag, p.vert, c.n, c.nE, c.per_band != 0, c.nsel);
    }
    if (bad) return bad;
    // an energy alone is worked through with the same groups
    const TetDosPlan one = tet_dos_plan(c.n, c.dk, npts, 1, c.per_band != 0, c.nsel ? 1 : 0);
    if (one.cell.G != p.cell.G || one.vert.G != p.vert.G || one.chunk != p.chunk) return printf("%s: the groups depend on the energies or the selection\n", tag);
    const size_t D = sizeof(double);
    const int64_t part = std::max(p.cell.part_doubles, p.vert.part_doubles);
    std::vector<std::pair<size_t, size_t>> buf = {
        {p.off_k, (size_t)npts * c.dk * D},     {p.off_e, (size_t)npts * c.n * D},         {p.off_en, (size_t)c.nE * D},
        {p.off_sel, (size_t)c.nsel * 4},        {p.off_acc, (size_t)p.cell.acc_doubles * D}, {p.off_part, (size_t)part * D},
        {p.off_pacc, (size_t)p.vert.acc_doubles * D},
    };
    if (p.pdos) {
        buf.push_back({p.off_chunks + p.cw.off[0], (size_t)p.chunk * c.dk * D});
        buf.push_back({p.off_chunks + p.cw.off[1], (size_t)p.chunk * c.n * D});
        buf.push_back({p.off_chunks + p.cw.off[2], (size_t)p.chunk * c.n * c.n * sizeof(cd)});
    }
    bad = check_buffers(tag, buf, p.total);
    if (bad) return bad;
    const TetFermiPlan f = tet_fermi_plan(c.n, c.dk, npts);
    if (f.cell.G != p.cell.G || f.cell.ET != kTetTrials || f.cell.BT != 1 || f.cell.net != 1 || f.cell.nbt != 1 || f.gx < 1 || f.gx > 1024)
        return printf("%s: the plan of the Fermi search\n", tag);
    bad = check_buffers(tag, {{f.off_k, (size_t)npts * c.dk * D}, {f.off_e, (size_t)npts * c.n * D}, {f.off_en, (size_t)kTetTrials * D},
                              {f.off_acc, (size_t)f.cell.acc_doubles * D}, {f.off_part, (size_t)f.cell.part_doubles * D},
                              {f.off_mm, (size_t)c.n * f.gx * 2 * D}}, f.total);
    if (bad) return bad;
    const TetWeightsPlan w = tet_weights_plan(c.n, c.dk, npts);
    return check_buffers(tag, {{w.off_k, (size_t)npts * c.dk * D}, {w.off_e, (size_t)npts * c.n * D}, {w.off_w, (size_t)npts * c.n * D}}, w.total);
}

// ---------------------------------------------------------------- the argument checks
static int check_args() {
    const char* fn = "tetra_plan_check";
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
    const double en[3] = {0.5, -1.0, 0.5};
    const int32_t sel[3] = {2, 0, 1};
    ok(tet_dos_check(fn, 2, 3, mesh, 3, en, 0, 0, nullptr, npts), "three energies");
    if (npts != 20) bad |= printf("npts=%lld\n", (long long)npts);
    ok(tet_dos_check(fn, 3, 3, mesh, 3, en, 1, 3, sel, npts), "three energies per band with a selection");
    no(tet_dos_check(fn, 0, 3, mesh, 3, en, 0, 0, nullptr, npts), "dim_k = 0");
    no(tet_dos_check(fn, 4, 3, mesh, 3, en, 0, 0, nullptr, npts), "dim_k = 4");
    {
        const int32_t mb[3] = {4, 0, 6}, huge[3] = {65536, 32768, 1};
        no(tet_dos_check(fn, 2, 3, mb, 3, en, 0, 0, nullptr, npts), "a mesh axis of 0 points");
        no(tet_dos_check(fn, 2, 3, huge, 3, en, 0, 0, nullptr, npts), "2^31 mesh points");
    }
    no(tet_dos_check(fn, 2, 3, mesh, 0, en, 0, 0, nullptr, npts), "no energy");
    no(tet_dos_check(fn, 2, 3, mesh, 3, nullptr, 0, 0, nullptr, npts), "no energy array");
    {
        std::vector<double> many(65537, 0.25);
        ok(tet_dos_check(fn, 2, 3, mesh, 65536, many.data(), 0, 0, nullptr, npts), "65536 energies");
        no(tet_dos_check(fn, 2, 3, mesh, 65537, many.data(), 0, 0, nullptr, npts), "65537 energies");
        ok(tet_dos_check(fn, 2, 64, mesh, 65536, many.data(), 1, 0, nullptr, npts), "nsta nE at the cap");
        no(tet_dos_check(fn, 2, 65, mesh, 65536, many.data(), 1, 0, nullptr, npts), "nsta nE over the cap");
        ok(tet_dos_check(fn, 2, 3, mesh, 65536, many.data(), 0, 3, sel, npts), "a selection under the cap");
        no(tet_dos_check(fn, 2, 64, mesh, 65536, many.data(), 1, 3, sel, npts), "nsel nsta nE over the cap");
        const double eb[3] = {0.5, nan, 0.1}, ei[3] = {0.5, 0.1, -inf};
        no(tet_dos_check(fn, 2, 3, mesh, 3, eb, 0, 0, nullptr, npts), "a NaN energy");
        no(tet_dos_check(fn, 2, 3, mesh, 3, ei, 0, 0, nullptr, npts), "an infinite energy");
    }
    {
        const int32_t twice[3] = {2, 0, 2}, out[3] = {2, 3, 1}, neg[3] = {2, -1, 1};
        std::vector<int32_t> many(17);
        for (int i = 0; i < 17; ++i) many[i] = i;
        no(tet_dos_check(fn, 2, 3, mesh, 3, en, 0, 3, twice, npts), "a state selected twice");
        no(tet_dos_check(fn, 2, 3, mesh, 3, en, 0, 3, out, npts), "a state out of range");
        no(tet_dos_check(fn, 2, 3, mesh, 3, en, 0, 3, neg, npts), "a negative state");
        no(tet_dos_check(fn, 2, 3, mesh, 3, en, 0, 3, nullptr, npts), "a selection without its list");
        no(tet_dos_check(fn, 2, 3, mesh, 3, en, 0, 0, sel, npts), "a list of no state");
        ok(tet_dos_check(fn, 2, 40, mesh, 3, en, 0, 16, many.data(), npts), "16 states");
        no(tet_dos_check(fn, 2, 40, mesh, 3, en, 0, 17, many.data(), npts), "17 states");
    }
    ok(tet_weights_check(fn, 2, 3, mesh, 0.1, 0, 0, npts), "weights");
    ok(tet_weights_check(fn, 2, 3, mesh, 0.1, 0, 1, npts), "derivative weights");
    ok(tet_weights_check(fn, 3, 3, mesh, 0.1, 1, 0, npts), "corrected weights in 3-D");
    no(tet_weights_check(fn, 2, 3, mesh, 0.1, 1, 0, npts), "the correction in 2-D");
    no(tet_weights_check(fn, 1, 3, mesh, 0.1, 1, 0, npts), "the correction in 1-D");
    no(tet_weights_check(fn, 3, 3, mesh, 0.1, 1, 1, npts), "the correction of the derivative");
    for (double mu : {nan, inf, -inf}) no(tet_weights_check(fn, 2, 3, mesh, mu, 0, 0, npts), "a bad Fermi level");
    {
        const int32_t most[3] = {65536, 32767, 1};
        ok(tet_weights_check(fn, 2, 1, most, 0.1, 0, 0, npts), "just under 2^31 weights");
        no(tet_weights_check(fn, 2, 2, most, 0.1, 0, 0, npts), "more than 2^31 weights");
    }
    ok(tet_fermi_check(fn, 2, 3, mesh, 1.0, npts), "one electron of three");
    ok(tet_fermi_check(fn, 2, 3, mesh, 2.999, npts), "nearly three electrons");
    for (double x : {0.0, 3.0, -0.05, 3.05, nan, inf}) no(tet_fermi_check(fn, 2, 3, mesh, x, npts), "a filling outside (0, nsta)");
    no(tet_fermi_check(fn, 0, 3, mesh, 1.0, npts), "dim_k = 0");
    return bad;
}

int main() {
    int bad = check_cut() ? 1 : 0, cases = 0;
    bad |= check_eval<1>() ? 1 : 0;
    bad |= check_eval<2>() ? 1 : 0;
    bad |= check_eval<3>() ? 1 : 0;
    bad |= check_search() ? 1 : 0;
    for (const Case& c : kCases) {
        bad |= check_case(c) ? 1 : 0;
        ++cases;
    }
    bad |= check_args() ? 1 : 0;
    if (bad) return printf("tetra_plan_check: FAILED\n"), 1;
    printf("tetra_plan_check: the cut, the simplex arithmetic, the search, %d plans and the argument checks ok\n", cases);
    return 0;
}
