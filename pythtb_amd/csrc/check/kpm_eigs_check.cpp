// Stand-alone host check of the host-only parts of tbk_kpm_eigs (tbk_kpm_eigs.h; no device call): built under AddressSanitizer +
// UBSan by `make -C pythtb_amd/csrc eigs-check` and run as an ordinary program.
//   1. kpm_eigs_coefficients against the closed form in long double, and the filter they make: 1/2 at the widened edges, >= 1/2 on
//      the window, small far outside, finite when the widening is clipped at the bounds.
//   2. kpm_eigs_check_args: every error case of include/tbk.h returns TBK_EINVAL, the good calls TBK_OK.
//   3. KpmEigsWork::carve over a real host block: every buffer starts at a multiple of 256, none overlaps another (each is
//      filled with its own index and read back under the sanitizer), the total holds 3 n_search nsta 16 bytes.
//   4. The dense algebra between two device passes on a synthetic subspace with dependent columns: the sums in the layout of
//      k_kpm_gram -> kpm_eigs_assemble -> (a Jacobi eigh of this program in the place of the device solver) -> kpm_eigs_whiten ->
//      kpm_eigs_project -> kpm_eigs_rotation: the rotated columns are orthonormal, the ones past the rank zero, and the Ritz
//      values those of the operator on the span.
//   5. kpm_eigs_verdict: selection, order, saturation and the NaN residual.
#include <complex>
#include <vector>
#include "../tbk_kpm_eigs.h"
#include "check_common.h"

typedef std::complex<double> cplx;

static double filter_at(const std::vector<double>& c, double x) {
    double s = 0.0;
    const double th = acos(x);
    for (size_t m = 0; m < c.size(); ++m) s += c[m] * cos((double)m * th);
    return s;
}

static int check_coefficients() {
    const double emin = -4.2, emax = 4.1, a = 0.5 * (emax - emin), b = 0.5 * (emax + emin);
    int bad = 0;
    for (int degree : {2, 64, 257, 4096}) {
        const double e_lo = -0.35, e_hi = 0.4;
        std::vector<double> c((size_t)degree + 1);
        kpm_eigs_coefficients(e_lo, e_hi, emin, emax, degree, c.data());
        double w_lo, w_hi;
        kpm_eigs_widened(e_lo, e_hi, emin, emax, degree, &w_lo, &w_hi);
        const long double tl = acosl(((long double)w_lo - b) / a), th = acosl(((long double)w_hi - b) / a), pi = acosl(-1.0L);
        const int M = degree + 1;
        double worst = 0.0;
        for (int m = 0; m < M; ++m) {
            const long double q = pi / (M + 1.0L);
            const long double g = ((M - m + 1.0L) * cosl(q * m) + sinl(q * m) / tanl(q)) / (M + 1.0L);
            const long double ref = g * (m == 0 ? (tl - th) / pi : 2.0L * (sinl(m * tl) - sinl(m * th)) / (m * pi));
            worst = std::max(worst, (double)fabsl(ref - c[(size_t)m]));
        }
        // a widened edge clipped to the bounds sits where arccos is ill-conditioned: 1e-9 a from the end, an error of ~1e-12
        const bool clipped = w_lo > e_lo - 2.0 * M_PI * a / degree || w_hi < e_hi + 2.0 * M_PI * a / degree;
        if (worst > (clipped ? 1e-11 : 1e-13)) bad += printf("coefficients, degree %d: %.2e from the closed form\n", degree, worst);
        if (degree < 64) continue;
        const double p_lo = filter_at(c, (w_lo - b) / a), p_hi = filter_at(c, (w_hi - b) / a);
        if (fabs(p_lo - 0.5) > 1e-2 || fabs(p_hi - 0.5) > 1e-2) bad += printf("degree %d: filter at the widened edges %g %g\n", degree, p_lo, p_hi);
        for (int i = 0; i <= 20; ++i) {
            const double e = e_lo + (e_hi - e_lo) * i / 20.0, p = filter_at(c, (e - b) / a);
            if (!(p >= 0.5 && p <= 1.0 + 1e-12)) bad += printf("degree %d: filter %g at %g inside the window\n", degree, p, e);
        }
        const double delta = 2.0 * M_PI * a / degree;
        for (double e : {w_lo - 3.0 * delta, w_hi + 3.0 * delta})
            if (e > emin && e < emax && fabs(filter_at(c, (e - b) / a)) > 1e-2) bad += printf("degree %d: filter %g at %g outside\n", degree, filter_at(c, (e - b) / a), e);
    }
    {   // a window at the edge of the bounds: the widening is clipped, every coefficient finite
        std::vector<double> c(65);
        kpm_eigs_coefficients(emin + 1e-3, emin + 0.2, emin, emax, 64, c.data());
        for (double x : c)
            if (!std::isfinite(x)) bad += printf("clipped window: coefficient not finite\n");
        double w_lo, w_hi;
        kpm_eigs_widened(emin + 1e-3, emax - 1e-3, emin, emax, 64, &w_lo, &w_hi);
        if (!(w_lo > emin && w_hi < emax)) bad += printf("clipped window: (%g, %g)\n", w_lo, w_hi);
    }
    return bad;
}

static int check_args() {
    tbk_sparse sp;
    sp.nsta = 126;
    sp.dim_k = 0;
    int nf = 0, bad = 0;
    double ev[8], vec[16];
    int32_t info[4];
    auto call = [&](const tbk_sparse* s, const double* k, double lo, double hi, double emin, double emax, int ns, int deg, double tol,
                    int it, int* n_found = nullptr) {
        return kpm_eigs_check_args(s, k, lo, hi, emin, emax, ns, deg, tol, it, n_found, ev, vec, info);
    };
    const double inf = INFINITY;
    struct { int got, want; const char* what; } rows[] = {
        {call(&sp, nullptr, -0.3, 0.3, -4, 4, 64, 128, 1e-10, 40, &nf), TBK_OK, "a good call"},
        {call(&sp, nullptr, 0.1, 0.1, -4, 4, 8, 2, 1e-10, 2, &nf), TBK_OK, "a window of one point, the smallest arguments"},
        {call(&sp, nullptr, -0.3, 0.3, -4, 4, 120, 128, 1e-10, 40, &nf), TBK_OK, "n_search = nsta rounded down to 8"},
        {call(nullptr, nullptr, -0.3, 0.3, -4, 4, 64, 128, 1e-10, 40, &nf), TBK_EINVAL, "null operator"},
        {call(&sp, nullptr, -0.3, 0.3, -4, 4, 64, 128, 1e-10, 40, nullptr), TBK_EINVAL, "null n_found"},
        {call(&sp, nullptr, 0.3, -0.3, -4, 4, 64, 128, 1e-10, 40, &nf), TBK_EINVAL, "empty window"},
        {call(&sp, nullptr, -4.0, 0.3, -4, 4, 64, 128, 1e-10, 40, &nf), TBK_EINVAL, "window at emin"},
        {call(&sp, nullptr, -0.3, 4.5, -4, 4, 64, 128, 1e-10, 40, &nf), TBK_EINVAL, "window beyond emax"},
        {call(&sp, nullptr, -0.3, inf, -4, 4, 64, 128, 1e-10, 40, &nf), TBK_EINVAL, "infinite window"},
        {call(&sp, nullptr, -0.3, 0.3, 4, -4, 64, 128, 1e-10, 40, &nf), TBK_EINVAL, "bounds reversed"},
        {call(&sp, nullptr, -0.3, 0.3, -4, 4, 0, 128, 1e-10, 40, &nf), TBK_EINVAL, "n_search 0"},
        {call(&sp, nullptr, -0.3, 0.3, -4, 4, 12, 128, 1e-10, 40, &nf), TBK_EINVAL, "n_search not a multiple of 8"},
        {call(&sp, nullptr, -0.3, 0.3, -4, 4, 128, 128, 1e-10, 40, &nf), TBK_EINVAL, "n_search above nsta"},
        {call(&sp, nullptr, -0.3, 0.3, -4, 4, 64, 1, 1e-10, 40, &nf), TBK_EINVAL, "degree 1"},
        {call(&sp, nullptr, -0.3, 0.3, -4, 4, 64, KPME_MAX_DEGREE + 1, 1e-10, 40, &nf), TBK_EINVAL, "degree too large"},
        {call(&sp, nullptr, -0.3, 0.3, -4, 4, 64, 128, 0.0, 40, &nf), TBK_EINVAL, "tol 0"},
        {call(&sp, nullptr, -0.3, 0.3, -4, 4, 64, 128, NAN, 40, &nf), TBK_EINVAL, "tol NaN"},
        {call(&sp, nullptr, -0.3, 0.3, -4, 4, 64, 128, 1e-10, 1, &nf), TBK_EINVAL, "max_iter 1"},
    };
    for (const auto& r : rows)
        if (r.got != r.want) bad += printf("argument check, %s: %d, not %d\n", r.what, r.got, r.want);
    tbk_sparse per;
    per.nsta = 5000;
    per.dim_k = 2;
    const double k[2] = {0.1, 0.2};
    if (call(&per, nullptr, -0.3, 0.3, -4, 4, 64, 128, 1e-10, 40, &nf) != TBK_EINVAL) bad += printf("argument check: null k accepted\n");
    if (call(&per, k, -0.3, 0.3, -4, 4, 2048, 128, 1e-10, 40, &nf) != TBK_OK) bad += printf("argument check: n_search 2048 refused\n");
    if (call(&per, k, -0.3, 0.3, -4, 4, 2056, 128, 1e-10, 40, &nf) != TBK_EINVAL) bad += printf("argument check: n_search 2056 accepted\n");
    return bad;
}

static int check_layout() {
    int bad = 0;
    const int shapes[][4] = {{15, 8, 64, 1}, {63, 56, 2, 0}, {240, 72, 257, 0}, {2112, 64, 512, 0}, {65569, 8, 64, 1}, {5000, 1024, 64, 2}};
    for (const auto& s : shapes) {
        tbk_sparse sp;
        sp.nsta = s[0];
        sp.dim_k = s[3];
        sp.nnz = 7 * (int64_t)s[0];
        KpmEigsWork w(&sp, s[1], s[2]);
        KpmCarve c;
        w.carve(c);
        const size_t total = c.off;
        if (total < (size_t)3 * s[1] * s[0] * 16) bad += printf("layout %d x %d: total %zu below X, Y, HY\n", s[0], s[1], total);
        unsigned char* base = (unsigned char*)aligned_alloc(256, total);
        if (!base) return printf("layout: no host block of %zu bytes\n", total), 1;
        c = KpmCarve{base, 0};
        w.carve(c);
        constexpr int NV = KPM_NV, NC = 2 * NV;
        const size_t bl = (size_t)s[0] * NV, nn = (size_t)s[1] * s[1];
        struct { void* p; size_t bytes; } buf[] = {
            {w.val, (s[3] > 0 ? (size_t)sp.nnz : 0) * 16}, {w.X, w.nb * bl * 16}, {w.Y, w.nb * bl * 16}, {w.HY, w.nb * bl * 16},
            {w.cur, bl * 16}, {w.prev, bl * 16}, {w.coef, ((size_t)s[2] + 1) * 16}, {w.part, w.P.part_len() * 8},
            {w.dots, ((size_t)s[2] + 1) * NC * 8}, {w.rec, KPMS_GUARD * 8}, {w.gpart, (size_t)w.pair_chunk * 256 * w.gram_wg * 8},
            {w.gram, (size_t)w.npairs * 256 * 8}, {w.rot, nn * 16}, {w.eig_h, nn * 16}, {w.eig_v, nn * 16}, {w.eig_e, (size_t)s[1] * 8},
            {w.theta, (size_t)s[1] * 8}, {w.res, (size_t)w.nb * NC * 8}, {w.k_dev, (size_t)std::max(s[3], 1) * 8}};
        int i = 0;
        for (const auto& b : buf) {
            ++i;
            if (!b.bytes) continue;
            const size_t off = (size_t)((unsigned char*)b.p - base);
            if (!b.p || off % 256 || off + b.bytes > total) bad += printf("layout %d x %d: buffer %d at %zu + %zu of %zu\n", s[0], s[1], i, off, b.bytes, total);
            else memset(b.p, i, b.bytes);
        }
        i = 0;
        for (const auto& b : buf) {
            ++i;
            const unsigned char* p = (const unsigned char*)b.p;
            for (size_t j = 0; j < b.bytes; j += (j + 4096 < b.bytes ? 4096 : 1))
                if (p[j] != (unsigned char)i) {
                    bad += printf("layout %d x %d: buffer %d is overwritten at byte %zu\n", s[0], s[1], i, j);
                    break;
                }
        }
        if (w.gram_wg < 1 || w.gram_wg > KPME_GRAM_WG || w.pair_chunk < 1 || w.pair_chunk > KPME_GRAM_PAIRS)
            bad += printf("layout %d x %d: gram grid %d x %d\n", s[0], s[1], w.gram_wg, w.pair_chunk);
        free(base);
    }
    return bad;
}

// cyclic Jacobi for a Hermitian matrix (row-major, destroyed): lam ascending, V[d][i] = component i of eigenvector d
static void jacobi_eigh(int n, std::vector<cplx> a, double* lam, cd* V) {
    std::vector<cplx> v((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) v[(size_t)i * n + i] = 1.0;
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < n; ++p)
            for (int q = p + 1; q < n; ++q) off += std::norm(a[(size_t)p * n + q]);
        if (off < 1e-300) break;
        for (int p = 0; p < n; ++p)
            for (int q = p + 1; q < n; ++q) {
                const cplx apq = a[(size_t)p * n + q];
                if (std::abs(apq) == 0.0) continue;
                const double app = a[(size_t)p * n + p].real(), aqq = a[(size_t)q * n + q].real();
                const cplx ph = apq / std::abs(apq);
                const double th = 0.5 * atan2(2.0 * std::abs(apq), app - aqq), c = cos(th), s = sin(th);
                for (int k = 0; k < n; ++k) {       // columns p, q <- (c p + s conj(ph) q, -s ph p + c q)
                    const cplx x = a[(size_t)k * n + p], y = a[(size_t)k * n + q];
                    a[(size_t)k * n + p] = c * x + s * std::conj(ph) * y;
                    a[(size_t)k * n + q] = -s * ph * x + c * y;
                    const cplx vx = v[(size_t)k * n + p], vy = v[(size_t)k * n + q];
                    v[(size_t)k * n + p] = c * vx + s * std::conj(ph) * vy;
                    v[(size_t)k * n + q] = -s * ph * vx + c * vy;
                }
                for (int k = 0; k < n; ++k) {       // rows, with the conjugate transformation
                    const cplx x = a[(size_t)p * n + k], y = a[(size_t)q * n + k];
                    a[(size_t)p * n + k] = c * x + s * ph * y;
                    a[(size_t)q * n + k] = -s * std::conj(ph) * x + c * y;
                }
            }
    }
    std::vector<int> order((size_t)n);
    for (int i = 0; i < n; ++i) order[(size_t)i] = i;
    std::sort(order.begin(), order.end(), [&](int x, int y) { return a[(size_t)x * n + x].real() < a[(size_t)y * n + y].real(); });
    for (int d = 0; d < n; ++d) {
        lam[d] = a[(size_t)order[(size_t)d] * n + order[(size_t)d]].real();
        for (int i = 0; i < n; ++i) {
            const cplx z = v[(size_t)i * n + order[(size_t)d]];
            V[(size_t)d * n + i] = cd{z.real(), z.imag()};
        }
    }
}

static int check_algebra() {
    constexpr int NV = KPM_NV;
    const int n = 40, nb = 2, ns = nb * NV, true_rank = 11;
    int bad = 0;
    unsigned long long seed = 12345;
    auto rnd = [&]() {
        seed = seed * 6364136223846793005ull + 1442695040888963407ull;
        return (double)(seed >> 11) * 0x1.0p-53 - 0.5;
    };
    // Y = Q C: Q n x true_rank random, C true_rank x ns random -> rank 11 of 16; H = diag(h)
    std::vector<cplx> Q((size_t)n * true_rank), Cm((size_t)true_rank * ns), Y((size_t)n * ns, 0.0);
    std::vector<double> h((size_t)n);
    for (auto& z : Q) z = cplx(rnd(), rnd());
    for (auto& z : Cm) z = cplx(rnd(), rnd());
    for (auto& x : h) x = 3.0 * rnd();
    for (int r = 0; r < n; ++r)
        for (int j = 0; j < ns; ++j)
            for (int t = 0; t < true_rank; ++t) Y[(size_t)r * ns + j] += Q[(size_t)r * true_rank + t] * Cm[(size_t)t * ns + j];
    // the sums in the layout of k_kpm_gram, upper block triangle
    std::vector<double> gram((size_t)(nb * (nb + 1) / 2) * 4 * NV * NV, 0.0);
    int pair = 0;
    for (int p = 0; p < nb; ++p)
        for (int q = p; q < nb; ++q, ++pair)
            for (int i = 0; i < NV; ++i)
                for (int j = 0; j < NV; ++j) {
                    cplx g = 0.0, a = 0.0;
                    for (int r = 0; r < n; ++r) {
                        g += std::conj(Y[(size_t)r * ns + p * NV + i]) * Y[(size_t)r * ns + q * NV + j];
                        a += std::conj(Y[(size_t)r * ns + p * NV + i]) * h[(size_t)r] * Y[(size_t)r * ns + q * NV + j];
                    }
                    double* s = gram.data() + (size_t)pair * 4 * NV * NV;
                    s[i * NV + j] = g.real();
                    s[NV * NV + i * NV + j] = g.imag();
                    s[2 * NV * NV + i * NV + j] = a.real();
                    s[3 * NV * NV + i * NV + j] = a.imag();
                }
    std::vector<cd> G((size_t)ns * ns), A((size_t)ns * ns), U((size_t)ns * ns), wh((size_t)ns * ns), tmp((size_t)ns * ns), B((size_t)ns * ns),
        W((size_t)ns * ns), rot((size_t)ns * ns);
    std::vector<double> lam((size_t)ns), theta((size_t)ns);
    kpm_eigs_assemble(nb, gram.data(), G.data(), A.data());
    for (int r = 0; r < ns; ++r)
        for (int c = 0; c < ns; ++c)
            if (G[(size_t)r * ns + c].x != G[(size_t)c * ns + r].x || G[(size_t)r * ns + c].y != -G[(size_t)c * ns + r].y) bad += printf("assemble: G not Hermitian\n");
    std::vector<cplx> Gc((size_t)ns * ns);
    for (size_t i = 0; i < Gc.size(); ++i) Gc[i] = cplx(G[i].x, G[i].y);
    jacobi_eigh(ns, Gc, lam.data(), U.data());
    const int rank = kpm_eigs_whiten(ns, lam.data(), U.data(), wh.data());
    if (rank != true_rank) bad += printf("whiten: rank %d, not %d\n", rank, true_rank);
    kpm_eigs_project(ns, rank, A.data(), wh.data(), tmp.data(), B.data());
    std::vector<cplx> Bc((size_t)rank * rank);
    for (size_t i = 0; i < Bc.size(); ++i) Bc[i] = cplx(B[i].x, B[i].y);
    jacobi_eigh(rank, Bc, theta.data(), W.data());
    kpm_eigs_rotation(ns, rank, wh.data(), W.data(), rot.data());
    // X = Y rot: orthonormal Ritz vectors, zero past the rank
    std::vector<cplx> X((size_t)n * ns, 0.0);
    for (int r = 0; r < n; ++r)
        for (int s = 0; s < ns; ++s)
            for (int i = 0; i < ns; ++i) X[(size_t)r * ns + s] += Y[(size_t)r * ns + i] * cplx(rot[(size_t)i * ns + s].x, rot[(size_t)i * ns + s].y);
    double e_orth = 0.0, e_ritz = 0.0, e_zero = 0.0;
    for (int s = 0; s < ns; ++s)
        for (int t = 0; t < ns; ++t) {
            cplx o = 0.0, m = 0.0;
            for (int r = 0; r < n; ++r) {
                o += std::conj(X[(size_t)r * ns + s]) * X[(size_t)r * ns + t];
                m += std::conj(X[(size_t)r * ns + s]) * h[(size_t)r] * X[(size_t)r * ns + t];
            }
            if (s >= rank || t >= rank) {
                e_zero = std::max(e_zero, std::abs(o));
                continue;
            }
            e_orth = std::max(e_orth, std::abs(o - (s == t ? 1.0 : 0.0)));
            e_ritz = std::max(e_ritz, std::abs(m - (s == t ? theta[(size_t)s] : 0.0)));
        }
    printf("subspace algebra: rank %d of %d, orthonormality %.1e, X^H H X - theta %.1e, columns past the rank %.1e\n", rank, ns, e_orth,
           e_ritz, e_zero);
    if (e_orth > 1e-10 || e_ritz > 1e-10 || e_zero != 0.0) bad += printf("subspace algebra: beyond 1e-10\n");
    return bad;
}

static int check_verdict() {
    int bad = 0, sel[8];
    const double theta[6] = {-0.5, -0.1, 0.05, 0.2, 0.3, 0.9}, tau[6] = {0.9, 0.8, 0.3, 0.99, 0.7, 0.6};
    double resid[6] = {1.0, 1e-12, 5.0, 2e-11, 3e-11, 1.0};
    KpmEigsVerdict v = kpm_eigs_verdict(6, theta, resid, tau, -0.3, 0.3, 1e-10, sel);
    if (v.nstrong != 5 || v.nsel != 3 || sel[0] != 1 || sel[1] != 3 || sel[2] != 4 || !v.converged || !v.room || v.worst != 3e-11)
        bad += printf("verdict: strong %d selected %d converged %d room %d worst %g\n", v.nstrong, v.nsel, v.converged, v.room, v.worst);
    v = kpm_eigs_verdict(5, theta, resid, tau, -0.3, 0.3, 1e-11, sel);      // the spurious pair (tau 0.3) is no direction less
    if (v.converged || v.nstrong != 4 || !v.room) bad += printf("verdict: tighter limit\n");
    const double all[6] = {0.9, 0.9, 0.9, 0.9, 0.9, 0.9};
    v = kpm_eigs_verdict(6, theta, resid, all, -0.3, 0.3, 10.0, sel);
    if (!v.converged || v.room || v.nsel != 4) bad += printf("verdict: saturated subspace not seen\n");
    resid[3] = NAN;
    v = kpm_eigs_verdict(6, theta, resid, tau, -0.3, 0.3, 1e-10, sel);
    if (v.converged) bad += printf("verdict: a NaN residual passes\n");
    v = kpm_eigs_verdict(6, theta, resid, tau, 0.4, 0.6, 1e-10, sel);        // no pair in the window: converged, nothing selected
    if (!v.converged || v.nsel != 0) bad += printf("verdict: empty window\n");
    return bad;
}

int main() {
    int bad = check_coefficients() + check_args() + check_layout() + check_algebra() + check_verdict();
    if (bad) return printf("kpm_eigs_check: FAILED\n"), 1;
    printf("kpm_eigs_check: ok\n");
    return 0;
}
