// Stand-alone host check of tbk_sparse_flatten_host (no device call): built with the host code of tbk_kpm.hip under
// AddressSanitizer + UBSan by `make -C pythtb_amd/csrc kpm-check` and run as an ordinary program.  Two tables: the spinless
// Haldane cell (dim_k = 2) and a spinful three-orbital molecule (dim_k = 0) with a repeated hop, an R = 0 self-pair and an
// isolated zero-energy orbital.  It expands the CSR table to a dense matrix, compares with the matrix built from the definition
// (ham[i,s,j,t] += amp e^{2 pi i k.(R + tau_j - tau_i)}, plus the Hermitian conjugate), and checks the structure.  The velocity
// bounds of tbk_sparse_velocity_bounds_host (the guard of tbk_kpm_double_moments) are compared with the row sums of the table's
// entries and, as upper bounds, with the row sums of dH/dk_d built from the definition at that k.
// A second part drives kpm_slot_schedule (tbk_kpm.h), the order of steps and reductions every KPM call follows, with callables that
// only record: every step 0 .. nsteps is reduced exactly once, into dots[step] and from the slot it was written to, and no slot is
// written again before its reduction.
#include <complex>
#include <vector>
#include "../tbk_kpm.h"
#include "check_common.h"

// what tbk_kpm.hip takes from tbk_core.hip (this program links the one translation unit alone)

typedef std::complex<double> cplx;

struct Table {
    int dim_k, norb, nspin;
    std::vector<double> orb, onsite, hop_amp;
    std::vector<int32_t> hop_i, hop_j, hop_R;
};

static int check(const Table& t, const double* k, const char* name) {
    const int ns = t.nspin, n = t.norb * ns, dk = t.dim_k;
    const int64_t nhop = (int64_t)t.hop_i.size();
    int64_t nnz = -1;
    double gersh[2] = {0.0, 0.0};
    int rc = tbk_sparse_flatten_host(dk, t.norb, ns, t.orb.data(), t.onsite.data(), nhop, t.hop_i.data(), t.hop_j.data(),
                                     t.hop_R.data(), t.hop_amp.data(), 0, &nnz, nullptr, nullptr, nullptr, nullptr, gersh);
    if (rc || nnz < 0) return printf("%s: sizing call failed: %s\n", name, g_err), 1;
    std::vector<int64_t> row_ptr(n + 1, -1);
    std::vector<int32_t> col(nnz, -1), R(4 * nnz, 99);
    std::vector<double> amp(2 * nnz, 0.0);
    rc = tbk_sparse_flatten_host(dk, t.norb, ns, t.orb.data(), t.onsite.data(), nhop, t.hop_i.data(), t.hop_j.data(), t.hop_R.data(),
                                 t.hop_amp.data(), nnz, &nnz, row_ptr.data(), col.data(), R.data(), amp.data(), gersh);
    if (rc) return printf("%s: %s\n", name, g_err), 1;
    auto phase = [&](int a, int b, const int32_t* Rv, int sign) {
        double x = 0.0;
        for (int d = 0; d < dk; ++d) x += k[d] * (sign * Rv[d] + t.orb[(b / ns) * dk + d] - t.orb[(a / ns) * dk + d]);
        return std::polar(1.0, 2.0 * M_PI * x);
    };
    std::vector<cplx> ref((size_t)n * n), got((size_t)n * n);
    std::vector<cplx> dref[4];
    for (int d = 0; d < dk; ++d) dref[d].assign((size_t)n * n, cplx(0.0, 0.0));
    auto disp = [&](int a, int b, const int32_t* Rv, int sign, int d) { return sign * Rv[d] + t.orb[(b / ns) * dk + d] - t.orb[(a / ns) * dk + d]; };
    for (int o = 0; o < t.norb; ++o)
        for (int s = 0; s < ns; ++s)
            for (int u = 0; u < ns; ++u) {
                const double* p = &t.onsite[2 * ((o * ns + s) * ns + u)];
                ref[(size_t)(o * ns + s) * n + o * ns + u] += cplx(p[0], p[1]);
            }
    for (int64_t h = 0; h < nhop; ++h)
        for (int s = 0; s < ns; ++s)
            for (int u = 0; u < ns; ++u) {
                const double* p = &t.hop_amp[2 * ((h * ns + s) * ns + u)];
                const int a = t.hop_i[h] * ns + s, b = t.hop_j[h] * ns + u;
                const int32_t* Rv = dk ? &t.hop_R[h * dk] : nullptr;
                ref[(size_t)a * n + b] += cplx(p[0], p[1]) * phase(a, b, Rv, 1);
                ref[(size_t)b * n + a] += cplx(p[0], -p[1]) * phase(b, a, Rv, -1);
                for (int d = 0; d < dk; ++d) {
                    dref[d][(size_t)a * n + b] += cplx(0.0, 2.0 * M_PI * disp(a, b, Rv, 1, d)) * cplx(p[0], p[1]) * phase(a, b, Rv, 1);
                    dref[d][(size_t)b * n + a] += cplx(0.0, 2.0 * M_PI * disp(b, a, Rv, -1, d)) * cplx(p[0], -p[1]) * phase(b, a, Rv, -1);
                }
            }
    int bad = 0;
    if (row_ptr[0] != 0 || row_ptr[n] != nnz) bad++;
    for (int a = 0; a < n; ++a) {
        if (row_ptr[a + 1] < row_ptr[a]) bad++;
        for (int64_t e = row_ptr[a]; e < row_ptr[a + 1]; ++e) {
            if (col[e] < 0 || col[e] >= n) {
                bad++;
                continue;
            }
            if (e > row_ptr[a]) {      // (col, R) strictly ascending
                int c = col[e - 1] < col[e] ? -1 : (col[e - 1] > col[e] ? 1 : 0);
                for (int d = 0; d < 4 && c == 0; ++d) c = R[4 * (e - 1) + d] < R[4 * e + d] ? -1 : (R[4 * (e - 1) + d] > R[4 * e + d] ? 1 : 0);
                if (c >= 0) bad++;
            }
            got[(size_t)a * n + col[e]] += cplx(amp[2 * e], amp[2 * e + 1]) * phase(a, col[e], &R[4 * e], 1);
        }
    }
    double vb[4] = {-1.0, -1.0, -1.0, -1.0};
    rc = tbk_sparse_velocity_bounds_host(dk, t.norb, ns, t.orb.data(), t.onsite.data(), nhop, t.hop_i.data(), t.hop_j.data(), t.hop_R.data(),
                                         t.hop_amp.data(), vb);
    if (rc) return printf("%s: velocity bounds: %s\n", name, g_err), 1;
    for (int d = 0; d < 4; ++d) {
        double table = 0.0, dense = 0.0;     // largest row sum of the table's entries, and of |dH/dk_d| at this k
        for (int a = 0; a < n && d < dk; ++a) {
            double rs = 0.0, rd = 0.0;
            for (int64_t e = row_ptr[a]; e < row_ptr[a + 1]; ++e)
                if (col[e] >= 0 && col[e] < n) rs += 2.0 * M_PI * std::abs(cplx(amp[2 * e], amp[2 * e + 1])) * std::fabs(disp(a, col[e], &R[4 * e], 1, d));
            for (int b = 0; b < n; ++b) rd += std::abs(dref[d][(size_t)a * n + b]);
            table = std::max(table, rs);
            dense = std::max(dense, rd);
        }
        if (!(std::fabs(vb[d] - table) <= 1e-14 * (1.0 + table)) || !(dense <= vb[d] * (1.0 + 1e-14) + 1e-300) || (d >= dk && vb[d] != 0.0)) {
            printf("%s: velocity bound of axis %d is %g, the table gives %g, |dH/dk| at k has row sum %g\n", name, d, vb[d], table, dense);
            bad++;
        }
    }
    double err = 0.0, big = 0.0;
    for (size_t i = 0; i < ref.size(); ++i) {
        err = std::max(err, std::abs(ref[i] - got[i]));
        big = std::max(big, std::abs(ref[i]));
    }
    printf("%s: n = %d, nnz = %lld, Gershgorin (%g, %g), |csr - dense| = %.2e of %.2e, structure faults %d\n", name, n, (long long)nnz,
           gersh[0], gersh[1], err, big, bad);
    return (bad || !(err <= 1e-14 * big) || !(gersh[0] < gersh[1])) ? 1 : 0;
}

// slot_of[s] = the step slot s holds and has not given up yet (-1: free); reduced[j] = how often step j reached dots[j]
static int check_schedule(int nsteps, int nslots) {
    std::vector<int> slot_of((size_t)nslots, -1), reduced((size_t)nsteps + 1, 0);
    int bad = 0;
    slot_of[0] = 0;      // the start vectors
    int rc = kpm_slot_schedule(
        nsteps, nslots,
        [&](int j, int slot) {
            if (slot < 0 || slot >= nslots || slot_of[(size_t)slot] != -1) return ++bad;     // outside part, or over an unreduced step
            slot_of[(size_t)slot] = j;
            return 0;
        },
        [&](int first, int count) {
            if (count < 1 || count > nslots || first < 0 || first + count > nsteps + 1) return ++bad;
            for (int i = 0; i < count; ++i) {          // k_kpm_reduce: dots[first + i] = the sums of slot i
                if (slot_of[(size_t)i] != first + i) bad++;
                else reduced[(size_t)(first + i)]++;
                slot_of[(size_t)i] = -1;
            }
            return 0;
        });
    for (int j = 0; j <= nsteps; ++j)
        if (reduced[(size_t)j] != 1) bad++;
    if (rc || bad) printf("slot schedule nsteps = %d, nslots = %d: rc %d, %d faults\n", nsteps, nslots, rc, bad);
    return (rc || bad) ? 1 : 0;
}

int main() {
    int fail = 0;
    for (int nsteps : {0, 1, 2, 127, 128, 129, 300})
        for (int nslots : {1, 2, 128}) fail += check_schedule(nsteps, nslots);
    if (kpm_plan(65569, 300).nwg != 2048 || kpm_plan(65569, 300).nslots != 128 || kpm_plan(33, 0).nwg != 2 || kpm_plan(33, 0).nslots != 1)
        fail += printf("kpm_plan: unexpected launch plan\n");
    {
        Table t{2, 2, 1, {1.0 / 3, 1.0 / 3, 2.0 / 3, 2.0 / 3}, {-0.2, 0.0, 0.2, 0.0}, {}, {}, {}, {}};
        const double t2[2] = {0.0, 0.15};
        const int hops[9][4] = {{0, 1, 0, 0}, {1, 0, 1, 0}, {1, 0, 0, 1}, {0, 0, 1, 0}, {1, 1, 1, -1}, {1, 1, 0, 1}, {1, 1, 1, 0}, {0, 0, 1, -1}, {0, 0, 0, 1}};
        for (int h = 0; h < 9; ++h) {
            t.hop_i.push_back(hops[h][0]);
            t.hop_j.push_back(hops[h][1]);
            t.hop_R.push_back(hops[h][2]);
            t.hop_R.push_back(hops[h][3]);
            t.hop_amp.push_back(h < 3 ? -1.0 : t2[0]);
            t.hop_amp.push_back(h < 3 ? 0.0 : (h < 6 ? t2[1] : -t2[1]));
        }
        const double k[2] = {0.137, 0.731};
        fail += check(t, k, "haldane");
    }
    {
        Table t{0, 3, 2, {}, {}, {}, {}, {}, {}};
        const double on[3][8] = {{0.5, 0, 0.1, -0.2, 0.1, 0.2, -0.3, 0}, {-0.4, 0, 0, 0, 0, 0, 0.7, 0}, {0, 0, 0, 0, 0, 0, 0, 0}};
        for (auto& o : on) t.onsite.insert(t.onsite.end(), o, o + 8);
        const int hops[3][2] = {{0, 1}, {0, 1}, {1, 1}};     // a repeated hop and an R = 0 self-pair; orbital 2 is isolated
        const double amps[3][8] = {{1, 0.5, 0.2, 0, -0.3, 0.1, 0.9, -0.4}, {1, 0.5, 0.2, 0, -0.3, 0.1, 0.9, -0.4}, {0.3, 0.2, 0.1, 0.6, -0.2, 0.4, 0.05, -0.1}};
        for (int h = 0; h < 3; ++h) {
            t.hop_i.push_back(hops[h][0]);
            t.hop_j.push_back(hops[h][1]);
            t.hop_amp.insert(t.hop_amp.end(), amps[h], amps[h] + 8);
        }
        fail += check(t, nullptr, "molecule");
    }
    // argument errors come back as codes
    int64_t nnz = 0;
    const double on1[2] = {0.0, 0.0};
    const int32_t bad_i[1] = {3}, ok_j[1] = {0};
    const double amp1[2] = {1.0, 0.0};
    if (tbk_sparse_flatten_host(0, 1, 1, nullptr, on1, 1, bad_i, ok_j, nullptr, amp1, 0, &nnz, nullptr, nullptr, nullptr, nullptr, nullptr) !=
        TBK_EINVAL)
        fail += printf("orbital index out of range not refused\n");
    printf(fail ? "FAILED\n" : "kpm_flatten_check ok\n");
    return fail ? 1 : 0;
}
