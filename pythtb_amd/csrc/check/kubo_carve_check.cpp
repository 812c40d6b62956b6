// Stand-alone host check of KuboCarve (tbk_kubo.h; no device call): built under AddressSanitizer + UBSan by
// `make -C pythtb_amd/csrc kubo-check` and run as an ordinary program.  It registers the buffer lists of the ten host entries that
// carve their workspace with it (gen_dham, curv_list, curv_mesh, tbk_orb_moment_list, tbk_orb_mag_mesh, tbk_band_velocity_list,
// tbk_anom_transport_mesh, tbk_drude_mesh, tbk_qgt_list, tbk_qgt_mesh in both branches) at n = 1, 2, 16, 33 states, 2-D and 3-D
// meshes, band set, Fermi and kT variants, over a real host block of the requested size, and checks: a buffer of zero bytes is
// null, every other one starts at a multiple of 256 behind the 256 leading bytes, the last one ends at the total, and no two
// overlap (every buffer is filled with its own index and read back, under the sanitizer).  The lists below are copies of the
// entries' registrations, written out by hand: the program checks the carver's arithmetic on lists of their shape, not the call
// sites, and has to follow an entry whose list changes.  A ninth buffer must be refused (KuboCarve::full).
#include <vector>
#include "../tbk_kubo.h"
#include "check_common.h"

// what tbk_kubo.h's host functions take from tbk_core.hip (this program links no translation unit of the library)

static int g_lists = 0;

// one entry's list: the byte counts in registration order
static int verify(const char* name, const std::vector<size_t>& bytes) {
    std::vector<unsigned char*> buf(bytes.size(), (unsigned char*)&buf);   // (anything but null: place() must set every pointer)
    if (buf.size() > (size_t)KuboCarve::kMax) return printf("%s: %zu buffers\n", name, buf.size()), 1;
    KuboCarve ws;
    for (size_t i = 0; i < bytes.size(); ++i) ws.add(buf[i], bytes[i]);
    unsigned char* base = (unsigned char*)aligned_alloc(256, ws.total);
    if (!base) return printf("%s: no host block of %zu bytes\n", name, ws.total), 1;
    ws.place(base);
    size_t end = 256;
    int bad = 0;
    for (int i = 0; i < ws.cnt && !bad; ++i) {
        unsigned char* p = buf[i];
        if (!bytes[i]) {
            if (p) bad = printf("%s: buffer %d of zero bytes is not null\n", name, i);
            continue;
        }
        if (!p || p < base || (size_t)(p - base) % 256 || (size_t)(p - base) < end)
            bad = printf("%s: buffer %d at offset %td (the previous one ends at %zu)\n", name, i, p - base, end);
        else {
            end = (size_t)(p - base) + bytes[i];
            memset(p, i + 1, bytes[i]);
        }
    }
    if (!bad && al256(end) != ws.total) bad = printf("%s: the last buffer ends at %zu, the total is %zu\n", name, end, ws.total);
    for (int i = 0; i < ws.cnt && !bad; ++i) {
        const unsigned char* p = buf[i];
        for (size_t j = 0; j < bytes[i]; ++j)
            if (p[j] != (unsigned char)(i + 1)) {
                bad = printf("%s: buffer %d is overwritten at byte %zu\n", name, i, j);
                break;
            }
    }
    free(base);
    ++g_lists;
    return bad ? 1 : 0;
}

int main() {
    const size_t D = sizeof(double), C = sizeof(cd);
    const int sizes[4] = {1, 2, 16, 33};
    const int meshes[2][3] = {{7, 5, 1}, {6, 5, 4}};
    const int64_t nk = 70;
    const int nmu = 37;
    int bad = 0;
    for (int n : sizes)
        for (int dk = 2; dk <= 3; ++dk) {
            const int* N = meshes[dk - 2];
            const int64_t npts = (int64_t)N[0] * N[1] * N[2];
            PlaneArgs P{};
            P.npts = npts;
            P.nplane = (int64_t)N[0] * N[1];
            P.nslice = N[2];
            const size_t nn = (size_t)n * n;
            for (int spin = 0; spin < 2; ++spin)
                bad |= verify("gen_dham", {(size_t)nk * dk * D, nk * nn * C, spin ? nk * nn * C : 0});
            bad |= verify("tbk_band_velocity_list", {(size_t)nk * dk * D, (size_t)dk * n * nk * D, KuboChunks(n, dk, kubo_chunk_len(n, nk), 0, 0, 0).bytes()});
            for (int variant = 0; variant < 4; ++variant) {   // per band, band set, Fermi, kT
                const bool manifold = variant == 1, fermi = variant >= 2, hot = variant == 3, general = n != 2;
                const size_t cl = kubo_contract_chunks(n, dk, nk, manifold, 3).bytes(), cm = kubo_contract_chunks(n, dk, npts, manifold, 3).bytes();
                if (variant < 2) {
                    const size_t nout = (size_t)(manifold ? 1 : n) * nk;
                    bad |= verify("curv_list", {(size_t)nk * dk * D, nout * D, general ? cl : 0});
                    bad |= verify("tbk_orb_moment_list", {(size_t)nk * dk * D, (manifold && general ? 3 * nk : nout) * D, general ? cl : 0});
                    bad |= verify("tbk_qgt_list", {(size_t)nk * dk * D, nout * dk * dk * D, general ? cl : 0});
                }
                if (!hot) {
                    const int nch = fermi ? nmu : (manifold || !general ? 1 : n);
                    const int gx = fermi ? kubo_fermi_gx(P, n, nmu, 1) : kubo_plane_gx(P);
                    const size_t nrows = (size_t)P.nslice * nch;
                    bad |= verify("curv_mesh", {nrows * gx * D, nrows * D, (size_t)(fermi ? nmu : 1) * D,
                                                general ? (size_t)(manifold ? 1 : n) * npts * D : 0, general && fermi ? n * npts * D : 0,
                                                general ? cm : 0});
                }
                if (variant >= 1) {
                    const int gx = manifold ? kubo_plane_gx(P) : (hot ? kubo_thermal_groups(P, n, nmu, 1) : kubo_fermi_gx(P, n, nmu, 2));
                    const size_t nrows = (size_t)P.nslice * (manifold ? 3 : (hot ? nmu : 2 * nmu));
                    bad |= verify("tbk_orb_mag_mesh", {nrows * gx * D, nrows * D, (size_t)(fermi ? nmu : 1) * D,
                                                       general && manifold ? 3 * npts * D : 0,
                                                       (general && !manifold) || hot ? 3 * n * npts * D : 0, general ? cm : 0});
                }
                if (hot) {
                    const int nq = 2 + dk, nw = dk * (dk + 1) / 2;
                    const size_t rec = (size_t)n * npts * D;
                    size_t nrows = (size_t)P.nslice * nmu * nq;
                    bad |= verify("tbk_anom_transport_mesh", {nrows * kubo_thermal_groups(P, n, nmu, nq) * D, nrows * D, nmu * D, nq * rec,
                                                              n > 32 ? dk * rec : 0, kubo_contract_chunks(n, dk, npts, false, 1).bytes()});
                    PlaneArgs W = P;
                    W.nplane = npts;
                    W.nslice = 1;
                    nrows = (size_t)nmu * nw;
                    bad |= verify("tbk_drude_mesh", {nrows * kubo_thermal_groups(W, n, nmu, nw) * D, nrows * D, nmu * D, (1 + nw) * rec,
                                                     n > 32 ? dk * rec : 0, KuboChunks(n, dk, kubo_chunk_len(n, npts), 0, 0, 0).bytes()});
                }
                if (variant < 2) {
                    const size_t nc = (size_t)dk * dk;
                    PlaneArgs W = P;
                    W.nplane = npts;
                    if (!general) {
                        bad |= verify("tbk_qgt_mesh (n = 2)", {nc * kubo_plane_gx(W) * D, nc * D});
                    } else {
                        const KuboChunks cw = kubo_contract_chunks(n, dk, npts, manifold, 2);
                        const size_t nrows = nc * (manifold ? 1 : n), nchunks = (size_t)((npts + cw.chunk - 1) / cw.chunk);
                        W.nplane = cw.chunk;
                        bad |= verify("tbk_qgt_mesh (chunked)", {nrows * cw.chunk * D, nrows * kubo_plane_gx(W) * D, nchunks * nrows * D,
                                                                 cw.bytes()});
                    }
                }
            }
        }
    bad |= verify("nothing wanted", {0, 0});
    {
        KuboCarve ws;
        unsigned char* p[KuboCarve::kMax + 1];
        for (int i = 0; i <= KuboCarve::kMax; ++i) ws.add(p[i], 8);
        if (!ws.full || ws.cnt != KuboCarve::kMax) bad |= printf("a buffer beyond kMax is not refused\n");
    }
    if (bad) return printf("kubo_carve_check: FAILED\n"), 1;
    printf("kubo_carve_check: %d buffer lists ok\n", g_lists);
    return 0;
}
