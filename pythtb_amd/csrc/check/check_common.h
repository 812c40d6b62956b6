// check_common.h -- what the stand-alone host checks of this directory share.  Included after the header under test.
#pragma once
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

// what the headers' host functions take from the library (a check links no translation unit of it, or only the one under test);
// the text of the last error is kept for the checks that look at it
[[maybe_unused]] static char g_err[512];
void tbk_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
int tbk_ctx_scratch(tbk_ctx*, size_t, void**) { return TBK_EHIP; }
int tbk_k_uniform_mesh_range_dev(tbk_ctx*, int, const int32_t*, int64_t, int64_t, double*) { return TBK_EHIP; }
int tbk_solve_list_dev_checked(tbk_model*, const double*, int64_t, double*, double*) { return TBK_EHIP; }
ProfScope::ProfScope(tbk_ctx* c, const char* n) : ctx(c), name(n) {}
ProfScope::~ProfScope() {}

// (offset, bytes) of the buffers of a scratch block in order: at multiples of 256, none overlapping, the last ending at the total;
// a block of at most fill_max bytes is allocated, every buffer filled with its own index and read back (under the sanitizer)
[[maybe_unused]] static int check_buffers(const char* tag, const size_t (*buf)[2], int nb, size_t total, size_t fill_max = (size_t)512 << 20) {
    size_t end = 256;
    for (int i = 0; i < nb; ++i) {
        if (buf[i][0] % 256 || buf[i][0] < end)
            return printf("%s: buffer %d at offset %zu (the previous one ends at %zu)\n", tag, i, buf[i][0], end);
        end = buf[i][0] + buf[i][1];
    }
    if (end > total || total - end >= 256) return printf("%s: the last buffer ends at %zu, the total is %zu\n", tag, end, total);
    if (total > fill_max) return 0;
    unsigned char* base = (unsigned char*)aligned_alloc(256, (total + 255) / 256 * 256);
    if (!base) return printf("%s: no host block of %zu bytes\n", tag, total);
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

// the G k-groups [g cnt / G, (g + 1) cnt / G) of a full chunk and of the last, shorter one cover the points once, in order
[[maybe_unused]] static int check_groups(const char* tag, int G, int64_t npts, int64_t chunk, int64_t nchunks) {
    for (int64_t cnt : {chunk, npts - (nchunks - 1) * chunk}) {
        int64_t at = 0;
        for (int g = 0; g < G; ++g) {
            const int64_t p0 = (int64_t)g * cnt / G, p1 = (int64_t)(g + 1) * cnt / G;
            if (p0 != at || p1 < p0) return printf("%s: group %d of %lld points starts at %lld\n", tag, g, (long long)cnt, (long long)p0);
            at = p1;
        }
        if (at != cnt) return printf("%s: the groups end at %lld of %lld points\n", tag, (long long)at, (long long)cnt);
    }
    return 0;
}
