// Stand-alone host check of the buffer grower (tbk_devbuf.h) and of the launch arithmetic the mesh-solve drivers share
// (tbk_solve_plan.h); no device call: built under AddressSanitizer + UBSan by `make -C pythtb_amd/csrc plan-check` and run as an
// ordinary program.
//  * tbk_devbuf_regrow over a substituted allocator (host memory, can be told to fail): growth, reuse at smaller sizes, the
//    minimum size, and the state after a failed allocation -- pointer null, capacity 0, TBK_ENOMEM -- from which the next call of a
//    SMALLER size allocates again instead of trusting the capacity the buffer had before (what two hand-written copies of the
//    block got wrong: a null pointer handed to a kernel that stores through it).  Every live block is written through, so a
//    capacity with less memory behind it is a sanitizer report.
//  * tbk_tile_balance against plan_check_table.inc, the values of the expressions the two branches of the mesh solve held before
//    they shared the function.  Order of the table, outermost first: form (0 the row kernel: knob held to the row alone, want of
//    256 compute units x 32 and x 64; 1 the fused kernel: knob held to the cap too, x 32), cap 1 / 3 / 8, TBK_GRID_SEG unset / 1 /
//    100, rows 1 / 2 / 257 / 4097, cpr 1..70.  For every entry seg * tpr >= cpr > (seg - 1) * tpr and ntiles = rows * tpr; and
//    1 <= seg <= min(cap, cpr) -- except under a knob of the row-kernel form, which the cap never bound (1 <= seg <= cpr there:
//    TBK_GRID_SEG=100 on a 70-chunk row is one tile of 70, before and after).
//  * tbk_chunk_window for offsets 0 / 5 / 63, lengths 1 / 16 / 17 / 200, runs 1 / 16 / 64: the chains cover [off, off + nl) and
//    nothing else -- the first and the last chain touch it, every point of it lies in one of them.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../tbk_devbuf.h"
#include "../tbk_solve_plan.h"

static char g_err[512];
void tbk_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

static int g_fail_next = 0, g_live = 0, g_allocs = 0;
static hipError_t host_alloc(void** p, size_t n) {
    if (g_fail_next) {
        g_fail_next = 0;
        return hipErrorOutOfMemory;
    }
    *p = malloc(n);
    ++g_live;
    ++g_allocs;
    return hipSuccess;
}
static hipError_t host_release(void* p) {
    free(p);
    --g_live;
    return hipSuccess;
}
static int grow(TbkDevBuf& b, size_t need, size_t at_least = 0) {
    const int rc = tbk_devbuf_regrow(b, need, at_least, "test buffer", host_alloc, host_release);
    if (rc == TBK_OK && b.bytes) memset(b.p, 0x5a, b.bytes);
    return rc;
}

#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) return printf("line %d: %s\n", __LINE__, #cond), 1;  \
    } while (0)

static int check_grower() {
    TbkDevBuf b;
    EXPECT(grow(b, 0) == TBK_OK && !b.p && b.bytes == 0 && g_allocs == 0);
    EXPECT(grow(b, 1000) == TBK_OK && b.p && b.bytes == 1000 && g_allocs == 1);
    void* const first = b.p;
    EXPECT(grow(b, 10) == TBK_OK && b.p == first && b.bytes == 1000 && g_allocs == 1);     // reuse
    EXPECT(grow(b, 1000) == TBK_OK && b.p == first && g_allocs == 1);
    EXPECT(grow(b, 1001) == TBK_OK && b.bytes == 1001 && g_allocs == 2 && g_live == 1);    // growth releases the old block
    EXPECT(grow(b, 2000, 4096) == TBK_OK && b.bytes == 4096 && g_allocs == 3 && g_live == 1);   // minimum size
    EXPECT(grow(b, 4096, 1 << 20) == TBK_OK && b.bytes == 4096 && g_allocs == 3);          // ... only when it has to grow
    g_fail_next = 1;
    g_err[0] = 0;
    EXPECT(grow(b, 8192) == TBK_ENOMEM && !b.p && b.bytes == 0 && g_live == 0);
    EXPECT(strstr(g_err, "test buffer of 8192 bytes: ") == g_err);
    EXPECT(grow(b, 100) == TBK_OK && b.p && b.bytes == 100 && g_allocs == 4 && g_live == 1);   // smaller than before the failure
    g_fail_next = 1;
    EXPECT(grow(b, 50) == TBK_OK && g_fail_next == 1 && g_allocs == 4);                    // (fits: the allocator is not asked)
    EXPECT(grow(b, 200) == TBK_ENOMEM && !b.p && b.bytes == 0 && g_live == 0);
    EXPECT(grow(b, 200) == TBK_OK && b.bytes == 200 && g_live == 1);
    EXPECT(host_release(b.p) == hipSuccess && g_live == 0);
    return 0;
}

static const unsigned char kBalance[] = {
#include "plan_check_table.inc"
};

static int check_balance() {
    const unsigned char* t = kBalance;
    long entries = 0;
    for (int form = 0; form < 2; ++form)
        for (int64_t mult : {32, 64}) {
            if (form == 1 && mult == 64) continue;
            const int64_t want = 256 * mult;
            for (int cap : {1, 3, 8})
                for (int knob : {-1, 1, 100})
                    for (int64_t rows : {1, 2, 257, 4097})
                        for (int cpr = 1; cpr <= 70; ++cpr, t += 2, ++entries) {
                            struct { int seg, tpr; int64_t ntiles; } b;
                            b.ntiles = tbk_tile_balance(cpr, rows, want, cap, knob, form == 1, &b.seg, &b.tpr);
                            const bool capped = knob < 0 || form == 1;
                            const bool ok = b.seg == t[0] && b.tpr == t[1] && b.ntiles == rows * b.tpr && b.seg * b.tpr >= cpr &&
                                            (b.seg - 1) * b.tpr < cpr && b.seg >= 1 && b.seg <= (capped ? std::min(cap, cpr) : cpr);
                            if (!ok)
                                return printf("tile balance: form %d want %lld cap %d knob %d rows %lld cpr %d: seg %d tpr %d ntiles %lld, "
                                              "the table holds %d %d\n", form, (long long)want, cap, knob, (long long)rows, cpr, b.seg, b.tpr,
                                              (long long)b.ntiles, t[0], t[1]), 1;
                        }
        }
    EXPECT(t == kBalance + sizeof kBalance && entries == 7560);
    // beyond the last-level cache the fused driver asks for no tiles at all (want = INT64_MAX): one chunk per tile unless the knob says so
    int seg = 0, tpr = 0;
    EXPECT(tbk_tile_balance(64, 683, INT64_MAX, 3, -1, true, &seg, &tpr) == 683 * 64 && seg == 1 && tpr == 64);
    EXPECT(tbk_tile_balance(64, 683, INT64_MAX, 3, 2, true, &seg, &tpr) == 683 * 32 && seg == 2 && tpr == 32);
    return 0;
}

static int check_window() {
    for (int64_t off : {0, 5, 63})
        for (int64_t nl : {1, 16, 17, 200})
            for (int64_t run : {1, 16, 64}) {
                struct { int64_t first; int nchunk; } w;
                w.nchunk = tbk_chunk_window(off, nl, run, &w.first);
                const int64_t lo = w.first * run, hi = (w.first + w.nchunk) * run;   // the chains cover [lo, hi)
                const bool ok = w.nchunk >= 1 && lo <= off && off < lo + run && hi >= off + nl && hi - run < off + nl;
                if (!ok)
                    return printf("chunk window: off %lld nl %lld run %lld: first %lld nchunk %d\n", (long long)off, (long long)nl,
                                  (long long)run, (long long)w.first, w.nchunk), 1;
            }
    return 0;
}

int main() {
    if (check_grower() || check_balance() || check_window()) return 1;
    printf("plan_check ok: grower (5 allocations, 2 refused), 7560 tile balances, 36 chunk windows\n");
    return 0;
}
