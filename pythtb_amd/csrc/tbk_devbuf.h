// tbk_devbuf.h -- a device buffer that only grows: a pointer with its capacity, and the ONE routine that regrows it
// (tbk_ctx::work and ::scratch, the per-array buffers of tbk_wfs).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "../../include/tbk.h"

void tbk_set_error(const char* fmt, ...);

struct TbkDevBuf {
    void* p = nullptr;
    size_t bytes = 0;   // capacity; never non-zero beside a null pointer
    template <class T>
    T* as() const { return static_cast<T*>(p); }
};

// Release and allocate again when `need` exceeds the capacity (max(need, at_least) bytes; the contents are not kept).  Pointer
// null and capacity 0 stand between the release and the allocation, and the capacity is set only once the allocation has
// succeeded: a failure leaves an empty buffer that the next call grows again, never a capacity with nothing behind it.
// `alloc` / `release`: hipMalloc / hipFree, or what a host check substitutes (check/plan_check.cpp).
template <class Alloc = hipError_t (*)(void**, size_t), class Free = hipError_t (*)(void*)>
static inline int tbk_devbuf_regrow(TbkDevBuf& b, size_t need, size_t at_least, const char* what, Alloc alloc = hipMalloc,
                                    Free release = hipFree) {
    if (need <= b.bytes) return TBK_OK;
    const hipError_t ef = b.p ? release(b.p) : hipSuccess;
    if (ef != hipSuccess) {
        tbk_set_error("%s: releasing %zu bytes failed: %s", what, b.bytes, hipGetErrorString(ef));
        return TBK_EHIP;
    }
    b.p = nullptr;
    b.bytes = 0;
    const size_t want = need > at_least ? need : at_least;
    const hipError_t e = alloc(&b.p, want);
    if (e != hipSuccess) {
        b.p = nullptr;
        tbk_set_error("%s of %zu bytes: %s", what, want, hipGetErrorString(e));
        return TBK_ENOMEM;
    }
    b.bytes = want;
    return TBK_OK;
}
