// The one owner of host-side device memory (context.cpp, multi.cpp).  Host only: of HIP it needs the runtime API header alone, so a CPU
// program with stand-in hipMalloc / hipFree can include it (tests/csrc/device_mem_check.cpp).
// Devices: whoever lets a buffer go makes its device current first -- a context under its DevGuard, mkt_multi with its set / restore pair.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>

namespace mkt {

struct __attribute__((visibility("hidden"))) DevBuf {   // (library-internal: its members are no exported symbols)
    void *p = nullptr; size_t cap = 0;   // cap: the bytes asked for
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
    ~DevBuf() { release(); }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    // a fresh buffer of a call's own (what was held is let go first); zero bytes still give a valid pointer.  A failure leaves the buffer empty
    hipError_t alloc(size_t bytes) {
        release();
        const hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
        if (e != hipSuccess) p = nullptr; else cap = bytes;
        return e;
    }
    // THE grow rule of every buffer that is kept between calls: enough is left alone; too small is freed, then allocated anew at the size asked
    // (nothing is copied over, and the old and the new buffer never exist side by side)
    hipError_t reserve(size_t bytes) { return bytes <= cap ? hipSuccess : alloc(bytes); }
    template <class T> T *as() const { return static_cast<T *>(p); }
};

// Buffers that grow together, sized by one count of units (gates, packs): `units` is what they hold now, bytes[i] the whole size of m[i] for
// `want` units (0: the member is not needed and stays empty).  Every member is let go before the first new one is allocated, so the peak is
// the new sizes alone; the count is recorded once all of them stand, and a failure part-way leaves it 0 -- the next call starts clean.
// (A caller that sets `units` to 0 has the whole group allocated anew by the next call.)
template <size_t K> __attribute__((visibility("hidden"))) hipError_t reserve_group(size_t &units, size_t want, DevBuf *const (&m)[K], const size_t (&bytes)[K]) {
    if (want <= units) return hipSuccess;
    for (DevBuf *b : m) b->release();
    units = 0;
    for (size_t i = 0; i < K; i++)
        if (bytes[i]) { const hipError_t e = m[i]->alloc(bytes[i]); if (e != hipSuccess) return e; }
    units = want;
    return hipSuccess;
}

}  // namespace mkt
