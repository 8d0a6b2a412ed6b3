// The one owner of host-side device memory (context.cpp, multi.cpp).  Host only: of HIP it needs the runtime API header alone, so a CPU
// program with stand-in hipMalloc / hipFree can include it (tests/csrc/device_mem_check.cpp).
// Devices: whoever lets a buffer go makes its device current first -- a context under its DevGuard, mkt_multi with its set / restore pair.
//
// GUARD MODE (diagnostic, off by default; MKT_MEM_GUARD, include/mktfhe.h): every buffer allocated while guard_length() != 0 lies between two
// guards of that many bytes, filled with GUARD_BYTE.  A store that leaves the buffer by less than a guard changes a guard byte instead of a
// neighbour's memory; the guards are compared when the buffer is released and by sweep() (mkt_get_metric "mem_guard_check").  With the mode
// off the header makes exactly the runtime calls it makes without it: one hipMalloc per allocation, one hipFree per release.
#pragma once
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstddef>
#include <map>
#include <mutex>
#include <string>
#include <vector>

namespace mkt {

namespace memguard __attribute__((visibility("hidden"))) {   // (one state per library, and no exported symbol)
constexpr unsigned char GUARD_BYTE = 0xC7;
struct Entry { size_t guard, cap; int device; };   // of a live guarded buffer, by its true base: a move hands the base on, so the registry follows it
struct Finding { bool back; size_t cap, offset; };  // which guard, the bytes the buffer was asked for, the first changed byte counted from that guard's start
struct State {
    std::atomic<size_t> length{0};                  // bytes of each guard of the buffers allocated from now on; 0: off
    std::mutex mu;                                  // everything below
    std::map<void *, Entry> live;
    std::vector<Finding> found;                     // every finding since the process started
    size_t swept = 0, released = 0;                 // buffers the last sweep looked at; guarded buffers compared at their release so far
};
inline State &state() { static State s; return s; }

inline size_t guard_length() { return state().length.load(std::memory_order_relaxed); }
// a multiple of 256 bytes, so that a buffer keeps the alignment hipMalloc gave its base; anything else is refused and changes nothing
inline bool set_guard_length(size_t bytes) { if (bytes % 256) return false; state().length.store(bytes, std::memory_order_relaxed); return true; }

inline std::string text(const Finding &f) {
    return std::string("mem_guard: the ") + (f.back ? "back" : "front") + " guard of a buffer of " + std::to_string(f.cap) + " bytes was written, first at byte " + std::to_string(f.offset) + " of the guard";
}
// compare both guards of one buffer (its device current, the device drained by the caller); a changed guard is recorded once and filled anew.  mu held
inline void compare(State &s, void *base, const Entry &e) {
    std::vector<unsigned char> host(e.guard);
    for (int back = 0; back < 2; back++) {
        unsigned char *g = static_cast<unsigned char *>(base) + (back ? e.guard + e.cap : 0);
        if (hipMemcpy(host.data(), g, e.guard, hipMemcpyDeviceToHost) != hipSuccess) continue;
        size_t i = 0;
        while (i < e.guard && host[i] == GUARD_BYTE) i++;
        if (i == e.guard) continue;
        s.found.push_back(Finding{back != 0, e.cap, i});
        (void)hipMemset(g, GUARD_BYTE, e.guard);
        (void)hipDeviceSynchronize();
    }
}
// drain the current device and compare the guards of every live guarded buffer that was allocated on it -> findings since the process started
inline size_t sweep(int device) {
    State &s = state();
    std::lock_guard<std::mutex> lock(s.mu);
    s.swept = 0;
    if (s.live.empty()) return s.found.size();
    (void)hipDeviceSynchronize();
    for (const auto &b : s.live) if (b.second.device == device) { compare(s, b.first, b.second); s.swept++; }
    return s.found.size();
}
inline size_t swept() { State &s = state(); std::lock_guard<std::mutex> lock(s.mu); return s.swept; }
inline size_t released() { State &s = state(); std::lock_guard<std::mutex> lock(s.mu); return s.released; }
inline size_t findings() { State &s = state(); std::lock_guard<std::mutex> lock(s.mu); return s.found.size(); }
inline bool last_finding(Finding &f) { State &s = state(); std::lock_guard<std::mutex> lock(s.mu); if (s.found.empty()) return false; f = s.found.back(); return true; }

// guard + bytes + guard, both guards filled and the fill landed before the buffer is handed out -> the pointer behind the front guard
inline hipError_t alloc(void **p, size_t bytes, size_t guard) {
    void *base = nullptr;
    hipError_t e = hipMalloc(&base, bytes + 2 * guard);
    if (e != hipSuccess) return e;
    unsigned char *b = static_cast<unsigned char *>(base);
    e = hipMemset(b, GUARD_BYTE, guard);
    if (e == hipSuccess) e = hipMemset(b + guard + bytes, GUARD_BYTE, guard);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    int device = 0;
    if (e == hipSuccess) e = hipGetDevice(&device);
    if (e != hipSuccess) { (void)hipFree(base); return e; }
    State &s = state();
    std::lock_guard<std::mutex> lock(s.mu);
    s.live[base] = Entry{guard, bytes, device};
    *p = b + guard;
    return hipSuccess;
}
// the guards compared (the device drained first: a store still in flight on some stream counts), then the true base freed
inline void release(void *p, size_t guard) {
    void *base = static_cast<unsigned char *>(p) - guard;
    State &s = state();
    {
        std::lock_guard<std::mutex> lock(s.mu);
        const auto it = s.live.find(base);
        if (it != s.live.end()) {
            (void)hipDeviceSynchronize();
            compare(s, base, it->second);
            s.released++;
            s.live.erase(it);
        }
    }
    (void)hipFree(base);
}
}  // namespace memguard

struct __attribute__((visibility("hidden"))) DevBuf {   // (library-internal: its members are no exported symbols)
    void *p = nullptr; size_t cap = 0;   // cap: the bytes asked for
    size_t guard = 0;                    // guard mode: the bytes of each guard this buffer was allocated with (p lies `guard` behind the true base); 0: none
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap), guard(o.guard) { o.p = nullptr; o.cap = 0; o.guard = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { release(); p = o.p; cap = o.cap; guard = o.guard; o.p = nullptr; o.cap = 0; o.guard = 0; } return *this; }
    ~DevBuf() { release(); }
    void release() { if (p) { if (guard) memguard::release(p, guard); else (void)hipFree(p); } p = nullptr; cap = 0; guard = 0; }
    // a fresh buffer of a call's own (what was held is let go first); zero bytes still give a valid pointer.  A failure leaves the buffer empty
    hipError_t alloc(size_t bytes) {
        release();
        const size_t g = memguard::guard_length();
        const hipError_t e = g ? memguard::alloc(&p, bytes, g) : hipMalloc(&p, bytes ? bytes : 1);
        if (e != hipSuccess) p = nullptr; else { cap = bytes; guard = g; }
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
