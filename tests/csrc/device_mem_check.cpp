// Host check of mktfhe_amd/csrc/device_mem.h (no GPU, no HIP runtime): DevBuf and reserve_group over stand-in hipMalloc / hipFree that keep a
// call log and the set of live allocations.  Exit status 0 only if every rule of the header holds; built with -fsanitize=address,undefined,
// so a leak, a double free or a use after free of the stand-ins' malloc / free ends the run too.
// The rules are checked first with the guard mode off -- the log of that part is printed as a count and a digest, which
// tests/test_device_mem_cpu.py holds to the values of the header before it had a guard mode, and no other runtime call may be made -- then
// with guards of 512 bytes (check_guard): sizes, pointers, the same rules again, and that a byte stored into a guard is found, once, by the
// sweep and by release.  "stub-clean" as the only argument makes the stand-in hipMemcpy hand back untouched guards: the run must then FAIL.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>
#include <vector>

#include "device_mem.h"

namespace {
struct Event { char what; size_t bytes; size_t live_before; };   // 'M' / 'F'
std::vector<Event> log_;
std::set<void *> live;
int fail_in = 0;          // n > 0: the n-th allocation from now fails
int bad_frees = 0;        // frees of what is not live (a second free, a pointer never handed out)
int failures = 0;
size_t aux_calls = 0;     // hipMemset, hipMemcpy, hipDeviceSynchronize, hipGetDevice: what only the guard mode may call
void *last_base = nullptr;   // what the last successful hipMalloc handed out
int cur_device = 0;
bool stub_clean = false;
}  // namespace

extern "C" hipError_t hipMalloc(void **ptr, size_t size) {
    log_.push_back(Event{'M', size, live.size()});
    if (fail_in > 0 && --fail_in == 0) { *ptr = reinterpret_cast<void *>(0x1); return hipErrorOutOfMemory; }   // (a failed call may leave rubbish behind)
    *ptr = std::malloc(size ? size : 1);
    live.insert(*ptr);
    last_base = *ptr;
    return hipSuccess;
}
extern "C" hipError_t hipMemset(void *dst, int value, size_t n) { aux_calls++; std::memset(dst, value, n); return hipSuccess; }
extern "C" hipError_t hipMemcpy(void *dst, const void *src, size_t n, hipMemcpyKind) {
    aux_calls++;
    if (stub_clean) std::memset(dst, mkt::memguard::GUARD_BYTE, n); else std::memcpy(dst, src, n);
    return hipSuccess;
}
extern "C" hipError_t hipDeviceSynchronize(void) { aux_calls++; return hipSuccess; }
extern "C" hipError_t hipGetDevice(int *dev) { aux_calls++; *dev = cur_device; return hipSuccess; }
extern "C" hipError_t hipFree(void *ptr) {
    log_.push_back(Event{'F', 0, live.size()});
    if (!ptr) return hipSuccess;
    if (!live.erase(ptr)) { bad_frees++; return hipErrorInvalidValue; }
    std::free(ptr);
    return hipSuccess;
}

#define CHECK(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

using mkt::DevBuf;

static void check_reserve() {
    DevBuf b;
    CHECK(b.p == nullptr && b.cap == 0);
    CHECK(b.reserve(100) == hipSuccess && b.p && b.cap == 100 && live.size() == 1);
    void *first = b.p;
    size_t n = log_.size();
    CHECK(b.reserve(100) == hipSuccess && b.reserve(40) == hipSuccess && b.reserve(0) == hipSuccess);
    CHECK(log_.size() == n && b.p == first && b.cap == 100);                      // enough: no runtime call, the same pointer
    CHECK(b.reserve(101) == hipSuccess && b.cap == 101 && b.p && live.size() == 1);
    CHECK(log_.size() == n + 2 && log_[n].what == 'F' && log_[n + 1].what == 'M');   // free, then malloc
    CHECK(log_[n + 1].live_before == 0 && log_[n + 1].bytes == 101);             // nothing live at the moment of the new malloc; the size asked
    fail_in = 1;
    n = log_.size();
    CHECK(b.reserve(500) == hipErrorOutOfMemory && b.p == nullptr && b.cap == 0 && live.empty());   // the error, and an empty buffer
    CHECK(log_.size() == n + 2 && log_[n].what == 'F' && log_[n + 1].what == 'M' && log_[n + 1].live_before == 0);
    CHECK(b.reserve(8) == hipSuccess && b.p && b.cap == 8 && live.size() == 1);   // the next call succeeds, from the smallest size on
    CHECK(bad_frees == 0);
}

static void check_alloc_and_lifetime() {
    CHECK(live.empty());
    {
        DevBuf z;
        CHECK(z.alloc(0) == hipSuccess && z.p != nullptr && z.cap == 0 && live.size() == 1);   // zero bytes: still a valid pointer
        CHECK(z.alloc(16) == hipSuccess && z.cap == 16 && live.size() == 1);                   // a fresh buffer lets the held one go
        CHECK(z.as<int>() == static_cast<int *>(z.p));
        z.release();
        CHECK(z.p == nullptr && z.cap == 0 && live.empty());
        size_t n = log_.size();
        z.release();                                                                           // twice: harmless, and no runtime call
        CHECK(log_.size() == n && bad_frees == 0);
        fail_in = 1;
        CHECK(z.alloc(4) == hipErrorOutOfMemory && z.p == nullptr && z.cap == 0);
    }
    {
        DevBuf a;
        CHECK(a.alloc(32) == hipSuccess);
        void *p = a.p;
        DevBuf b(std::move(a));
        CHECK(a.p == nullptr && a.cap == 0 && b.p == p && b.cap == 32 && live.size() == 1);
        DevBuf c;
        CHECK(c.alloc(64) == hipSuccess && live.size() == 2);
        c = std::move(b);                                                                      // what c held goes, b is left empty
        CHECK(b.p == nullptr && c.p == p && c.cap == 32 && live.size() == 1);
        std::vector<DevBuf> v(3);
        CHECK(v[1].reserve(10) == hipSuccess);
        v.resize(40);                                                                          // reallocation moves the owners
        CHECK(v[1].cap == 10 && live.size() == 2);
        size_t frees = 0;
        for (const Event &e : log_) frees += e.what == 'F';
        a.release(); b.release();                                                              // moved-from owners free nothing
        size_t frees2 = 0;
        for (const Event &e : log_) frees2 += e.what == 'F';
        CHECK(frees2 == frees);
    }
    CHECK(live.empty() && bad_frees == 0);                                                     // the destructors freed each buffer exactly once
}

static void check_group() {
    DevBuf a, b, c;
    DevBuf *const g[] = {&a, &b, &c};
    size_t units = 0;
    const size_t small[] = {10, 20, 30}, big[] = {100, 200, 300}, two[] = {1000, 0, 3000};
    CHECK(mkt::reserve_group(units, 1, g, small) == hipSuccess && units == 1 && a.cap == 10 && b.cap == 20 && c.cap == 30 && live.size() == 3);
    size_t n = log_.size();
    CHECK(mkt::reserve_group(units, 1, g, big) == hipSuccess && mkt::reserve_group(units, 0, g, big) == hipSuccess);
    CHECK(log_.size() == n && units == 1 && a.cap == 10);                                      // no growth: no runtime call
    CHECK(mkt::reserve_group(units, 10, g, big) == hipSuccess && units == 10 && a.cap == 100 && b.cap == 200 && c.cap == 300 && live.size() == 3);
    CHECK(log_.size() == n + 6);
    for (size_t i = 0; i < 3 && log_.size() == n + 6; i++) CHECK(log_[n + i].what == 'F' && log_[n + 3 + i].what == 'M');   // every member released before the first allocation
    CHECK(log_.size() == n + 6 && log_[n + 3].live_before == 0);
    fail_in = 2;                                                                               // the second of three members fails
    CHECK(mkt::reserve_group(units, 20, g, big) == hipErrorOutOfMemory && units == 0 && b.p == nullptr && c.p == nullptr && live.size() == 1);
    n = log_.size();
    CHECK(mkt::reserve_group(units, 2, g, small) == hipSuccess && units == 2 && a.cap == 10 && b.cap == 20 && c.cap == 30 && live.size() == 3);   // starts clean: all three anew, even for fewer units
    size_t mallocs = 0;
    for (size_t i = n; i < log_.size(); i++) mallocs += log_[i].what == 'M';
    CHECK(mallocs == 3 && log_[log_.size() - 3].live_before == 0);
    units = 0;                                                                                 // what an option that resets the workspace does
    CHECK(mkt::reserve_group(units, 1, g, two) == hipSuccess && units == 1 && a.cap == 1000 && b.p == nullptr && b.cap == 0 && c.cap == 3000 && live.size() == 2);   // a member no longer needed does not linger
    CHECK(bad_frees == 0);
}

// ---- guard mode ----
namespace G = mkt::memguard;
constexpr size_t GLEN = 512;

static unsigned char *bytes_of(const DevBuf &b) { return static_cast<unsigned char *>(b.p); }
static bool last_is(bool back, size_t cap, size_t offset) { G::Finding f{}; return G::last_finding(f) && f.back == back && f.cap == cap && f.offset == offset; }

static void check_guard() {
    CHECK(G::guard_length() == 0 && G::findings() == 0);
    CHECK(!G::set_guard_length(100) && !G::set_guard_length(511) && G::guard_length() == 0);      // no multiple of 256: refused, nothing changed
    DevBuf plain;
    CHECK(plain.alloc(24) == hipSuccess && plain.guard == 0 && plain.p == last_base);              // allocated before the mode is on: stays unguarded
    CHECK(G::set_guard_length(GLEN) && G::guard_length() == GLEN);
    CHECK(aux_calls == 0);
    {
        DevBuf b;
        CHECK(b.alloc(100) == hipSuccess && log_.back().what == 'M' && log_.back().bytes == 100 + 2 * GLEN);
        CHECK(b.p == static_cast<unsigned char *>(last_base) + GLEN && b.cap == 100 && b.guard == GLEN && live.size() == 2);
        bool filled = true;
        for (size_t i = 0; i < GLEN; i++) filled = filled && bytes_of(b)[-1 - (long)i] == G::GUARD_BYTE && bytes_of(b)[100 + i] == G::GUARD_BYTE;
        CHECK(filled);
        // the grow rule as before
        void *first = b.p;
        size_t n = log_.size();
        CHECK(b.reserve(100) == hipSuccess && b.reserve(40) == hipSuccess && b.reserve(0) == hipSuccess && log_.size() == n && b.p == first && b.cap == 100);
        CHECK(b.reserve(101) == hipSuccess && b.cap == 101 && live.size() == 2);
        CHECK(log_.size() == n + 2 && log_[n].what == 'F' && log_[n + 1].what == 'M' && log_[n + 1].live_before == 1 && log_[n + 1].bytes == 101 + 2 * GLEN);   // (plain is the one live)
        fail_in = 1;
        CHECK(b.reserve(500) == hipErrorOutOfMemory && b.p == nullptr && b.cap == 0 && b.guard == 0 && live.size() == 1);
        CHECK(b.alloc(0) == hipSuccess && b.p == static_cast<unsigned char *>(last_base) + GLEN && b.cap == 0 && log_.back().bytes == 2 * GLEN);   // zero bytes: a valid pointer between two guards
        // a clean sweep: this one guarded buffer, nothing found (plain is not in the registry)
        CHECK(G::sweep(0) == 0 && G::swept() == 1);
        // move: the registry follows, the moved-from owner is not swept and frees nothing
        CHECK(b.alloc(64) == hipSuccess);
        void *p = b.p;
        DevBuf c(std::move(b));
        CHECK(b.p == nullptr && b.cap == 0 && b.guard == 0 && c.p == p && c.cap == 64 && c.guard == GLEN);
        CHECK(G::sweep(0) == 0 && G::swept() == 1);
        DevBuf d;
        CHECK(d.alloc(8) == hipSuccess && G::sweep(0) == 0 && G::swept() == 2);
        d = std::move(c);                                                                          // what d held is compared and freed
        CHECK(c.p == nullptr && d.p == p && d.cap == 64 && d.guard == GLEN && live.size() == 2 && G::sweep(0) == 0 && G::swept() == 1);
        // one byte before and one behind, found by the sweep: each once, with its side and offset
        bytes_of(d)[-1] = 0;
        CHECK(G::sweep(0) == 1 && last_is(false, 64, GLEN - 1));
        CHECK(G::sweep(0) == 1);                                                                   // reported once: the guard was filled anew
        bytes_of(d)[64] = G::GUARD_BYTE ^ 1;
        CHECK(G::sweep(0) == 2 && last_is(true, 64, 0));
        bytes_of(d)[64 + 7] = 0xFF;
        bytes_of(d)[64 + 300] = 0;
        CHECK(G::sweep(0) == 3 && last_is(true, 64, 7));                                           // several bytes of one guard: one finding, the first byte
        CHECK(G::sweep(0) == 3 && bad_frees == 0);
        CHECK(G::text(G::Finding{true, 64, 7}).find("back guard") != std::string::npos && G::text(G::Finding{false, 1, 2}).find("front guard") != std::string::npos);
        // ... and by release
        const size_t rel = G::released();
        bytes_of(d)[-1] = 1;
        d.release();
        CHECK(G::findings() == 4 && last_is(false, 64, GLEN - 1) && G::released() == rel + 1 && live.size() == 1);
        CHECK(d.alloc(33) == hipSuccess);
        bytes_of(d)[33] = 0;
        d.release();
        CHECK(G::findings() == 5 && last_is(true, 33, 0));
        CHECK(d.alloc(33) == hipSuccess);
        bytes_of(d)[-(long)GLEN] = 1; bytes_of(d)[33 + GLEN - 1] = 0;                              // the far end of either guard, both in one release
        d.release();
        CHECK(G::findings() == 7 && last_is(true, 33, GLEN - 1) && G::released() == rel + 3);
        CHECK(d.alloc(33) == hipSuccess);
        bytes_of(d)[0] = 0; bytes_of(d)[32] = 0;                                                   // stores inside the buffer are its own
        d.release();
        CHECK(G::findings() == 7 && G::released() == rel + 4);
        // a buffer is swept with its device only
        DevBuf e0, e1;
        CHECK(e0.alloc(16) == hipSuccess);
        cur_device = 1;
        CHECK(e1.alloc(16) == hipSuccess);
        bytes_of(e1)[16] = 0;
        CHECK(G::sweep(0) == 7 && G::swept() == 1 && G::sweep(1) == 8 && G::swept() == 1 && last_is(true, 16, 0));
        cur_device = 0;
    }
    CHECK(live.size() == 1 && bad_frees == 0);                                                     // the destructors freed each true base once
    {   // the group helper under guards
        DevBuf a, b, c;
        DevBuf *const g[] = {&a, &b, &c};
        size_t units = 0;
        const size_t small[] = {10, 20, 30}, two[] = {1000, 0, 3000};
        CHECK(mkt::reserve_group(units, 1, g, small) == hipSuccess && units == 1 && a.cap == 10 && b.cap == 20 && c.cap == 30 && live.size() == 4);
        size_t n = log_.size();
        CHECK(mkt::reserve_group(units, 1, g, two) == hipSuccess && log_.size() == n);
        fail_in = 2;
        CHECK(mkt::reserve_group(units, 5, g, two) == hipErrorOutOfMemory && units == 0 && c.p == nullptr && live.size() == 2);
        CHECK(mkt::reserve_group(units, 5, g, two) == hipSuccess && units == 5 && a.cap == 1000 && b.p == nullptr && c.cap == 3000 && live.size() == 3);
        CHECK(log_.back().bytes == 3000 + 2 * GLEN && G::sweep(0) == 8 && G::swept() == 2);
        // the mode switched off under live guarded buffers: they keep their guards, new ones have none
        CHECK(G::set_guard_length(0));
        const size_t aux = aux_calls;
        CHECK(b.alloc(50) == hipSuccess && b.guard == 0 && b.p == last_base && log_.back().bytes == 50 && aux_calls == aux);
        CHECK(G::sweep(0) == 8 && G::swept() == 2);
        static_cast<unsigned char *>(a.p)[1000] = 0;
    }
    CHECK(G::findings() == 9 && last_is(true, 1000, 0));                                           // found as the group went
    plain.release();
    CHECK(live.empty() && bad_frees == 0 && G::sweep(0) == 9 && G::swept() == 0);
}

int main(int argc, char **argv) {
    stub_clean = argc > 1 && std::strcmp(argv[1], "stub-clean") == 0;
    check_reserve();
    CHECK(live.empty());
    check_alloc_and_lifetime();
    check_group();
    CHECK(live.empty() && bad_frees == 0 && fail_in == 0);
    CHECK(aux_calls == 0);                                                                         // mode off: hipMalloc and hipFree alone
    unsigned long long h = 1469598103934665603ull;                                                 // FNV-1a over (what, bytes, live before) of every call so far
    for (const Event &e : log_)
        for (unsigned long long v : {(unsigned long long)e.what, (unsigned long long)e.bytes, (unsigned long long)e.live_before}) { h ^= v; h *= 1099511628211ull; }
    std::printf("mode off: %zu runtime calls, digest %016llx\n", log_.size(), h);
    check_guard();
    CHECK(live.empty() && bad_frees == 0 && fail_in == 0);
    std::printf("%zu runtime calls, %d failed checks\n", log_.size(), failures);
    return failures != 0;
}
