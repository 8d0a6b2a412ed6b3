// Host check of mktfhe_amd/csrc/device_mem.h (no GPU, no HIP runtime): DevBuf and reserve_group over stand-in hipMalloc / hipFree that keep a
// call log and the set of live allocations.  Exit status 0 only if every rule of the header holds; built with -fsanitize=address,undefined,
// so a leak, a double free or a use after free of the stand-ins' malloc / free ends the run too.
#include <cstdio>
#include <cstdlib>
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
}  // namespace

extern "C" hipError_t hipMalloc(void **ptr, size_t size) {
    log_.push_back(Event{'M', size, live.size()});
    if (fail_in > 0 && --fail_in == 0) { *ptr = reinterpret_cast<void *>(0x1); return hipErrorOutOfMemory; }   // (a failed call may leave rubbish behind)
    *ptr = std::malloc(size ? size : 1);
    live.insert(*ptr);
    return hipSuccess;
}
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

int main() {
    check_reserve();
    CHECK(live.empty());
    check_alloc_and_lifetime();
    check_group();
    CHECK(live.empty() && bad_frees == 0 && fail_in == 0);
    std::printf("%zu runtime calls, %d failed checks\n", log_.size(), failures);
    return failures != 0;
}
