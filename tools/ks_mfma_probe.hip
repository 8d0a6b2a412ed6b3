// The tile loop of the matrix-core key switch (mktfhe_amd/csrc/ks_mfma.h) on its own: is it exact, and what int8 MFMA rate does the
// part sustain at the headline's dimensions (KMS k = 2, N = 1024: 1 024 gates x K = 4 * 8 192 x 2 256 byte columns per party)?
//   (i)  small shapes, random key rows packed by the host packer, random digit words: the slab sums against a plain loop on the host;
//   (ii) the headline dimensions on random bytes, for several slab counts: time per launch, products per second, bytes of key per second.
//   make -C tools bin/ks_mfma_probe && tools/bin/ks_mfma_probe > profiles/ks_mfma_probe.txt
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <vector>
#include <algorithm>
#include "ks_mfma.h"

using namespace mktd;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); exit(2); } } while (0)

template <int F>
__global__ __launch_bounds__(64 * KSM_WAVES, 1) void probe_kernel(const KsmArgs a) { ksm_workgroup<F>(a); }

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 16); }

static void launch(const KsmArgs &a, hipStream_t s) {
    const int gtiles = (a.B + KSM_WAVE_GATES * KSM_WAVES - 1) / (KSM_WAVE_GATES * KSM_WAVES);
    const dim3 grid((unsigned)(gtiles * a.slabs), (unsigned)(a.mk ? a.kacc : 1), (unsigned)ksm_coltiles(a.n1p));
    if (a.f == 8) hipLaunchKernelGGL(probe_kernel<8>, grid, dim3(64 * KSM_WAVES), 0, s, a);
    else hipLaunchKernelGGL(probe_kernel<0>, grid, dim3(64 * KSM_WAVES), 0, s, a);
}

// key: 0 random, 1 every word 0xFFFFFFFF and every digit 3, 2 every word 0x80000000
static bool check(int B, int N, int f, int n, int kacc, int mk, int slabs, int key) {
    const int n1p = (n + 1 + 3) / 4 * 4, drows = 3, ngroups = (B + 31) / 32, parties = mk ? kacc : 1;
    const size_t comp_words = (size_t)N * drows * f * n1p, blk_bytes = ksm_block_bytes(N, f, n1p);
    std::vector<uint32_t> rows(comp_words * kacc), dig((size_t)kacc * ngroups * N * 32);
    for (auto &w : rows) w = key == 1 ? 0xFFFFFFFFu : key == 2 ? 0x80000000u : rnd();
    for (auto &w : dig) w = key == 1 ? (1u << (2 * f)) - 1 : rnd() & ((1u << (2 * f)) - 1);
    std::vector<int8_t> planes(blk_bytes * kacc);
    for (int c = 0; c < kacc; c++)
        for (size_t o = 0; o < blk_bytes; o++) planes[c * blk_bytes + o] = ksm_plane_byte(rows.data() + c * comp_words, N, f, drows, n1p, o);
    std::vector<uint32_t> ref((size_t)parties * B * n1p, 0);
    for (int c = 0; c < kacc; c++)
        for (int g = 0; g < B; g++)
            for (int j = 0; j < N; j++) {
                const uint32_t w = dig[(((size_t)c * ngroups + g / 32) * N + j) * 32 + g % 32];
                for (int t = 0; t < f; t++) {
                    const int d = (w >> (2 * (f - 1 - t))) & 3;
                    if (!d) continue;
                    const uint32_t *row = rows.data() + c * comp_words + (((size_t)j * drows + d - 1) * f + t) * n1p;
                    uint32_t *o = ref.data() + ((size_t)(mk ? c : 0) * B + g) * n1p;
                    for (int q = 0; q < n1p; q++) o[q] += row[q];
                }
            }
    int8_t *d_pl; uint32_t *d_dig, *d_part;
    const size_t pw = (size_t)slabs * parties * B * n1p;
    CK(hipMalloc(&d_pl, planes.size())); CK(hipMalloc(&d_dig, dig.size() * 4)); CK(hipMalloc(&d_part, pw * 4));
    CK(hipMemcpy(d_pl, planes.data(), planes.size(), hipMemcpyHostToDevice));
    CK(hipMemcpy(d_dig, dig.data(), dig.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemset(d_part, 0xA5, pw * 4));
    KsmArgs a{d_pl, blk_bytes, d_dig, d_part, B, ngroups, N, f, n1p, kacc, mk, slabs};
    launch(a, 0);
    CK(hipGetLastError()); CK(hipDeviceSynchronize());
    std::vector<uint32_t> part(pw);
    CK(hipMemcpy(part.data(), d_part, pw * 4, hipMemcpyDeviceToHost));
    size_t bad = 0;
    for (size_t i = 0; i < ref.size(); i++) {
        uint32_t v = 0;
        for (int sl = 0; sl < slabs; sl++) v += part[sl * ref.size() + i];
        bad += v != ref[i];
    }
    printf("check B=%d N=%d f=%d n=%d kacc=%d mk=%d slabs=%d key=%d: %zu of %zu words differ\n", B, N, f, n, kacc, mk, slabs, key, bad, ref.size());
    CK(hipFree(d_pl)); CK(hipFree(d_dig)); CK(hipFree(d_part));
    return bad == 0;
}

static void rate(int B, int N, int f, int n, int kacc, int slabs) {
    const int n1p = (n + 1 + 3) / 4 * 4, ngroups = (B + 31) / 32;
    const size_t blk_bytes = ksm_block_bytes(N, f, n1p), pw = (size_t)slabs * kacc * B * n1p;
    std::vector<uint32_t> hp(blk_bytes * kacc / 4), hd((size_t)kacc * ngroups * N * 32);
    for (auto &w : hp) w = rnd() ^ (rnd() << 16);
    for (auto &w : hd) w = rnd() & ((1u << (2 * f)) - 1);
    int8_t *d_pl; uint32_t *d_dig, *d_part;
    CK(hipMalloc(&d_pl, blk_bytes * kacc)); CK(hipMalloc(&d_dig, hd.size() * 4)); CK(hipMalloc(&d_part, pw * 4));
    CK(hipMemcpy(d_pl, hp.data(), blk_bytes * kacc, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_dig, hd.data(), hd.size() * 4, hipMemcpyHostToDevice));
    KsmArgs a{d_pl, blk_bytes, d_dig, d_part, B, ngroups, N, f, n1p, kacc, 1, slabs};
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    for (int i = 0; i < 3; i++) launch(a, 0);
    CK(hipDeviceSynchronize());
    const int reps = 20;
    std::vector<float> ms(reps);
    for (int i = 0; i < reps; i++) {
        CK(hipEventRecord(e0, 0)); launch(a, 0); CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1));
        CK(hipEventElapsedTime(&ms[i], e0, e1));
    }
    // ... and with the caches emptied before every launch, as after a blind rotation (its keys stream through the Infinity Cache)
    const size_t flush_bytes = (size_t)1 << 30;
    void *d_flush; CK(hipMalloc(&d_flush, flush_bytes));
    std::vector<float> cold(reps);
    for (int i = 0; i < reps; i++) {
        CK(hipMemsetAsync(d_flush, i, flush_bytes, 0));
        CK(hipEventRecord(e0, 0)); launch(a, 0); CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1));
        CK(hipEventElapsedTime(&cold[i], e0, e1));
    }
    CK(hipFree(d_flush));
    std::sort(cold.begin(), cold.end());
    CK(hipGetLastError());
    std::sort(ms.begin(), ms.end());
    const double med = ms[reps / 2], macs = (double)kacc * B * (4.0 * N * f) * (4.0 * n1p);
    const int gtiles = (B + 511) / 512;
    printf("rate B=%d N=%d f=%d n1p=%d parties=%d slabs=%d workgroups=%d: min %.4f median %.4f max %.4f ms, after a cache flush median %.4f ms; %.1f T int8 products/s (%.1f TOPS), key planes %.1f MB read %d x = %.2f TB/s, partial rows %.1f MB\n",
           B, N, f, n1p, kacc, slabs, gtiles * slabs * kacc * ksm_coltiles(n1p), ms[0], med, ms[reps - 1], cold[reps / 2], macs / med * 1e-9, 2 * macs / med * 1e-9,
           blk_bytes * kacc * 1e-6, gtiles, blk_bytes * kacc * (double)gtiles / med * 1e-9, pw * 4e-6);
    CK(hipFree(d_pl)); CK(hipFree(d_dig)); CK(hipFree(d_part));
}

int main() {
    bool ok = true;
    ok &= check(40, 32, 2, 8, 2, 1, 3, 0);     // K = 192 + a ragged last step, three column... n1p = 12: one ragged tile
    ok &= check(33, 32, 3, 9, 2, 0, 2, 0);     // ragged K, both components into one row
    ok &= check(150, 16, 8, 40, 2, 1, 5, 0);   // the f = 8 path, two column tiles, two waves, a ragged gate tile
    ok &= check(600, 16, 8, 35, 1, 0, 1, 0);   // two gate tiles of 512
    ok &= check(17, 32, 2, 8, 1, 1, 1, 1);     // largest byte sums
    ok &= check(17, 32, 8, 8, 2, 1, 2, 2);     // the sign bit alone
    printf("exactness: %s\n", ok ? "ok" : "FAILED");
    if (!ok) return 1;
    for (int slabs : {1, 2, 4, 7, 14}) rate(1024, 1024, 8, 560, 2, slabs);
    rate(512, 1024, 8, 560, 2, 7);
    rate(128, 1024, 8, 560, 2, 28);
    rate(4096, 1024, 8, 560, 2, 2);
    rate(4096, 1024, 8, 560, 2, 4);     // the launch rule: whole rounds of the part
    rate(2048, 1024, 8, 560, 2, 3);
    rate(2048, 1024, 8, 560, 2, 5);     // the launch rule
    return 0;
}
