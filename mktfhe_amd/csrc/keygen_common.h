// Steps the device key generators share (keygen.hip: the full keys; keygen_seeded.hip: the bodies of the seeded form; pack_keys.hip: the
// bodies of the seeded packing key; ring_share.hip: the noise and the product term): a workgroup of KG_THREADS lanes fills a polynomial from
// a counter-based stream in parallel -- lane t generates keystream blocks t, t + 256, ... (8 uniform draws or 4 Gaussian deviates each) --
// and multiplies it with a small secret polynomial, N^2 / 2 word additions spread over the workgroup.  Every RLWE body is one step,
//     body = -sum_c a_c (*) z_c + e + message:   accumulate_masks, then noise_and_store;
// UniEnc adds its ternary r (draw_ternary) and its row d_j = crs_j r + s_i g_j + e (unienc_d_row).  A kernel states where its masks, its
// noise and its message come from and nothing else.  The words are those of the sequential host loops (client.cpp).  Internal to the library.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rng_chacha.h"

#pragma clang fp contract(off)

namespace mktd {
namespace {

using mktrng::Rng;
constexpr int KG_THREADS = 256;

// dst[q] = draw number (first + q) of the stream & wm, q < N  (N a multiple of 8, first a multiple of 8)
__device__ __forceinline__ void fill_uniform(const Rng &proto, uint64_t first, uint64_t *dst, int N, uint64_t wm) {
    for (int b = threadIdx.x; b < N / 8; b += KG_THREADS) {
        uint32_t w[16];
        mktrng::chacha20_block(proto.key, (uint32_t)(first / 8) + (uint32_t)b, proto.nonce, w);
#pragma unroll
        for (int i = 0; i < 8; i++) dst[8 * b + i] = ((uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32)) & wm;
    }
}
// dst[q] = noise(sigma) from draws first + 2q, first + 2q + 1  (Rng::noise order)
__device__ __forceinline__ void fill_noise(const Rng &proto, uint64_t first, uint64_t *dst, int N, double sigma) {
    for (int b = threadIdx.x; b < N / 4; b += KG_THREADS) {
        uint32_t w[16];
        mktrng::chacha20_block(proto.key, (uint32_t)(first / 8) + (uint32_t)b, proto.nonce, w);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint64_t r1 = (uint64_t)w[4 * i] | ((uint64_t)w[4 * i + 1] << 32), r2 = (uint64_t)w[4 * i + 2] | ((uint64_t)w[4 * i + 3] << 32);
            dst[4 * b + i] = (uint64_t)(int64_t)rint(sigma * mktrng::box_muller(r1, r2));
        }
    }
}

template <typename WORD> __device__ __forceinline__ uint64_t wmask_of() { return sizeof(WORD) == 8 ? ~0ull : 0xFFFFFFFFull; }

// al[q] <- coefficient q of the mask polynomial at index `idx` of the public stream `stream` (13: the bootstrapping key; 19: the packing key),
// q < N: one keystream block per lane and pass, 16 coefficients of the 32-bit ring or 8 of the 64-bit one, low word first
template <typename WORD>
__device__ __forceinline__ void fill_mask_poly(const uint32_t mkey[8], uint32_t stream, uint32_t party, uint64_t idx, uint64_t *al, int N) {
    constexpr int PER = sizeof(WORD) == 8 ? 8 : 16;                 // coefficients per keystream block
    for (int b = threadIdx.x; b < N / PER; b += KG_THREADS) {
        uint32_t w[16];
        mktrng::stream_block(mkey, stream, party, idx, (uint32_t)b, w);
#pragma unroll
        for (int i = 0; i < PER; i++) al[PER * b + i] = sizeof(WORD) == 8 ? ((uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32)) : (uint64_t)w[i];
    }
}

// the term s_i a[(m - i) mod N] of coefficient m of a negacyclic product, s_i = +-1; `flip` negates it
__device__ __forceinline__ uint64_t negacyclic_term(const uint64_t *a_lds, int N, int m, int i, int si, bool flip) {
    const uint64_t v = a_lds[(m - i) & (N - 1)];
    const bool wrap = i > m;                        // the term came around X^N = -1
    return ((si < 0) != (wrap != flip)) ? (uint64_t)0 - v : v;
}

// acc[r] (+)= sum_i s_i * a[(m - i) mod N] with the negacyclic sign, m = t + r * KG_THREADS; s in {-1, 0, 1};
// client.cpp mul_small_acc (out[i + j] -/+= a[j]) restated per output coefficient.  `negate` flips the sign.
template <int MAXR>
__device__ __forceinline__ void mul_small_acc_dev(const uint64_t *a_lds, const int8_t *s, uint64_t (&acc)[MAXR], int N, bool negate) {
    const int t = threadIdx.x, nr = N / KG_THREADS > 0 ? N / KG_THREADS : 1;
    for (int i = 0; i < N; i++) {
        const int si = s[i];                        // wave-uniform
        if (!si) continue;
#pragma unroll
        for (int r = 0; r < MAXR; r++) {
            if (r >= nr) break;
            const int m = t + r * KG_THREADS;
            if (m >= N) break;
            acc[r] += negacyclic_term(a_lds, N, m, i, si, negate);
        }
    }
}

// dst[q] = (WORD)al[q], q < N: a polynomial leaves LDS as it is
template <typename WORD> __device__ __forceinline__ void store_words(WORD *dst, const uint64_t *al, int N) {
    for (int q = threadIdx.x; q < N; q += KG_THREADS) dst[q] = (WORD)al[q];
}

// acc -= sum_{cc < kz} a_cc (*) z_cc, z the kz key polynomials end to end: fill(cc) puts mask cc into al; hook(cc) runs once the workgroup sees
// it and before it is multiplied (the full key forms store it there, the seeded ones have nothing to do)
template <int MAXR, typename FILL, typename HOOK>
__device__ __forceinline__ void accumulate_masks(uint64_t *al, const int8_t *z, int kz, int N, uint64_t (&acc)[MAXR], FILL fill, HOOK hook) {
    for (int cc = 0; cc < kz; cc++) {
        fill(cc);
        __syncthreads();
        hook(cc);
        mul_small_acc_dev<MAXR>(al, z + (size_t)cc * N, acc, N, true);
        __syncthreads();
    }
}
template <int MAXR, typename FILL>
__device__ __forceinline__ void accumulate_masks(uint64_t *al, const int8_t *z, int kz, int N, uint64_t (&acc)[MAXR], FILL fill) {
    accumulate_masks<MAXR>(al, z, kz, N, acc, fill, [](int) {});
}

// out[m] = (acc + e[m] + msg(m)) & wm over the lane's coefficients m = t + r * KG_THREADS, e the N noise words from draws first .. of the
// stream (through al, which the last product has left); acc <- 0 for the next row
template <typename WORD, int MAXR, typename MSG>
__device__ __forceinline__ void noise_and_store(WORD *out, uint64_t *al, uint64_t (&acc)[MAXR], int N, const Rng &rng, uint64_t first, double sigma, MSG msg) {
    fill_noise(rng, first, al, N, sigma);
    __syncthreads();
    const uint64_t wm = wmask_of<WORD>();
#pragma unroll
    for (int r = 0; r < MAXR; r++) {
        const int m = threadIdx.x + r * KG_THREADS;
        if (m >= N) break;
        out[m] = (WORD)((acc[r] + al[m] + msg(m)) & wm);
    }
#pragma unroll
    for (int r = 0; r < MAXR; r++) acc[r] = 0;      // all of them, not only the ones stored: a reset behind the bound check costs the UniEnc kernels registers
}

// rt[q] <- the ternary r of UniEnc (unienc.jl:36-55), q < N: draws [0, N) of the row's stream, (draw mod 3) - 1; through al
__device__ __forceinline__ void draw_ternary(const Rng &rng, uint64_t *al, int8_t *rt, int N) {
    fill_uniform(rng, 0, al, N, ~0ull);
    __syncthreads();
    for (int q = threadIdx.x; q < N; q += KG_THREADS) rt[q] = (int8_t)((int)(al[q] % 3) - 1);
    __syncthreads();
}

// d_j = crs_j r + sg X^0 + e, sg = s_i g_j, the noise from draws [base, base + 2 N) of the row's stream; al is free again on return
template <typename WORD, int MAXR>
__device__ __forceinline__ void unienc_d_row(WORD *dj, const WORD *crsj, const int8_t *rt, uint64_t sg, const Rng &rng, uint64_t base, double sigma,
                                             uint64_t *al, uint64_t (&acc)[MAXR], int N) {
    for (int q = threadIdx.x; q < N; q += KG_THREADS) al[q] = crsj[q];
    __syncthreads();
    mul_small_acc_dev<MAXR>(al, rt, acc, N, false);                             // crs_j r
    __syncthreads();
    noise_and_store<WORD>(dj, al, acc, N, rng, base, sigma, [&](int m) { return m == 0 ? sg : (uint64_t)0; });
    __syncthreads();
}

}  // namespace
}  // namespace mktd

// launches K<WORD, MAXR> for the ring width W and the ring size N: 4 accumulator registers per lane up to N = 4 KG_THREADS, 16 above
#define MKT_KG_LAUNCH(K, W, N, grid, lds, s, a) \
    do { \
        if ((W) == 64 && (N) <= 4 * KG_THREADS) hipLaunchKernelGGL((K<uint64_t, 4>), dim3(grid), dim3(KG_THREADS), lds, s, a); \
        else if ((W) == 64) hipLaunchKernelGGL((K<uint64_t, 16>), dim3(grid), dim3(KG_THREADS), lds, s, a); \
        else if ((N) <= 4 * KG_THREADS) hipLaunchKernelGGL((K<uint32_t, 4>), dim3(grid), dim3(KG_THREADS), lds, s, a); \
        else hipLaunchKernelGGL((K<uint32_t, 16>), dim3(grid), dim3(KG_THREADS), lds, s, a); \
    } while (0)
