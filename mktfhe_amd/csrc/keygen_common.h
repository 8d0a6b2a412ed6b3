// Steps the device key generators share (keygen.hip: the full keys; keygen_seeded.hip: the bodies of the seeded form): a workgroup of
// KG_THREADS lanes fills a polynomial from a counter-based stream in parallel -- lane t generates keystream blocks t, t + 256, ... (8 uniform
// draws or 4 Gaussian deviates each) -- and multiplies it with a small secret polynomial, N^2 / 2 word additions spread over the workgroup.
// The words are those of the sequential host loops (client.cpp).  Internal to the library.
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

// acc[r] (+)= sum_i s_i * a[(m - i) mod N] with the negacyclic sign, m = t + r * KG_THREADS; s in {-1, 0, 1};
// client.cpp mul_small_acc (out[i + j] -/+= a[j]) restated per output coefficient.  `negate` flips the sign.
template <int MAXR>
__device__ __forceinline__ void mul_small_acc_dev(const uint64_t *a_lds, const int8_t *s, uint64_t (&acc)[MAXR], int N, bool negate) {
    const int t = threadIdx.x, nr = N / KG_THREADS > 0 ? N / KG_THREADS : 1;
    for (int i = 0; i < N; i++) {
        const int si = s[i];                        // wave-uniform
        if (!si) continue;
        const bool neg = (si < 0) != negate;
#pragma unroll
        for (int r = 0; r < MAXR; r++) {
            if (r >= nr) break;
            const int m = t + r * KG_THREADS;
            if (m >= N) break;
            const uint64_t v = a_lds[(m - i) & (N - 1)];
            const bool wrap = i > m;                // the term came around X^N = -1
            acc[r] += (neg != wrap) ? (uint64_t)0 - v : v;
        }
    }
}

}  // namespace
}  // namespace mktd
