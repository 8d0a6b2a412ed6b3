// Evaluation-key generation on the device: the two large keys of a party -- the RGSW / UniEnc
// bootstrapping key and the LWE key-switching key -- sampled with exact integer arithmetic on the GPU from the party's
// secret keys.  Reference: keygen.jl:13-23, :39-51, :71-79, :106-114, :143-151; lwe.jl:11-22, :78-93; gsw.jl:174-178;
// lev.jl:31-37, :88-102; unienc.jl:36-55.  The seeded streams, their consumption order and every arithmetic step are
// those of mkt_client_party_keygen (client.cpp), so the generated words are identical to the host path's; the
// bootstrapping key is left in coefficient form for the caller to pre-transform (context.cpp).
//
// Randomness: the ChaCha20 streams of client.cpp (rng_chacha.h).  The streams are counter-based, so the workgroup
// fills a whole polynomial in parallel and still produces exactly the words the sequential host loop draws.  The two
// polynomial kernels are built from the steps of keygen_common.h (accumulate_masks, noise_and_store, draw_ternary,
// unienc_d_row): what stands here is where their masks, noise and messages come from, and that the masks are stored.
// The key-switching kernel is an algorithm of its own: one lane per coefficient, drawing sequentially.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_api.h"
#include "keygen_common.h"

#pragma clang fp contract(off)

namespace mktd {
namespace {

// One RLWE sample of an RGSW row (gsw.jl:174-178, lev.jl:88-102, lwe.jl:78-93) per workgroup:
// sample index = (i * rows + c * l + j); out polys (b, a_0..a_{kr-1}) at native width.  Masks: draws [cc N, (cc + 1) N) of the
// sample's secret stream 2, stored as they are multiplied; noise: the 2 N draws behind them.
template <typename WORD, int MAXR>
__global__ __launch_bounds__(KG_THREADS) void keygen_rgsw_kernel(KeygenArgs a) {
    extern __shared__ uint64_t kg_smem[];
    uint64_t *al = kg_smem;                        // [N] mask polynomial, then the noise
    const int N = a.N, t = threadIdx.x;
    const uint64_t wm = wmask_of<WORD>();
    const int rows = (a.kr + 1) * a.l, polys = a.kr + 1;
    const int sample = blockIdx.x, i = sample / rows, cj = sample % rows, c = cj / a.l, j = cj % a.l;
    WORD *out = reinterpret_cast<WORD *>(a.out) + (size_t)sample * polys * N;
    const Rng rng(a.key, (uint32_t)a.party, 2, (uint32_t)i, (uint32_t)cj);
    uint64_t acc[MAXR] = {};
    accumulate_masks<MAXR>(al, a.zring + (size_t)a.zoff * N, a.kr, N, acc,
                           [&](int cc) { fill_uniform(rng, (uint64_t)cc * N, al, N, wm); },
                           [&](int cc) { store_words(out + (size_t)(1 + cc) * N, al, N); });
    noise_and_store<WORD>(out, al, acc, N, rng, (uint64_t)a.kr * N, a.sigma_ring, [](int) { return (uint64_t)0; });
    __syncthreads();
    // message: + s_i * g_j on coefficient 0 of polynomial c (c = 0: b; c >= 1: a_{c-1})
    const uint64_t g = (uint64_t)1 << (a.W - (j + 1) * a.logB);
    if (t == 0) out[(size_t)c * N] = (WORD)((out[(size_t)c * N] + (uint64_t)a.lwekey[i] * g) & wm);
}

// UniEnc_z(s_i) (unienc.jl:36-55) per workgroup: d[j] = crs[j] * r + s_i g_j + e ; f[j] = RLWE_z(g_j r)
template <typename WORD, int MAXR>
__global__ __launch_bounds__(KG_THREADS) void keygen_unienc_kernel(KeygenArgs a) {
    extern __shared__ uint64_t kg_smem[];
    const int N = a.N, l = a.l, i = blockIdx.x;
    uint64_t *al = kg_smem;                        // [N] words
    int8_t *rt = reinterpret_cast<int8_t *>(kg_smem + N);   // [N] ternary r
    const uint64_t wm = wmask_of<WORD>();
    WORD *out = reinterpret_cast<WORD *>(a.out) + (size_t)i * 3 * l * N;
    const WORD *crs = reinterpret_cast<const WORD *>(a.crs);
    const Rng rng(a.key, (uint32_t)a.party, 2, (uint32_t)i);
    // stream layout of the host loop: draws [0, N) ternary r; per j at base = N + 5 N j: noise of d (2 draws each),
    // base + 2N: mask of f[j], base + 3N: noise of f[j]
    draw_ternary(rng, al, rt, N);
    for (int j = 0; j < l; j++) {
        uint64_t acc[MAXR] = {};
        const uint64_t g = (uint64_t)1 << (a.W - (j + 1) * a.logB);
        const uint64_t base = (uint64_t)N + (uint64_t)5 * N * j;
        unienc_d_row<WORD, MAXR>(out + (size_t)j * N, crs + (size_t)j * N, rt, (uint64_t)a.lwekey[i] * g, rng, base, a.sigma_ring, al, acc, N);
        // f.stack[j] = RLWE_z(g_j * r): a uniform, b = -a z + e + g r
        WORD *fb = out + (size_t)(l + 2 * j) * N, *fa = fb + N;
        accumulate_masks<MAXR>(al, a.zring + (size_t)a.zoff * N, 1, N, acc,
                               [&](int) { fill_uniform(rng, base + (uint64_t)2 * N, al, N, wm); },
                               [&](int) { store_words(fa, al, N); });
        noise_and_store<WORD>(fb, al, acc, N, rng, base + (uint64_t)3 * N, a.sigma_ring, [&](int m) { return g * (uint64_t)(int64_t)rt[m]; });
        __syncthreads();
    }
}

// Key-switching key (keygen.jl:17-23 etc., lev.jl:31-37, lwe.jl:11-22): one lane per extracted coefficient (c, j),
// rows [(c*N + j)][d][t] of n + 1 words at stride n1p.
__global__ void keygen_ksk_kernel(KeygenArgs a, uint32_t *ksk, int n1p, int kk, int dr, int is_block) {
    const int cj = blockIdx.x * blockDim.x + threadIdx.x;
    if (cj >= kk * a.N) return;
    const int c = cj / a.N, j = cj % a.N, n = a.n;
    if (is_block && (long)c * a.N + j < n) return;                    // keygen.jl:46, :147
    Rng rng(a.key, (uint32_t)a.party, 5, (uint32_t)cj);
    const uint32_t zj = (uint32_t)a.zring[(size_t)(a.zoff + c) * a.N + j];
    for (int d = 0; d < dr; d++)
        for (int t = 0; t < a.f; t++) {
            uint32_t *row = ksk + ((((size_t)c * a.N + j) * dr + d) * a.f + t) * n1p;
            const uint32_t msg = (uint32_t)(zj * (uint32_t)(d + 1)) << (32 - (t + 1) * a.logD);
            uint32_t dot = 0;
            for (int q = 0; q < n; q++) { const uint32_t w = (uint32_t)rng.next(); row[q] = w; dot += w * a.lwekey[q]; }
            row[n] = (uint32_t)rng.noise(a.sigma_lwe) - dot + msg;
        }
}

}  // namespace

hipError_t launch_keygen_brk(const KeygenArgs &a, int unienc, hipStream_t s) {
    const int N = a.N;
    if (N > 16 * KG_THREADS) return hipErrorInvalidValue;
    const size_t lds = (size_t)N * 8 + (unienc ? (size_t)N : 0);
    const unsigned grid = unienc ? (unsigned)a.n : (unsigned)(a.n * (a.kr + 1) * a.l);
    if (unienc) MKT_KG_LAUNCH(keygen_unienc_kernel, a.W, N, grid, lds, s, a);
    else MKT_KG_LAUNCH(keygen_rgsw_kernel, a.W, N, grid, lds, s, a);
    return hipGetLastError();
}

hipError_t launch_keygen_ksk(const KeygenArgs &a, uint32_t *ksk, int n1p, int kk, int dr, int is_block, hipStream_t s) {
    const int total = kk * a.N;
    hipLaunchKernelGGL(keygen_ksk_kernel, dim3((total + 63) / 64), dim3(64), 0, s, a, ksk, n1p, kk, dr, is_block);
    return hipGetLastError();
}

}  // namespace mktd
