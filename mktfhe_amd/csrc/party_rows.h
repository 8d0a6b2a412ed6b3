// The frame of the party-local row kernels (partial_decrypt.hip; seeded.hip, encrypt), for gfx950: one word per row, out[r] = dot(r) + noise(r)
// (mod 2^32), dot(r) a wrapping dot product with the party's LWE key, noise(r) one ChaCha20 block and one Box-Muller (rng_chacha.h).
// Shape.  Run on the lane that holds a row's sum, the cipher would cost some thousand instruction issues of a wave with ONE active lane,
// far more than the dot product.  So a workgroup takes tiles of 64 consecutive rows and has five waves: waves 0 .. 3 compute the 64 dot
// products, 16 rows each, while wave 4 draws the tile's 64 noise words, one row per lane, beside them; after one barrier wave 4 adds the two
// and stores 64 consecutive words.  The key is staged in LDS once per workgroup (grid-stride over the tiles).
#pragma once
#include "kernel_common.h"

namespace mktd {

constexpr int PR_TILE = 64;                         // rows per tile = lanes of the noise wave
constexpr int PR_DOT_WAVES = 4;                     // waves that compute dot products
constexpr int PR_ROWS = PR_TILE / PR_DOT_WAVES;     // rows of a tile per such wave
constexpr int PR_THREADS = 64 * (PR_DOT_WAVES + 1);
constexpr unsigned PR_MAX_GRID = 2048;              // workgroups of one launch, more tiles than that: grid-stride (seeded.hip's expand kernel shares the cap)

// the sum of v over the aligned group of `width` lanes this lane is in; width a power of two, 1 .. 64
__device__ __forceinline__ uint32_t lanes_sum(uint32_t v, int width) {
#pragma unroll
    for (int o = width >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ks[0 .. padded) <- the n key words, zeros behind them
__device__ __forceinline__ void stage_key(uint32_t *ks, const uint32_t *key, int n, int padded) {
    for (int q = threadIdx.x; q < padded; q += PR_THREADS) ks[q] = q < n ? key[q] : 0u;
    __syncthreads();
}

// The tile loop.  dots: [2][PR_TILE] words of LDS.  dot(wave, tile, d), run by waves 0 .. 3, writes the sums of rows tile * PR_TILE +
// wave * PR_ROWS + i, i < PR_ROWS, to d[wave * PR_ROWS + i] (a row beyond B: anything); noise(r), run by wave 4, one row r < B per lane.
template <class Dot, class Noise>
__device__ __forceinline__ void party_rows_tiles(uint32_t *dots, size_t B, uint32_t *out, Dot dot, Noise noise) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t tiles = (B + PR_TILE - 1) / PR_TILE;
    int buf = 0;
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x, buf ^= 1) {
        const size_t r = tile * PR_TILE + lane;
        uint32_t e = 0;
        if (wave == PR_DOT_WAVES) { if (r < B) e = noise(r); }
        else dot(wave, tile, dots + buf * PR_TILE);
        // One barrier per tile suffices because dots is double-buffered: behind it the dot waves go on to the next tile and write the OTHER
        // buffer; they meet wave 4 again at that tile's barrier, which it reaches only after the reads below, and write this buffer after it.
        __syncthreads();
        if (wave == PR_DOT_WAVES && r < B) out[r] = dots[buf * PR_TILE + lane] + e;
    }
}

// the launcher's tail: tiles -> grid, key_words + the two dot buffers of LDS, launch (B > 0)
template <class K, class A>
hipError_t launch_party_rows(K kern, const A &a, size_t B, size_t key_words, hipStream_t s) {
    const size_t tiles = (B + PR_TILE - 1) / PR_TILE;
    const unsigned grid = (unsigned)(tiles < PR_MAX_GRID ? tiles : PR_MAX_GRID);
    const size_t lds = (key_words + 2 * PR_TILE) * sizeof(uint32_t);
    hipError_t e = set_lds(kern, lds); if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(PR_THREADS), lds, s, a);
    return hipGetLastError();
}

}  // namespace mktd
