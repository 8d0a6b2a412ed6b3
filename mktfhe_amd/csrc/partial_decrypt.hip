// Distributed decryption on the device (include/mktfhe.h "distributed decryption"), for gfx950: one party's shares of a batch,
//     out[j] = sum_q a[j][q] * s[q] + e[j]  (mod 2^32),    a[j] = the party's block of row j,  e[j] = smudge_word(key, party, row0 + j, sigma)
// -- the words of mkt_client_partial_decrypt (client.cpp) for the same seed: the dot product is wrapping integer arithmetic, whose order
// does not matter, and the noise goes through the one smudge_word of rng_chacha.h on both sides (contraction off on both compilers).
//
// Shape.  The kernel streams the party's blocks once from HBM, and it runs one ChaCha20 block and one Box-Muller per row.  Run on the
// lane that holds a row's sum, the cipher would cost some thousand instruction issues of a wave with ONE active lane, far more than
// reading the row.  So a workgroup takes tiles of 64 consecutive rows and has five waves: waves 0 .. 3 compute the 64 dot products, 16 rows
// each, while wave 4 draws the 64 noise words of the tile, one row per lane, beside them; after one barrier wave 4 adds the two and
// stores 64 consecutive words.  The key is staged in LDS once per workgroup (grid-stride over the tiles).
// Dot products.  A row has nparty * n + 1 words, an odd count: a block starts on a 4-byte boundary that changes from row to row.  Per row
// the wave peels up to three words to the next 16-byte boundary, reads the body as 16-byte accesses (lane l words 4 l .. 4 l + 3 of each
// 1 KiB) and the up to three words behind it singly; the key words come from LDS at the same, unaligned, offsets as single words.  Four
// rows are in flight per wave, then each sum is reduced across the wave with lane exchanges; no atomics.
#include "kernel_common.h"
#include "rng_chacha.h"

namespace mktd {
namespace {

constexpr int PD_TILE = 64;                         // rows per tile = lanes of the noise wave
constexpr int PD_DOT_WAVES = 4;                     // waves that read rows
constexpr int PD_ROWS = PD_TILE / PD_DOT_WAVES;     // rows of a tile per such wave
constexpr int PD_GROUP = 4;                         // rows in flight per wave
constexpr int PD_THREADS = 64 * (PD_DOT_WAVES + 1);
constexpr unsigned PD_MAX_GRID = 2048;              // workgroups of one launch; more tiles than that: grid-stride

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ void __launch_bounds__(PD_THREADS) partial_decrypt_kernel(PartialDecryptArgs a) {
    uint32_t *ks = reinterpret_cast<uint32_t *>(mkt_smem);   // [n] the party's key
    uint32_t *dots = ks + a.n;                               // [2][PD_TILE] the tile's dot products, double-buffered: one barrier per tile
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, n = a.n;
    for (int q = t; q < n; q += PD_THREADS) ks[q] = a.lwekey[q];
    __syncthreads();
    const size_t tiles = (a.B + PD_TILE - 1) / PD_TILE;
    int buf = 0;
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x, buf ^= 1) {
        uint32_t e = 0;
        if (wave == PD_DOT_WAVES) {
            const size_t r = tile * PD_TILE + lane;
            if (r < a.B) e = mktrng::smudge_word(a.key, (uint32_t)a.party, a.row0 + r, a.sigma);
        } else {
            const size_t r0 = tile * PD_TILE + (size_t)wave * PD_ROWS;
            uint32_t mine = 0;                               // lane i: the sum of row r0 + i
#pragma unroll 1
            for (int g = 0; g < PD_ROWS; g += PD_GROUP) {
                const uint32_t *row[PD_GROUP];
                int peel[PD_GROUP], nvec[PD_GROUP], maxvec = 0;
                uint32_t acc[PD_GROUP];
#pragma unroll
                for (int u = 0; u < PD_GROUP; u++) {
                    const size_t r = r0 + g + u;
                    const bool live = r < a.B;               // wave-uniform; a row beyond the batch is never read
                    row[u] = a.lwe + (live ? r : 0) * (size_t)a.lwe_stride + (size_t)a.party * n;
                    const int nl = live ? n : 0;
                    const int p = (int)((4u - (unsigned)((reinterpret_cast<uintptr_t>(row[u]) >> 2) & 3u)) & 3u);
                    peel[u] = p < nl ? p : nl;
                    nvec[u] = (nl - peel[u]) >> 2;
                    maxvec = nvec[u] > maxvec ? nvec[u] : maxvec;
                    acc[u] = 0;
                    // the words before the 16-byte body (lanes 0 .. 2) and behind it (lanes 4 .. 6)
                    const int q = lane < 4 ? lane : peel[u] + 4 * nvec[u] + lane - 4;
                    if ((lane < 4 && lane < peel[u]) || (lane >= 4 && lane < 8 && q < nl)) acc[u] = row[u][q] * ks[q];
                }
                for (int j = lane; j < maxvec; j += 64) {
                    uint4 v[PD_GROUP];
#pragma unroll
                    for (int u = 0; u < PD_GROUP; u++)
                        if (j < nvec[u]) v[u] = *reinterpret_cast<const uint4 *>(row[u] + peel[u] + 4 * j);
#pragma unroll
                    for (int u = 0; u < PD_GROUP; u++)
                        if (j < nvec[u]) {
                            const uint32_t *kk = ks + peel[u] + 4 * j;
                            acc[u] += v[u].x * kk[0] + v[u].y * kk[1] + v[u].z * kk[2] + v[u].w * kk[3];
                        }
                }
#pragma unroll
                for (int u = 0; u < PD_GROUP; u++) {
                    const uint32_t s = wave_sum(acc[u]);
                    if (lane == g + u) mine = s;
                }
            }
            if (lane < PD_ROWS) dots[buf * PD_TILE + wave * PD_ROWS + lane] = mine;
        }
        __syncthreads();
        // (the other waves go on to the next tile's rows and write the other buffer; they meet this wave again at that tile's barrier,
        // which it reaches only after these reads)
        if (wave == PD_DOT_WAVES) {
            const size_t r = tile * PD_TILE + lane;
            if (r < a.B) a.out[r] = dots[buf * PD_TILE + lane] + e;
        }
    }
}

}  // namespace

hipError_t launch_partial_decrypt(const PartialDecryptArgs &a, hipStream_t s) {
    if (!a.B) return hipSuccess;
    if (a.n < 1 || a.party < 0 || a.lwe_stride < (a.party + 1) * a.n + 1) return hipErrorInvalidValue;   // the party's block lies inside a row
    const size_t tiles = (a.B + PD_TILE - 1) / PD_TILE;
    const unsigned grid = (unsigned)(tiles < PD_MAX_GRID ? tiles : PD_MAX_GRID);
    const size_t lds = ((size_t)a.n + 2 * PD_TILE) * sizeof(uint32_t);
    hipError_t e = set_lds(partial_decrypt_kernel, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(partial_decrypt_kernel, dim3(grid), dim3(PD_THREADS), lds, s, a);
    return hipGetLastError();
}

}  // namespace mktd
