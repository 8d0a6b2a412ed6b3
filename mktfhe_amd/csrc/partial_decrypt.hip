// Distributed decryption on the device (include/mktfhe.h "distributed decryption"), for gfx950: one party's shares of a batch,
//     out[j] = sum_q a[j][q] * s[q] + e[j]  (mod 2^32),    a[j] = the party's block of row j,  e[j] = smudge_word(key, party, row0 + j, sigma)
// -- the words of mkt_client_partial_decrypt (client.cpp) for the same seed: the dot product is wrapping integer arithmetic, whose order
// does not matter, and the noise goes through the one smudge_word of rng_chacha.h on both sides (contraction off on both compilers).
// The five-wave tile and the launch are party_rows.h; the dot step here streams the party's blocks once from HBM.
// Dot products.  A row has nparty * n + 1 words, an odd count: a block starts on a 4-byte boundary that changes from row to row.  Per row
// the wave peels up to three words to the next 16-byte boundary, reads the body as 16-byte accesses (lane l words 4 l .. 4 l + 3 of each
// 1 KiB) and the up to three words behind it singly; the key words come from LDS at the same, unaligned, offsets as single words.  Four
// rows are in flight per wave, then each sum is reduced across the wave with lane exchanges; no atomics.
#include "party_rows.h"
#include "rng_chacha.h"

namespace mktd {
namespace {

constexpr int PD_GROUP = 4;                         // rows in flight per wave

__global__ void __launch_bounds__(PR_THREADS) partial_decrypt_kernel(PartialDecryptArgs a) {
    uint32_t *ks = reinterpret_cast<uint32_t *>(mkt_smem), *dots = ks + a.n;   // [n] the party's key, [2][PR_TILE] the frame's dot products
    const int lane = threadIdx.x & 63, n = a.n;
    stage_key(ks, a.lwekey, n, n);
    const auto dot = [&](int wave, size_t tile, uint32_t *d) {
        const size_t r0 = tile * PR_TILE + (size_t)wave * PR_ROWS;
        uint32_t mine = 0;                               // lane i: the sum of row r0 + i
#pragma unroll 1
        for (int g = 0; g < PR_ROWS; g += PD_GROUP) {
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
                uint4 v[PD_GROUP] = {};                  // (zeroed: words no branch below assigns are otherwise carried round the loops, 74 VGPRs for 72 and a wave less per SIMD)
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
                const uint32_t s = lanes_sum(acc[u], 64);
                if (lane == g + u) mine = s;
            }
        }
        if (lane < PR_ROWS) d[wave * PR_ROWS + lane] = mine;
    };
    party_rows_tiles(dots, a.B, a.out, dot, [&](size_t r) { return mktrng::smudge_word(a.key, (uint32_t)a.party, a.row0 + r, a.sigma); });
}

}  // namespace

hipError_t launch_partial_decrypt(const PartialDecryptArgs &a, hipStream_t s) {
    if (!a.B) return hipSuccess;
    if (a.n < 1 || a.party < 0 || a.lwe_stride < (a.party + 1) * a.n + 1) return hipErrorInvalidValue;   // the party's block lies inside a row
    return launch_party_rows(partial_decrypt_kernel, a, a.B, (size_t)a.n, s);
}

}  // namespace mktd
