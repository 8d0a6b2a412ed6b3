// Seeded ciphertexts on the device (include/mktfhe.h "seeded ciphertexts"), for gfx950: the evaluator's expansion of (mask seed, bodies) into
// ordinary rows, and a party's batched encryption that produces the bodies -- the words of mkt_client_seeded_expand / _encrypt (client.cpp),
// which are the definition.  Both sides draw a row's mask through the one mask_block of rng_chacha.h and its noise through the one
// row_noise_word (contraction off on both compilers); everything else is wrapping integer arithmetic, whose order does not matter.
// Both kernels get a lane's keystream block from lane_block() below; key and party are wave-uniform kernel arguments and stay on the scalar
// side, the rotate of the quarter round is one v_alignbit_b32 (checked in the ISA), there is no inline assembly and no scratch.
//
// EXPAND.  The output [B][lwe_len] is dense, so the whole batch is ONE span of B * lwe_len words -- zeros, masks and bodies alike -- and the
// kernel tiles that span by words, not by rows (a row of a 32-party set is tens of KiB; a row of a test set is two words).
//   1. Coalesced stores.  One ChaCha block per lane leaves a lane with 64 consecutive bytes.  A tile therefore has two phases around one
//      barrier: lane s computes the s-th keystream block that BEGINS inside the tile and puts its 16 words in LDS (rows of 17 words: the
//      writes are conflict-free, the reads at most two-way); then the workgroup streams the tile out, lane l writing the 16-byte word l of
//      each 4 KiB, aligned to the ABSOLUTE address.  Each output word is classified by its column (body: read body[row]; the party's
//      block: read LDS; else zero).  Rows have an odd word count, so the 16-byte phase changes from row to row; with the span seen as one
//      run of words that matters only at the two ends of a tile's span, where up to three single words are peeled.  LDS is double-buffered:
//      one barrier per tile.
//   2. Zero blocks cost no cipher work: only blocks of the party's own mask are enumerated.  No keystream block is computed twice: a block
//      that straddles a tile boundary belongs to the tile in which it begins, and the next tile's span starts behind it (tile_start), so
//      tile spans are [t T + carry_t, (t + 1) T + carry_{t+1}) with carry < 16.
//   3. T (SeededArgs::tile_words) is 4096 words, less where blocks are denser than one per 16 words (n < 16, or rows of few words): the
//      launcher lowers it until at most SE_SLOTS = 256 blocks can begin in T + 15 words, one per lane of the 256-thread workgroup
//      (seeded_expand_tile_words).  By count a block is ~1000 vector instructions per 64 bytes, so single-party sets are bound by the
//      cipher and sets of k >= 2 parties approach the write stream; measured figures: DESIGN.md 1f.
//   4. At most PR_MAX_GRID workgroups per launch, grid-stride beyond.
// ENCRYPT.  body[j] = e[j] - <a[j], s> + mu[j], on the five-wave tile of party_rows.h: the dot step stores the NEGATED sum and the noise step
// adds the message, so the frame's one addition gives the body.  The mask never leaves registers: a lane multiplies its 16 words with the
// key words at the same offsets, staged in LDS zero-padded to whole blocks and read as four 16-byte words, and the row's sum is gathered
// with lane exchanges.  `width` lanes share a row (SeededArgs::width, a power of two, 4 .. 64): lane i of them takes blocks i, i + width, ...;
// 64 / width rows are in flight per wave, log2(width) exchanges per row.  The launcher picks the largest width that idles at most one
// lane-pass in eight (n = 560: 35 blocks on 4 lanes, 9 passes, 35 / 36 busy).
#include "party_rows.h"
#include "rng_chacha.h"

namespace mktd {
namespace {

constexpr int SE_THREADS = 256;
constexpr int SE_SLOTS = 256;                       // keystream blocks that may begin in one tile = rows of the LDS image
constexpr int SE_PITCH = 17;                        // words per LDS row
constexpr int SE_TILE_WORDS = 4096;

// the keystream block both kernels are built on: mask words 16 blk .. 16 blk + 15 of row `row`, in this lane's registers
__device__ __forceinline__ void lane_block(const SeededArgs &a, uint64_t row, uint32_t blk, uint32_t (&x)[16]) {
    mktrng::mask_block(a.mkey, (uint32_t)a.party, a.row0 + row, blk, x);
}

struct Pos { uint64_t f, row; uint32_t c; };        // a word of the span: its index, its row and its column

// first word of tile t: t * tile_words, moved behind the keystream block that straddles that boundary (it belongs to tile t - 1)
__device__ __forceinline__ Pos tile_start(const SeededArgs &a, uint64_t t, uint64_t total) {
    Pos p;
    p.f = t * (uint64_t)a.tile_words;
    if (p.f >= total) { p.f = total; p.row = a.B; p.c = 0; return p; }
    p.row = p.f / (uint32_t)a.lwe_len;
    p.c = (uint32_t)(p.f - p.row * (uint32_t)a.lwe_len);
    const uint32_t q = p.c - (uint32_t)(a.party * a.n), n = (uint32_t)a.n;
    if (q < n && (q & 15u)) {
        const uint32_t adv = min(16u - (q & 15u), n - q);      // stays inside the row: the body word follows the last block
        p.f += adv; p.c += adv;
    }
    return p;
}

__global__ void __launch_bounds__(SE_THREADS) seeded_expand_kernel(SeededArgs a) {
    uint32_t *img = reinterpret_cast<uint32_t *>(mkt_smem);    // [2][SE_SLOTS][SE_PITCH]
    const uint32_t t = threadIdx.x, len = (uint32_t)a.lwe_len, n = (uint32_t)a.n, pn = (uint32_t)(a.party * a.n), nb = (n + 15u) >> 4;
    const uint64_t total = (uint64_t)a.B * len;
    const uint64_t tiles = (total + (uint32_t)a.tile_words - 1) / (uint32_t)a.tile_words;
    const uint32_t dq = (4u * SE_THREADS) / len, dr = (4u * SE_THREADS) % len;     // a lane's step from one 16-byte word to its next
    // index of the block that begins at or behind column c, among the nb blocks of a row
    auto block_of = [&](uint32_t c) { return c <= pn ? 0u : (c >= pn + n ? nb : (c - pn) >> 4); };
    int buf = 0;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x, buf ^= 1) {
        const Pos p0 = tile_start(a, tile, total), p1 = tile_start(a, tile + 1, total);
        uint32_t *im = img + buf * (SE_SLOTS * SE_PITCH);
        const uint32_t b0 = block_of(p0.c);
        uint32_t nblk = (uint32_t)(p1.row - p0.row) * nb + block_of(p1.c) - b0;
        nblk = nblk < (uint32_t)SE_SLOTS ? nblk : (uint32_t)SE_SLOTS;              // (the launcher's tile_words keeps it below)
        for (uint32_t s = t; s < nblk; s += SE_THREADS) {
            const uint32_t g = s + b0, r = g / nb;
            uint32_t x[16];
            lane_block(a, p0.row + r, g - r * nb, x);
#pragma unroll
            for (int i = 0; i < 16; i++) im[s * SE_PITCH + i] = x[i];
        }
        __syncthreads();
        // (a wave that runs ahead fills the other buffer; it meets the others again at the next barrier, behind these reads)
        const uint32_t span = (uint32_t)(p1.f - p0.f);
        uint32_t *base = a.out + p0.f;
        auto word_at = [&](uint32_t r, uint32_t c) -> uint32_t {                     // row r of the tile (from p0.row), column c
            if (c == len - 1) return a.in[p0.row + r];
            const uint32_t q = c - pn;
            return q < n ? im[(r * nb + (q >> 4) - b0) * SE_PITCH + (q & 15u)] : 0u;
        };
        // single words up to the first 16-byte boundary (lanes 0 .. 2) and behind the last one (lanes 4 .. 6)
        const uint32_t head = (4u - (uint32_t)((reinterpret_cast<uintptr_t>(base) >> 2) & 3u)) & 3u;
        const uint32_t nquad = span > head ? (span - head) >> 2 : 0u;
        if (t < 8) {
            const uint32_t rel = t < 4 ? t : head + 4u * nquad + (t - 4u);
            if ((t >= 4 || t < head) && rel < span) {
                const uint32_t cc = p0.c + rel, r = cc / len;
                base[rel] = word_at(r, cc - r * len);
            }
        }
        if (t < nquad) {
            const uint32_t cc = p0.c + head + 4u * t;
            uint32_t rq = cc / len, cq = cc - rq * len;
            for (uint32_t k = t; k < nquad; k += SE_THREADS) {
                uint32_t r = rq, c = cq, v[4];
#pragma unroll
                for (int w = 0; w < 4; w++) {
                    v[w] = word_at(r, c);
                    if (++c == len) { c = 0; r++; }
                }
                *reinterpret_cast<uint4 *>(base + head + 4u * k) = make_uint4(v[0], v[1], v[2], v[3]);
                rq += dq; cq += dr;
                if (cq >= len) { cq -= len; rq++; }
            }
        }
    }
}

__global__ void __launch_bounds__(PR_THREADS) seeded_encrypt_kernel(SeededArgs a) {
    const int lane = threadIdx.x & 63, nb = (a.n + 15) >> 4;
    uint32_t *ks = reinterpret_cast<uint32_t *>(mkt_smem), *dots = ks + 16 * nb;   // [16 nb] the party's key, zeros behind word n; [2][PR_TILE] the frame's dot products
    stage_key(ks, a.lwekey, a.n, 16 * nb);
    const int width = a.width, sub = lane & (width - 1), rsub = lane / width, per_pass = 64 / width;
    const auto dot = [&](int wave, size_t tile, uint32_t *d) {
#pragma unroll 1
        for (int rp = 0; rp < PR_ROWS; rp += per_pass) {
            const int rt = wave * PR_ROWS + rp + rsub;   // row of the tile; rsub < per_pass <= PR_ROWS
            const size_t r = tile * PR_TILE + rt;
            uint32_t acc = 0;
            if (r < a.B) {
#pragma unroll 1
                for (int bq = sub; bq < nb; bq += width) {
                    uint32_t x[16];
                    lane_block(a, r, (uint32_t)bq, x);
                    const uint4 *kk = reinterpret_cast<const uint4 *>(ks + 16 * bq);
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const uint4 k4 = kk[i];
                        acc += x[4 * i] * k4.x + x[4 * i + 1] * k4.y + x[4 * i + 2] * k4.z + x[4 * i + 3] * k4.w;
                    }
                }
            }
            acc = lanes_sum(acc, width);
            if (sub == 0) d[rt] = 0u - acc;
        }
    };
    party_rows_tiles(dots, a.B, a.out, dot, [&](size_t r) { return mktrng::row_noise_word(a.nkey, (uint32_t)a.party, mktrng::STREAM_ENC_NOISE, a.row0 + r, a.sigma) + a.in[r]; });
}

// most keystream blocks that begin in any window of L consecutive words of the span: the begins repeat with the row length, nb per row,
// 16 words apart inside a row; a window shorter than a row crosses one row boundary at most
int blocks_in_window(int L, int len, int nb) {
    const int part = (L % len) / 16 + 2;
    return (L / len) * nb + (part < nb ? part : nb);
}

}  // namespace

int seeded_expand_tile_words(int n, int lwe_len) {
    const int nb = (n + 15) / 16;
    int tw = SE_TILE_WORDS;
    while (tw > 4 && blocks_in_window(tw + 15, lwe_len, nb) > SE_SLOTS) tw -= 4;
    return tw;
}

hipError_t launch_seeded_expand(SeededArgs a, hipStream_t s) {
    if (!a.B) return hipSuccess;
    if (a.n < 1 || a.party < 0 || a.lwe_len < (a.party + 1) * a.n + 1) return hipErrorInvalidValue;   // the party's block lies inside a row
    a.tile_words = seeded_expand_tile_words(a.n, a.lwe_len);
    if (a.tile_words < 32) return hipErrorInvalidValue;                                               // a block never spans two boundaries
    const uint64_t total = (uint64_t)a.B * (uint64_t)a.lwe_len;
    const uint64_t tiles = (total + a.tile_words - 1) / a.tile_words;
    const unsigned grid = (unsigned)(tiles < PR_MAX_GRID ? tiles : PR_MAX_GRID);
    const size_t lds = 2 * (size_t)SE_SLOTS * SE_PITCH * sizeof(uint32_t);
    hipLaunchKernelGGL(seeded_expand_kernel, dim3(grid), dim3(SE_THREADS), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_seeded_encrypt(SeededArgs a, hipStream_t s) {
    if (!a.B) return hipSuccess;
    if (a.n < 1 || a.party < 0) return hipErrorInvalidValue;
    const int nb = (a.n + 15) / 16;
    a.width = 4;
    for (int w = 64; w > 4; w >>= 1)
        if (((nb + w - 1) / w * w - nb) * 8 <= nb) { a.width = w; break; }
    return launch_party_rows(seeded_encrypt_kernel, a, a.B, (size_t)16 * nb, s);
}

}  // namespace mktd
