// Seeded evaluation keys on the device (include/mktfhe.h "seeded evaluation keys"), for gfx950: the evaluator's expansion of (mask seed, bodies)
// into the two large keys of a party -- the words of mkt_client_seeded_keys_expand (client.cpp), which is the definition.  Nothing here is
// secret: the seed is public and the bodies are what the party shipped.
// Both kernels are built like seeded.hip's expand kernel: the unit of cipher work is one ChaCha20 block (stream_block of rng_chacha.h), 16
// keystream words = 64 consecutive bytes of the output, computed by ONE lane.  A tile is SK_SLOTS = 256 consecutive units, one per lane of the
// 256-thread workgroup, and has two phases around one barrier: lane s computes unit s and puts its 16 words in LDS (rows of 17 words: the
// writes are conflict-free, the reads at most two-way); then the workgroup streams the tile out as 16-byte words, lane v writing quad v of
// each 4 KiB, so every store instruction of a wave covers 1 KiB of consecutive, 16-byte aligned addresses.  LDS is double-buffered: one
// barrier per tile.  No inline assembly, no scratch, plain vector stores.  At most PR_MAX_GRID workgroups per launch, grid-stride beyond.
//
// KEY-SWITCHING KEY.  The output is the resident table itself: rows of n + 1 words at a pitch of n1p = 4 ceil((n + 1) / 4) words, so every row
// starts 16-byte aligned and the table is one dense run of n1p / 4 quads per row.  A row is cut into ceil(n1p / 16) units; unit blk holds the
// words 16 blk .. of the row: mask words below n (keystream block blk of the row's stream, the surplus of the last block dropped), the body
// word at n (read from the compact array), zeros behind it (the pad), and nothing but zeros in a row a block scheme leaves out (no cipher work).
// The last unit of a row is short where n1p is no multiple of 16; the quads of a tile are numbered in address order across that.
// BOOTSTRAPPING KEY.  The output is the coefficient layout of mkt_load_brk, dense, polynomials of N ring words: N W / 512 units each.  A
// polynomial is either a body, copied from the compact upload (its lanes do no cipher work; whole waves of them from N = 1024 on), or mask
// polynomial P: unit u is keystream block u of P's stream on either ring (32-bit: coefficients 16 u ..; 64-bit: coefficients 8 u .., low word first).
// PACKING KEY (mktfhe_pack.h "SEEDED"; launched from pack_keys.hip).  The same kernel: a packing key is n l_pk groups of (b, a_0 .. a_{kr-1}) like
// an RGSW key, its masks on stream 19 with the gadget in the high word of the stream index (SeededBrkArgs::stream, idx_hi).  t_rows != 0 writes
// the layout an MKT_ARITH_EXACT context keeps resident, [polynomial][row], each polynomial still a dense run of 16-byte stores.
#include "party_rows.h"
#include "rng_chacha.h"

namespace mktd {
namespace {

constexpr int SK_THREADS = 256;
constexpr int SK_SLOTS = 256;                       // units per tile = rows of the LDS image
constexpr int SK_PITCH = 17;                        // words per LDS row

__global__ void __launch_bounds__(SK_THREADS) seeded_ksk_expand_kernel(SeededKskArgs a) {
    uint32_t *img = reinterpret_cast<uint32_t *>(mkt_smem);    // [2][SK_SLOTS][SK_PITCH]
    const uint32_t t = threadIdx.x, n = (uint32_t)a.n, Q = (uint32_t)a.n1p >> 2, nbp = (Q + 3u) >> 2;
    const uint64_t units = a.rows * nbp, tiles = (units + SK_SLOTS - 1) / SK_SLOTS;
    int buf = 0;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x, buf ^= 1) {
        const uint64_t g0 = tile * SK_SLOTS, R0 = g0 / nbp;
        const uint32_t b0 = (uint32_t)(g0 - R0 * nbp);                                   // first unit of the tile: unit b0 of row R0
        const uint32_t cnt = (uint32_t)(units - g0 < (uint64_t)SK_SLOTS ? units - g0 : (uint64_t)SK_SLOTS);
        uint32_t *im = img + buf * (SK_SLOTS * SK_PITCH);
        if (t < cnt) {
            const uint32_t r = (t + b0) / nbp, blk = t + b0 - r * nbp;
            const uint64_t R = R0 + r;
            uint32_t x[16];
            const bool absent = R / a.rows_per_cj < (uint64_t)a.absent_below;                  // (c, j) = R / (Drows f)
            if (!absent && 16u * blk < n) mktrng::stream_block(a.mkey, mktrng::STREAM_KSK_MASK, (uint32_t)a.party, R, blk, x);
            else {
#pragma unroll
                for (int i = 0; i < 16; i++) x[i] = 0u;
            }
            const uint32_t body = (!absent && (n >> 4) == blk) ? a.body[R] : 0u;
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const uint32_t q = 16u * blk + (uint32_t)i;
                im[t * SK_PITCH + i] = q < n ? x[i] : (q == n ? body : 0u);
            }
        }
        __syncthreads();
        // (a wave that runs ahead fills the other buffer; it meets the others again at the next barrier, behind these reads)
        const uint32_t r1 = (b0 + cnt) / nbp, b1 = b0 + cnt - r1 * nbp;
        const uint32_t nquad = r1 * Q + 4u * b1 - 4u * b0;                               // a tile ends on a unit boundary, and 4 b < Q for every unit b of a row
        uint4 *base = reinterpret_cast<uint4 *>(a.out) + (R0 * Q + 4u * b0);
        for (uint32_t v = t; v < nquad; v += SK_THREADS) {
            const uint32_t w = 4u * b0 + v, r = w / Q, qi = w - r * Q;
            const uint32_t *src = im + (r * nbp + (qi >> 2) - b0) * SK_PITCH + 4u * (qi & 3u);
            base[v] = make_uint4(src[0], src[1], src[2], src[3]);
        }
    }
}

// where an output polynomial of the bootstrapping key comes from: a body of the compact section (idx = its polynomial there) or mask polynomial
// idx.  The polynomial is number rem + d of group `grp` onwards, groups of kr + 1 (one RGSW sample) or 3 l (one UniEnc key bit) polynomials:
// a tile divides its first polynomial's 64-bit index once, its lanes go on in 32 bits
struct BrkPoly { bool mask; uint64_t idx; };
__device__ __forceinline__ BrkPoly brk_poly(const SeededBrkArgs &a, uint64_t grp, uint32_t x) {
    if (!a.unienc) {
        const uint32_t polys = (uint32_t)a.kr + 1u, ds = x / polys, q = x - ds * polys;
        const uint64_t S = grp + ds;
        return q == 0 ? BrkPoly{false, S} : BrkPoly{true, S * (uint32_t)a.kr + (q - 1u)};
    }
    const uint32_t l = (uint32_t)a.l, di = x / (3u * l), tt = x - di * (3u * l);
    const uint64_t i = grp + di;
    if (tt < l) return BrkPoly{false, i * (2u * l) + tt};                                // d_j
    const uint32_t j = (tt - l) >> 1;
    return ((tt - l) & 1u) ? BrkPoly{true, i * l + j} : BrkPoly{false, i * (2u * l) + l + j};   // f_j.a : f_j.b
}

__global__ void __launch_bounds__(SK_THREADS) seeded_brk_expand_kernel(SeededBrkArgs a) {
    uint32_t *img = reinterpret_cast<uint32_t *>(mkt_smem);    // [2][SK_SLOTS][SK_PITCH]
    const uint32_t t = threadIdx.x, lc = (uint32_t)a.log_units;                          // units per polynomial = 1 << lc
    const uint32_t period = a.unienc ? 3u * (uint32_t)a.l : (uint32_t)a.kr + 1u, umask = (1u << lc) - 1u;
    const uint64_t units = a.npolys << lc, tiles = (units + SK_SLOTS - 1) / SK_SLOTS;
    const uint4 *body = reinterpret_cast<const uint4 *>(a.body);
    int buf = 0;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x, buf ^= 1) {
        const uint64_t g0 = tile * SK_SLOTS;
        const uint32_t cnt = (uint32_t)(units - g0 < (uint64_t)SK_SLOTS ? units - g0 : (uint64_t)SK_SLOTS);
        uint32_t *im = img + buf * (SK_SLOTS * SK_PITCH);
        const uint64_t op0 = g0 >> lc, grp = op0 / period;                              // the tile's first polynomial: number rem of group grp
        const uint32_t rem = (uint32_t)(op0 - grp * period), u0 = (uint32_t)g0 & umask; // its first unit: unit u0 of that polynomial
        if (t < cnt) {
            const BrkPoly bp = brk_poly(a, grp, rem + ((u0 + t) >> lc));
            if (bp.mask) {
                uint32_t x[16];
                mktrng::stream_block(a.mkey, a.stream, (uint32_t)a.party, bp.idx | ((uint64_t)a.idx_hi << 32), (u0 + t) & umask, x);
#pragma unroll
                for (int i = 0; i < 16; i++) im[t * SK_PITCH + i] = x[i];
            }
        }
        __syncthreads();
        uint4 *base = reinterpret_cast<uint4 *>(a.out) + g0 * 4u;
        for (uint32_t v = t; v < 4u * cnt; v += SK_THREADS) {
            const uint32_t s = v >> 2, k = v & 3u, x = rem + ((u0 + s) >> lc);
            const BrkPoly bp = brk_poly(a, grp, x);
            uint4 *dst = base + v;
            if (a.t_rows) {                                                              // [polynomial][row]: polynomial q of row grp + ds
                const uint32_t ds = x / period, q = x - ds * period;
                dst = reinterpret_cast<uint4 *>(a.out) + (((((uint64_t)q * a.t_rows + grp + ds) << lc) + ((u0 + s) & umask)) << 2) + k;
            }
            if (bp.mask) {
                const uint32_t *src = im + s * SK_PITCH + 4u * k;
                *dst = make_uint4(src[0], src[1], src[2], src[3]);
            } else *dst = body[(((bp.idx << lc) + ((u0 + s) & umask)) << 2) + k];
        }
    }
}

unsigned sk_grid(uint64_t units) {
    const uint64_t tiles = (units + SK_SLOTS - 1) / SK_SLOTS;
    return (unsigned)(tiles < PR_MAX_GRID ? tiles : PR_MAX_GRID);
}
constexpr size_t SK_LDS = 2 * (size_t)SK_SLOTS * SK_PITCH * sizeof(uint32_t);

}  // namespace

hipError_t launch_seeded_ksk_expand(const SeededKskArgs &a, hipStream_t s) {
    if (!a.rows) return hipSuccess;
    if (a.n < 1 || a.party < 0 || a.n1p < a.n + 1 || (a.n1p & 3) || !a.rows_per_cj || a.absent_below < 0) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(a.out) & 15u) || !a.body) return hipErrorInvalidValue;           // 16-byte stores
    const uint64_t nbp = ((uint64_t)a.n1p / 4 + 3) / 4;
    hipLaunchKernelGGL(seeded_ksk_expand_kernel, dim3(sk_grid(a.rows * nbp)), dim3(SK_THREADS), SK_LDS, s, a);
    return hipGetLastError();
}

hipError_t launch_seeded_brk_expand(const SeededBrkArgs &a, hipStream_t s) {
    if (!a.npolys) return hipSuccess;
    if (a.party < 0 || a.log_units < 0 || a.log_units > 16 || (a.unienc ? a.l < 1 : a.kr < 1) || !a.stream) return hipErrorInvalidValue;
    if (a.t_rows && (a.unienc || a.t_rows * ((uint64_t)a.kr + 1) != a.npolys)) return hipErrorInvalidValue;      // the transposed form: whole rows of kr + 1
    if (((reinterpret_cast<uintptr_t>(a.out) | reinterpret_cast<uintptr_t>(a.body)) & 15u) || !a.body || !a.out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(seeded_brk_expand_kernel, dim3(sk_grid(a.npolys << a.log_units)), dim3(SK_THREADS), SK_LDS, s, a);
    return hipGetLastError();
}

}  // namespace mktd
