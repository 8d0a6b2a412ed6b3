// The seeded key form generated on the device (include/mktfhe.h "seeded evaluation keys"), for gfx950: the compact sections of one party --
// the body polynomials of its bootstrapping key and the body words of its key-switching key -- from the party's secrets and a PUBLIC mask
// seed, the words of mkt_client_party_keygen_seeded (client.cpp), which is the definition.  The masks are keystream of the public streams
// 12 and 13 (stream_block of rng_chacha.h): they are generated where they are multiplied and never stored, the evaluator regenerates them
// (seeded_keys.hip).  The noise comes from the party's secret streams 14, 15 and 16.  Everything but the Gaussian deviate is wrapping integer
// arithmetic, whose order does not matter; the deviate is the one box_muller of rng_chacha.h, contraction off.  No inline assembly, plain stores.
//
// BOOTSTRAPPING KEY, RGSW.  One workgroup per sample S = i rows + c l + j, the steps of keygen_rgsw_kernel (keygen.hip), stated once in
// keygen_common.h: accumulate_masks with mask polynomial P = S kr + cc of stream 13 for cc < kr (fill_mask_poly: one keystream block per lane
// and pass, 16 coefficients of the 32-bit ring or 8 of the 64-bit one, low word first), then noise_and_store with the N noise words of
// stream 14 at index S and the message IN THE BODY: s_i g_j at coefficient 0 for c = 0, s_i g_j z_{c-1} on every coefficient for c >= 1.
// Only the body is stored: 1 / (kr + 1) of the full generator's stores.
// BOOTSTRAPPING KEY, UniEnc (CCS).  One workgroup per key bit i, ONE secret stream (16, index i) in the order of the host loop: draws
// [0, N) the ternary r (draw_ternary); then per gadget row j the 2 N draws of d_j's noise at N + 4 N j and the 2 N draws of f_j.b's noise
// behind them (no mask is drawn from this stream, unlike stream 2 of keygen_unienc_kernel).  d_j = crs_j r + s_i g_j X^0 + e is stored
// whole (unienc_d_row), f_j.b = -a z + e + g_j r is the body step again with a = mask polynomial i l + j of stream 13.
// KEY-SWITCHING KEY.  One word per row R = ((c N + j) Drows + d) f + t: body[R] = e_R - <a_R, s> + msg(R), a sibling of seeded.hip's encrypt
// kernel on the five-wave tile of party_rows.h: the LWE key staged in LDS zero-padded to whole blocks (the surplus words of a row's last
// block multiply zeros), `width` lanes share a row's keystream blocks of stream 12 and gather the sum with lane exchanges, the noise wave
// draws e_R (stream 15) and adds msg = ((d + 1) z_c[j]) << (32 - (t + 1) logD).  A row a block scheme leaves out (c N + j < n) gets body 0
// and does no cipher work.  At most PR_MAX_GRID workgroups per launch, grid-stride beyond.
#include "keygen_common.h"
#include "party_rows.h"

namespace mktd {
namespace {

// al[q] <- coefficient q of mask polynomial P of the bootstrapping key (stream 13), q < N
template <typename WORD>
__device__ __forceinline__ void fill_brk_mask(const KeygenSeededArgs &a, uint64_t P, uint64_t *al, int N) {
    fill_mask_poly<WORD>(a.mkey, mktrng::STREAM_BRK_MASK, (uint32_t)a.party, P, al, N);   // (keygen_common.h: shared with pack_keys.hip)
}

template <typename WORD, int MAXR>
__global__ __launch_bounds__(KG_THREADS) void keygen_seeded_rgsw_kernel(KeygenSeededArgs a) {
    uint64_t *al = reinterpret_cast<uint64_t *>(mkt_smem);          // [N] a mask polynomial, then the noise
    const int N = a.N;
    const int rows = (a.kr + 1) * a.l;
    const uint32_t S = blockIdx.x;
    const int i = (int)(S / (uint32_t)rows), cj = (int)(S % (uint32_t)rows), c = cj / a.l, j = cj % a.l;
    WORD *out = reinterpret_cast<WORD *>(a.brk_body) + (size_t)S * N;
    uint64_t acc[MAXR] = {};
    accumulate_masks<MAXR>(al, a.zring, a.kr, N, acc, [&](int cc) { fill_brk_mask<WORD>(a, (uint64_t)S * (uint32_t)a.kr + (uint32_t)cc, al, N); });
    const Rng rng(a.key, (uint32_t)a.party, mktrng::STREAM_BRK_NOISE, S, 0u);
    const uint64_t g = (uint64_t)a.lwekey[i] << (a.W - (j + 1) * a.logB);
    const int8_t *zm = a.zring + (size_t)(c > 0 ? c - 1 : 0) * N;   // m_c = z_{c-1} for c >= 1
    noise_and_store<WORD>(out, al, acc, N, rng, 0, a.sigma_ring,
                          [&](int m) { return g * (c == 0 ? (m == 0 ? (uint64_t)1 : (uint64_t)0) : (uint64_t)(int64_t)zm[m]); });
}

template <typename WORD, int MAXR>
__global__ __launch_bounds__(KG_THREADS) void keygen_seeded_unienc_kernel(KeygenSeededArgs a) {
    uint64_t *al = reinterpret_cast<uint64_t *>(mkt_smem);          // [N] words
    const int N = a.N, l = a.l, i = blockIdx.x;
    int8_t *rt = reinterpret_cast<int8_t *>(al + N);                // [N] ternary r
    WORD *out = reinterpret_cast<WORD *>(a.brk_body) + (size_t)i * 2 * l * N;    // d_0 .. d_{l-1}, f_0.b .. f_{l-1}.b
    const WORD *crs = reinterpret_cast<const WORD *>(a.crs);
    const Rng rng(a.key, (uint32_t)a.party, mktrng::STREAM_UNI_NOISE, (uint32_t)i);
    draw_ternary(rng, al, rt, N);
    for (int j = 0; j < l; j++) {
        uint64_t acc[MAXR] = {};
        const uint64_t g = (uint64_t)1 << (a.W - (j + 1) * a.logB);
        const uint64_t base = (uint64_t)N + (uint64_t)4 * N * j;    // first draw of d_j's noise; f_j.b's follows 2 N draws on
        unienc_d_row<WORD, MAXR>(out + (size_t)j * N, crs + (size_t)j * N, rt, (uint64_t)a.lwekey[i] * g, rng, base, a.sigma_ring, al, acc, N);
        accumulate_masks<MAXR>(al, a.zring, 1, N, acc, [&](int) { fill_brk_mask<WORD>(a, (uint64_t)i * (uint32_t)l + (uint32_t)j, al, N); });   // -a z
        noise_and_store<WORD>(out + (size_t)(l + j) * N, al, acc, N, rng, base + (uint64_t)2 * N, a.sigma_ring,
                              [&](int m) { return g * (uint64_t)(int64_t)rt[m]; });
        __syncthreads();
    }
}

__global__ void __launch_bounds__(PR_THREADS) keygen_seeded_ksk_kernel(KeygenSeededArgs a) {
    const int lane = threadIdx.x & 63, nb = (a.n + 15) >> 4;
    uint32_t *ks = reinterpret_cast<uint32_t *>(mkt_smem), *dots = ks + 16 * nb;   // [16 nb] the party's key, zeros behind word n; [2][PR_TILE] the frame's dot products
    stage_key(ks, a.lwekey, a.n, 16 * nb);
    const size_t B = (size_t)a.ksk_rows;
    const uint32_t per_cj = (uint32_t)(a.drows * a.f);
    const auto absent = [&](size_t R) { return R / per_cj < (size_t)a.absent_below; };               // (c, j) = R / (Drows f)
    const int width = a.width, sub = lane & (width - 1), rsub = lane / width, per_pass = 64 / width;
    const auto dot = [&](int wave, size_t tile, uint32_t *d) {
#pragma unroll 1
        for (int rp = 0; rp < PR_ROWS; rp += per_pass) {
            const int rt = wave * PR_ROWS + rp + rsub;   // row of the tile; rsub < per_pass <= PR_ROWS
            const size_t R = tile * PR_TILE + rt;
            uint32_t acc = 0;
            if (R < B && !absent(R)) {
#pragma unroll 1
                for (int bq = sub; bq < nb; bq += width) {
                    uint32_t x[16];
                    mktrng::stream_block(a.mkey, mktrng::STREAM_KSK_MASK, (uint32_t)a.party, (uint64_t)R, (uint32_t)bq, x);
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
    party_rows_tiles(dots, B, a.ksk_body, dot, [&](size_t R) -> uint32_t {
        if (absent(R)) return 0u;
        const size_t cj = R / per_cj;                                                               // c N + j: the ring keys lie end to end
        const uint32_t u = (uint32_t)(R - cj * per_cj), d = u / (uint32_t)a.f, tt = u - d * (uint32_t)a.f;
        const uint32_t z = (uint32_t)(int32_t)a.zring[(size_t)a.zoff * a.N + cj];
        const uint32_t msg = (uint32_t)(z * (d + 1u)) << (32 - (int)(tt + 1u) * a.logD);
        return mktrng::row_noise_word(a.key, (uint32_t)a.party, mktrng::STREAM_KSK_NOISE, (uint64_t)R, a.sigma_lwe) + msg;
    });
}

}  // namespace

hipError_t launch_keygen_seeded_brk(const KeygenSeededArgs &a, int unienc, hipStream_t s) {
    const int N = a.N;
    if (N < 32 || (N & (N - 1)) || N > 16 * KG_THREADS || a.n < 1 || a.l < 1 || (!unienc && a.kr < 1) || a.party < 0) return hipErrorInvalidValue;
    if (!a.brk_body || !a.lwekey || !a.zring || (unienc && !a.crs)) return hipErrorInvalidValue;
    const size_t lds = (size_t)N * 8 + (unienc ? (size_t)N : 0);
    const unsigned grid = unienc ? (unsigned)a.n : (unsigned)(a.n * (a.kr + 1) * a.l);
    if (unienc) MKT_KG_LAUNCH(keygen_seeded_unienc_kernel, a.W, N, grid, lds, s, a);
    else MKT_KG_LAUNCH(keygen_seeded_rgsw_kernel, a.W, N, grid, lds, s, a);
    return hipGetLastError();
}

hipError_t launch_keygen_seeded_ksk(KeygenSeededArgs a, hipStream_t s) {
    if (!a.ksk_rows) return hipSuccess;
    if (a.n < 1 || a.party < 0 || a.f < 1 || a.drows < 1 || a.absent_below < 0 || a.zoff < 0) return hipErrorInvalidValue;
    if (!a.ksk_body || !a.lwekey || !a.zring || a.ksk_rows % ((uint64_t)a.drows * a.f)) return hipErrorInvalidValue;
    const int nb = (a.n + 15) / 16;
    a.width = 4;                                   // the largest width that idles at most one lane-pass in eight (seeded.hip, encrypt)
    for (int w = 64; w > 4; w >>= 1)
        if (((nb + w - 1) / w * w - nb) * 8 <= nb) { a.width = w; break; }
    return launch_party_rows(keygen_seeded_ksk_kernel, a, (size_t)a.ksk_rows, (size_t)16 * nb, s);
}

}  // namespace mktd
