// The seeded packing key on the device (include/mktfhe_pack.h "SEEDED"), for gfx950: the evaluator's expansion of (mask seed, bodies) into an
// ordinary packing key, and the party's generation of the bodies on its own GPU.  The definitions are mkt_client_packing_key_expand and
// mkt_client_packing_keygen_seeded (client.cpp); both sides run one ChaCha20 block function and wrapping integer arithmetic, the one Float64
// step is the shared box_muller with contraction off.  No inline assembly, no global atomics, plain vector stores, no scratch.
//
// EXPANSION.  A packing key is n l_pk groups of 1 + kr polynomials (b, a_0 ..): the shape of an RGSW bootstrapping key with one row per sample.
// So it runs on seeded_brk_expand_kernel (seeded_keys.hip) itself -- one ChaCha20 block per lane, a 256-unit tile through LDS at pitch 17,
// 16-byte stores covering 1 KiB per wave, double-buffered, at most PR_MAX_GRID workgroups and grid-stride beyond -- with the three things that
// differ passed as arguments: the stream (19), the high word of the stream index (the gadget, pack_mask_index of rng_chacha.h) and, for the
// resident layout of an MKT_ARITH_EXACT context, the [polynomial][row] destination.  Body polynomials are copied and do no cipher work.
//
// GENERATION.  One workgroup of KG_THREADS lanes per row S = q l_pk + t, the two steps of keygen_common.h like keygen_seeded_rgsw_kernel at
// c = 0: accumulate_masks with mask polynomial P = S kr + c of stream 19 for c < kr, then noise_and_store with the N noise words of stream 20
// at index (q, t) and the message s[q] g_t at coefficient 0.  Only the body is stored.
#include "device_api.h"
#include "keygen_common.h"
#include "kernel_common.h"

namespace mktd {
namespace {

template <typename WORD, int MAXR>
__global__ __launch_bounds__(KG_THREADS) void pack_keygen_kernel(PackKeygenArgs a) {
    uint64_t *al = reinterpret_cast<uint64_t *>(mkt_smem);          // [N] a mask polynomial, then the noise
    const int N = a.N;
    const uint32_t S = blockIdx.x, q = S / (uint32_t)a.l, tt = S - q * (uint32_t)a.l;
    WORD *out = reinterpret_cast<WORD *>(a.body) + (size_t)S * N;
    uint64_t acc[MAXR] = {};
    accumulate_masks<MAXR>(al, a.zring, a.kr, N, acc, [&](int c) {
        fill_mask_poly<WORD>(a.mkey, mktrng::STREAM_PACK_MASK, (uint32_t)a.party, mktrng::pack_mask_index(S * (uint32_t)a.kr + (uint32_t)c, a.l, a.logB), al, N);
    });
    const Rng rng(a.key, (uint32_t)a.party, mktrng::STREAM_PACK_NOISE, q, tt);
    const uint64_t g = (uint64_t)a.lwekey[q] << (a.W - (int)(tt + 1u) * a.logB);
    noise_and_store<WORD>(out, al, acc, N, rng, 0, a.sigma_ring, [&](int m) { return m == 0 ? g : (uint64_t)0; });
}

}  // namespace

hipError_t launch_pack_key_expand(const PackKeyExpandArgs &a, hipStream_t s) {
    if (a.kr < 1 || a.l < 1 || a.logB < 1 || a.logB > 16) return hipErrorInvalidValue;
    SeededBrkArgs b{};
    for (int i = 0; i < 8; i++) b.mkey[i] = a.mkey[i];
    b.stream = mktrng::STREAM_PACK_MASK;
    b.idx_hi = (uint32_t)(mktrng::pack_mask_index(0u, a.l, a.logB) >> 32);
    b.t_rows = a.transposed ? a.rows : 0;
    b.party = a.party; b.unienc = 0; b.kr = a.kr; b.l = a.l; b.log_units = a.log_units;
    b.body = a.body; b.out = a.out; b.npolys = a.rows * ((uint64_t)a.kr + 1);
    return launch_seeded_brk_expand(b, s);
}

hipError_t launch_pack_keygen(const PackKeygenArgs &a, hipStream_t s) {
    const int N = a.N;
    if (N < 32 || (N & (N - 1)) || N > 16 * KG_THREADS || a.n < 1 || a.l < 1 || a.kr < 1 || a.party < 0) return hipErrorInvalidValue;
    if (a.logB < 1 || a.l * a.logB > 32 || (a.W != 32 && a.W != 64) || !a.body || !a.lwekey || !a.zring) return hipErrorInvalidValue;
    const size_t lds = (size_t)N * 8;
    const unsigned grid = (unsigned)(a.n * a.l);
    MKT_KG_LAUNCH(pack_keygen_kernel, a.W, N, grid, lds, s, a);
    return hipGetLastError();
}

}  // namespace mktd
