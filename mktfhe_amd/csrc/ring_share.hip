// A party's ring shares of packed ciphertexts on the device (include/mktfhe_ring_share.h), for gfx950:
//     out[g] = sum_{c < kr} a_slot(party, c)[g] (*) z_c + e[g]   (mod 2^W),   e[g][j] = draw j of stream 18 at pack row0 + g, lifted by W - 32 bits
// -- the words of mkt_client_rlwe_partial_decrypt (client.cpp: ring_share_acc, then the stream-18 loop) for the same seed.  The product is
// wrapping integer arithmetic, whose order is free; the noise is the shared box_muller with contraction off, reached by random access
// (fill_noise of keygen_common.h).  No inline assembly, no global atomics, plain vector stores, no scratch.
//
// SHAPE.  pack_keygen_kernel (pack_keys.hip) gives a whole polynomial to one workgroup, which is right for thousands of rows; a party opens
// 1 .. 16 packs as often as thousands, and one workgroup per pack would leave 255 compute units idle.  So a pack is dealt over `slices`
// workgroups by slices of L = N / slices OUTPUT coefficients, L a power of two in 16 .. 256 (ring_share_slices: the fewer packs, the narrower
// the slice, until about RS_FILL workgroups exist).  A workgroup of RS_THREADS = 256 lanes stages the whole mask polynomial a_c (N ring words,
// widened to 64 bits: 32 KiB at N = 4096) and the key polynomial z_c (N bytes) in LDS and computes its L coefficients of the negacyclic
// product: lane t holds ONE coefficient m = m0 + (t mod L) and walks the key entries i = t / L, t / L + P, ... (P = 256 / L parts), so
// neighbouring lanes read neighbouring LDS words and a wave's lanes of one part share the key byte.  The P partial sums of a coefficient meet
// in LDS.  A slice starts at a multiple of 16 coefficients, hence on a keystream block (4 deviates a block), and draws its own L noise words
// into the staging area once the product has left it.  Staging costs N / 256 loads per lane and polynomial against N / P product steps.
// The caller's buffers carry the alignment of a ring word and no more (mktfhe.h ALIGNMENT), so they are read and written a word per lane,
// coalesced.  At most RS_MAX_GRID workgroups per launch, grid-stride over (pack, slice) beyond.
#include "device_api.h"
#include "keygen_common.h"
#include "kernel_common.h"

namespace mktd {
namespace {

constexpr int RS_THREADS = KG_THREADS;              // lanes of a workgroup (fill_noise strides by KG_THREADS)
constexpr int RS_MIN_SLICE = 16;                    // fewest output coefficients of a workgroup: 16 parts of N / 16 product steps each
constexpr unsigned RS_FILL = 512;                   // workgroups wanted before slices stop narrowing: two per compute unit
constexpr unsigned RS_MAX_GRID = 2048;              // workgroups of one launch, more (pack, slice) pairs than that: grid-stride

template <typename WORD>
__global__ __launch_bounds__(RS_THREADS) void ring_share_kernel(RingShareArgs a) {
    uint64_t *al = reinterpret_cast<uint64_t *>(mkt_smem);          // [N] a mask polynomial, then the slice's L noise words
    int8_t *zl = reinterpret_cast<int8_t *>(al + a.N);              // [N] a key polynomial
    uint64_t *red = reinterpret_cast<uint64_t *>(zl + a.N);         // [RS_THREADS] partial sums (N is a multiple of 32: 8-byte aligned)
    const int N = a.N, t = threadIdx.x;
    const int L = N / a.slices, P = RS_THREADS / L;                 // 16 <= L <= 256: one coefficient per lane, P lanes per coefficient
    const int col = t & (L - 1), part = t / L;
    const uint64_t wm = wmask_of<WORD>();
    const uint64_t total = (uint64_t)a.G * (uint64_t)a.slices;
    for (uint64_t w = blockIdx.x; w < total; w += gridDim.x) {
        const uint64_t g = w / (uint64_t)a.slices;
        const int m0 = (int)(w - g * (uint64_t)a.slices) * L, m = m0 + col;
        const WORD *ct = reinterpret_cast<const WORD *>(a.rlwe) + g * (uint64_t)a.npoly * N;
        uint64_t acc = 0;
        for (int c = 0; c < a.kr; c++) {
            const WORD *ap = ct + (size_t)(a.poly0 + c * a.poly_step) * N;
            const int8_t *zp = a.zring + (size_t)c * N;
            __syncthreads();                                        // the staging area is free: the last product, or the last slice's noise, is read
            for (int q = t; q < N; q += RS_THREADS) { al[q] = (uint64_t)ap[q]; zl[q] = zp[q]; }
            __syncthreads();
            for (int i = part; i < N; i += P) {
                const int si = zl[i];                               // wave-uniform from L = 64 up
                if (!si) continue;
                acc += negacyclic_term(al, N, m, i, si, false);
            }
        }
        __syncthreads();
        const Rng rng(a.key, (uint32_t)a.party, mktrng::STREAM_PACK_SMUDGE, (uint32_t)(a.row0 + g), (uint32_t)((a.row0 + g) >> 32));
        fill_noise(rng, 2 * (uint64_t)m0, al, L, a.sigma);          // coefficient j reads draws 2 j, 2 j + 1: m0 a multiple of 4 starts a keystream block
        red[t] = acc;
        __syncthreads();
        if (part == 0) {
            uint64_t sum = 0;
            for (int r = 0; r < P; r++) sum += red[r * L + col];
            reinterpret_cast<WORD *>(a.out)[g * (uint64_t)N + m] = (WORD)((sum + (al[col] << (a.W - 32))) & wm);
        }
    }
}

}  // namespace

int ring_share_slices(int N, size_t G) {
    const int lo = N / RS_THREADS > 0 ? N / RS_THREADS : 1, hi = N / RS_MIN_SLICE;
    int s = lo;
    while (s < hi && (uint64_t)G * (uint64_t)s < RS_FILL) s *= 2;
    return s;
}

hipError_t launch_ring_share(RingShareArgs a, hipStream_t s) {
    if (!a.G) return hipSuccess;
    const int N = a.N;
    if (N < 32 || (N & (N - 1)) || N > 16 * RS_THREADS || (a.W != 32 && a.W != 64) || a.kr < 1 || a.party < 0 || !a.rlwe || !a.zring || !a.out) return hipErrorInvalidValue;
    if (a.poly0 < 1 || a.poly_step < 0 || a.poly0 + (a.kr - 1) * a.poly_step >= a.npoly) return hipErrorInvalidValue;   // every polynomial read lies inside a ciphertext
    a.slices = ring_share_slices(N, a.G);
    const uint64_t total = (uint64_t)a.G * (uint64_t)a.slices;
    const unsigned grid = (unsigned)(total < RS_MAX_GRID ? total : RS_MAX_GRID);
    const size_t lds = (size_t)N * 9 + (size_t)RS_THREADS * 8;
    if (a.W == 64) hipLaunchKernelGGL(ring_share_kernel<uint64_t>, dim3(grid), dim3(RS_THREADS), lds, s, a);
    else hipLaunchKernelGGL(ring_share_kernel<uint32_t>, dim3(grid), dim3(RS_THREADS), lds, s, a);
    return hipGetLastError();
}

}  // namespace mktd
