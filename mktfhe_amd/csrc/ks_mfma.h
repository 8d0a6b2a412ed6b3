// Key switch on the matrix cores (ks_mfma.hip): the second resident form of a key-switching key and its tile loop (the admission bound:
// host_internal.h ks_mfma_fits).
//
// The key switch of the unbalanced D = 4 sets is out[g][q] = sum over (c, j, t) of row[c][j][digit(g, c, j, t)][t][q] mod 2^32, digit 0
// adding nothing (kernels.hip).  As a matrix product: A[g][k] one-hot over the digit value, B[k][column] the key rows.  An int8 MFMA
// with 32-bit accumulators sums exactly, so the key words are split into four SIGNED bytes s_b, w = sum_b s_b 256^b mod 2^32, one byte
// plane each, and out = sum_b S_b << 8b of the four plane sums S_b.
//
// K order: k = 4 (j f + t) + d, d = 0..3 -- four rows per digit, row 0 all zero, so that a lane's share of A for one digit is the
// one word 1 << 8 d.  (Three rows per digit would save the quarter of the products that meets the zero row and cost a byte-granular
// one-hot over register boundaries; the A build already takes half the vector issue slots beside the MFMAs.)
// One K-step is one v_mfma_i32_32x32x32_i8: 32 k = 8 digits, lane (r = lane & 31, h = lane >> 5) holding k = 16 h + e, e = 0..15, of
// gate r (A) or column r (B).  The planes are stored in exactly that order,
//     [block (party or component)][step][column tile of 32 words][plane 0..3][lane 0..63][16 bytes],
// so a wave's four B operands of a step are 4 KiB contiguous and every lane reads 16 bytes of them with one load.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <type_traits>

#ifndef __HIPCC__
#define KSM_HD inline
#else
#include <hip/hip_runtime.h>
#define KSM_HD __host__ __device__ inline
#endif

namespace mktd {

constexpr int KSM_STEP_DIGITS = 8;      // digits per K-step (32 k)
constexpr int KSM_TILE_WORDS = 32;      // key words per column tile (x 4 planes = 128 byte columns)
constexpr int KSM_BLOCK_BYTES = 4096;   // one (step, column tile): 4 planes x 64 lanes x 16 bytes
constexpr int KSM_WAVE_GATES = 128;     // four 32-row tiles per wave
constexpr int KSM_WAVES = 4;            // per workgroup: 512 gates

KSM_HD int ksm_steps(int N, int f) { return (N * f + KSM_STEP_DIGITS - 1) / KSM_STEP_DIGITS; }
KSM_HD int ksm_coltiles(int n1p) { return (n1p + KSM_TILE_WORDS - 1) / KSM_TILE_WORDS; }
// bytes of one block's planes (one party's key, or one component's rows of a single-key scheme)
KSM_HD size_t ksm_block_bytes(int N, int f, int n1p) { return (size_t)ksm_steps(N, f) * ksm_coltiles(n1p) * KSM_BLOCK_BYTES; }

// signed byte b of w: w = sum_b ksm_byte(w, b) * 256^b mod 2^32
KSM_HD int ksm_byte(uint32_t w, int b) {
    for (int i = 0; i < b; i++) w = (w - (uint32_t)(int32_t)(int8_t)(w & 0xFF)) >> 8;
    return (int8_t)(w & 0xFF);
}

// Byte `off` of the planes of one block, from its rows [N][drows][f][n1p] in the resident pitch
KSM_HD int8_t ksm_plane_byte(const uint32_t *rows, int N, int f, int drows, int n1p, size_t off) {
    const int coltiles = ksm_coltiles(n1p);
    const size_t blk = off / KSM_BLOCK_BYTES;
    const int o = (int)(off % KSM_BLOCK_BYTES);
    const int step = (int)(blk / coltiles), tile = (int)(blk % coltiles);
    const int plane = o >> 10, lane = (o >> 4) & 63, e = o & 15;
    const int q = tile * KSM_TILE_WORDS + (lane & 31), d = e & 3;
    const long s = (long)step * KSM_STEP_DIGITS + 4 * (lane >> 5) + (e >> 2);
    if (d == 0 || d > drows || s >= (long)N * f || q >= n1p) return 0;
    const int j = (int)(s / f), t = (int)(s % f);
    return (int8_t)ksm_byte(rows[(((size_t)j * drows + (d - 1)) * f + t) * n1p + q], plane);
}

struct KsmArgs {
    const int8_t *planes;       // block 0
    size_t block_stride;        // bytes from one block to the next
    const uint32_t *digits;     // [kacc][ngroups][N][32] prepared digit words (ks_digits_kernel)
    uint32_t *partial;          // [slab][party][B][n1p]
    int B, ngroups, N, f, n1p, kacc, mk, slabs;
};

#ifdef __HIPCC__
typedef int ksm_v4 __attribute__((ext_vector_type(4)));
typedef int ksm_v16 __attribute__((ext_vector_type(16)));

// The digits of one step for lane half h: F = 8 -- the step is coefficient `step`, its prepared word holds the half's four digits in byte
// 1 - h; F = 0 -- any digit count, a division per digit, the four digits gathered into byte 0 (first digit in the top two bits).
template <int F>
__device__ __forceinline__ uint32_t ksm_digit_word(const uint32_t *dg, int step, int h, int N, int f) {
    if constexpr (F == 8) return dg[(size_t)step * 32];
    else {
        uint32_t b8 = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int s = step * KSM_STEP_DIGITS + 4 * h + i;
            uint32_t d = 0;
            if (s < N * f) { const int j = s / f, t = s - j * f; d = (dg[(size_t)j * 32] >> (2 * (f - 1 - t))) & 3u; }
            b8 = (b8 << 2) | d;
        }
        return b8;
    }
}
// ... and the A operand they make: digit d -> the word 1 << 8 d (k = 4 digit + d); sh: the bit of `w` where the half's byte begins
__device__ __forceinline__ ksm_v4 ksm_a_operand(uint32_t w, int sh) {
    ksm_v4 v;
#pragma unroll
    for (int i = 0; i < 4; i++) v[i] = (int)(1u << (((w >> (sh + 6 - 2 * i)) & 3u) << 3));
    return v;
}

// The tile of one wave: 128 gates x 32 key words (4 planes) x the steps [s0, s1) of components [c_begin, c_end).  sum[m][p]: gate tile m,
// plane p, in the C/D layout of the 32x32 MFMA (column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)).
// One wave per SIMD, no LDS, no barrier: the loop is pipelined by hand over a ring of KSM_RING register sets.  While the sixteen MFMAs
// of a step run, the B operands of the next KSM_RING - 1 steps and the digit words of the next KSM_RING are in flight and the A operands
// of the next step are built on the vector unit.  The four waves of a workgroup read the same key bytes, so a compute unit has only
// 4 KiB of key in flight per step of look-ahead: with one step the kernel streamed the planes at 1.25 TB/s whatever the batch
// (profiles/ks_mfma_probe.txt, first record).  The loop is written KSM_RING steps at a time so that no loaded value is ever copied
// from one register set to the next -- a copy waits for its load.
constexpr int KSM_RING = 6;   // even: the A operands alternate between two sets
template <int F>
__device__ __forceinline__ void ksm_tile_loop(const KsmArgs &a, ksm_v16 (&sum)[4][4], int grp0, int tile, int c_begin, int c_end, int s0, int s1) {
    constexpr int R = KSM_RING;
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int f = F ? F : a.f, sh = F == 8 ? 8 * (1 - h) : 0;
    const size_t step_bytes = (size_t)ksm_coltiles(a.n1p) * KSM_BLOCK_BYTES;
    if (s0 >= s1) return;
    for (int c = c_begin; c < c_end; c++) {
        const int8_t *pl = a.planes + (size_t)c * a.block_stride + (size_t)tile * KSM_BLOCK_BYTES + (size_t)lane * 16;
        const uint32_t *dg[4];
#pragma unroll
        for (int m = 0; m < 4; m++) {
            const int grp = grp0 + m < a.ngroups ? grp0 + m : a.ngroups - 1;
            dg[m] = a.digits + ((size_t)c * a.ngroups + grp) * a.N * 32 + r;
        }
        const int last = s1 - 1;
        auto clamp = [=](int s) { return s < last ? s : last; };   // past the slab: the last step again, loaded and not counted
        ksm_v4 bv[R][4], av[2][4];
        uint32_t w[R][4];
        // the first loads, in the order the steps below issue theirs (the words of step k + 1 behind the B operands of step k): the
        // compiler takes the waits of a round from both ways into it, and an order of its own here costs every round a full wait
        uint32_t w0[4];
#pragma unroll
        for (int m = 0; m < 4; m++) w0[m] = ksm_digit_word<F>(dg[m], s0, h, a.N, f);
#pragma unroll
        for (int k = 0; k < R - 1; k++) {
            asm volatile("" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int p = 0; p < 4; p++) bv[k][p] = *reinterpret_cast<const ksm_v4 *>(pl + (size_t)clamp(s0 + k) * step_bytes + p * 1024);
#pragma unroll
            for (int m = 0; m < 4; m++) w[k + 1][m] = ksm_digit_word<F>(dg[m], clamp(s0 + k + 1), h, a.N, f);
        }
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int m = 0; m < 4; m++) av[0][m] = ksm_a_operand(w0[m], sh);
        // step `step` on ring slot I: B of slot I, A of set I & 1; loads B of step + R - 1 into the slot of the step before and the digit
        // words of step + R into slot I (its own were made into A operands a step ago); builds the A operands of step + 1
        auto one_step = [&](auto slot, int step) {
            constexpr int I = decltype(slot)::value, PREV = (I + R - 1) % R, NEXT = (I + 1) % R;
            const int nb = clamp(step + R - 1), nw = clamp(step + R);
#pragma unroll
            for (int p = 0; p < 4; p++) bv[PREV][p] = *reinterpret_cast<const ksm_v4 *>(pl + (size_t)nb * step_bytes + p * 1024);
#pragma unroll
            for (int m = 0; m < 4; m++) w[I][m] = ksm_digit_word<F>(dg[m], nw, h, a.N, f);
            // The loads are issued HERE, ahead of the step's MFMAs.  Left alone the compiler sinks each to its first use (the top of
            // the step that needs it) or schedules them behind the sixteen MFMAs.  The fence keeps them in this step, the scheduling
            // barrier ahead of what follows
            asm volatile("" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            const uint32_t live = step + 1 <= last ? ~0u : 0u;
#pragma unroll
            for (int m = 0; m < 4; m++) av[(I + 1) & 1][m] = ksm_a_operand(w[NEXT][m] & live, sh);
#pragma unroll
            for (int m = 0; m < 4; m++)
#pragma unroll
                for (int p = 0; p < 4; p++) sum[m][p] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av[I & 1][m], bv[I][p], sum[m][p], 0, 0, 0);
            // ... and the next step's A operands are built in this step, between its MFMAs (the compiler would sink them to the next step too)
#pragma unroll
            for (int m = 0; m < 4; m++) asm volatile("" : "+v"(av[(I + 1) & 1][m]));
        };
        // whole rounds of the ring, no exit inside a round (every exit edge makes the compiler wait for all loads in flight at the
        // top of the round): a step past the slab runs with digit words of zero, which select the planes' all-zero row 0
        for (int step = s0; step < s1; step += R) {
            one_step(std::integral_constant<int, 0>{}, step);
            one_step(std::integral_constant<int, 1>{}, step + 1);
            one_step(std::integral_constant<int, 2>{}, step + 2);
            one_step(std::integral_constant<int, 3>{}, step + 3);
            one_step(std::integral_constant<int, 4>{}, step + 4);
            one_step(std::integral_constant<int, 5>{}, step + 5);
        }
        static_assert(R == 6, "the loop above names every ring slot");
    }
}

// One workgroup: 4 waves x 128 gates, one column tile (grid.z), one slab of the steps, the party's block (grid.y) or every component.
// Each wave stores its sums as words, out = sum_b S_b << 8b, into the partial rows [slab][party][B][n1p] that ks_reduce_kernel adds.
template <int F>
__device__ __forceinline__ void ksm_workgroup(const KsmArgs &a) {
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int gtiles = (a.B + KSM_WAVE_GATES * KSM_WAVES - 1) / (KSM_WAVE_GATES * KSM_WAVES);
    const int gt = (int)(blockIdx.x % (unsigned)gtiles), slab = (int)(blockIdx.x / (unsigned)gtiles);
    const int g0 = (gt * KSM_WAVES + wv) * KSM_WAVE_GATES;
    if (g0 >= a.B) return;
    const int tile = blockIdx.z;
    const int c_begin = a.mk ? (int)blockIdx.y : 0, c_end = a.mk ? c_begin + 1 : a.kacc, blk = a.mk ? c_begin : 0;
    const int nsteps = ksm_steps(a.N, F ? F : a.f), per = (nsteps + a.slabs - 1) / a.slabs;
    const int s0 = slab * per, s1 = s0 + per < nsteps ? s0 + per : nsteps;
    ksm_v16 sum[4][4];
#pragma unroll
    for (int m = 0; m < 4; m++)
#pragma unroll
        for (int p = 0; p < 4; p++)
#pragma unroll
            for (int i = 0; i < 16; i++) sum[m][p][i] = 0;
    ksm_tile_loop<F>(a, sum, g0 / 32, tile, c_begin, c_end, s0, s1);
    const int q = tile * KSM_TILE_WORDS + r;
    if (q >= a.n1p) return;
    uint32_t *dst = a.partial + ((size_t)slab * gridDim.y + blk) * a.B * a.n1p + q;
#pragma unroll
    for (int m = 0; m < 4; m++)
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int g = g0 + 32 * m + (i & 3) + 8 * (i >> 2) + 4 * h;
            if (g < a.B) dst[(size_t)g * a.n1p] = (uint32_t)sum[m][0][i] + ((uint32_t)sum[m][1][i] << 8) + ((uint32_t)sum[m][2][i] << 16) + ((uint32_t)sum[m][3][i] << 24);
        }
}
#endif  // __HIPCC__

}  // namespace mktd
