// Programmable bootstrap (include/mktfhe.h "programmable bootstrap", "many-table bootstrap"): the small kernels around the blind rotation, for gfx950.
//   lut_testvector_kernel  acc = (X^btilde * T, 0 ...) for a caller-supplied test-vector polynomial T (bootstrapping.jl:11-23 builds this for
//                          the constant -1/8 table only); for the many-table form btilde and the mask words go onto a coarser grid
//   lut_extract_kernel     the many-table form's extraction as a unit call (mkt_lut_extract_batch): the nout copies X^-v * acc, v < nout; no
//                          bootstrap runs it -- with the plain key switch it is the composition the many-table bootstrap is tested against
//   ks_at_table_kernel     every bootstrap with more than one output per input (many-table, coefficient list): which accumulator and which
//                          coefficient every output row of the key switch reads
//   lut_linear_kernel      the gather front end of a circuit level: a weighted sum of up to four pool rows plus a constant on the b word
// Neither does floating point.
#include "kernel_common.h"

namespace mktd {

// V ring words moved as one access: 16 bytes where the pointers admit it (V = 4 / 2 on the 32- / 64-bit ring), else one word
template <typename WORD, int V> struct alignas(sizeof(WORD) * V) LutPack { WORD v[V]; };

// One workgroup per ciphertext (grid-stride over the batch).  With r = btilde mod N and s = -1 for N <= btilde < 2N, else +1 (btilde = 2N is
// the identity):  acc.b[i] = s T[i - r] for i >= r,  -s T[N + i - r] for i < r.  The selected row is staged in LDS with contiguous wide loads;
// every lane then assembles V consecutive output words from it (the rotated read is contiguous with one wrap, so it is unaligned by
// r mod V: from LDS that costs nothing in HBM traffic) and stores them as one wide access.  sel NULL = row 0; a row beyond the table
// is clamped to its last row.
// Many-table form (nu = log2 of the table count, 0 = the plain form): every word goes onto the grid 2^nu times coarser,
// sw(w) = divbits(w, 32 - logN - 1 + nu) << nu, a multiple of 2^nu in [0, 2N].  btilde is the b word's; the lwe_stride - 1 switched mask
// words go to atilde (NULL: not wanted), which may be lin itself -- a word is read and written by one lane, the b word is never written --
// so neither carries __restrict__.
template <typename WORD, int V>
__global__ void __launch_bounds__(256) lut_testvector_kernel(const WORD *__restrict__ luts, uint32_t last_lut, const uint32_t *__restrict__ sel,
                                                             const uint32_t *lin, int lwe_stride, int logN, int kacc, int nu,
                                                             uint32_t *atilde, int at_stride, WORD *__restrict__ acc, size_t B) {
    using Pack = LutPack<WORD, V>;
    const int N = 1 << logN;
    const int bit = 32 - logN - 1 + nu;
    WORD *tl = reinterpret_cast<WORD *>(mkt_smem);
    for (size_t g = blockIdx.x; g < B; g += gridDim.x) {
        const uint32_t *ct = lin + g * lwe_stride;
        const uint32_t tb = divbits<uint32_t>(ct[lwe_stride - 1], bit) << nu;   // bootstrapping.jl:9, 0 .. 2N
        if (atilde) for (int i = threadIdx.x; i < lwe_stride - 1; i += blockDim.x) atilde[g * at_stride + i] = divbits<uint32_t>(ct[i], bit) << nu;
        uint32_t row = sel ? sel[g] : 0u;
        row = row < last_lut ? row : last_lut;
        const WORD *T = luts + (size_t)row * N;
        for (int i = threadIdx.x * V; i < N; i += blockDim.x * V) *reinterpret_cast<Pack *>(tl + i) = *reinterpret_cast<const Pack *>(T + i);
        __syncthreads();
        const int r = (int)(tb & (uint32_t)(N - 1));
        const bool neg = tb >= (uint32_t)N && tb < 2u * (uint32_t)N;
        WORD *a = acc + g * (size_t)(1 + kacc) * N;
        for (int i = threadIdx.x * V; i < N; i += blockDim.x * V) {
            Pack o;
#pragma unroll
            for (int e = 0; e < V; e++) {
                const int j = i + e;
                const WORD m = ((j >= r) != neg) ? (WORD)0 : (WORD)~(WORD)0;   // v -> (v ^ m) - m negates where m = ~0
                o.v[e] = (WORD)((tl[(j - r) & (N - 1)] ^ m) - m);
            }
            *reinterpret_cast<Pack *>(a + i) = o;
        }
        Pack z;
#pragma unroll
        for (int e = 0; e < V; e++) z.v[e] = 0;
        for (int i = threadIdx.x * V; i < kacc * N; i += blockDim.x * V) *reinterpret_cast<Pack *>(a + N + i) = z;
        __syncthreads();   // the next ciphertext of this workgroup restages the row
    }
}

// accs[g][v] = X^-v * acc[g] for v < nout: coefficient 0 of copy v is coefficient v of the rotated accumulator, which the key switch then
// extracts as it always does.  On each of the 1 + kacc polynomials  out[i] = in[i + v] for i + v < N, -in[i + v - N] for the last v words.
// One workgroup per ciphertext (grid-stride over the batch); a polynomial is read once, with contiguous wide loads into LDS, and its nout
// copies are assembled from there (the read is unaligned by v mod V) and stored as wide accesses: the (copy, word group) pairs are dealt over
// the lanes.  An HBM stream: 1 read, nout writes.
template <typename WORD, int V>
__global__ void __launch_bounds__(256) lut_extract_kernel(const WORD *__restrict__ acc, int nout, int logN, int kacc, WORD *__restrict__ accs, size_t B) {
    using Pack = LutPack<WORD, V>;
    const int N = 1 << logN, npoly = 1 + kacc, groups = N / V;
    WORD *tl = reinterpret_cast<WORD *>(mkt_smem);
    for (size_t g = blockIdx.x; g < B; g += gridDim.x) {
        for (int c = 0; c < npoly; c++) {
            const WORD *src = acc + (g * npoly + c) * (size_t)N;
            for (int i = threadIdx.x * V; i < N; i += blockDim.x * V) *reinterpret_cast<Pack *>(tl + i) = *reinterpret_cast<const Pack *>(src + i);
            __syncthreads();
            for (int t = threadIdx.x; t < nout * groups; t += blockDim.x) {
                const int v = t / groups, i = (t - v * groups) * V;
                Pack o;
#pragma unroll
                for (int e = 0; e < V; e++) {
                    const int j = i + e + v;
                    const WORD m = j < N ? (WORD)0 : (WORD)~(WORD)0;   // as in lut_testvector_kernel: negates where m = ~0
                    o.v[e] = (WORD)((tl[j & (N - 1)] ^ m) - m);
                }
                *reinterpret_cast<Pack *>(accs + (((g * nout + v) * npoly) + c) * (size_t)N + i) = o;
            }
            __syncthreads();   // the next polynomial restages
        }
    }
}

// The rows of a key switch at a coefficient (device_api.h KsArgs::src / ::coef) for ncoef outputs per rotated accumulator: output row
// g = j * ncoef + i reads accumulator j at coef[i].  The list is the caller's, as it is (the key switch reads it mod N); coef NULL = the list
// 0 .. ncoef - 1, the many-table bootstrap's
__global__ void __launch_bounds__(256) ks_at_table_kernel(const uint32_t *__restrict__ coef, uint32_t ncoef, uint32_t *__restrict__ src, uint32_t *__restrict__ coef_rows, size_t rows) {
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < rows; g += (size_t)gridDim.x * blockDim.x) {
        const size_t j = g / ncoef;
        src[g] = (uint32_t)j;
        const size_t i = g - j * ncoef;
        coef_rows[g] = coef ? coef[i] : (uint32_t)i;
    }
}

// lin[g] = cst[g] e_b + sum_{t < 4} wt[g][t] pool[idx[g][t]]: one workgroup per gate (grid-stride over gates), shaped as gate3_linear_kernel --
// the four row indices, weights and the constant are the same for the whole workgroup, the rows are streamed coalesced.  A weight of 0
// skips its term (its row is not read); rows are clamped into the pool as everywhere (kernels.hip gate_linear_kernel).
__global__ void __launch_bounds__(256) lut_linear_kernel(const uint32_t *__restrict__ pool, size_t pool_rows, const uint32_t *__restrict__ idx,
                                                         const int8_t *__restrict__ wt, const uint32_t *__restrict__ cst, uint32_t *__restrict__ out,
                                                         int len, size_t B) {
    const size_t last = pool_rows - 1;
    for (size_t g = blockIdx.x; g < B; g += gridDim.x) {
        const uint32_t *row[4];
        uint32_t w[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const size_t r = idx[g * 4 + t];
            row[t] = pool + (r < pool_rows ? r : last) * len;
            w[t] = (uint32_t)(int32_t)wt[g * 4 + t];
        }
        const uint32_t k = cst[g];
        uint32_t *po = out + g * len;
        for (int c = threadIdx.x; c < len; c += blockDim.x) {
            uint32_t s = c == len - 1 ? k : 0u;
#pragma unroll
            for (int t = 0; t < 4; t++) if (w[t]) s += w[t] * row[t][c];
            po[c] = s;
        }
    }
}

template <typename WORD>
static hipError_t launch_lut_tv(const void *luts, size_t nluts, const uint32_t *sel, const uint32_t *lin, int lwe_stride, int logN, int kacc, int nu, uint32_t *atilde, int at_stride,
                                void *acc, size_t B, hipStream_t s) {
    constexpr int V = 16 / (int)sizeof(WORD);
    const int N = 1 << logN;
    const uint32_t last = (uint32_t)(nluts - 1 < 0xffffffffull ? nluts - 1 : 0xffffffffull);
    const unsigned grid = (unsigned)(B < 65536 ? B : 65536);
    const size_t lds = (size_t)N * sizeof(WORD);
    // 16-byte accesses need 16-byte rows: the engine's own buffers always are, a caller's device pointer may not be
    const bool wide = N >= V && ((reinterpret_cast<uintptr_t>(luts) | reinterpret_cast<uintptr_t>(acc)) & 15u) == 0;
    const int threads = N / (wide ? V : 1) >= 256 ? 256 : 64;
    if (wide) hipLaunchKernelGGL((lut_testvector_kernel<WORD, V>), dim3(grid), dim3(threads), lds, s, (const WORD *)luts, last, sel, lin, lwe_stride, logN, kacc, nu, atilde, at_stride, (WORD *)acc, B);
    else hipLaunchKernelGGL((lut_testvector_kernel<WORD, 1>), dim3(grid), dim3(threads), lds, s, (const WORD *)luts, last, sel, lin, lwe_stride, logN, kacc, nu, atilde, at_stride, (WORD *)acc, B);
    return hipGetLastError();
}

hipError_t launch_lut_many_testvector(int W, const void *luts, size_t nluts, const uint32_t *sel, const uint32_t *lin, int lwe_stride, int logN, int kacc, int nu,
                                      uint32_t *atilde, int at_stride, void *acc, size_t B, hipStream_t s) {
    if (!B) return hipSuccess;
    if (!nluts || logN < 0 || logN > 12) return hipErrorInvalidValue;   // (a row to clamp to; the staged row fits LDS: 4096 words of 8 bytes)
    if (nu < 0 || nu > 3 || nu > logN || lwe_stride < 1 || (atilde && at_stride < lwe_stride - 1)) return hipErrorInvalidValue;
    return W == 64 ? launch_lut_tv<uint64_t>(luts, nluts, sel, lin, lwe_stride, logN, kacc, nu, atilde, at_stride, acc, B, s)
                   : launch_lut_tv<uint32_t>(luts, nluts, sel, lin, lwe_stride, logN, kacc, nu, atilde, at_stride, acc, B, s);
}

hipError_t launch_lut_testvector(int W, const void *luts, size_t nluts, const uint32_t *sel, const uint32_t *lin, int lwe_stride, int logN, int kacc, void *acc, size_t B, hipStream_t s) {
    return launch_lut_many_testvector(W, luts, nluts, sel, lin, lwe_stride, logN, kacc, 0, nullptr, 0, acc, B, s);
}

template <typename WORD>
static hipError_t launch_lut_ex(const void *acc, int nout, int logN, int kacc, void *accs, size_t B, hipStream_t s) {
    constexpr int V = 16 / (int)sizeof(WORD);
    const int N = 1 << logN;
    const unsigned grid = (unsigned)(B < 65536 ? B : 65536);
    const size_t lds = (size_t)N * sizeof(WORD);
    const bool wide = N >= V && ((reinterpret_cast<uintptr_t>(acc) | reinterpret_cast<uintptr_t>(accs)) & 15u) == 0;   // as launch_lut_tv
    const int threads = nout * (N / (wide ? V : 1)) >= 256 ? 256 : 64;
    if (wide) hipLaunchKernelGGL((lut_extract_kernel<WORD, V>), dim3(grid), dim3(threads), lds, s, (const WORD *)acc, nout, logN, kacc, (WORD *)accs, B);
    else hipLaunchKernelGGL((lut_extract_kernel<WORD, 1>), dim3(grid), dim3(threads), lds, s, (const WORD *)acc, nout, logN, kacc, (WORD *)accs, B);
    return hipGetLastError();
}

hipError_t launch_lut_extract(int W, const void *acc, int nout, int logN, int kacc, void *accs, size_t B, hipStream_t s) {
    if (!B) return hipSuccess;
    if (logN < 0 || logN > 12 || kacc < 0 || (nout != 1 && nout != 2 && nout != 4 && nout != 8) || nout > (1 << logN)) return hipErrorInvalidValue;
    return W == 64 ? launch_lut_ex<uint64_t>(acc, nout, logN, kacc, accs, B, s) : launch_lut_ex<uint32_t>(acc, nout, logN, kacc, accs, B, s);
}

hipError_t launch_ks_at_table(const uint32_t *coef, size_t ncoef, uint32_t *src, uint32_t *coef_rows, size_t rows, hipStream_t s) {
    if (!rows) return hipSuccess;
    if (!ncoef || ncoef > 0xffffffffull || rows / ncoef > 0xffffffffull) return hipErrorInvalidValue;
    const size_t blocks = (rows + 255) / 256;
    hipLaunchKernelGGL(ks_at_table_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, coef, (uint32_t)ncoef, src, coef_rows, rows);
    return hipGetLastError();
}

hipError_t launch_lut_linear(const uint32_t *pool, size_t pool_rows, const uint32_t *idx, const int8_t *wt, const uint32_t *cst, uint32_t *out, int len, size_t B, hipStream_t s) {
    if (!B || len <= 0) return hipSuccess;
    if (!pool_rows) return hipErrorInvalidValue;
    const int threads = len >= 256 ? 256 : ((len + 63) / 64) * 64;   // as launch_gate3_linear
    const unsigned grid = (unsigned)(B < 65536 ? B : 65536);
    hipLaunchKernelGGL(lut_linear_kernel, dim3(grid), dim3(threads), 0, s, pool, pool_rows, idx, wt, cst, out, len, B);
    return hipGetLastError();
}

}  // namespace mktd
