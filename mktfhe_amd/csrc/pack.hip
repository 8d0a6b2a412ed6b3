// Packed outputs (mktfhe_pack.h): N LWE rows folded into one RLWE ciphertext by the packing key switch.  Three kernels per call:
//   1. pack_columns_kernel   the picked rows, lifted to ring words, transposed into columns cols[pack][column][N] (column i n + q = the mask
//                            word q of party i over the pack's rows, column nparty n = the body words), through LDS tiles
//   2. pack_product_kernel   one workgroup per (pack, party, chunk of PACK_QCHUNK mask words): for each q the gadget product of column
//                            (i, q) with key rows (q, 0 .. l-1), formed as bootstrapping.jl:62-72 forms one, added in integers to 1 + kr
//                            register accumulators; one slab store per workgroup
//   3. pack_reduce_kernel    the integer sum of the slabs and of the body column into the ciphertext (the pattern of ks_reduce_kernel)
// No global atomics, no kernel-selection switch.  MKT_ARITH_EXACT runs 1 and, per chunk of columns, mkt_decompose_batch's kernel, the exact
// product kernel behind mkt_exact_polymul_batch and pack_accumulate_kernel (context.cpp).
#include "kernel_common.h"

#pragma clang fp contract(off)

namespace mktd {

// ---- 1. rows -> lifted columns ----
// A tile is PACK_TILE rows x PACK_TILE columns of 32-bit words.  Rows of k n + 1 words are only 4-byte aligned (the length is odd), so a row
// is read one dword per lane, 256 contiguous bytes per wave; a column is written one ring word per lane, contiguous.  The LDS tile is padded
// by one word per row: both the row-wise write and the column-wise read are conflict-free.
constexpr int PACK_TILE = 64;
template <typename WORD>
__global__ __launch_bounds__(256) void pack_columns_kernel(PackArgs a) {
    __shared__ uint32_t tile[PACK_TILE][PACK_TILE + 1];
    constexpr int SH = WordTraits<WORD>::W - 32;
    const int N = 1 << a.logN, len = a.lwe_len;
    const int tx = threadIdx.x & (PACK_TILE - 1), ty = threadIdx.x / PACK_TILE;      // 64 x 4
    const int j0 = blockIdx.x * PACK_TILE, c0 = blockIdx.y * PACK_TILE;
    const size_t g = a.pack0 + blockIdx.z;
#pragma unroll 4
    for (int r = ty; r < PACK_TILE; r += 4) {
        const int j = j0 + r, col = c0 + tx;
        const size_t row = g * (size_t)N + j;                       // index into the call's picked rows
        uint32_t v = 0;
        if (j < N && row < a.B && col < len) {
            size_t src = a.idx ? (size_t)a.idx[row] : row;
            if (src >= a.pool_rows) src = a.pool_rows - 1;          // memory safety whatever a device-side index array holds
            v = a.pool[src * (size_t)len + col];
        }
        tile[r][tx] = v;
    }
    __syncthreads();
    WORD *cols = static_cast<WORD *>(a.cols) + (size_t)blockIdx.z * len * N;
#pragma unroll 4
    for (int r = ty; r < PACK_TILE; r += 4) {
        const int col = c0 + r, j = j0 + tx;
        if (col < len && j < N) cols[(size_t)col * N + j] = (WORD)((WORD)tile[tx][r] << SH);
    }
}

// ---- 2. gadget products ----
// Thread t of NT = M / 4 holds the coefficients e NT + t and e NT + t + M of a column (the first window of the forward transform), the same
// coefficients of its NP = 1 + kr integer accumulators, and after a forward transform the points 4 t + e, which the resident key stores at
// e NT + t (slot-major, dev_pos order 1): every key load is 16 bytes per lane, one contiguous KiB per wave.  Multiplies and adds stay
// separate (contraction off); the twiddle table Psi is resident in LDS and serves both directions.
template <int LOGM, typename WORD, int NP>
__global__ __launch_bounds__((Plan<LOGM, LOGR>::NT)) void pack_product_kernel(const PackArgs a) {
    using P = Plan<LOGM, LOGR>;
    constexpr int R = P::R, NT = P::NT, M = P::M, N = 2 * M;
    cplx *lds = reinterpret_cast<cplx *>(mkt_smem);
    cplx *psi_l = lds + P::LDS_CPLX;
    const int t = threadIdx.x;
    XS xs = make_xs();
    for (int i = t; i < M; i += NT) psi_l[i] = a.tw.psi[i];
    __syncthreads();
    const int chunk = blockIdx.x, party = blockIdx.y, pk = blockIdx.z;
    const int q0 = chunk * PACK_QCHUNK, q1 = q0 + PACK_QCHUNK < a.n ? q0 + PACK_QCHUNK : a.n;
    const Gadget<WORD> gd(a.l, a.logB);
    cplx rt[R], ri[R];
#pragma unroll
    for (int e = 0; e < R; e++) { rt[e] = a.tw.roots[e * NT + t]; ri[e] = a.tw.rootsinv[e * NT + t]; }
    WORD sum[NP][R][2];
#pragma unroll
    for (int c = 0; c < NP; c++)
#pragma unroll
        for (int e = 0; e < R; e++) sum[c][e][0] = sum[c][e][1] = 0;
    const WORD *cols = static_cast<const WORD *>(a.cols) + ((size_t)pk * a.lwe_len + (size_t)party * a.n) * N;
    const cplx *key = a.key + (size_t)party * a.key_party_stride;
    for (int q = q0; q < q1; q++) {
        WORD tp[R][2];
#pragma unroll
        for (int e = 0; e < R; e++) {
            tp[e][0] = gd.prep(cols[(size_t)q * N + e * NT + t]);
            tp[e][1] = gd.prep(cols[(size_t)q * N + M + e * NT + t]);
        }
        cplx tacc[NP][R];
        czero(tacc);                                                 // initialise! (bootstrapping.jl:62)
        for (int j = 0; j < a.l; j++) {
            cplx z[R];
            digit_points<WORD, R>(z, tp, gd, j, rt);                 // fftto! of digit polynomial j (fft.jl:57-63)
            fft_forward1<LOGM>(z, psi_l, lds, t, xs);
            const cplx *row = key + ((size_t)q * a.l + j) * NP * M;
#pragma unroll
            for (int c = 0; c < NP; c++)
#pragma unroll
                for (int e = 0; e < R; e++) tacc[c][e] = cadd(tacc[c][e], cmul(z[e], row[(size_t)c * M + e * NT + t]));   // muladdto!
        }
#pragma unroll
        for (int c = 0; c < NP; c++) {                               // ifftto! (fft.jl:74-81), then the integer sum over q
            fft_inverse<LOGM, LOGR, 1, true>(reinterpret_cast<cplx(&)[1][R]>(tacc[c]), psi_l, lds, t, xs.lx);
#pragma unroll
            for (int e = 0; e < R; e++) {
                const cplx v = cmul(tacc[c][e], ri[e]);
                sum[c][e][0] = native_add<WORD>(sum[c][e][0], v.re);
                sum[c][e][1] = native_add<WORD>(sum[c][e][1], -v.im);
            }
        }
    }
    WORD *slab = static_cast<WORD *>(a.slabs) + (((size_t)pk * a.nparty + party) * a.nchunk + chunk) * NP * N;
#pragma unroll
    for (int c = 0; c < NP; c++)
#pragma unroll
        for (int e = 0; e < R; e++) {
            slab[(size_t)c * N + e * NT + t] = sum[c][e][0];
            slab[(size_t)c * N + M + e * NT + t] = sum[c][e][1];
        }
}

// ---- 3. slabs -> ciphertext ----
// out[pack][p][x]: p = 0 gathers polynomial 0 of every (party, chunk) slab and the body column; p = 1 + slot gathers polynomial 1 of party
// `slot`'s slabs (multi-key) or polynomial p of party 0's (CGGI / LMSS).  Consecutive lanes take consecutive x.
template <typename WORD>
__global__ __launch_bounds__(256) void pack_reduce_kernel(const PackArgs a, size_t npacks) {
    const int N = 1 << a.logN, NP = a.np;
    const size_t total = npacks * (size_t)(1 + a.kacc) * N;
    const WORD *slabs = static_cast<const WORD *>(a.slabs), *cols = static_cast<const WORD *>(a.cols);
    WORD *out = static_cast<WORD *>(a.out);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % N), p = (int)((i / N) % (1 + a.kacc));
        const size_t pk = i / ((size_t)(1 + a.kacc) * N);
        const size_t per_party = (size_t)a.nchunk * NP * N;
        const WORD *s; int count; WORD v = 0;
        if (p == 0) { s = slabs + pk * a.nparty * per_party; count = a.nparty * a.nchunk; v = cols[(pk * a.lwe_len + (size_t)a.nparty * a.n) * N + x]; }
        else if (a.mk) { s = slabs + (pk * a.nparty + (p - 1)) * per_party + N; count = a.nchunk; }
        else { s = slabs + pk * per_party + (size_t)p * N; count = p < NP ? a.nchunk : 0; }
        for (int c = 0; c < count; c++) v = (WORD)(v + s[(size_t)c * NP * N + x]);
        out[i] = v;
    }
}

// MKT_ARITH_EXACT: dst[x] += sum_{r < rows} prod[r][x], one polynomial of a ciphertext the host has started from the body column or from zero
template <typename WORD>
__global__ __launch_bounds__(256) void pack_accumulate_kernel(WORD *__restrict__ dst, const WORD *__restrict__ prod, size_t rows, int N) {
    for (int x = blockIdx.x * blockDim.x + threadIdx.x; x < N; x += gridDim.x * blockDim.x) {
        WORD v = dst[x];
        for (size_t r = 0; r < rows; r++) v = (WORD)(v + prod[r * N + x]);
        dst[x] = v;
    }
}

hipError_t launch_pack_columns(int W, const PackArgs &a, size_t npacks, hipStream_t s) {
    if (!npacks) return hipSuccess;
    const int N = 1 << a.logN;
    const dim3 grid((unsigned)((N + PACK_TILE - 1) / PACK_TILE), (unsigned)((a.lwe_len + PACK_TILE - 1) / PACK_TILE), (unsigned)npacks);
    if (W == 64) hipLaunchKernelGGL(pack_columns_kernel<uint64_t>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(pack_columns_kernel<uint32_t>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

template <int LM, typename WORD, int NP>
static hipError_t launch_product_one(const PackArgs &a, size_t npacks, hipStream_t s) {
    using P = Plan<LM, LOGR>;
    constexpr size_t LB = P::LDS_BYTES + (size_t)P::M * sizeof(cplx);
    hipError_t e = set_lds(pack_product_kernel<LM, WORD, NP>, LB);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((pack_product_kernel<LM, WORD, NP>), dim3((unsigned)a.nchunk, (unsigned)a.nparty, (unsigned)npacks), dim3(P::NT), LB, s, a);
    return hipGetLastError();
}
template <int LM, typename WORD>
static hipError_t launch_product_np(const PackArgs &a, size_t npacks, hipStream_t s) {
    switch (a.np) {
    case 2: return launch_product_one<LM, WORD, 2>(a, npacks, s);
    case 3: return launch_product_one<LM, WORD, 3>(a, npacks, s);
    case 4: return launch_product_one<LM, WORD, 4>(a, npacks, s);
    default: return hipErrorInvalidValue;
    }
}
bool pack_supported(int np) { return np >= 2 && np <= 4; }
hipError_t launch_pack_product(int logM, int W, const PackArgs &a, size_t npacks, hipStream_t s) {
    if (!npacks) return hipSuccess;
    MKT_DISPATCH_LOGM(logM, { return W == 64 ? launch_product_np<LM, uint64_t>(a, npacks, s) : launch_product_np<LM, uint32_t>(a, npacks, s); });
    return hipErrorInvalidValue;
}

hipError_t launch_pack_reduce(int W, const PackArgs &a, size_t npacks, hipStream_t s) {
    if (!npacks) return hipSuccess;
    const int blocks = blocks_for(npacks * (size_t)(1 + a.kacc) << a.logN, 256);
    if (W == 64) hipLaunchKernelGGL(pack_reduce_kernel<uint64_t>, dim3(blocks), dim3(256), 0, s, a, npacks);
    else hipLaunchKernelGGL(pack_reduce_kernel<uint32_t>, dim3(blocks), dim3(256), 0, s, a, npacks);
    return hipGetLastError();
}

hipError_t launch_pack_accumulate(int W, void *dst, const void *prod, size_t rows, int N, hipStream_t s) {
    const int blocks = blocks_for((size_t)N, 256);
    if (W == 64) hipLaunchKernelGGL(pack_accumulate_kernel<uint64_t>, dim3(blocks), dim3(256), 0, s, (uint64_t *)dst, (const uint64_t *)prod, rows, N);
    else hipLaunchKernelGGL(pack_accumulate_kernel<uint32_t>, dim3(blocks), dim3(256), 0, s, (uint32_t *)dst, (const uint32_t *)prod, rows, N);
    return hipGetLastError();
}

}  // namespace mktd
