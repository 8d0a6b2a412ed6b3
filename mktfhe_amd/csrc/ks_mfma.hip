// Key switch on the matrix cores: the kernels of ks_mfma.h.
//   ks_mfma_pack_kernel   the byte planes of one block of a key-switching key from its resident rows (once per key load)
//   ks_mfma_kernel        digit words x byte planes -> partial sums per slab (between ks_digits_kernel and ks_reduce_kernel, kernels.hip)
#include "ks_mfma.h"
#include "device_api.h"

namespace mktd {

// 16 bytes per thread, in the planes' own order: the stores are contiguous, the row reads gather (once per key)
__global__ __launch_bounds__(256) void ks_mfma_pack_kernel(const uint32_t *rows, int8_t *planes, int N, int f, int drows, int n1p, size_t bytes) {
    const size_t off = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 16;
    if (off >= bytes) return;
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 16; e++) w[e >> 2] |= (uint32_t)(uint8_t)ksm_plane_byte(rows, N, f, drows, n1p, off + e) << (8 * (e & 3));
    *reinterpret_cast<uint4 *>(planes + off) = make_uint4(w[0], w[1], w[2], w[3]);
}

template <int F>
__global__ __launch_bounds__(64 * KSM_WAVES, 1) void ks_mfma_kernel(const KsmArgs a) { ksm_workgroup<F>(a); }

hipError_t launch_ks_mfma_pack(const uint32_t *rows, int8_t *planes, int N, int f, int drows, int n1p, hipStream_t s) {
    const size_t bytes = ksm_block_bytes(N, f, n1p);   // a multiple of 4096
    hipLaunchKernelGGL(ks_mfma_pack_kernel, dim3((unsigned)((bytes / 16 + 255) / 256)), dim3(256), 0, s, rows, planes, N, f, drows, n1p, bytes);
    return hipGetLastError();
}

hipError_t launch_ks_mfma(const KsmArgs &a, hipStream_t s) {
    if (a.B < 1 || a.slabs < 1) return hipErrorInvalidValue;
    const int gtiles = (a.B + KSM_WAVE_GATES * KSM_WAVES - 1) / (KSM_WAVE_GATES * KSM_WAVES);
    const dim3 grid((unsigned)(gtiles * a.slabs), (unsigned)(a.mk ? a.kacc : 1), (unsigned)ksm_coltiles(a.n1p));
    if (a.f == 8) hipLaunchKernelGGL(ks_mfma_kernel<8>, grid, dim3(64 * KSM_WAVES), 0, s, a);
    else hipLaunchKernelGGL(ks_mfma_kernel<0>, grid, dim3(64 * KSM_WAVES), 0, s, a);
    return hipGetLastError();
}

}  // namespace mktd
