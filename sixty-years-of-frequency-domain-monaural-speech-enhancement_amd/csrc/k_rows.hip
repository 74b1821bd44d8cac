// Per-window view of the per-row sizes of a ragged call (window_rows.h).
#include "window_rows.h"
#include "common.h"

namespace se {

__global__ __launch_bounds__(256) void window_rows_kernel(const int* __restrict__ src, int* __restrict__ dst, int MB, int B, int t_hi) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    dst[b] = src[b];
    dst[MB + b] = src[MB + b];
    dst[2 * MB + b] = min(src[2 * MB + b], t_hi);
    dst[3 * MB + b] = src[3 * MB + b];
}

void launch_window_rows(const int* src, int* dst, int MB, int B, int t_hi, hipStream_t s) {
    hipLaunchKernelGGL(window_rows_kernel, dim3((B + 255) / 256), dim3(256), 0, s, src, dst, MB, B, t_hi);
    SE_HIP(hipGetLastError());
}

}  // namespace se
