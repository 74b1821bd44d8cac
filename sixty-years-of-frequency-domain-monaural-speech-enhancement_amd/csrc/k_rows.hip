// Per-window view of the per-row sizes of a ragged call, and the window-relative zero tail of chunk tensors (window_rows.h).
#include "window_rows.h"
#include "common.h"
#include <algorithm>
#include <cstdint>

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

static thread_local const WindowEnds* g_window_ends = nullptr;
const WindowEnds* window_ends_ctx() { return g_window_ends; }
void set_window_ends_ctx(const WindowEnds* w) { g_window_ends = w; }

// Columns [cut, Tw) of every row of x[b] <- 0 (blockIdx.y = b, blockIdx.z = tensor).  A store-only kernel: no loads but tlen[b], no
// LDS.  The tail of a row is w = Tw - cut floats at a column offset that need not be a multiple of four (Tw is HC + n, any n), so a
// tail is cut into the 16 B slots of memory it touches: a slot that lies wholly inside the tail is one 16 B store, the two at its
// ragged edges are stored float by float.  A row takes `lpr` lanes (a power of two: one slot per lane for tails up to 252 floats, the
// chunk sizes of a frame-online-sized window take one or two lanes a row), a block 256 / lpr rows a pass; every lane's stores are
// independent, so they all stay in flight.
__global__ __launch_bounds__(256) void window_zero_tail_kernel(const ZeroTailBatch zb, int Tw, const int* __restrict__ tlen, int t0,
                                                               int HC) {
    const int b = blockIdx.y;
    const int cut = window_cut(tlen[b], t0, HC, Tw);
    if (cut >= Tw) return;      // the row has not ended inside this window (block-uniform)
    const long rows = zb.rows[blockIdx.z];
    float* __restrict__ x = zb.buf[blockIdx.z] + (long)b * rows * Tw;
    const int mis = (int)(((uintptr_t)x >> 2) & 3);      // x - mis is 16 B aligned: element indices below are relative to it
    const int slots = (Tw - cut + 3) / 4 + 1;            // 16 B slots a tail can touch
    int sh = 0;
    while ((1 << sh) < slots && sh < 6) ++sh;
    const int lpr = 1 << sh, j = threadIdx.x & (lpr - 1);
    const long rpass = 256 >> sh;
    for (long r = blockIdx.x * rpass + (threadIdx.x >> sh); r < rows; r += gridDim.x * rpass) {
        const long lo = r * Tw + cut + mis, hi = r * Tw + Tw + mis;      // the tail, [lo, hi)
        for (long e = (lo & ~3L) + 4 * j; e < hi; e += 4 * lpr) {
            float* p = x + (e - mis);
            if (e >= lo && e + 4 <= hi) {
                *reinterpret_cast<float4*>(p) = make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (e + i >= lo && e + i < hi) p[i] = 0.f;
            }
        }
    }
}

void launch_window_zero_tail_batch(const ZeroTailBatch& zb, int B, int Tw, const int* tlen, int t0, int HC, hipStream_t s) {
    if (zb.n <= 0 || B <= 0) return;
    SE_CHECK(zb.n <= ZeroTailBatch::MAX, "launch_window_zero_tail_batch: too many tensors");
    SE_CHECK(tlen && Tw >= 1 && HC >= 0 && HC <= Tw, "launch_window_zero_tail_batch: bad window");
    long most = 0;
    for (int k = 0; k < zb.n; ++k) {
        SE_CHECK(zb.buf[k] && zb.rows[k] >= 1, "launch_window_zero_tail_batch: empty tensor");
        most = std::max(most, zb.rows[k]);
    }
    // 64 rows a block where a tail is short (four passes of one or two lanes a row); at most 64 blocks a (row, tensor) - whole
    // windows behind a row's end are 64 x 7 blocks of 64-lane rows
    const unsigned gx = (unsigned)std::min<long>((most + 63) / 64, 64);
    hipLaunchKernelGGL(window_zero_tail_kernel, dim3(gx, (unsigned)B, (unsigned)zb.n), dim3(256), 0, s, zb, Tw, tlen, t0, HC);
    SE_HIP(hipGetLastError());
}

void launch_window_zero_tail(float* x, int B, long rows, int Tw, const int* tlen, int t0, int HC, hipStream_t s) {
    ZeroTailBatch zb;
    zb.add(x, rows);
    launch_window_zero_tail_batch(zb, B, Tw, tlen, t0, HC, s);
}

}  // namespace se
