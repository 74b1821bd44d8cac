// Parking and resuming a frame-online stream (se_stream_save / se_stream_restore): every carried buffer of a stream - conv
// history, LSTM (h, c), the cLN networks' call-order slots, the scales, the live input samples - moves between the engine and a
// snapshot's payload in ONE launch, however many buffers the model has (DCCRN ~25, the cLN networks well over 100): a one-frame
// push is bound by its launch count, and a server that time-slices one engine pays a save and a restore per push.
//
// The segments are rows of a table in device memory (kernels.h: StateSeg), built when a layout is first seen.  Each segment is
// `rows` runs of `len` floats (a flat buffer: one run); run r goes from src + r * src_pitch to dst + r * dst_pitch.  The work is
// cut into tiles of STATE_TILE floats, one workgroup per tile, and the table carries the first tile of every segment: the grid is
// the total tile count - sized to the bytes, so a large segment spreads over as many workgroups as it has tiles - and a
// workgroup finds its segment by bisection (<= 9 steps of wave-uniform 8 B loads for 300 segments).  The input window is the one
// segment whose extent changes from call to call (the live samples [keep, n_total)): its offsets and run length are kernel
// arguments, its tiles follow the table's.
//
// Access width (MI355X: 16 B per lane is the widest global access, 64 lanes x 16 B = 1 KiB per wave instruction): payload offsets
// are 16 B aligned and so is every buffer hipMalloc returns, so flat segments move as float4.  A run whose two ends are 16 B
// aligned relative to each other is copied as a scalar head up to the first aligned destination, float4 body, scalar tail; a run
// whose ends are not (a window row whose pitch or origin is no multiple of 4 floats against the compact payload rows) moves as
// scalars.  Nothing outside [0, len) of a run is read or written.
#include "k_stream_state.h"
#include "kernels.h"

namespace se {

// n floats from s to d by the 256 threads of a workgroup
__device__ __forceinline__ void state_copy_run(const float* __restrict__ s, float* __restrict__ d, int n) {
    const int tid = threadIdx.x;
    const int head = min(n, (int)(((16u - (unsigned)((uintptr_t)d & 15u)) & 15u) >> 2));
    if ((((uintptr_t)(s + head)) & 15u) != 0) {
        for (int i = tid; i < n; i += 256) d[i] = s[i];
        return;
    }
    if (tid < head) d[tid] = s[tid];
    const int nv = (n - head) >> 2;
    const float4* __restrict__ s4 = reinterpret_cast<const float4*>(s + head);
    float4* __restrict__ d4 = reinterpret_cast<float4*>(d + head);
    for (int i = tid; i < nv; i += 256) d4[i] = s4[i];
    const int done = head + (nv << 2);
    if (tid < n - done) d[done + tid] = s[done + tid];
}

__global__ __launch_bounds__(256) void stream_state_copy_kernel(const StateSeg* __restrict__ tab, int nfix, int fix_tiles,
                                                                int win, long win_src_off, long win_dst_off, long win_src_pitch,
                                                                long win_dst_pitch, int win_len, int win_tpr) {
    const int b = blockIdx.x;
    const float* src;
    float* dst;
    long sp, dp;
    int rows, len, tpr, t;
    if (b < fix_tiles) {
        int lo = 0, hi = nfix - 1;          // the last segment whose first tile is <= b (empty segments share their successor's)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (tab[mid].tile0 <= b) lo = mid;
            else hi = mid - 1;
        }
        const StateSeg sg = tab[lo];
        src = sg.src;
        dst = sg.dst;
        sp = sg.src_pitch;
        dp = sg.dst_pitch;
        rows = sg.rows;
        len = sg.len;
        tpr = (len + STATE_TILE - 1) / STATE_TILE;
        t = b - sg.tile0;
    } else {
        if (win < 0) return;
        const StateSeg sg = tab[win];
        src = sg.src + win_src_off;
        dst = sg.dst + win_dst_off;
        sp = win_src_pitch;
        dp = win_dst_pitch;
        rows = sg.rows;
        len = win_len;
        tpr = win_tpr;
        t = b - fix_tiles;
    }
    if (tpr <= 0) return;
    const int r = t / tpr;
    const int c0 = (t - r * tpr) * STATE_TILE;
    if (r >= rows || c0 >= len) return;
    state_copy_run(src + (long)r * sp + c0, dst + (long)r * dp + c0, min(STATE_TILE, len - c0));
}

long state_seg_tiles(int rows, int len) { return (long)rows * ((len + STATE_TILE - 1) / STATE_TILE); }

void launch_stream_state_copy(const StateSeg* tab_dev, int nfix, long fix_tiles, int win, const StateWindow& w, hipStream_t s) {
    SE_CHECK(nfix >= 0 && fix_tiles >= 0 && w.len >= 0 && w.rows >= 0, "launch_stream_state_copy: bad table");
    const int tpr = (w.len + STATE_TILE - 1) / STATE_TILE;
    const long tiles = fix_tiles + (win >= 0 ? (long)w.rows * tpr : 0);
    if (tiles == 0) return;
    SE_CHECK(tiles < (1L << 31), "launch_stream_state_copy: too many tiles");
    hipLaunchKernelGGL(stream_state_copy_kernel, dim3((unsigned)tiles), dim3(256), 0, s, tab_dev, nfix, (int)fix_tiles, win, w.src_off,
                       w.dst_off, w.src_pitch, w.dst_pitch, w.len, tpr);
    SE_HIP(hipGetLastError());
}

// ---- se_stream_state_select / se_stream_state_concat: rows of parked groups into a new payload ---------------------------------
// The same walk - one workgroup per tile of STATE_TILE destination floats, its segment found by bisection - over a table that
// carries the row layout of every segment (kernels.h GatherSeg): the destination is [outer][Bd][inner], a thread's flat index j
// there is (o, bd, i), and it reads (o, row, i) of the part the row map names for bd.  Consecutive threads write consecutive
// addresses; they read consecutive addresses within a run of `inner` floats, and for the inner == 1 layouts (LSTM state: the batch is
// the fastest axis) the lanes of a wave read rows of ONE o - a gather inside a few cache lines.  A layout whose runs are whole
// float4s (inner a multiple of 4: every run then starts 16 B aligned in both payloads, whose segments start 16 B aligned) moves 16 B
// per lane; the others move floats and also write the zeros between the segment's end and the next 16 B boundary.
//
// se_stream_state_join runs the same walk with one more table (k_stream_state.h JoinWindow): the parts of a join may hold input windows of
// different lengths, and the result keeps the columns [col, col + inner) of each - so for the window segment alone a source row has
// the part's own length and starts at the part's own column.  Those rows are no whole float4s in general (a live window is
// n_total - keep samples long): the window moves as floats, a few hundred per row.  JOIN == false is the kernel select and concat launch.
template <bool JOIN>
__device__ __forceinline__ void state_gather_tile(const GatherArgs& a, const JoinWindow& w) {
    const int b = blockIdx.x;
    int lo = 0, hi = a.nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.tab[mid].tile0 <= b) lo = mid;
        else hi = mid - 1;
    }
    const GatherSeg sg = a.tab[lo];
    const unsigned n = (unsigned)sg.n, inner = (unsigned)sg.inner, run = (unsigned)a.Bd * inner;
    const unsigned j0 = (unsigned)(b - sg.tile0) * STATE_TILE;
    if (inner == 0 || j0 >= ((n + 3u) & ~3u)) return;
    const long* __restrict__ off = a.src_off + lo;
    const bool window = JOIN && lo == w.seg;
    const bool rotate = JOIN && lo >= w.ring_lo && lo < w.ring_hi;
    const bool origin = JOIN && lo == w.origin_seg;
    auto source = [&](unsigned j) -> const float* {
        const unsigned o = j / run, rem = j - o * run, bd = rem / inner, i = rem - bd * inner;
        const int2 pr = a.rowmap[bd];
        const float* base = a.part_base[pr.x] + off[(long)pr.x * a.nseg];
        if (window) return base + ((long)o * a.part_B[pr.x] + pr.y) * w.part_inner[pr.x] + w.part_col[pr.x] + i;
        if (rotate) return base + ((long)o * a.part_B[pr.x] + pr.y) * inner + ((i - (unsigned)w.part_rot[pr.x]) & (inner - 1u));
        return base + ((long)o * a.part_B[pr.x] + pr.y) * inner + i;
    };
    if ((inner & 3u) == 0 && !window && !rotate) {
        for (unsigned q = threadIdx.x; q < STATE_TILE / 4; q += 256) {
            const unsigned j = j0 + 4 * q;
            if (j >= n) break;
            *reinterpret_cast<float4*>(sg.dst + j) = *reinterpret_cast<const float4*>(source(j));
        }
    } else {
        const unsigned npad = (n + 3u) & ~3u;
        for (unsigned q = threadIdx.x; q < STATE_TILE; q += 256) {
            const unsigned j = j0 + q;
            if (j >= npad) break;
            if (origin) {      // [Bd] int32 (inner == 1, so j is the row): the part's shift in frames rides on the copy
                reinterpret_cast<int*>(sg.dst)[j] = j < n ? *reinterpret_cast<const int*>(source(j)) + w.part_frames[a.rowmap[j].x] : 0;
                continue;
            }
            sg.dst[j] = j < n ? *source(j) : 0.f;
        }
    }
}

__global__ __launch_bounds__(256) void stream_state_gather_kernel(const GatherArgs a) { state_gather_tile<false>(a, JoinWindow{}); }
__global__ __launch_bounds__(256) void stream_state_join_kernel(const GatherArgs a, const JoinWindow w) { state_gather_tile<true>(a, w); }

long state_gather_tiles(long n) { return (n + STATE_TILE - 1) / STATE_TILE; }

void launch_stream_state_gather(const GatherArgs& a, long tiles, hipStream_t s) {
    SE_CHECK(a.nseg >= 1 && a.Bd >= 1 && tiles >= 0 && tiles < (1L << 31), "launch_stream_state_gather: bad table");
    if (tiles == 0) return;
    hipLaunchKernelGGL(stream_state_gather_kernel, dim3((unsigned)tiles), dim3(256), 0, s, a);
    SE_HIP(hipGetLastError());
}

void launch_stream_state_join(const GatherArgs& a, const JoinWindow& w, long tiles, hipStream_t s) {
    SE_CHECK(a.nseg >= 1 && a.Bd >= 1 && tiles >= 0 && tiles < (1L << 31), "launch_stream_state_join: bad table");
    SE_CHECK(w.seg >= 0 && w.seg < a.nseg && w.part_inner && w.part_col, "launch_stream_state_join: no window segment");
    SE_CHECK(w.ring_lo >= w.ring_hi || (w.ring_lo >= 0 && w.ring_hi <= a.nseg && w.part_rot), "launch_stream_state_join: bad ring segments");
    SE_CHECK(w.origin_seg < 0 || (w.origin_seg < a.nseg && w.origin_seg != w.seg && w.part_frames), "launch_stream_state_join: bad origin segment");
    if (tiles == 0) return;
    hipLaunchKernelGGL(stream_state_join_kernel, dim3((unsigned)tiles), dim3(256), 0, s, a, w);
    SE_HIP(hipGetLastError());
}

}  // namespace se
