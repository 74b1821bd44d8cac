// Band-limited sinc resampler (48 kHz VoiceBank+DEMAND clips -> the models' 16 kHz): the GPU side of
// `librosa.resample(y, orig_sr, 16000, fix=True, scale=False)` at DCCRN/dccrn_decode_vb.py:26, LSTM/lstm_decode_vb.py:34.
//
// librosa / resampy are third-party, absent and unversioned in the reference: this follows the
// published resampy 'kaiser_best' algorithm - Kaiser-windowed sinc table (64 zero crossings x 512 samples), linear
// interpolation between table entries, float64 accumulation - restated in oracle/resample.py; parity is pinned to
// that restatement only.  One thread per output sample; the table (256 KB of doubles) lives in L2.
//
// Three kernels share the tap arithmetic (resample_taps): resample_kernel, stateless, for whole clips of one length;
// resample_ragged_kernel, stateless, for whole clips of different lengths in one call (se_resample_ragged: the staged batch of the
// file driver); and resample_stream_kernel for the stateful StreamResampler below, which is fed piecewise.  The last two are held to
// equality with the first: a row of a ragged call, and the pushes of a stream concatenated, are the very numbers resample_kernel
// gives for that signal alone - the same float64 sum term by term, at the same read positions.
//   ragged   : one grid over (row, block of 256 outputs); the rows' n_in / n_calc are kernel arguments, 64 rows a launch
//              (resample_ragged.h: sizes, refusals, the split - host code alone), so the lengths reach the device without a copy or
//              a wait.  Input is float or raw PCM_16: the tap read forms x / 32768 as pcm16_decode_kernel does, so no float copy of
//              the batch is made.  Threads behind a row's computed samples write zeros up to the longest row's output (fix_length
//              tail and se_enhance_ragged's row padding alike).  Filter table and, for ratios that are no integer decimation, the
//              table of read positions are kept per (ratio, device) for the life of the process; the positions depend on the output
//              index and the ratio alone, so one table serves all rows and all calls, and a call waits for the device only when a
//              longer row makes the table grow (hipDeviceSynchronize: other hipStreams may read the old one).  The tap loop is the
//              plain per-thread one: staging the integer-decimation coefficient set in LDS was left out.
//   window   : per row the last 2 * reach input samples ("history": reach = the taps one wing can span, resample_pos.h - an
//              output not yet released sits at most reach samples before the end and looks less than reach further back)
//              in one of two buffers; a push reads [history | the caller's new samples] in place and writes the next
//              history into the OTHER buffer in the same launch, so nothing is read and written at once.  Both buffers, the
//              scaled table and the position ring are allocated at create; push and flush allocate nothing.
//   wings    : clamped by absolute position as offline - the left one by n + 1, the right one by the samples that have
//              arrived.  A push releases an output only when its whole right wing has arrived, so the right clamp bites at
//              flush alone, where the arrived samples are the final length.  History is never assumed to be zero-filled.
//   positions: integer decimation (48 / 32 -> 16 kHz): t * inc in the kernel; a push then enqueues one launch and calls
//              nothing that waits for the device.  Other ratios: resampy's running sum, carried across pushes on the host; the
//              few positions of a push travel through a ring of 8 pinned slots (hipMemcpyAsync, one event per slot).  The one
//              wait left on that path: hipEventSynchronize on a slot's event before the host rewrites the slot, i.e. on the
//              copy enqueued 8 pushes earlier - it blocks only a caller that runs 8 pushes ahead of the device.
//   parking  : save / restore (se_resampler_save / _restore) copy the live history [w0, n_total) of every row to and from the packed
//              rows of a ResamplerState, one launch of resampler_state_copy_kernel; the counters travel in the host record
//              (resampler_manifest.h).  Which buffer is current, the ring and the table are not saved: nothing later reads them.
//              Parked signals of an integer decimation that began at different times are joined into one group by rebasing their
//              counters (se_resampler_state_join; resampler_join.h has the conditions and their derivation).
//   launch   : one output per thread, 64-thread blocks.  A 10 ms push at 48 kHz makes 160 outputs per row: three waves of
//              ~384 dependent float64 steps each.  The launch is bound by that chain's latency, not by occupancy or f64
//              rate, so the outputs are spread over as many CUs as there are waves instead of filling one 256-thread block.
#include "kernels.h"
#include "common.h"
#include "hip_owned.h"
#include "parked.h"
#include "resample_pos.h"
#include "resample_ragged.h"
#include "resampler.h"
#include "resampler_manifest.h"
#include "resampler_join.h"
#include <climits>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

namespace se {

namespace {

constexpr double RS_ROLLOFF = 0.9475937167399596, RS_BETA = 14.769656459379492;

double bessel_i0(double x) {
    double s = 1.0, term = 1.0;
    const double q = 0.25 * x * x;
    for (int k = 1; k < 200; ++k) {
        term *= q / ((double)k * k);
        s += term;
        if (term < 1e-18 * s) break;
    }
    return s;
}

// right half of the filter, as resampy.filters.sinc_window builds it
std::vector<double> build_window() {
    const int n = RS_ZEROS * RS_BITS;
    std::vector<double> w(n + 1);
    const double i0b = bessel_i0(RS_BETA);
    const double pi = 3.14159265358979323846;
    for (int k = 0; k <= n; ++k) {
        const double t = (double)k * RS_ZEROS / n;                  // np.linspace(0, num_zeros, n + 1)
        const double a = RS_ROLLOFF * t;
        const double sinc = a == 0.0 ? 1.0 : std::sin(pi * a) / (pi * a);
        const double r = (double)k / n;                             // kaiser(2n+1)[n + k]: position k of n from the centre
        const double taper = bessel_i0(RS_BETA * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
        w[k] = taper * RS_ROLLOFF * sinc;
    }
    return w;
}

struct ResampleArgs {
    const float* x; long in_pitch; int n_in;
    float* y; long out_pitch; int n_calc, n_out;
    const double* win;       // [RS_NWIN] (already scaled by the ratio when downsampling)
    const double* treg;      // [n_calc] read positions, or nullptr -> t * inc exactly (integer decimation)
    double inc, scale;
    int index_step;
};

// x by absolute sample position: a whole clip, or a stream's [history | new samples]
struct ClipAt {
    const float* __restrict__ x;
    __device__ float operator()(int p) const { return x[p]; }
};
struct WindowAt {
    const float* __restrict__ hist;   // hist[0] is sample w0
    const float* __restrict__ in;     // in[0] is sample split (never read when nothing is new)
    int w0, split;
    __device__ float operator()(int p) const { return p < split ? hist[p - w0] : in[p - split]; }
};

// One output sample: the taps around input position n + pos_frac of a signal of n_in samples - table look-up with linear
// interpolation, float64 accumulation, left wing then right wing.
template <typename X>
__device__ __forceinline__ double resample_taps(const X& x, const double* __restrict__ win, int n, double pos_frac, int n_in,
                                                double scale, int index_step) {
    double acc = 0.0;
    const double frac = scale * pos_frac;
    const double index_frac = frac * RS_BITS;
    const int offset = (int)index_frac;
    const double eta = index_frac - offset;
    const int i_max = min(n + 1, (RS_NWIN - offset) / index_step);
    for (int i = 0; i < i_max; ++i) {
        const int idx = offset + i * index_step;
        const double d = idx + 1 < RS_NWIN ? win[idx + 1] - win[idx] : 0.0;
        acc += (win[idx] + eta * d) * (double)x(n - i);
    }
    const double frac2 = scale - frac;
    const double index_frac2 = frac2 * RS_BITS;
    const int offset2 = (int)index_frac2;
    const double eta2 = index_frac2 - offset2;
    const int k_max = min(n_in - n - 1, (RS_NWIN - offset2) / index_step);
    for (int k = 0; k < k_max; ++k) {
        const int idx = offset2 + k * index_step;
        const double d = idx + 1 < RS_NWIN ? win[idx + 1] - win[idx] : 0.0;
        acc += (win[idx] + eta2 * d) * (double)x(n + k + 1);
    }
    return acc;
}

__global__ __launch_bounds__(256) void resample_kernel(const ResampleArgs a) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= a.n_out) return;
    float* yp = a.y + (long)blockIdx.y * a.out_pitch;
    if (t >= a.n_calc) {                                            // librosa fix_length: zero tail up to ceil(n * ratio)
        yp[t] = 0.f;
        return;
    }
    const ClipAt x{a.x + (long)blockIdx.y * a.in_pitch};
    const double tr = a.treg ? a.treg[t] : (double)t * a.inc;
    const int n = (int)tr;
    yp[t] = (float)resample_taps(x, a.win, n, tr - n, a.n_in, a.scale, a.index_step);
}

// One push (or the flush) of a StreamResampler: blocks [0, out_blocks) compute outputs t0 .. t0 + n_emit, blocks behind them
// copy the samples from w0_next on into the other history buffer.
struct ResampleStreamArgs {
    const float* hist; float* hist_next; long hist_pitch;
    const float* in; long in_pitch;
    float* y; long out_pitch;
    const double* win;
    const double* treg;      // [n_calc] read positions of this launch's outputs, or nullptr -> (t0 + j) * inc
    double inc, scale;
    int index_step;
    int w0, split, n_total;  // absolute positions: first history sample, first new sample, samples arrived (new ones included)
    int w0_next;             // first sample of the next history (n_total: no history is written)
    int t0, n_calc, n_emit;  // first output; outputs computed; outputs written (the rest is the fix_length zero tail, at flush)
    int out_blocks;
};

constexpr int RS_STREAM_BLOCK = 64;

__global__ __launch_bounds__(RS_STREAM_BLOCK) void resample_stream_kernel(const ResampleStreamArgs a) {
    const long b = blockIdx.y;
    const WindowAt x{a.hist + b * a.hist_pitch, a.in ? a.in + b * a.in_pitch : nullptr, a.w0, a.split};
    if ((int)blockIdx.x >= a.out_blocks) {
        const int j = ((int)blockIdx.x - a.out_blocks) * RS_STREAM_BLOCK + threadIdx.x;
        if (j < a.n_total - a.w0_next) a.hist_next[b * a.hist_pitch + j] = x(a.w0_next + j);
        return;
    }
    const int j = blockIdx.x * RS_STREAM_BLOCK + threadIdx.x;
    if (j >= a.n_emit) return;
    float* yp = a.y + b * a.out_pitch;
    if (j >= a.n_calc) {
        yp[j] = 0.f;
        return;
    }
    const int t = a.t0 + j;
    const double tr = a.treg ? a.treg[j] : (double)t * a.inc;
    const int n = (int)tr;
    yp[j] = (float)resample_taps(x, a.win, n, tr - n, a.n_total, a.scale, a.index_step);
}

// se_resampler_save / se_resampler_restore: `keep` live history samples of every row, from rows of src_pitch to rows of dst_pitch
// (save: the current history buffer -> the packed rows of a snapshot's payload; restore: the other way).  Rows are a few hundred
// floats at most, so the launch is the cost: one coalesced load and store per thread.
__global__ __launch_bounds__(256) void resampler_state_copy_kernel(const float* __restrict__ src, long src_pitch, float* __restrict__ dst,
                                                                   long dst_pitch, int keep) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < keep) dst[(long)blockIdx.y * dst_pitch + j] = src[(long)blockIdx.y * src_pitch + j];
}

// se_resampler_state_select / _concat / _join: row y of the destination <- `keep` floats from src[y] on; up to 64 rows a launch, their
// sources as a kernel argument (a group is a few dozen rows, and the rows a few hundred floats).  src[y] is a packed row of its part,
// or (join: the parts' rows differ in length, resampler_join.h) a column inside one - so it is a float's alignment and no more
struct RowPtrs {
    const float* src[64];
};
__global__ __launch_bounds__(256) void resampler_state_gather_kernel(const RowPtrs rp, float* __restrict__ dst, int keep) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < keep) dst[(long)blockIdx.y * keep + j] = rp.src[blockIdx.y][j];
}

// What se_resample and se_resample_ragged keep per ratio and device for the life of the process: the (scaled) filter table and, when
// the ratio is no integer decimation, the position table - on the host as far as it has been summed, on the device as far as the
// longest row seen needed it.  A table is written once and then only read, and a position table that must grow is replaced after
// the device has gone idle: a launch on one hipStream never has its tables rewritten by a call on another (one table per device,
// rewritten for every new ratio behind a wait for the CALLER's stream alone, was the rule of se_resample until two calls on two
// streams were tested: DESIGN.md 4.5).
struct RatioTables {
    int sr_in = 0, sr_out = 0;
    double* win = nullptr;
    std::vector<double> tr;
    double acc = 0.0;
    double* dev_tr = nullptr;
    size_t dev_cap = 0;
};
struct ResampleTables {
    std::mutex mu;
    std::vector<double> host;
    std::vector<std::unique_ptr<RatioTables>> ratios;
};
ResampleTables& resample_tables() {
    static ResampleTables t[64];      // one set of tables per device
    int dev = 0;
    SE_HIP(hipGetDevice(&dev));
    SE_CHECK(dev >= 0 && dev < 64, "device ordinal");
    return t[dev];
}
// the entry of a ratio, made by the first call at this ratio on this device (T.mu held)
RatioTables* ratio_tables(ResampleTables& T, const ResamplePlan& plan, int sr_in, int sr_out) {
    for (auto& r : T.ratios)
        if (r->sr_in == sr_in && r->sr_out == sr_out) return r.get();
    if (T.host.empty()) T.host = build_window();
    std::vector<double> w(T.host);
    if (plan.ratio < 1.0)
        for (auto& v : w) v *= plan.ratio;                          // interp_win *= sample_ratio
    std::unique_ptr<RatioTables> fresh(new RatioTables());
    fresh->sr_in = sr_in; fresh->sr_out = sr_out;
    SE_HIP(hipMalloc(&fresh->win, RS_NWIN * sizeof(double)));
    const hipError_t e = hipMemcpy(fresh->win, w.data(), RS_NWIN * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) (void)hipFree(fresh->win);
    SE_HIP(e);
    T.ratios.push_back(std::move(fresh));
    return T.ratios.back().get();
}
// read positions [0, n_calc) of a ratio that is no integer decimation, on the device (T.mu held): resampy advances the read
// position by repeated float64 addition, and the sum is carried on from where it stopped
const double* ratio_positions(RatioTables* R, const ResamplePlan& plan, size_t n_calc) {
    if (n_calc > R->dev_cap) {
        // the table grows: the one place a call waits - launches on other hipStreams may still read the old table
        const size_t cap = std::max<size_t>(n_calc, 2 * R->dev_cap);
        ragged_positions_extend(plan, R->tr, R->acc, (int64_t)cap);
        SE_HIP(hipDeviceSynchronize());
        if (R->dev_tr) (void)hipFree(R->dev_tr);
        R->dev_tr = nullptr;
        R->dev_cap = 0;
        SE_HIP(hipMalloc(&R->dev_tr, cap * sizeof(double)));
        SE_HIP(hipMemcpy(R->dev_tr, R->tr.data(), cap * sizeof(double), hipMemcpyHostToDevice));
        R->dev_cap = cap;
    }
    return R->dev_tr;
}

}  // namespace

// ---- PCM_16 <-> float at the two ends of the decode driver (e.g. DCCRN/dccrn_decode_vb.py:25,64).  soundfile.read:
// int16 / 32768 -> float (libsndfile s2f, 1 / 0x8000).  soundfile.write, default subtype of .wav = PCM_16: libsndfile's
// float -> short conversion with normalisation scales by 0x7FFF (NOT 0x8000) and rounds to nearest even (lrint); it does not
// clip unless SFC_SET_CLIPPING is on - a sample beyond +-1 wraps there.  The engine takes the 0x7FFF scale and CLIPS instead of
// wrapping (deliberate: a wrapped sample is a full-scale click).  soundfile is absent from this image: restated from
// libsndfile's pcm.c as published, unpinned.  x / 32768 is exact in fp32; y * 32767 is formed in fp64 so that the
// device and the host path (wavio.pcm16_bytes) agree bit for bit, while the host only moves raw 2-byte samples.
namespace {
__global__ __launch_bounds__(256) void pcm16_decode_kernel(const short* __restrict__ in, long in_pitch, float* __restrict__ out,
                                                           long out_pitch, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[(long)blockIdx.y * out_pitch + i] = (float)in[(long)blockIdx.y * in_pitch + i] * (1.f / 32768.f);
}
__global__ __launch_bounds__(256) void pcm16_encode_kernel(const float* __restrict__ in, long in_pitch, short* __restrict__ out,
                                                           long out_pitch, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double v = rint((double)in[(long)blockIdx.y * in_pitch + i] * 32767.0);   // round half to even, like lrint / np.rint
    out[(long)blockIdx.y * out_pitch + i] = (short)fmin(fmax(v, -32768.0), 32767.0);
}
}  // namespace
void launch_pcm16_decode(const short* in, long in_pitch, int batch, int n, float* out, long out_pitch, hipStream_t s) {
    SE_CHECK(batch > 0 && n > 0, "pcm16 decode: bad arguments");
    hipLaunchKernelGGL(pcm16_decode_kernel, dim3((n + 255) / 256, batch), dim3(256), 0, s, in, in_pitch, out, out_pitch, n);
    SE_HIP(hipGetLastError());
}
void launch_pcm16_encode(const float* in, long in_pitch, int batch, int n, short* out, long out_pitch, hipStream_t s) {
    SE_CHECK(batch > 0 && n > 0, "pcm16 encode: bad arguments");
    hipLaunchKernelGGL(pcm16_encode_kernel, dim3((n + 255) / 256, batch), dim3(256), 0, s, in, in_pitch, out, out_pitch, n);
    SE_HIP(hipGetLastError());
}

long resample_out_samples(int n_in, int sr_in, int sr_out) {
    if (sr_in == sr_out) return n_in;
    return (long)std::ceil((double)n_in * ((double)sr_out / sr_in));
}

void launch_resample(const float* x, long in_pitch, int batch, int n_in, int sr_in, int sr_out, float* y, long out_pitch,
                     hipStream_t s) {
    SE_CHECK(sr_in > 0 && sr_out > 0 && n_in > 0 && batch > 0, "resample: bad arguments");
    const ResamplePlan plan = resample_plan(sr_in, sr_out);
    ResampleArgs a{};
    a.x = x; a.in_pitch = in_pitch; a.n_in = n_in; a.y = y; a.out_pitch = out_pitch;
    a.n_calc = (int)((double)n_in * plan.ratio);                    // resampy: int(shape * sample_ratio)
    a.n_out = (int)resample_out_samples(n_in, sr_in, sr_out);
    a.scale = plan.scale; a.index_step = plan.index_step; a.inc = plan.inc;
    {
        ResampleTables& T = resample_tables();
        std::lock_guard<std::mutex> lock(T.mu);
        RatioTables* R = ratio_tables(T, plan, sr_in, sr_out);
        a.win = R->win;
        // (integer decimation: t * inc is exact, the same values as the running sum)
        a.treg = (plan.exact || a.n_calc <= 0) ? nullptr : ratio_positions(R, plan, (size_t)a.n_calc);
    }
    hipLaunchKernelGGL(resample_kernel, dim3((a.n_out + 255) / 256, batch), dim3(256), 0, s, a);
    SE_HIP(hipGetLastError());
}

// ---- se_resample_ragged: rows of different lengths in one call (sizes, refusals and the split over launches: resample_ragged.h)
namespace {

// a row of raw PCM_16 samples read as pcm16_decode_kernel would have written it: x / 32768, exact in fp32
struct ClipAtS16 {
    const short* __restrict__ x;
    __device__ float operator()(int p) const { return (float)x[p] * (1.f / 32768.f); }
};

struct RaggedArgs {
    const void* x; long in_pitch;                 // row 0 of THIS launch
    float* y; long out_pitch;
    const double* win;
    const double* treg;      // [>= the longest row's n_calc] read positions shared by all rows, or nullptr -> t * inc exactly
    double inc, scale;
    int index_step;
    int n_out_max;           // every row is written up to here: its outputs, then zeros
    int pass;                // sr_in == sr_out: y[t] = x[t]
    int n_in[RS_RAGGED_ROWS], n_calc[RS_RAGGED_ROWS];
};

// grid (blocks of outputs, rows of the launch): each row under its own n_in and n_calc; the blocks (and threads) behind a row's
// computed samples write its zeros - the fix_length tail and the padding up to the longest row's output alike
template <typename X, typename S>
__global__ __launch_bounds__(RS_RAGGED_BLOCK) void resample_ragged_kernel(const RaggedArgs a) {
    const long tl = (long)blockIdx.x * RS_RAGGED_BLOCK + threadIdx.x;
    if (tl >= a.n_out_max) return;
    const int t = (int)tl;
    const int row = blockIdx.y;
    float* yp = a.y + (long)row * a.out_pitch;
    if (t >= a.n_calc[row]) {
        yp[t] = 0.f;
        return;
    }
    const X x{static_cast<const S*>(a.x) + (long)row * a.in_pitch};
    if (a.pass) {
        yp[t] = x(t);
        return;
    }
    const double tr = a.treg ? a.treg[t] : (double)t * a.inc;
    const int n = (int)tr;
    yp[t] = (float)resample_taps(x, a.win, n, tr - n, a.n_in[row], a.scale, a.index_step);
}

}  // namespace

void launch_resample_ragged(const void* x, int in_format, long in_pitch, int batch, const int32_t* n_in, int sr_in, int sr_out, float* y,
                            long out_pitch, hipStream_t s) {
    const std::string fn = "se_resample_ragged: ";
    RaggedPlan p{};
    const std::string why = ragged_plan(RaggedCall{x != nullptr, y != nullptr, in_format, in_pitch, batch, n_in, sr_in, sr_out, out_pitch}, p);
    SE_CHECK(why.empty(), fn + why);
    RaggedArgs a{};
    a.y = y; a.in_pitch = in_pitch; a.out_pitch = out_pitch;
    a.n_out_max = p.n_out_max; a.pass = p.pass;
    a.inc = p.plan.inc; a.scale = p.plan.scale; a.index_step = p.plan.index_step;
    ResampleTables& T = resample_tables();
    std::lock_guard<std::mutex> lock(T.mu);
    if (!p.pass) {
        RatioTables* R = ratio_tables(T, p.plan, sr_in, sr_out);
        a.win = R->win;
        if (!p.plan.exact && p.n_calc_max > 0) {
            // resampy advances the read position by repeated float64 addition: the sum is carried on from where it stopped
            const size_t want = std::max<size_t>((size_t)p.n_calc_max, R->dev_cap);
            ragged_positions_extend(p.plan, R->tr, R->acc, (int64_t)want);
            for (int b = 0; b < batch; ++b) {                       // the last position a row reads at lies inside the row
                const RaggedRow r = ragged_row(p, n_in[b]);
                SE_CHECK(r.n_calc == 0 || (int64_t)R->tr[(size_t)r.n_calc - 1] < r.n_in, fn + "a read position past the end of row " + std::to_string(b));
            }
            a.treg = ratio_positions(R, p.plan, (size_t)p.n_calc_max);
        }
    }
    // ---- every refusal is above
    const size_t esz = in_format == RS_SAMPLES_S16 ? sizeof(short) : sizeof(float);
    const dim3 block(RS_RAGGED_BLOCK);
    for (int k = 0; k < p.launches; ++k) {
        int32_t row0 = 0, rows = 0;
        ragged_launch_rows(batch, k, row0, rows);
        a.x = static_cast<const char*>(x) + (size_t)row0 * (size_t)in_pitch * esz;
        a.y = y + (size_t)row0 * (size_t)out_pitch;
        for (int r = 0; r < rows; ++r) {
            const RaggedRow rr = ragged_row(p, n_in[row0 + r]);
            a.n_in[r] = rr.n_in;
            a.n_calc[r] = rr.n_calc;
        }
        const dim3 grid((unsigned)(((long)p.n_out_max + RS_RAGGED_BLOCK - 1) / RS_RAGGED_BLOCK), (unsigned)rows);
        if (in_format == RS_SAMPLES_S16) hipLaunchKernelGGL((resample_ragged_kernel<ClipAtS16, short>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((resample_ragged_kernel<ClipAt, float>), grid, block, 0, s, a);
        SE_HIP(hipGetLastError());
    }
}

// ---- the stateful resampler (se_resampler_* of include/se_engine.h; layout and rules in the header comment of this file)

// A parked signal (parked.h): the host record (resampler_manifest.h) + one device payload, the rows' live history back to back.  The
// payload is sized by the first save for the most a signal of that batch keeps (batch x pitch_ floats), so saving again allocates nothing.
struct ResamplerState : Parked {
    ResamplerManifest man;
    float* rows() const { return reinterpret_cast<float*>(side->dev.get()); }
    int64_t dev_cap() const { return has_payload() ? (int64_t)(side->bytes / sizeof(float)) : 0; }      // floats
    // a payload of at least `floats` on `dev` (current); the old contents are dropped when a new buffer is made
    void payload_alloc(int64_t floats, int dev) {
        if (!(has_payload() && device == dev && dev_cap() >= floats)) fresh_payload((size_t)floats * sizeof(float), dev);
    }
    // ... that holds the imported image: once, until the object is saved into again
    void to_device(int64_t floats, int dev) {
        if (on_device(dev)) return;
        payload_alloc(floats, dev);
        upload_host();
    }
};

class StreamResampler {
  public:
    StreamResampler(int sr_in, int sr_out, int max_batch, int max_push);
    void begin(int batch, hipStream_t s);
    int push(const float* in, long in_pitch, int n_new, float* out, long out_pitch, hipStream_t s);
    int flush(float* out, long out_pitch, hipStream_t s);
    void save(ResamplerState& s, hipStream_t st);
    void restore(ResamplerState& s, hipStream_t st);

  private:
    static constexpr int RING = 8;
    void order_behind_last(hipStream_t s);
    void copy_state(const float* src, long src_pitch, float* dst, long dst_pitch, int64_t n_total, int64_t w0, int batch, hipStream_t st);
    const double* upload_positions(ResamplePos& pos, int64_t n_in, int64_t t_end, int64_t count, hipStream_t s);
    void launch(const float* in, long in_pitch, float* out, long out_pitch, int n_total, int w0_next, int t0, int n_calc,
                int n_emit, const double* treg, hipStream_t s);

    int sr_in_, sr_out_, max_batch_, max_push_, dev_ = 0;
    ResamplePlan plan_{};
    bool pass_;                      // sr_in == sr_out: samples are copied through, nothing else is allocated
    long pitch_ = 0;                 // floats per row of a history buffer (2 * reach, rounded up to 4)
    // (owners, hip_owned.h: released with the object, also when the constructor throws half way)
    DevBuf<float> hist_[2];
    DevBuf<double> win_;             // the table, scaled by the ratio when downsampling
    PinnedBuf<double> ring_host_;    // pinned [RING][ring_cap_]
    DevBuf<double> ring_dev_;        // device [RING][ring_cap_]
    long ring_cap_ = 0;              // the most outputs one push or the flush can release
    Event ring_ev_[RING];
    int ring_next_ = 0;
    Event ev_order_;
    bool has_last_ = false;
    hipStream_t last_st_ = nullptr;
    // the stream: rows, which buffer holds the history, samples arrived, first sample of the history, next output
    bool active_ = false;
    bool ended_ = false;             // the last signal was flushed and none has begun since (what a refused save says)
    int batch_ = 0, cur_ = 0, w0_ = 0;
    int64_t n_total_ = 0;
    ResamplePos pos_;
};

StreamResampler::StreamResampler(int sr_in, int sr_out, int max_batch, int max_push)
    : sr_in_(sr_in), sr_out_(sr_out), max_batch_(max_batch), max_push_(max_push), pass_(sr_in == sr_out) {
    SE_CHECK(sr_in > 0 && sr_out > 0 && max_batch > 0 && max_push > 0, "se_resampler_create: bad arguments");
    plan_ = resample_plan(sr_in, sr_out);
    SE_CHECK(pass_ || plan_.index_step > 0, "se_resampler_create: sr_out / sr_in below the table's resolution");
    SE_HIP(hipGetDevice(&dev_));
    if (pass_) return;
    const long hist = 2L * plan_.reach;
    pitch_ = (hist + 3) / 4 * 4;
    SE_CHECK((double)max_batch * (double)pitch_ < 1e9, "se_resampler_create: max_batch too large");
    for (auto& h : hist_) h.alloc((size_t)max_batch * pitch_);
    std::vector<double> w = build_window();
    if (plan_.ratio < 1.0)
        for (auto& v : w) v *= plan_.ratio;                         // interp_win *= sample_ratio
    win_.alloc(RS_NWIN);
    SE_HIP(hipMemcpy(win_.get(), w.data(), RS_NWIN * sizeof(double), hipMemcpyHostToDevice));
    ring_cap_ = (long)std::ceil((double)std::max(max_push, plan_.reach + 1) * plan_.ratio) + 2;
    if (!plan_.exact) {
        ring_host_.alloc((size_t)ring_cap_ * RING);
        ring_dev_.alloc((size_t)ring_cap_ * RING);
    }
}

// a call on ANOTHER hipStream than the last one re-uses the history buffers: it is ordered behind the work in flight there
void StreamResampler::order_behind_last(hipStream_t s) {
    if (has_last_ && last_st_ != s) SE_HIP(hipStreamWaitEvent(s, ev_order_.get(), 0));
}

void StreamResampler::begin(int batch, hipStream_t s) {
    SE_CHECK(batch >= 1 && batch <= max_batch_, "se_resampler_begin: batch " + std::to_string(batch) + " outside 1..max_batch (" +
                                                    std::to_string(max_batch_) + ")");
    if (!pass_) {
        DeviceScope ds(dev_);
        order_behind_last(s);
    }
    active_ = true;
    ended_ = false;
    batch_ = batch;
    cur_ = w0_ = 0;
    n_total_ = 0;
    pos_ = ResamplePos{};
}

// the read positions of the next `count` outputs, host -> device through the next pinned slot; `pos` moves past them
const double* StreamResampler::upload_positions(ResamplePos& pos, int64_t n_in, int64_t t_end, int64_t count, hipStream_t s) {
    const int slot = ring_next_;
    ring_next_ = (slot + 1) % RING;
    SE_HIP(hipEventSynchronize(ring_ev_[slot].get()));      // the copy that last used this slot has run (no-op when unused)
    double* h = ring_host_.get() + (size_t)slot * ring_cap_;
    double* d = ring_dev_.get() + (size_t)slot * ring_cap_;
    const int64_t k = resample_advance(plan_, pos, n_in, t_end, h, count);
    SE_CHECK(k == count, "resampler: position count changed between two walks");
    SE_HIP(hipMemcpyAsync(d, h, sizeof(double) * count, hipMemcpyHostToDevice, s));
    SE_HIP(hipEventRecord(ring_ev_[slot].get(), s));
    return d;
}

void StreamResampler::launch(const float* in, long in_pitch, float* out, long out_pitch, int n_total, int w0_next, int t0,
                             int n_calc, int n_emit, const double* treg, hipStream_t s) {
    ResampleStreamArgs a{};
    a.hist = hist_[cur_].get(); a.hist_next = hist_[cur_ ^ 1].get(); a.hist_pitch = pitch_;
    a.in = in; a.in_pitch = in_pitch; a.y = out; a.out_pitch = out_pitch;
    a.win = win_.get(); a.treg = treg; a.inc = plan_.inc; a.scale = plan_.scale; a.index_step = plan_.index_step;
    a.w0 = w0_; a.split = (int)n_total_; a.n_total = n_total; a.w0_next = w0_next;
    a.t0 = t0; a.n_calc = n_calc; a.n_emit = n_emit;
    a.out_blocks = (n_emit + RS_STREAM_BLOCK - 1) / RS_STREAM_BLOCK;
    const int keep = n_total - w0_next;
    // what the kernel indexes, checked where the sizes are known: the history it reads, the history it writes
    SE_CHECK(w0_ >= 0 && a.split - w0_ <= pitch_ && w0_next >= w0_ && keep >= 0 && keep <= pitch_, "resampler: window out of range");
    const int blocks = a.out_blocks + (keep + RS_STREAM_BLOCK - 1) / RS_STREAM_BLOCK;
    if (blocks == 0) return;
    hipLaunchKernelGGL(resample_stream_kernel, dim3(blocks, batch_), dim3(RS_STREAM_BLOCK), 0, s, a);
    SE_HIP(hipGetLastError());
}

int StreamResampler::push(const float* in, long in_pitch, int n_new, float* out, long out_pitch, hipStream_t s) {
    // every refusal comes before the first change of state
    SE_CHECK(active_, "se_resampler_push without se_resampler_begin");
    SE_CHECK(n_new >= 0 && n_new <= max_push_, "se_resampler_push: " + std::to_string(n_new) + " samples in one push, the object takes 0..max_push (" +
                                                   std::to_string(max_push_) + ")");
    SE_CHECK(in && out, "null argument");
    SE_CHECK(batch_ == 1 || in_pitch >= n_new, "input row pitch too small");
    const int64_t n_after = n_total_ + n_new;
    SE_CHECK(n_after <= INT_MAX && std::ceil((double)n_after * plan_.ratio) <= (double)INT_MAX,
             "se_resampler_push: the stream would pass the " + std::to_string(INT_MAX) + " samples (in or out) se_resample accepts");
    if (n_new == 0) return 0;
    if (pass_) {
        SE_CHECK(batch_ == 1 || out_pitch >= n_new, "output row pitch too small");
        SE_HIP(hipMemcpy2DAsync(out, sizeof(float) * (batch_ == 1 ? n_new : out_pitch), in, sizeof(float) * (batch_ == 1 ? n_new : in_pitch),
                                sizeof(float) * n_new, batch_, hipMemcpyDeviceToDevice, s));
        n_total_ = n_after;
        return n_new;
    }
    ResamplePos pos = pos_;
    const int64_t count = resample_advance(plan_, pos, n_after, INT64_MAX, nullptr, 0);
    SE_CHECK(count <= ring_cap_, "resampler: a push released more outputs than planned");
    SE_CHECK(batch_ == 1 || out_pitch >= count, "output row pitch too small");
    // the oldest tap of the first output lies inside the history
    SE_CHECK(count == 0 || std::max<int64_t>(0, (int64_t)resample_pos_of(plan_, pos_) - (plan_.reach - 2)) >= w0_,
             "resampler: history too short");
    DeviceScope ds(dev_);
    order_behind_last(s);
    const double* treg = nullptr;
    if (!plan_.exact && count > 0) {
        pos = pos_;
        treg = upload_positions(pos, n_after, INT64_MAX, count, s);
    }
    // (never below the origin the history has: w0_ is 0 from begin, so this is max(0, .) for a signal fed from its start; a signal
    // rebased by se_resampler_state_join may hold a shorter history than 2 * reach and keeps its origin until the window passes it)
    const int w0_next = (int)std::max<int64_t>(w0_, n_after - 2L * plan_.reach);
    launch(in, in_pitch, out, out_pitch, (int)n_after, w0_next, (int)pos_.t, (int)count, (int)count, treg, s);
    SE_HIP(hipEventRecord(ev_order_.get(), s));
    has_last_ = true;
    last_st_ = s;
    cur_ ^= 1;
    w0_ = w0_next;
    n_total_ = n_after;
    pos_ = pos;
    return (int)count;
}

int StreamResampler::flush(float* out, long out_pitch, hipStream_t s) {
    SE_CHECK(active_, "se_resampler_flush without se_resampler_begin");
    if (pass_ || n_total_ == 0) {
        active_ = false;
        ended_ = true;
        return 0;
    }
    const int64_t n_calc = resample_calc_samples(plan_, n_total_) - pos_.t;                    // still to compute
    const int64_t n_emit = resample_out_samples((int)n_total_, sr_in_, sr_out_) - pos_.t;      // + the fix_length zero tail
    SE_CHECK(n_calc >= 0 && n_emit >= n_calc && n_emit <= ring_cap_, "resampler: the flush holds more outputs than planned");
    SE_CHECK(out || n_emit == 0, "null argument");
    SE_CHECK(batch_ == 1 || out_pitch >= n_emit, "output row pitch too small");
    SE_CHECK(n_calc == 0 || std::max<int64_t>(0, (int64_t)resample_pos_of(plan_, pos_) - (plan_.reach - 2)) >= w0_,
             "resampler: history too short");
    // every remaining output reads at a position inside the signal: n + reach < n_total_ + reach
    const int64_t n_lim = n_total_ + plan_.reach;
    ResamplePos pos = pos_;
    SE_CHECK(resample_advance(plan_, pos, n_lim, pos_.t + n_calc, nullptr, 0) == n_calc, "resampler: a read position past the end");
    DeviceScope ds(dev_);
    order_behind_last(s);
    const double* treg = nullptr;
    if (!plan_.exact && n_calc > 0) {
        pos = pos_;
        treg = upload_positions(pos, n_lim, pos_.t + n_calc, n_calc, s);
    }
    // the right wing is clamped by n_total_, now the final length; no history is written (w0_next = n_total_)
    launch(nullptr, 0, out, out_pitch, (int)n_total_, (int)n_total_, (int)pos_.t, (int)n_calc, (int)n_emit, treg, s);
    SE_HIP(hipEventRecord(ev_order_.get(), s));
    has_last_ = true;
    last_st_ = s;
    active_ = false;
    ended_ = true;
    return (int)n_emit;
}

// ---- se_resampler_save / se_resampler_restore.  What a later output depends on: the history, read by absolute position
// (hist[p - w0]); the read positions, resample_advance from (t, acc); the wings, clamped by absolute position (n + 1 and n_total).
// So a snapshot is (w0, n_total, t, acc) + samples [w0, n_total) of every row, and it does not matter which of the two buffers
// they come back into: restore writes the current one, column 0 = sample w0 as a push leaves it.
void StreamResampler::copy_state(const float* src, long src_pitch, float* dst, long dst_pitch, int64_t n_total, int64_t w0, int batch,
                                 hipStream_t st) {
    const int64_t keep = n_total - w0;
    // what the kernel indexes, checked where the sizes are known: rows of the history buffer, rows of the payload
    SE_CHECK(keep >= 0 && keep <= pitch_ && keep == n_total_ - w0_ && batch >= 1 && batch <= max_batch_ && batch == batch_ &&
                 keep <= std::min(src_pitch, dst_pitch),
             "resampler state: history out of range");
    if (keep == 0) return;
    hipLaunchKernelGGL(resampler_state_copy_kernel, dim3((unsigned)((keep + 255) / 256), batch), dim3(256), 0, st, src, src_pitch, dst,
                       dst_pitch, (int)keep);
    SE_HIP(hipGetLastError());
}

void StreamResampler::save(ResamplerState& s, hipStream_t st) {
    SE_CHECK(!ended_ || active_, "se_resampler_save after se_resampler_flush: the signal has ended");
    SE_CHECK(active_, "se_resampler_save without se_resampler_begin");
    ResamplerManifest m;
    m.sr_in = sr_in_;
    m.sr_out = sr_out_;
    m.batch = batch_;
    m.n_total = n_total_;
    // (a pass-through signal keeps no history and releases what it receives)
    m.w0 = pass_ ? n_total_ : w0_;
    m.t = pass_ ? n_total_ : pos_.t;
    m.acc_bits = rsnap_bits_of(pass_ ? 0.0 : pos_.acc);
    const std::string why = rsnap_check(m);
    SE_CHECK(why.empty(), "se_resampler_save: " + why);
    if (!pass_) {
        SE_CHECK(rsnap_keep(m) <= pitch_, "se_resampler_save: more live history than a buffer row");
        DeviceScope ds(dev_);
        s.payload_alloc((int64_t)batch_ * pitch_, dev_);
        // nothing of the object or the signal has changed up to here (a payload made anew held nothing valid for this signal)
        order_behind_last(st);
        s.wait(st);
        const long keep = (long)rsnap_keep(m);
        copy_state(hist_[cur_].get(), pitch_, s.rows(), keep, n_total_, w0_, batch_, st);
        SE_HIP(hipEventRecord(ev_order_.get(), st));
        has_last_ = true;
        last_st_ = st;
        s.mark(st);
    }
    s.man = m;
    s.set_saved(!pass_);
}

void StreamResampler::restore(ResamplerState& s, hipStream_t st) {
    const std::string fn = "se_resampler_restore: ";
    SE_CHECK(s.filled, fn + "the resampler state object is empty");
    const ResamplerManifest& m = s.man;
    SE_CHECK(m.sr_in == sr_in_ && m.sr_out == sr_out_, fn + "the snapshot was taken at " + std::to_string(m.sr_in) + " -> " + std::to_string(m.sr_out) +
                                                           " Hz, this object converts " + std::to_string(sr_in_) + " -> " + std::to_string(sr_out_) + " Hz");
    SE_CHECK(m.batch >= 1 && m.batch <= max_batch_, fn + "snapshot of " + std::to_string(m.batch) + " rows exceeds max_batch " +
                                                        std::to_string(max_batch_) + " given at create");
    const int64_t keep = rsnap_keep(m);
    SE_CHECK(keep >= 0 && keep <= pitch_ && m.n_total <= INT_MAX && m.t <= INT_MAX, fn + "history or counters out of range");
    const bool upload = keep > 0 && !s.on_device(dev_);
    if (upload)
        SE_CHECK((int64_t)s.host.size() == rsnap_payload_bytes(m),
                 fn + "the payload lives on device " + std::to_string(s.device) + ", this object on device " + std::to_string(dev_) +
                     " (export the state and import it to move it)");
    // ---- every refusal is above: from here the call replaces whatever signal is open, as se_resampler_begin does
    if (upload) {             // an imported image, or one that moves to this device: once, until the object is saved into again
        DeviceScope ds(dev_);
        s.to_device((int64_t)m.batch * pitch_, dev_);
    }
    active_ = true;
    ended_ = false;
    batch_ = m.batch;
    w0_ = (int)m.w0;
    n_total_ = m.n_total;
    pos_.t = m.t;
    pos_.acc = rsnap_double_of(m.acc_bits);
    if (keep > 0) {
        DeviceScope ds(dev_);
        order_behind_last(st);
        s.wait(st);
        copy_state(s.rows(), (long)keep, hist_[cur_].get(), pitch_, n_total_, w0_, batch_, st);
        SE_HIP(hipEventRecord(ev_order_.get(), st));
        has_last_ = true;
        last_st_ = st;
        s.mark(st);
    }
}

ResamplerState* resampler_state_create() { return new ResamplerState(); }
void resampler_state_destroy(ResamplerState* s) {
    if (!s) return;
    std::unique_ptr<ResamplerState> own(s);
    s->drop_side();
}
int64_t resampler_state_bytes(const ResamplerState* s) {
    if (!s || !s->filled || s->man.sr_in == s->man.sr_out) return 0;
    return s->has_payload() ? (int64_t)s->side->bytes : rsnap_payload_bytes(s->man);
}
void resampler_state_counts(const ResamplerState* s, int32_t* sr_in, int32_t* sr_out, int32_t* batch, int64_t* n_in, int64_t* n_out) {
    SE_CHECK(s, "se_resampler_state_counts: null argument");
    SE_CHECK(s->filled, "se_resampler_state_counts: the resampler state object is empty");
    if (sr_in) *sr_in = s->man.sr_in;
    if (sr_out) *sr_out = s->man.sr_out;
    if (batch) *batch = s->man.batch;
    if (n_in) *n_in = s->man.n_total;
    if (n_out) *n_out = s->man.t;
}
void stream_resampler_save(StreamResampler* r, ResamplerState* s, hipStream_t st) { r->save(*s, st); }
void stream_resampler_restore(StreamResampler* r, ResamplerState* s, hipStream_t st) { r->restore(*s, st); }

int64_t resampler_state_export(const ResamplerState* s, void* host_buf, int64_t cap) {
    SE_CHECK(s, "se_resampler_state_export: null argument");
    SE_CHECK(s->filled, "se_resampler_state_export: the resampler state object is empty");
    const int64_t size = rsnap_image_bytes(s->man), pay = rsnap_payload_bytes(s->man);
    if (cap == 0) return size;
    SE_CHECK(host_buf && cap >= size, "se_resampler_state_export: the buffer holds " + std::to_string(cap) + " bytes, the image needs " + std::to_string(size));
    uint8_t* out = static_cast<uint8_t*>(host_buf);
    rsnap_write_head(s->man, out);
    if (pay == 0) return size;
    if (!s->host.empty()) SE_CHECK((int64_t)s->host.size() == pay, "se_resampler_state_export: host image of the wrong size");
    else SE_CHECK(s->resident() && pay <= (int64_t)s->side->bytes, "se_resampler_state_export: no payload");
    const_cast<ResamplerState*>(s)->export_payload(out + RSNAP_HEAD_BYTES, (size_t)pay);      // (the event is a cache of the object)
    return size;
}

void resampler_state_import(ResamplerState* s, const void* host_buf, int64_t bytes) {
    SE_CHECK(s && host_buf, "se_resampler_state_import: null argument");
    ResamplerManifest m;
    int64_t off = 0;
    const std::string why = rsnap_parse(host_buf, bytes, m, off);
    SE_CHECK(why.empty(), "se_resampler_state_import: " + why);
    std::vector<uint8_t> pay(static_cast<const uint8_t*>(host_buf) + off, static_cast<const uint8_t*>(host_buf) + bytes);
    // nothing of the object has changed up to here
    s->man = m;
    s->adopt_image(std::move(pay));
}

// ---- se_resampler_state_select / _concat / _join.  The rows of the result, in order, as (part, row); every refusal is made by the
// callers and here before the destination changes.  Sources that are all imported images (host payloads, nothing uploaded yet) are
// cut on the host and the result is such an image; otherwise the rows move on the device the sources live on - a host-only part is
// uploaded there first, as its first restore would do it.
namespace {
// m: the record of the result, its rows rsnap_keep(m) floats long.  Row j <- that many floats of row map[j].y of part map[j].x, from
// column col[part] on: a part's packed rows have the length of its own record (select and concat: the result's, and column 0)
void resampler_rows(ResamplerState* dst, const std::vector<ResamplerState*>& parts, const std::vector<int2>& map, const ResamplerManifest& m,
                    const std::vector<int64_t>& col, const std::string& fn, hipStream_t st) {
    const int64_t keep = rsnap_keep(m);
    if (keep == 0) {      // pass-through, or nothing live: counters only
        dst->man = m;
        dst->set_saved(false);
        return;
    }
    SE_CHECK(keep <= INT_MAX / 4, fn + "history out of range");
    int dev = -1;
    for (ResamplerState* p : parts)
        if (p->resident()) {
            SE_CHECK(dev < 0 || dev == p->device, fn + "the parts' payloads live on devices " + std::to_string(dev) + " and " + std::to_string(p->device) +
                                                      " (export and import a state to move it)");
            dev = p->device;
        }
    for (ResamplerState* p : parts)
        if (!p->resident()) SE_CHECK((int64_t)p->host.size() == rsnap_payload_bytes(p->man), fn + "a part has no payload");
        else SE_CHECK(p->dev_cap() >= (int64_t)p->man.batch * rsnap_keep(p->man), fn + "a part's payload is smaller than its rows");
    // ---- every refusal is above
    auto row_at = [&](size_t j) {      // where row j of the result starts in its part's payload, in floats
        const size_t p = (size_t)map[j].x;
        return (size_t)map[j].y * (size_t)rsnap_keep(parts[p]->man) + (size_t)col[p];
    };
    if (dev < 0) {
        std::vector<uint8_t> out((size_t)(m.batch * keep * 4));
        for (size_t j = 0; j < map.size(); ++j)
            std::memcpy(out.data() + j * (size_t)keep * 4, parts[(size_t)map[j].x]->host.data() + row_at(j) * 4, (size_t)keep * 4);
        dst->drop_side();
        dst->man = m;
        dst->adopt_image(std::move(out));
        return;
    }
    DeviceScope ds(dev);
    for (ResamplerState* p : parts) p->to_device((int64_t)p->man.batch * rsnap_keep(p->man), dev);
    dst->payload_alloc((int64_t)m.batch * keep, dev);
    for (ResamplerState* p : parts) p->wait(st);
    dst->wait(st);
    for (size_t y0 = 0; y0 < map.size(); y0 += 64) {
        const int ny = (int)std::min<size_t>(64, map.size() - y0);
        RowPtrs rp{};
        for (int y = 0; y < ny; ++y) rp.src[y] = parts[(size_t)map[y0 + y].x]->rows() + row_at(y0 + y);
        hipLaunchKernelGGL(resampler_state_gather_kernel, dim3((unsigned)((keep + 255) / 256), (unsigned)ny), dim3(256), 0, st, rp,
                           dst->rows() + y0 * (size_t)keep, (int)keep);
        SE_HIP(hipGetLastError());
    }
    dst->man = m;
    dst->set_saved();
    dst->mark(st);
    for (ResamplerState* p : parts) p->mark(st);
}
}  // namespace

void resampler_state_select(ResamplerState* dst, ResamplerState* src, const int32_t* rows, int32_t n_rows, hipStream_t st) {
    const std::string fn = "se_resampler_state_select: ";
    SE_CHECK(dst && src, fn + "null argument");
    SE_CHECK(dst != src, fn + "dst == src: the rows are read while they are written");
    SE_CHECK(src->filled, fn + "the resampler state object is empty");
    const std::string bad = rsnap_rows_check(rows, n_rows, src->man.batch);
    SE_CHECK(bad.empty(), fn + bad);
    std::vector<int2> map;
    for (int32_t j = 0; j < n_rows; ++j) map.push_back(make_int2(0, rows[j]));
    ResamplerManifest m = src->man;
    m.batch = n_rows;
    resampler_rows(dst, {src}, map, m, {0}, fn, st);
}

void resampler_state_concat(ResamplerState* dst, ResamplerState* const* cparts, int32_t n_parts, hipStream_t st) {
    const std::string fn = "se_resampler_state_concat: ";
    SE_CHECK(dst && cparts, fn + "null argument");
    const std::vector<ResamplerState*> parts = collect_parts(dst, cparts, n_parts, fn, "resampler state", [&](int32_t p, const ResamplerState* s) {
        const std::string why = p > 0 ? rsnap_concat_differs(cparts[0]->man, s->man) : "";
        SE_CHECK(why.empty(), fn + "parts[0] and parts[" + std::to_string(p) + "] differ: " + why);
    });
    const std::vector<int2> map = part_rows(parts);
    ResamplerManifest m = parts[0]->man;
    m.batch = (int32_t)map.size();
    resampler_rows(dst, parts, map, m, std::vector<int64_t>(parts.size(), 0), fn, st);
}

// ---- se_resampler_state_join: concat for parts whose counters differ by a multiple of sr_in / sr_out (resampler_join.h: when a parked
// signal can be rebased, the shifts, the joined history origin and the column of each part's rows it starts at).  The parts' packed
// rows differ in length; everything else - where the result lives, the upload of imported parts, the reuse of dst and the ordering on
// `st` - is concat's, in the same mover.  Every refusal is made before the destination changes.
void resampler_state_join(ResamplerState* dst, ResamplerState* const* cparts, int32_t n_parts, hipStream_t st) {
    const std::string fn = "se_resampler_state_join: ";
    SE_CHECK(dst && cparts, fn + "null argument");
    std::vector<const ResamplerManifest*> mans;
    const std::vector<ResamplerState*> parts =
        collect_parts(dst, cparts, n_parts, fn, "resampler state", [&](int32_t, const ResamplerState* s) { mans.push_back(&s->man); });
    const std::vector<int2> map = part_rows(parts);
    ResamplerJoinPlan plan;
    const std::string why = rsnap_join_plan(mans, plan);
    SE_CHECK(why.empty(), fn + why);
    const ResamplerManifest m = rsnap_joined(parts[0]->man, plan, (int32_t)map.size());
    const std::string bad = rsnap_check(m);
    SE_CHECK(bad.empty(), fn + bad);
    const int64_t live = plan.live;
    SE_CHECK(live == rsnap_keep(m) && live <= INT_MAX / 4, fn + "history out of range");
    for (size_t p = 0; p < parts.size(); ++p)       // what the gather indexes: columns [col, col + live) of rows of the part's own length
        SE_CHECK(plan.col[p] >= 0 && plan.col[p] + live == rsnap_keep(parts[p]->man), fn + "history out of range");
    resampler_rows(dst, parts, map, m, plan.col, fn, st);
}

StreamResampler* stream_resampler_create(int sr_in, int sr_out, int max_batch, int max_push) {
    return new StreamResampler(sr_in, sr_out, max_batch, max_push);
}
void stream_resampler_destroy(StreamResampler* r) { delete r; }
void stream_resampler_begin(StreamResampler* r, int batch, hipStream_t s) { r->begin(batch, s); }
int stream_resampler_push(StreamResampler* r, const float* in, long in_pitch, int n_new, float* out, long out_pitch, hipStream_t s) {
    return r->push(in, in_pitch, n_new, out, out_pitch, s);
}
int stream_resampler_flush(StreamResampler* r, float* out, long out_pitch, hipStream_t s) { return r->flush(out, out_pitch, s); }
long resample_ready_samples(long n_in, int sr_in, int sr_out) {
    if (n_in < 0 || sr_in <= 0 || sr_out <= 0) return -1;
    if (sr_in == sr_out) return n_in;
    const ResamplePlan p = resample_plan(sr_in, sr_out);
    return p.index_step > 0 ? (long)resample_ready(p, n_in) : -1;
}

}  // namespace se
