// Framed STFT / iSTFT-OLA for gfx950.
//
// Reference behaviour (file:line in /root/reference):
//   torch.stft(x, n_fft, hop, win, window=torch.hann_window(win))   DCCRN/dccrn_decode_vb.py:37-38,
//       FullSubNet/fullsubnet_sa_decode_vb.py:46-47, CTSNet/two_stage_com_decode_vb.py:70-71,
//       TaylorSENet/taylorsenet_decode_vb.py:36-37, Uformer/uformer.py:178,182
//   librosa.stft(x, n_fft=320, hop_length=160, window='hanning')    LSTM/lstm_decode_vb.py:37, CRN/crn_decode_vb.py:36,
//       GCRN/gcrn_decode_vb.py:37, DPCRN/dpcrn_decode_vb.py:37, G2Net_VB/com_decode.py:49
//   torch.istft / librosa.istft with Hann synthesis window, window-sum-square normalisation, `length=`.
// Both front ends are centre=True / reflect pad n_fft/2 / periodic Hann / one-sided.
//
// This file holds the launchers, the per-utterance RMS scale and the stage profiler; the transforms themselves (FFT
// points in registers) are in k_stft2.hip.
#include "kernels.h"
#include "common.h"
#include "fe_launch.h"
#include <algorithm>

namespace se {

static thread_local const Ragged* g_ragged = nullptr;
const Ragged* ragged_ctx() { return g_ragged; }
void set_ragged_ctx(const Ragged* r) { g_ragged = r; }

static thread_local std::vector<FeLaunchRec>* g_fe_log = nullptr;
void fe_set_launch_log(std::vector<FeLaunchRec>* log) { g_fe_log = log; }
std::vector<FeLaunchRec>* fe_launch_log() { return g_fe_log; }

static thread_local StageProf* g_stage_prof = nullptr;
StageProf* stage_prof() { return g_stage_prof; }
void set_stage_prof(StageProf* p) { g_stage_prof = p; }
void StageProf::begin(int stage, hipStream_t st) {
    Slot& s = slot[stage];
    if (s.used + 2 > s.ev.size())
        for (int i = 0; i < 2; ++i) {
            hipEvent_t e;
            SE_HIP(hipEventCreate(&e));
            s.ev.push_back(e);
        }
    SE_HIP(hipEventRecord(s.ev[s.used], st));
}
void StageProf::end(int stage, hipStream_t st, double bytes) {
    Slot& s = slot[stage];
    SE_HIP(hipEventRecord(s.ev[s.used + 1], st));
    s.used += 2;
    s.bytes += bytes;
    s.launches += 1;
}
void StageProf::reset() {
    for (auto& s : slot) {
        s.used = 0;
        s.bytes = 0.0;
        s.launches = 0;
    }
}
double StageProf::ms(int stage) {
    Slot& s = slot[stage];
    double tot = 0.0;
    for (size_t i = 0; i + 1 < s.used; i += 2) {
        SE_HIP(hipEventSynchronize(s.ev[i + 1]));
        float m = 0.f;
        SE_HIP(hipEventElapsedTime(&m, s.ev[i], s.ev[i + 1]));
        tot += m;
    }
    return tot;
}
StageProf::~StageProf() {
    for (auto& s : slot)
        for (auto e : s.ev) (void)hipEventDestroy(e);
}

// c[b] = sqrt(L / sum x^2) in two steps: RMS_SPLIT blocks per utterance each sum a slice in fp64 (one block per utterance
// pulled 256 kB through a single CU: 100 us flat whatever the batch), then one thread per utterance adds the slices in
// slice order - deterministic, no atomics.
constexpr int RMS_SPLIT = 16;
__global__ __launch_bounds__(256) void rms_partial_kernel(const float* __restrict__ wav, int L, long pitch,
                                                          double* __restrict__ part, const int* __restrict__ len) {
    const int b = blockIdx.y, k = blockIdx.x;
    if (len) L = len[b];
    const int per = (L + RMS_SPLIT - 1) / RMS_SPLIT;
    const int lo = k * per, hi = min(L, lo + per);
    const float* x = wav + (long)b * pitch;
    double s = 0.0;
    int i = lo + threadIdx.x;
    for (; i + 3 * 256 < hi; i += 4 * 256) {          // four independent loads in flight per thread
        const float v0 = x[i], v1 = x[i + 256], v2 = x[i + 512], v3 = x[i + 768];
        s += (double)v0 * v0;
        s += (double)v1 * v1;
        s += (double)v2 * v2;
        s += (double)v3 * v3;
    }
    for (; i < hi; i += 256) {
        const double v = x[i];
        s += v * v;
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    __shared__ double sh[4];
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[(long)b * RMS_SPLIT + k] = sh[0] + sh[1] + sh[2] + sh[3];
}
__global__ void rms_finish_kernel(const double* __restrict__ part, int L, float* __restrict__ c_out,
                                  const int* __restrict__ len, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    if (len) L = len[b];
    double tot = 0.0;
    for (int k = 0; k < RMS_SPLIT; ++k) tot += part[(long)b * RMS_SPLIT + k];
    c_out[b] = (float)sqrt((double)L / tot);
}

void launch_rms_scale(const float* wav, int B, int L, long pitch, float* c_out, hipStream_t s) {
    const Ragged* rg = ragged_ctx();
    StageScope prof(STAGE_RMS, s, 4.0 * L * B);
    double* part = reinterpret_cast<double*>(device_scratch(3, (size_t)B * RMS_SPLIT * sizeof(double), s));
    hipLaunchKernelGGL(rms_partial_kernel, dim3(RMS_SPLIT, B), dim3(256), 0, s, wav, L, pitch, part, rg ? rg->len : nullptr);
    hipLaunchKernelGGL(rms_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, s, part, L, c_out, rg ? rg->len : nullptr, B);
    SE_HIP(hipGetLastError());
}

void launch_stft(const StftGeom& g, const float* wav, long pitch, int B, int L, int Lpad, const float* c_scale,
                 float p_in, float* spec_ri, float* mag, int T, int Tp, hipStream_t s, int t_first, int col0, int w0,
                 const float* frame_c, int ring) {
    SE_CHECK(t_first >= 0 && t_first < T, "launch_stft: empty frame range");
    SE_CHECK(w0 >= 0 && (w0 == 0 || (long)t_first * g.hop - g.n_fft / 2 >= w0), "launch_stft: frames reach below the sample origin");
    SE_CHECK(g.n_fft == 512 || g.n_fft == 320, "unsupported n_fft (320 and 512 are the reference geometries)");
    StageScope prof(STAGE_STFT, s, 4.0 * L * B + (spec_ri ? 8.0 : 0.0) * g.F() * T * B + (mag ? 4.0 : 0.0) * g.F() * T * B);
    launch_stft2(g, wav, pitch, B, L, Lpad, c_scale, p_in, spec_ri, mag, T, Tp, s, t_first, col0, w0, frame_c, ring);
    // (the record restates launch_stft2's selection from the arguments passed on: k_stft2.hip, 32 frames and 4 waves per block)
    if (std::vector<FeLaunchRec>* log = fe_launch_log()) {
        FeLaunchRec r;
        r.kernel = "stft2"; r.N = g.n_fft; r.MAG = mag != nullptr; r.FSC = frame_c != nullptr; r.CP = p_in == 1.f ? 0 : (p_in == 0.5f ? 1 : 2);
        r.gx = (T - t_first + 31) / 32; r.gy = B; r.block = 256;
        r.shmem = (long)std::max((size_t)4 * g.n_fft * 8, (size_t)g.F() * 33 * 4);
        r.ragged = ragged_ctx() != nullptr;
        log->push_back(r);
    }
}

void launch_istft(const StftGeom& g, const float* spec_ri, int B, int T, int Tp, float* /*frames: unused since the fused kernel*/,
                  const float* c_scale, float* wav_out, long out_pitch, int Lout, hipStream_t s, int t_off, int t_lo, int o_lo,
                  const float* frame_inv, int ring) {
    StageScope prof(STAGE_ISTFT, s, 8.0 * g.F() * T * B + 4.0 * Lout * B);
    SE_CHECK(Lout > o_lo, "launch_istft: empty output range");
    SE_CHECK(g.n_fft == 512 || g.n_fft == 320, "unsupported n_fft");
    launch_istft2(g, spec_ri, B, T, Tp, c_scale, wav_out, out_pitch, Lout, s, t_off, t_lo, o_lo, frame_inv, ring);
    // (as above: 32 frames per block of which `halo` are shared with the block below, 8 waves)
    if (std::vector<FeLaunchRec>* log = fe_launch_log()) {
        FeLaunchRec r;
        int halo = (g.n_fft + g.hop - 1) / g.hop - 1;
        halo += halo & 1;
        const int span = (32 - halo) * g.hop, pos_base = (o_lo + g.n_fft / 2) / g.hop * g.hop;
        r.kernel = "istft2"; r.N = g.n_fft; r.FSC = frame_inv != nullptr;
        r.gx = (g.n_fft / 2 + Lout - pos_base + span - 1) / span; r.gy = B; r.block = 512;
        r.shmem = (long)(std::max((size_t)32 * g.n_fft * 4, (size_t)g.F() * 33 * 4) + (size_t)g.n_fft * 4);
        r.ragged = ragged_ctx() != nullptr;
        log->push_back(r);
    }
}

}  // namespace se
