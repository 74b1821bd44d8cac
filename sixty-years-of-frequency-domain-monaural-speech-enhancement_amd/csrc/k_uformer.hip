// Uformer's private kernels and their launchers (model_uformer.hip calls the launchers; csrc/tests/att_probe.hip calls them one at a
// time for tests/test_gpu_uformer_kernels.py): the polar front / back end (uformer.py:182-210, :236-262), the interaction of the
// two branches (fusion.py:13-19) and the attentions along time and along frequency (t_att_cplx.py, f_att_cplx.py).
#include "k_uformer.h"
#include <algorithm>

namespace se {

namespace {

constexpr int NBIN = 257, HD = 16;
constexpr float UEPS = 1.1920928955078125e-07f;       // torch.finfo(float32).eps (uformer.py:16)

// ---- :187-210  mag = sqrt(clamp(re^2+im^2, EPS)) [**p_in], phase = atan2(im+EPS, re); network inputs drop the DC bin
__global__ __launch_bounds__(256) void uf_prep_kernel(const float* __restrict__ spec, float* __restrict__ mag0,
                                                      float* __restrict__ ph0, float* __restrict__ xc, float* __restrict__ xm,
                                                      int T, float p_in) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int k = blockIdx.y, b = blockIdx.z;
    if (t >= T) return;
    const long plane = (long)NBIN * T;
    const long o = ((long)b * 2 * NBIN + k) * T + t;
    const float re = spec[o], im = spec[o + plane];
    float m = sqrtf(fmaxf(re * re + im * im, UEPS));
    if (p_in != 1.f) m = powf(m, p_in);
    const float ph = atan2f(im + UEPS, re);
    mag0[((long)b * NBIN + k) * T + t] = m;
    ph0[((long)b * NBIN + k) * T + t] = ph;
    if (k > 0) {
        const long q = ((long)b * 2 * (NBIN - 1) + (k - 1)) * T + t;
        xc[q] = m * cosf(ph);
        xc[q + (long)(NBIN - 1) * T] = m * sinf(ph);
        xm[((long)b * (NBIN - 1) + (k - 1)) * T + t] = m;
    }
}

// ---- fusion.py:13-19 on cplx [B][2C][P] / mag [B][C][P], in place
__global__ __launch_bounds__(256) void uf_fusion_kernel(float* __restrict__ cplx, float* __restrict__ mag, long CP) {
    // grid (ceil(CP / 256), B): no 64-bit division per element; hardware exp for the two sigmoids
    const long r = (long)blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (r >= CP) return;
    float* cr = cplx + b * 2 * CP + r;
    float* mp = mag + b * CP + r;
    const float re = cr[0], im = cr[CP], m = mp[0];
    const float cm = sqrtf(fmaxf(re * re + im * im, UEPS));
    const float s = (1.f / (1.f + fm_exp(-m)));
    cr[0] = re + s;
    cr[CP] = im + s;
    mp[0] = m + (1.f / (1.f + fm_exp(-cm)));
}

// ---- attention along T (t_att_cplx.py:15-40, :58-67): pq [B][nh*48][F][T] rows (q,k,v) x 16 per head; online softmax;
// heads are combined with signs into out [B][nout*16][F][T] (complex: heads 0-3 -> real (+,-,-,-), heads 4-7 -> imag
// (+,+,+,-); real: 1 head).  On the matrix cores (v_mfma_f32_16x16x4_f32, exact fp32 products): scores and P.V of a
// 16-query x 16-key tile are 4 + 4 MFMAs instead of 2 x 16 x 16 x 16 VALU FMAs fed by LDS broadcast reads.
//   S^T[key][query] = K[key][:] . Q[query][:]      A = K tile (lane (m = key, g) holds K[key][4j + g]),  B = Q^T
//   O^T[d][query]  += V^T[d][key] . P^T[key][query] A = V^T (lane (m = d, g) holds V[4g + j][d]),          B = P^T
// The accumulator of S^T (lane (n = query, g), register i  <->  key 4g + i) IS the B operand of the second product with
// the key order 4g + j, so the probabilities never leave their registers; the softmax statistics are per query = per
// lane column, reduced over the four 16-lane groups with two cross-lane swaps.  One wave owns QT query tiles, a block
// (4 waves) 64 * QT queries of one (b, f); K ([16][Tk], dim-major) and V ([T][17], key-major) of a head sit in LDS.
typedef float uf_x4 __attribute__((ext_vector_type(4)));
constexpr int UF_QT = 2;
// keys per LDS block (68 KB of K / V per workgroup: two workgroups per CU at any clip length)
constexpr int UF_ATT_KB = 512;
static_assert(((size_t)HD * (UF_ATT_KB + 16) + (size_t)UF_ATT_KB * 17) * sizeof(float) <= 150 * 1024,
              "the time attention's K / V block must fit the LDS");
__global__ __launch_bounds__(256) void uf_att_t_mfma_kernel(const float* __restrict__ pq, float* __restrict__ out, int F,
                                                            int T, int nh, int Tk, int KB, const int* __restrict__ tlen) {
    extern __shared__ float kv[];
    float* Ks = kv;                        // [16][Tk], Tk % 32 == 16: the four dim rows of an A fragment hit distinct banks
    float* Vs = kv + HD * Tk;              // [KB][17]; Tk = KB (+16): one block of KB keys is resident at a time
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 15, g = lane >> 4;
    const int f = blockIdx.x % F, b = blockIdx.x / F;
    const int q0 = blockIdx.y * (64 * UF_QT) + wave * (16 * UF_QT);
    const long P = (long)F * T;
    const float* base = pq + (long)b * nh * 48 * P + (long)f * T;
    const int Tkeys = tlen ? tlen[b] : T;          // ragged batch: a clip attends to its own frames only
    const int nkt = (Tkeys + 15) >> 4;
    const int nks = (T + 15) >> 4;                 // key tiles staged (LDS layout is per launch, not per row)
    uf_x4 accr[UF_QT], acci[UF_QT];
#pragma unroll
    for (int qt = 0; qt < UF_QT; ++qt) accr[qt] = acci[qt] = uf_x4{0.f, 0.f, 0.f, 0.f};
    for (int h = 0; h < nh; ++h) {
        const float* hq = base + (long)h * 48 * P;
        float qf[UF_QT][4], mx[UF_QT], l[UF_QT];
        uf_x4 o[UF_QT];
#pragma unroll
        for (int qt = 0; qt < UF_QT; ++qt) {
            const int t = min(q0 + 16 * qt + n, T - 1);
#pragma unroll
            for (int j = 0; j < 4; ++j) qf[qt][j] = hq[(long)(4 * j + g) * P + t] * 0.25f;      // / hidden_channel ** 0.5
            mx[qt] = -3.0e38f;
            l[qt] = 0.f;
            o[qt] = uf_x4{0.f, 0.f, 0.f, 0.f};
        }
        // keys stream through LDS in blocks of KB (t_att_cplx.py:25 has no length limit): the online-softmax state
        // (mx, l, o) lives in registers across blocks; a clip of <= KB frames is one block, as before.  Frames >= Tkeys are staged as
        // zeros: the last live key tile multiplies them by p = 0, and 0 * NaN is NaN
        for (int kb0 = 0; kb0 < nkt * 16; kb0 += KB) {
        const int kbn = min(KB, nks * 16 - kb0);           // keys staged for this block (whole 16-key tiles)
        __syncthreads();
        for (int i = tid; i < HD * Tk; i += 256) {
            const int d = i / Tk, s = i - d * Tk;
            Ks[i] = (s < kbn && kb0 + s < Tkeys) ? hq[(long)(HD + d) * P + kb0 + s] : 0.f;
        }
        for (int i = tid; i < HD * kbn; i += 256) {
            const int d = i / kbn, s = i - d * kbn;
            Vs[s * 17 + d] = kb0 + s < Tkeys ? hq[(long)(2 * HD + d) * P + kb0 + s] : 0.f;
        }
        __syncthreads();
        const int kte = min(nkt, (kb0 + KB) >> 4);
        for (int kt = kb0 >> 4; kt < kte; ++kt) {
            const int key0 = kt * 16, kl = key0 - kb0;
            float ka[4], va[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                ka[j] = Ks[(4 * j + g) * Tk + kl + n];
                va[j] = Vs[(kl + 4 * g + j) * 17 + n];
            }
#pragma unroll
            for (int qt = 0; qt < UF_QT; ++qt) {
                uf_x4 sc = uf_x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < 4; ++j) sc = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[j], qf[qt][j], sc, 0, 0, 0);
                float cm = -3.0e38f;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (key0 + 4 * g + i >= Tkeys) sc[i] = -3.0e38f;
                    cm = fmaxf(cm, sc[i]);
                }
                cm = fmaxf(cm, __shfl_xor(cm, 16, 64));
                cm = fmaxf(cm, __shfl_xor(cm, 32, 64));
                const float mn = fmaxf(mx[qt], cm);
                const float corr = fm_exp(mx[qt] - mn);
                float ps = 0.f;
                uf_x4 pe;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    pe[i] = fm_exp(sc[i] - mn);          // masked keys: exp(-3e38 - mn) = 0
                    ps += pe[i];
                }
                ps += __shfl_xor(ps, 16, 64);
                ps += __shfl_xor(ps, 32, 64);
                l[qt] = l[qt] * corr + ps;
                o[qt] *= corr;
                mx[qt] = mn;
#pragma unroll
                for (int j = 0; j < 4; ++j) o[qt] = __builtin_amdgcn_mfma_f32_16x16x4f32(va[j], pe[j], o[qt], 0, 0, 0);
            }
        }
        }
        const float sg = (nh == 1) ? 1.f : ((h == 0 || (h >= 4 && h < 7)) ? 1.f : -1.f);
#pragma unroll
        for (int qt = 0; qt < UF_QT; ++qt) {
            const float w = sg / l[qt];
            if (nh == 1 || h < 4) accr[qt] += o[qt] * w;
            else acci[qt] += o[qt] * w;
        }
    }
    const int nout = nh == 1 ? 1 : 2;
#pragma unroll
    for (int qt = 0; qt < UF_QT; ++qt) {
        const int t = q0 + 16 * qt + n;
        if (t >= T) continue;
        float* ob = out + (long)b * nout * HD * P + (long)f * T + t;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ob[(long)(4 * g + i) * P] = accr[qt][i];
            if (nout == 2) ob[(long)(HD + 4 * g + i) * P] = acci[qt][i];
        }
    }
}

// ---- attention along F (f_att_cplx.py:13-29): one thread per (b, f_q, t)
__global__ __launch_bounds__(256) void uf_att_f_kernel(const float* __restrict__ pq, float* __restrict__ out, int F, int T,
                                                       int nh) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int fq = blockIdx.y, b = blockIdx.z;
    if (t >= T) return;
    const long P = (long)F * T;
    const float* base = pq + (long)b * nh * 48 * P + t;
    float accr[HD], acci[HD];
#pragma unroll
    for (int d = 0; d < HD; ++d) accr[d] = acci[d] = 0.f;
    for (int h = 0; h < nh; ++h) {
        const float* hq = base + (long)h * 48 * P;
        float q[HD];
#pragma unroll
        for (int d = 0; d < HD; ++d) q[d] = hq[(long)d * P + (long)fq * T] * 0.25f;
        float e[8];
        float mx = -3.0e38f;
        for (int g = 0; g < F; ++g) {
            float s = 0.f;
#pragma unroll
            for (int d = 0; d < HD; ++d) s += q[d] * hq[(long)(HD + d) * P + (long)g * T];
            e[g] = s;
            mx = fmaxf(mx, s);
        }
        float l = 0.f;
        for (int g = 0; g < F; ++g) {
            e[g] = fm_exp(e[g] - mx);
            l += e[g];
        }
        const float inv = 1.f / l;
        const float sg = (nh == 1) ? 1.f : ((h == 0 || (h >= 4 && h < 7)) ? 1.f : -1.f);
#pragma unroll
        for (int d = 0; d < HD; ++d) {
            float o = 0.f;
            for (int g = 0; g < F; ++g) o += e[g] * hq[(long)(2 * HD + d) * P + (long)g * T];
            if (nh == 1 || h < 4) accr[d] += sg * o * inv;
            else acci[d] += sg * o * inv;
        }
    }
    const int nout = nh == 1 ? 1 : 2;
    float* ob = out + (long)b * nout * HD * P + (long)fq * T + t;
#pragma unroll
    for (int d = 0; d < HD; ++d) {
        ob[(long)d * P] = accr[d];
        if (nout == 2) ob[(long)(HD + d) * P] = acci[d];
    }
}

// The same attention on the matrix cores (round 5; the north star names f_att next to t_att).  The problem is 4 x 4 per (b, t, head) -
// four frequency bins attend to four - which is exactly the block shape of v_mfma_f32_4x4x1_16b_f32: SIXTEEN independent 4 x 4 x 1
// products per instruction.  A wave owns 16 consecutive frames of one utterance (block <-> frame, lane = 4 * block + j):
//   S^T[g][fq] = sum_d k[g][d] q[fq][d]     A row g = k[g][d], B column fq = q[fq][d] / 4, 16 steps over d in 4 accumulator chains
//                                           (a dependent 4x4x1 issues at half rate, tools/mfma4bench.cpp);
//   D: lane (block, fq), register g  ->  all four scores of query fq sit in ONE lane: the softmax needs no cross-lane step, and the
//   probabilities are already the B operand (column fq, step g) of
//   O^T[d][fq] = sum_g v[g][d] p[g][fq]     A row d' = v[g][4 db + d'], four row blocks db, accumulated over the heads with the
//                                           sign of the complex product folded into p (f_att_cplx.py:31-88).
// Every q / k / v element is loaded exactly once (4 x 64 B per wave instruction).
__global__ __launch_bounds__(256) void uf_att_f_mfma_kernel(const float* __restrict__ pq, float* __restrict__ out, int T, int nh,
                                                            int ngroups) {
    constexpr int F = 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = blockIdx.x * 4 + wave, b = blockIdx.y;
    if (grp >= ngroups) return;
    const int blk = lane >> 2, j = lane & 3;
    const int t = grp * 16 + blk, tc = min(t, T - 1);
    const long P = (long)F * T;
    const float* base = pq + (long)b * nh * 48 * P + (long)j * T + tc;       // row j of every (head, dim) plane at this lane's frame
    uf_x4 accr[4], acci[4];
#pragma unroll
    for (int db = 0; db < 4; ++db) accr[db] = acci[db] = uf_x4{0.f, 0.f, 0.f, 0.f};
    for (int h = 0; h < nh; ++h) {
        const float* hq = base + (long)h * 48 * P;
        float qv[HD], kv[HD];
#pragma unroll
        for (int d = 0; d < HD; ++d) {
            qv[d] = hq[(long)d * P] * 0.25f;                  // / hidden_channel ** 0.5
            kv[d] = hq[(long)(HD + d) * P];
        }
        uf_x4 sc[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) sc[c] = uf_x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int d = 0; d < HD; ++d) sc[d & 3] = __builtin_amdgcn_mfma_f32_4x4x1f32(kv[d], qv[d], sc[d & 3], 0, 0, 0);
        float e[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) e[g] = (sc[0][g] + sc[1][g]) + (sc[2][g] + sc[3][g]);
        const float mx = fmaxf(fmaxf(e[0], e[1]), fmaxf(e[2], e[3]));
        float l = 0.f;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            e[g] = fm_exp(e[g] - mx);
            l += e[g];
        }
        const float sg = (nh == 1) ? 1.f : ((h == 0 || (h >= 4 && h < 7)) ? 1.f : -1.f);
        const float inv = sg / l;
        const bool to_r = nh == 1 || h < 4;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float pg = e[g] * inv;
            const float* vg = hq + (long)(2 * HD) * P + (long)(g - j) * T;       // row g (this lane's base points at row j)
#pragma unroll
            for (int db = 0; db < 4; ++db) {
                const float vv = vg[(long)(4 * db + j) * P];                     // A row d' = j of row block db: v[g][4 db + j]
                if (to_r) accr[db] = __builtin_amdgcn_mfma_f32_4x4x1f32(vv, pg, accr[db], 0, 0, 0);
                else acci[db] = __builtin_amdgcn_mfma_f32_4x4x1f32(vv, pg, acci[db], 0, 0, 0);
            }
        }
    }
    if (t >= T) return;
    const int nout = nh == 1 ? 1 : 2;
    float* ob = out + (long)b * nout * HD * P + (long)j * T + t;                 // lane (block, fq = j): every dim of query row fq
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ob[(long)(4 * db + i) * P] = accr[db][i];
            if (nout == 2) ob[(long)(HD + 4 * db + i) * P] = acci[db][i];
        }
}

// ---- :236-262  sigmoid magnitude mask, tanh complex-magnitude mask + phase add, average, polar -> RI [B][2][257][T]
__global__ __launch_bounds__(256) void uf_post_kernel(const float* __restrict__ dc, const float* __restrict__ dm,
                                                      const float* __restrict__ mag0, const float* __restrict__ ph0,
                                                      float* __restrict__ est, int T, float p_out) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int k = blockIdx.y, b = blockIdx.z;
    if (t >= T) return;
    const long i0 = ((long)b * NBIN + k) * T + t;
    const float m0 = mag0[i0], p0 = ph0[i0];
    float mmask = 0.f, cm = 0.f, cph = 0.f;
    if (k > 0) {
        const long q = ((long)b * 2 * (NBIN - 1) + (k - 1)) * T + t;
        const float mr = dc[q], mi = dc[q + (long)(NBIN - 1) * T];
        const float mg = dm[((long)b * (NBIN - 1) + (k - 1)) * T + t];
        mmask = 1.f / (1.f + expf(-mg));
        const float mm = sqrtf(fmaxf(mr * mr + mi * mi, UEPS));
        const float rp = mr / (mm + UEPS), ip = mi / (mm + UEPS);
        cm = tanhf(mm + UEPS);
        cph = atan2f(ip + UEPS, rp);
    }
    float em = (cm * m0 + mmask * m0) * 0.5f;
    if (p_out != 1.f) em = powf(em, p_out);
    const float ep = p0 + cph;
    const long o = ((long)b * 2 * NBIN + k) * T + t;
    est[o] = em * cosf(ep);
    est[o + (long)NBIN * T] = em * sinf(ep);
}

// ---- :182-194  src_cplx = |S| e^{j angle S} of the clean source's STFT with the clamp / EPS of the reference,
// [B][2][257][T] (spec and out share the row pitch T)
__global__ __launch_bounds__(256) void uf_src_cplx_kernel(const float* __restrict__ spec, float* __restrict__ out, int T,
                                                          float p_in) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int k = blockIdx.y, b = blockIdx.z;
    if (t >= T) return;
    const long plane = (long)NBIN * T;
    const long o = ((long)b * 2 * NBIN + k) * T + t;
    const float re = spec[o], im = spec[o + plane];
    float m = sqrtf(fmaxf(re * re + im * im, UEPS));
    if (p_in != 1.f) m = powf(m, p_in);
    const float ph = atan2f(im + UEPS, re);
    out[o] = m * cosf(ph);
    out[o + plane] = m * sinf(ph);
}

// launch record of the launchers below (k_uformer.h: UfLaunchRec); null outside tests
thread_local std::vector<UfLaunchRec>* g_uf_log = nullptr;
void uf_log_launch(const char* kernel, dim3 grid, size_t shmem, int nh = 0, int KB = 0, int Tk = 0, int nblocks = 0, int ragged = 0) {
    if (!g_uf_log) return;
    UfLaunchRec r;
    r.kernel = kernel; r.nh = nh; r.KB = KB; r.Tk = Tk; r.nblocks = nblocks; r.ragged = ragged;
    r.grid = (long)grid.x * grid.y * grid.z; r.block = 256; r.shmem = (long)shmem;
    g_uf_log->push_back(r);
}

}  // namespace

void uf_set_launch_log(std::vector<UfLaunchRec>* log) { g_uf_log = log; }

void launch_uf_prep(const float* spec, float* mag0, float* ph0, float* xc, float* xm, int B, int T, float p_in, hipStream_t st) {
    const dim3 grid((T + 255) / 256, NBIN, B);
    uf_log_launch("uf_prep", grid, 0);
    hipLaunchKernelGGL(uf_prep_kernel, grid, dim3(256), 0, st, spec, mag0, ph0, xc, xm, T, p_in);
}

void launch_uf_fusion(float* cplx, float* mag, int B, long CP, hipStream_t st) {
    const dim3 grid((unsigned)((CP + 255) / 256), B);
    uf_log_launch("uf_fusion", grid, 0);
    hipLaunchKernelGGL(uf_fusion_kernel, grid, dim3(256), 0, st, cplx, mag, CP);
}

void launch_uf_post(const float* dc, const float* dm, const float* mag0, const float* ph0, float* est, int B, int T, float p_out,
                    hipStream_t st) {
    const dim3 grid((T + 255) / 256, NBIN, B);
    uf_log_launch("uf_post", grid, 0);
    hipLaunchKernelGGL(uf_post_kernel, grid, dim3(256), 0, st, dc, dm, mag0, ph0, est, T, p_out);
}

void launch_uf_src_cplx(const float* spec, float* out, int B, int T, float p_in, hipStream_t st) {
    const dim3 grid((T + 255) / 256, NBIN, B);
    uf_log_launch("uf_src_cplx", grid, 0);
    hipLaunchKernelGGL(uf_src_cplx_kernel, grid, dim3(256), 0, st, spec, out, T, p_in);
}

void launch_uf_att_t(const float* pq, float* out, int B, int F, int T, int nh, hipStream_t st) {
    // key blocks of <= UF_ATT_KB frames
    const int KB = std::min((T + 15) / 16 * 16, UF_ATT_KB);
    int Tk = KB;
    if (Tk % 32 != 16) Tk += 16;
    const size_t lds = ((size_t)HD * Tk + (size_t)KB * 17) * sizeof(float);
    static bool seen[64] = {};
    if (first_on_device(seen))
        SE_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(uf_att_t_mfma_kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
    const int* tlen = ragged_ctx() ? ragged_ctx()->tlen : nullptr;
    const dim3 grid(B * F, (T + 64 * UF_QT - 1) / (64 * UF_QT));
    uf_log_launch("uf_att_t_mfma", grid, lds, nh, KB, Tk, (T + KB - 1) / KB, tlen != nullptr);
    hipLaunchKernelGGL(uf_att_t_mfma_kernel, grid, dim3(256), lds, st, pq, out, F, T, nh, Tk, KB, tlen);
}

void launch_uf_att_f(const float* pq, float* out, int B, int F, int T, int nh, hipStream_t st) {
    SE_CHECK(F <= 8, "F-attention kernel is built for the 4-bin bottleneck");
    // SE_UF_ATT_F_MFMA=0: the VALU kernel of rounds 1-4 (one thread per query)
    static const bool fmfma = !(getenv("SE_UF_ATT_F_MFMA") && atoi(getenv("SE_UF_ATT_F_MFMA")) == 0);
    if (fmfma && F == 4) {
        const int ng = (T + 15) / 16;
        const dim3 grid((ng + 3) / 4, B);
        uf_log_launch("uf_att_f_mfma", grid, 0, nh);
        hipLaunchKernelGGL(uf_att_f_mfma_kernel, grid, dim3(256), 0, st, pq, out, T, nh, ng);
    } else {
        const dim3 grid((T + 255) / 256, F, B);
        uf_log_launch("uf_att_f", grid, 0, nh);
        hipLaunchKernelGGL(uf_att_f_kernel, grid, dim3(256), 0, st, pq, out, F, T, nh);
    }
}

}  // namespace se
