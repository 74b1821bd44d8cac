// Launchers of Uformer's private kernels (k_uformer.hip): the polar front / back end, the interaction of the two branches and the
// attentions along time and along frequency.  model_uformer.hip calls them; csrc/tests/att_probe.hip calls them one at a time.
#pragma once
#include <vector>
#include "kernels.h"

namespace se {

// A complex tensor is [B][2C][F][T]: real planes, then imaginary planes.
// spec [B][2][257][T] -> mag0, ph0 [B][257][T] (uformer.py:187-210) and the network inputs without the DC bin, xc [B][2][256][T],
// xm [B][256][T]
void launch_uf_prep(const float* spec, float* mag0, float* ph0, float* xc, float* xm, int B, int T, float p_in, hipStream_t st);
// fusion.py:13-19 in place on cplx [B][2][CP] / mag [B][CP]
void launch_uf_fusion(float* cplx, float* mag, int B, long CP, hipStream_t st);
// masks dc [B][2][256][T], dm [B][256][T] on (mag0, ph0) -> est [B][2][257][T] (uformer.py:236-262)
void launch_uf_post(const float* dc, const float* dm, const float* mag0, const float* ph0, float* est, int B, int T, float p_out,
                    hipStream_t st);
// spec [B][2][257][T] -> |S|^p_in e^{j angle S} with the reference's clamp / EPS (uformer.py:182-194)
void launch_uf_src_cplx(const float* spec, float* out, int B, int T, float p_in, hipStream_t st);
// pq [B][nh * 48][F][T] (q, k, v x 16 rows per head) -> out [B][16 (nh = 1) or 32 (nh = 8: real, imaginary)][F][T]: attention
// along T (keys < tlen[b] of ragged_ctx() in a ragged batch) / along F (F <= 8)
void launch_uf_att_t(const float* pq, float* out, int B, int F, int T, int nh, hipStream_t st);
void launch_uf_att_f(const float* pq, float* out, int B, int F, int T, int nh, hipStream_t st);

// Form of one dispatch of the launchers above, for tests that must know which kernel a launch reached and with what geometry
// (csrc/tests/att_probe.hip).  Host-side only: nothing the kernels compute depends on it.  Fields a kernel does not have are 0.
struct UfLaunchRec {
    const char* kernel = "";     // "uf_att_t_mfma", "uf_att_f_mfma", "uf_att_f", "uf_prep", "uf_fusion", "uf_post", "uf_src_cplx"
    int nh = 0;                  // heads (attention kernels)
    int KB = 0, Tk = 0;          // uf_att_t_mfma: keys per LDS block, row pitch of the K block
    int nblocks = 0;             // key blocks of a full-length row
    int ragged = 0;              // the launch read the published per-row frame counts
    long grid = 0;               // workgroups (all grid dimensions)
    int block = 0;
    long shmem = 0;              // dynamic LDS bytes
};
// nullptr (the default): nothing is recorded.  Otherwise every dispatch of the launch_uf_* launchers on this thread appends its record.
void uf_set_launch_log(std::vector<UfLaunchRec>* log);

}  // namespace se
