/* se_engine.h - C ABI of the MI355X (gfx950) speech-enhancement decode engine (libse_engine.so).
 *
 * The reference (cszheng-ioa/Sixty-years-of-frequency-domain-monaural-speech-enhancement) has no FFI: its only
 * seams are Python ones.  Each entry point below states the reference interface it stands in for
 * (paths relative to the reference root).  Plain C types only; no torch types cross this boundary.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error; the message is read with se_last_error().
 *   - `*_dev` pointers are DEVICE pointers owned by the caller (e.g. torch-ROCm `tensor.data_ptr()`);
 *     the engine never frees them.  Scratch and weights are engine-owned, sized at create / finalize.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Work is enqueued, not synchronised;
 *     only se_engine_finalize() and se_engine_destroy() synchronise.
 *   - a handle is not thread-safe, and its calls are ordered: a call on a handle must come after that handle's previous call
 *     in stream order (the same stream, or one made to wait for it) - the workspace is one per handle.
 *   - several handles of one device may be driven from ONE host thread on DIFFERENT streams and be in flight at once: each
 *     returns bit for bit what it returns when called alone, with or without SE_CFG_GRAPHS (tests/test_gpu_two_engines.py).
 *     Handles share nothing that a running kernel writes: scratch is per (purpose, device, stream), and what a captured graph
 *     keeps the address of is the capturing handle's own.  Two host threads driving two handles at the same time are outside
 *     this contract (they would enqueue onto the same process-wide auxiliary streams unordered).
 *   - all floating-point data is fp32 (the reference feeds `torch.FloatTensor`).
 */
#ifndef SE_ENGINE_H
#define SE_ENGINE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct se_engine se_engine;

/* One id per reference model class on the decode path (constructor call sites cited). */
enum se_model_id {
    SE_MODEL_LSTM = 1,        /* lstm_net()   LSTM/lstm_decode_vb.py:18   (LSTM/LSTM.py:14-28)            */
    SE_MODEL_CRN = 2,         /* crn_net()    CRN/crn_decode_vb.py:18     (CRN/CRN.py:16-117)             */
    SE_MODEL_GCRN = 3,        /* Net()        GCRN/gcrn_decode_vb.py:19   (GCRN/GCRN_noncprs.py:86-165)   */
    SE_MODEL_DPCRN = 4,       /* dpcrn()      DPCRN/dpcrn_decode_vb.py:19 (DPCRN/DPCRN.py:16-174)         */
    SE_MODEL_DCCRN = 5,       /* DCCRN(rnn_units=256, masking_mode='E', use_clstm=True,
                                 kernel_num=[32,64,128,256,256,256])  DCCRN/dccrn_decode_vb.py:11         */
    SE_MODEL_FULLSUBNET = 6,  /* Model(...)   FullSubNet/fullsubnet_sa_decode_vb.py:11-24                 */
    SE_MODEL_CTSNET = 7,      /* Step1_net(), Step2_net(X=6,R=3)  CTSNet/two_stage_com_decode_vb.py:13-14 */
    SE_MODEL_G2NET = 8,       /* gaf_base(...)  G2Net_VB/com_decode.py:23                                 */
    SE_MODEL_TAYLORSENET = 9, /* TaylorSENet(...) TaylorSENet/taylorsenet_decode_vb.py:11-13              */
    SE_MODEL_UFORMER = 10     /* Uformer()    Uformer/uformer_decode_vb.py:19                             */
};

/* Replaces the module constants + hand-edited exponents of each decode script
 * (e.g. DCCRN/config.py:5-8 win_size/fft_num/win_shift; `** 1.0` vs `** 0.5 / ** 2.0` at
 * DCCRN/dccrn_decode_vb.py:40,48 and DCCRN/dccrn_decode.py:44,52).  n_fft/hop/win = 0 selects the
 * model's own front end. */
/* se_config.flags: replay se_enhance_batch as a hipGraph per (batch, n_samples) shape - captured on the second call of
 * a shape, caller buffers staged through engine-owned rows.  Results are bit-identical to the eager path.  Off by default:
 * measured on MI355X the replay does not shorten a batch-1 decode (the path is bound by its chain of dependent small
 * kernels, not by launch submission); models that fork onto auxiliary streams (FullSubNet) always run eagerly. */
#define SE_CFG_GRAPHS 1
/* DCCRN only.  `DCCRN/DCCRN_cprs.py:6` imports its operators from a third-party `complexnn.py` that is absent from the
 * reference and unversioned.  The engine follows the published upstream (huyanxin/DeepComplexCRN) as restated in
 * oracle/_complexnn_recall.py; the two conventions DCCRN_cprs.py itself does not determine can be
 * flipped here - they are weight-preparation switches at se_engine_finalize, so adopting the real file, should it differ,
 * is a flag and a fixture regeneration, not a kernel change.
 *   SE_CFG_DCCRN_BIAS_PER_PART: each part adds its own conv's bias once (real += b_real, imag += b_imag) instead of the
 *                               two-real-conv combination real += b_real - b_imag, imag += b_real + b_imag
 *   SE_CFG_DCCRN_PLAIN_CAT    : complex_cat([out, skip], 1) is a plain channel concat ([out_r, out_i, skip_r, skip_i])
 *                               instead of real halves together, imaginary halves together */
#define SE_CFG_DCCRN_BIAS_PER_PART 2
#define SE_CFG_DCCRN_PLAIN_CAT 4
/* FullSubNet only: `sequence_model="GRU"` of Model(...) - both sequence models are torch.nn.GRU stacks instead of nn.LSTM
 * (FullSubNet/fullsubnet_net_sa/sequence_model.py:36-43; the decode script passes "LSTM", fullsubnet_sa_decode_vb.py:16).
 * The state dict then carries the GRU's [3H, .] weight_ih / weight_hh / bias_ih / bias_hh entries. */
#define SE_CFG_FSN_GRU 8
/* FullSubNet with norm_type = "cumulative_laplace_norm" (FullSubNet/fullsubnet_net_sa/base_model.py:212-240, selected at
 * :296-303) instead of the decode script's "offline_laplace_norm": every input is divided by its running mean over the frames
 * seen so far.  The network is then causal up to its look_ahead = 2 frames, and se_stream_* accepts the engine. */
#define SE_CFG_FSN_CUMULATIVE 16
/* DCCRN(masking_mode=...) (DCCRN/DCCRN_cprs.py:205-223): 'E' (default, the decode script's: tanh-bounded magnitude mask and
 * phase rotation), 'C' (complex ratio mask: est = spec x mask), 'R' (one real mask per part: est_r = spec_r mask_r, est_i =
 * spec_i mask_i).  At most one of the two bits. */
#define SE_CFG_DCCRN_MASK_C 32
#define SE_CFG_DCCRN_MASK_R 64
/* DCCRN(use_clstm=False) (DCCRN/DCCRN_cprs.py:95-102; DCCRN-E / -R / -C of its `__main__`, :303-315): the real-LSTM core - the
 * 256 x 4 encoder features of a frame as ONE vector into nn.LSTM(1024, rnn_units, num_layers=2) (`enhance.*_l0 / _l1`) and
 * Linear(rnn_units, 1024) (`tranform.*`) - instead of the complex LSTM.  rnn_units and kernel_num[0] are read from the shapes of
 * enhance.weight_hh_l0 and encoder.0.0.real_conv.weight; se_engine_finalize accepts (rnn_units, kernel_num) = (256 or 128,
 * [16,32,64,128,256,256]) and (256, [32,64,128,256,256,256]).  Combines with SE_CFG_DCCRN_MASK_C / _R and the two
 * complexnn conventions above. */
#define SE_CFG_DCCRN_REAL_LSTM 128
/* G2Net / TaylorSENet: the constructor's repeat count, bits 8-11 of se_config.flags.
 *   gaf_base(..., stage_num = n)      G2Net_VB/gaf_net_320.py:27,55-58  (n GAF stages `gafs.<s>.`, 1 <= n <= 8)
 *   TaylorSENet(..., order_num = n)   TaylorSENet/TaylorSENet.py:27,66-70 (n high-order blocks `highorderblock_list.<k>.`, 0 <= n <= 8)
 * 0 in the field = the decode scripts' value (3 for both: G2Net_VB/com_decode.py:23, TaylorSENet/taylorsenet_decode_vb.py:11-13). */
#define SE_CFG_REPEATS(n) ((((n) + 1) & 15) << 8)
/* CTSNet: Step2_net(X, R) (CTSNet/Step2_network.py:13-21: R groups `tcm_list.<r>.` of X gated blocks `glu_list.<i>.`, dilation 2^i):
 * R in SE_CFG_REPEATS (1 <= R <= 8), X in bits 12-15 (1 <= X <= 6); 0 in a field = the decode script's 3 / 6
 * (two_stage_com_decode_vb.py:14). */
#define SE_CFG_REPEATS2(n) ((((n) + 1) & 15) << 12)
/* DCCRN of `DCCRN_SNR/` (DCCRN_SNR/DCCRN.py:9-183, built at DCCRN_SNR/dccrn_decode_snr.py:12 for the WSJ0-SI84 grid): the same
 * network as DCCRN/DCCRN_cprs.py except that after every transposed conv the decoder keeps `out[..., :-1]` (DCCRN_SNR/DCCRN.py:159)
 * where DCCRN_cprs.py:199 keeps `out[..., 1:]` - each decoder layer then looks BACK one frame instead of ahead, and the network is
 * causal end to end.  The class has the 'E' mask only (DCCRN.py:162-183): the bit does not combine with SE_CFG_DCCRN_MASK_C / _R
 * (se_engine_create fails); it combines with SE_CFG_DCCRN_REAL_LSTM (the class default `use_clstm=False`, DCCRN.py:82-91) and with
 * the two complexnn conventions.  Decode semantics are those of dccrn_decode_snr.py:31-67: the same front end (zero pad to a hop
 * multiple, torch.stft 512 / 128 / 512), torch.istft without `length`, the result cut to the clip's own length (:66) - so
 * se_output_samples(n) = n, not the hop-padded length of dccrn_decode_vb.py - and se_stream_* finalises every frame with no
 * extra delay (the `_vb` network: six frames late). */
#define SE_CFG_DCCRN_CAUSAL_DEC (1 << 16)
/* Frame-online streams (se_stream_*) that outlive max_samples: the engine keeps only the samples some not-yet-transformed
 * frame still needs, in a window of max_samples + n_fft + hop floats per row (two such buffers: a slide copies the live tail
 * from one into the other), instead of every sample since se_stream_begin.  A stream may then run to 2^31 - 1 - max_samples
 * samples (37 hours at 16 kHz; engines with max_samples < n_fft + 32 hop: 2^31 - 1 - n_fft - 32 hop), where se_stream_push
 * refuses; a single push may carry at most max_samples samples.  max_samples keeps its other meanings (offline limit, arena
 * size, cap on max_chunk_frames).  Any model that streams, se_stream_begin and se_stream_begin_running alike; the offline
 * calls are not affected, and a model that cannot stream still cannot. */
#define SE_CFG_STREAM_SLIDING (1 << 17)
/* SE_MODEL_DCCRN with the look-ahead decoder (without SE_CFG_DCCRN_CAUSAL_DEC) in se_enhance_long_ragged: the engine hands the
 * rows' whole-clip frame counts to the network, and every chunk of the window walk clears the columns at or past each row's own
 * last frame behind the encoder layers, the LSTM core and every decoder layer (one launch for the seven tensors that become
 * final together, one behind each of decoder layers 1 - 5; the cut is derived on the device, nothing waits on the host) - the
 * zeros a clip decoded alone has where its decoder looks one frame ahead.  Opt-in: without the bit se_enhance_long_ragged
 * refuses this network as before.  With it nothing else changes: se_enhance_batch, se_enhance_ragged, se_enhance_long (equal
 * rows) and se_stream_* enqueue exactly the launches of an engine without it.  DCCRN only, and not with
 * SE_CFG_DCCRN_CAUSAL_DEC (that decoder looks back and is accepted without the bit): se_engine_create fails for either.
 * Combines with SE_CFG_DCCRN_REAL_LSTM, SE_CFG_DCCRN_MASK_C / _R, the two complexnn conventions, SE_CFG_GRAPHS and
 * SE_CFG_STREAM_SLIDING.  Like every model bit it is part of a parked stream's identity (se_stream_restore / _state_select /
 * _state_concat / _state_join compare it). */
#define SE_CFG_DCCRN_ROW_ENDS (1 << 18)
/* Frame-online streams of the models whose state counts frames from the start of the stream - SE_MODEL_CTSNET, SE_MODEL_G2NET and
 * SE_MODEL_TAYLORSENET (the cumulative LayerNorm divides by the frames so far, the TCM rings are indexed by the frame), and
 * SE_MODEL_FULLSUBNET with SE_CFG_FSN_CUMULATIVE or SE_CFG_FSN_CUM_LAYERNORM and without SE_CFG_FSN_GRU (the cumulative norms, the
 * look-ahead skip):
 * the engine keeps one int32 per row on the device, the row's frame ORIGIN, and every kernel that read the group's frame index t
 * reads the row's own index t - origin[b] instead.  se_stream_begin / _begin_running / _begin_tracking zero the origins; a parked
 * stream carries them (a segment of its own in the snapshot); se_stream_state_join adds shift / hop to the origins of every part
 * it rebases, so a rebased row keeps dividing by its own frame count and indexing its own rings where it always did - and the
 * join, which refuses these models without the bit, is exact for them with it.  Origins accumulate over repeated joins and may be
 * negative (a part older than parts[0]).  Opt-in: without the bit nothing changes (the kernels get a null pointer, snapshots stay
 * byte-identical, the join refuses these models as before); with it a stream that is never joined computes, bit for bit, what it
 * computes without.  se_engine_create fails for any other model or configuration.  Like every model bit it is part of a parked
 * stream's identity (se_stream_restore / _state_select / _state_concat / _state_join compare it). */
#define SE_CFG_STREAM_ROW_ORIGINS (1 << 19)
/* FullSubNet with norm_type = "offline_gaussian_norm" (FullSubNet/fullsubnet_net_sa/base_model.py:242-255, selected at :296-308):
 * (x - mean) / (std + 1e-5), mean and the unbiased std (torch.std) over the whole utterance, the two look-ahead pad frames included
 * (model.py:79 pads before :84 norms).  Like offline_laplace_norm it spans the utterance: nothing streams, se_stream_begin and
 * se_enhance_long refuse the engine and name SE_CFG_FSN_CUM_LAYERNORM.  Combines with SE_CFG_FSN_GRU. */
#define SE_CFG_FSN_GAUSSIAN (1 << 20)
/* FullSubNet with norm_type = "cumulative_layer_norm" (base_model.py:258-294): every input minus its running mean, over its running
 * standard deviation, both over the frames seen so far.  Causal up to look_ahead = 2 frames as SE_CFG_FSN_CUMULATIVE is: se_stream_*,
 * the parked-stream calls, se_enhance_long and se_enhance_long_ragged accept the engine (without SE_CFG_FSN_GRU, which decodes offline
 * only), and so does SE_CFG_STREAM_ROW_ORIGINS.  A stream carries two running sums (x, x^2) per utterance and per sub-band sequence.
 * At most one of SE_CFG_FSN_CUMULATIVE, SE_CFG_FSN_GAUSSIAN, SE_CFG_FSN_CUM_LAYERNORM; se_engine_create fails for any other model. */
#define SE_CFG_FSN_CUM_LAYERNORM (1 << 21)
/* FullSubNet's shape, Model(look_ahead, fb_num_neighbors, sb_num_neighbors) (FullSubNet/fullsubnet_net_sa/model.py:9-63).  Two fields
 * with the zero-means-script-value convention of SE_CFG_REPEATS - a caller that passes nothing gets the decode script's model:
 *   SE_CFG_FSN_LOOK_AHEAD(n)     bits 22-24, stores n + 1, 0 <= n <= 6; 0 in the field = the script's look_ahead = 2, and
 *                                se_engine_create stores SE_CFG_FSN_LOOK_AHEAD(2) as the empty field: both spellings give ONE engine
 *                                identity, a stream parked on either is restored, selected and joined on the other.  The network
 *                                sees n zero frames behind the clip (model.py:79) and the mask of frame t is the output of step t + n
 *                                (:117); a stream is final n frames (n * 16 ms) late, with n = 0 every frame at once.
 *   SE_CFG_FSN_FB_NEIGHBORS(n)   bits 25-28, stores n, 0 <= n <= 15; the script's value is 0.  The sub-band model is fed 2 n + 1 bins
 *                                of the full-band output around its own, the frequency axis reflect-padded (base_model.py:13-42).
 * sb_num_neighbors (0..15) is no flag: se_engine_finalize reads it from the shape of sb_model.sequence_model.weight_ih_l0,
 * [4H or 3H, (2 sb_num_neighbors + 1) + (2 fb_num_neighbors + 1)], the way DCCRN's rnn_units is read from enhance.weight_hh_l0, and fails -
 * naming the width and fb_num_neighbors - when (width - 2 fb_num_neighbors - 2) is odd, negative or above 30.  Every value combines with
 * SE_CFG_FSN_GRU and the four norms, and everything the engine does with the script's shape it does with these: se_enhance_batch,
 * se_enhance_ragged, se_forward and - with a cumulative norm and the LSTM - se_stream_*, the parked-stream calls (both fields are flag
 * bits, so they are part of a parked stream's identity: a snapshot of look_ahead = 0 is refused by an engine of look_ahead = 2),
 * se_stream_state_join under SE_CFG_STREAM_ROW_ORIGINS, se_enhance_long and se_enhance_long_ragged.  Two engines that differ in
 * sb_num_neighbors alone differ in their WEIGHTS, which no parked-stream call compares (se_stream_restore): keeping them apart is the
 * caller's duty, as it is for any two sets of weights.  Still refused, because every kernel size follows from them: num_freqs other than
 * 257, hidden sizes other than 512 / 384, output activations other than ReLU / none.  se_engine_create fails for either field on
 * another model.  The look-ahead field is three bits wide and every value of it is a look_ahead the engine builds; a look_ahead of 7
 * or more does not fit it (the macro masks its argument), so callers check the range themselves, as se_amd.models.Model does. */
#define SE_CFG_FSN_LOOK_AHEAD(n) ((((n) + 1) & 7) << 22)
#define SE_CFG_FSN_FB_NEIGHBORS(n) (((n) & 15) << 25)

typedef struct se_config {
    int32_t model;        /* enum se_model_id */
    int32_t device;       /* HIP device ordinal */
    int32_t max_batch;    /* utterances per se_enhance_batch call (scratch is sized for this) */
    int32_t max_samples;  /* longest utterance, samples */
    float p_in;           /* magnitude exponent applied before the network (1.0 noncprs, 0.5 cprs) */
    float p_out;          /* magnitude exponent applied after the network  (1.0 noncprs, 2.0 cprs) */
    int32_t n_fft, hop, win;
    int32_t flags;        /* SE_CFG_* bits, 0 = defaults */
} se_config;

/* Model construction: `model = <Class>(...)` + `.cuda()`. */
int se_engine_create(const se_config* cfg, se_engine** out);
int se_engine_destroy(se_engine* e);

/* Error text of the last failing call on this handle (e == NULL: last se_engine_create failure). */
const char* se_last_error(const se_engine* e);

/* Weight load: one call per entry of `model.load_state_dict(torch.load('./BEST_MODEL/<name>.pth'))`
 * (e.g. CRN/crn_decode_vb.py:19).  `data` is HOST memory, copied; dtype 0 = float32, 1 = int64
 * (`num_batches_tracked` buffers: accepted and ignored).  Key names are the reference state-dict keys
 * (SURVEY.md Appendix D).  Unknown keys are rejected at finalize, like a strict load. */
int se_engine_set_tensor(se_engine* e, const char* key, const void* data, const int64_t* shape, int32_t ndim,
                         int32_t dtype);
/* End of load_state_dict (strict): checks every expected key is present with the right shape, folds
 * eval-mode BatchNorm into the adjacent convolution, packs weights for the MFMA kernels, uploads. Synchronises. */
int se_engine_finalize(se_engine* e);

/* `y = model(x)` under torch.no_grad()/eval(): model-only parity hook.  Shapes are the reference's
 * (SURVEY.md 8(a)), e.g. DCCRN [B,2,257,T] -> [B,2,257,T]; CRN [B,T,161] -> [B,T,161]. */
int se_forward(se_engine* e, const float* in_dev, const int64_t* in_shape, int32_t in_ndim, float* out_dev,
               void* stream);

/* Uformer's full return: `output, src, output_cplx, src_cplx = model(inputs, src)` (Uformer/uformer.py:172-287; the decode
 * script calls `model(x, x)[0]`, uformer_decode_vb.py:40).  inputs_dev / src_dev: waveforms [batch][n_samples] (dense rows).
 *   output_dev      [batch][se_output_samples(n)]   enhanced waveform (uformer.py:276) - what se_forward returns
 *   src_out_dev     [batch][se_output_samples(n)]   istft(stft(src)) (uformer.py:186), NULL = not wanted
 *   output_cplx_dev [batch][2][257][T]              the RI estimate the waveform is synthesised from (uformer.py:264-286)
 *   src_cplx_dev    [batch][2][257][T]              |S| e^{j angle S} of the source's STFT (uformer.py:187-194)
 * T = se_num_frames(e, n_samples); rows of T frames, T contiguous.  src_dev == NULL skips the two source outputs.
 * Only for engines created with SE_MODEL_UFORMER. */
int se_uformer_forward(se_engine* e, const float* inputs_dev, const float* src_dev, int32_t batch, int32_t n_samples,
                       float* output_dev, float* src_out_dev, float* output_cplx_dev, float* src_cplx_dev, void* stream);

/* The per-utterance body of `enhance(args)` for a batch of equal-length clips, device to device:
 * unit-RMS normalise -> (tail pad) -> STFT -> compress -> network (+mask) -> decompress -> iSTFT -> /c.
 * wav_in_dev [B][in_pitch] (first n_samples of each row valid), wav_out_dev [B][out_pitch]; the number of
 * output samples per utterance is se_output_samples(e, n_samples) (DCCRN returns the hop-padded length,
 * dccrn_decode_vb.py:59-64 - with SE_CFG_DCCRN_CAUSAL_DEC it returns L, dccrn_decode_snr.py:66; Uformer hop*floor(L/hop);
 * others L). */
int se_enhance_batch(se_engine* e, const float* wav_in_dev, int64_t in_pitch, int32_t batch, int32_t n_samples,
                     float* wav_out_dev, int64_t out_pitch, void* stream);
int64_t se_output_samples(const se_engine* e, int32_t n_samples);

/* The same loop body for a batch of clips of DIFFERENT lengths (the reference decodes one clip at a time, so every clip
 * has its own length: ~824 distinct lengths on VoiceBank+DEMAND, `for file_id in file_list`, DCCRN/dccrn_decode_vb.py:24).
 * `lengths` is a HOST array of `batch` sample counts; row b of wav_in_dev holds lengths[b] valid samples (the rest of the
 * row is ignored), row b of wav_out_dev receives se_output_samples(e, lengths[b]) samples followed by zeros up to
 * se_output_samples(e, max lengths).  Each row gets exactly the result of decoding it alone: its own unit-RMS scale, its
 * own reflect padding and frame count in the STFT / iSTFT, and utterance-wide statistics (InstanceNorm - CTSNet, G2Net,
 * TaylorSENet, e.g. CTSNet/Step1_network.py:121-145; FullSubNet's offline_laplace_norm, base_model.py:197-209) taken over
 * its own frames only; operators that look ahead in time (DCCRN's decoder, Uformer's symmetric dilated convs and its
 * attention over time) see zeros / masked keys past a clip's own last frame, as they do when the clip is decoded alone. */
int se_enhance_ragged(se_engine* e, const float* wav_in_dev, int64_t in_pitch, int32_t batch, const int32_t* lengths,
                      float* wav_out_dev, int64_t out_pitch, void* stream);

/* Frame-online ("streaming") decoding for the causal models - SURVEY.md 8(f) rank 4.  The reference only ever runs its
 * causal architectures offline (`for file_id in file_list`, whole utterance per forward, e.g. CRN/crn_decode_vb.py:33-52;
 * CRN.py:38 / :112-117 pad-top-1 + Chomp_T make every (de)conv look back exactly one frame, the LSTMs are unidirectional).
 * Here the same decode runs incrementally over `batch` parallel streams: se_stream_push() appends n_new samples per row,
 * transforms every STFT frame whose samples have all arrived, advances the network by those frames (one history frame per
 * conv layer and the LSTM (h, c) are carried in the engine) and returns the output samples that are now final - those
 * covered by no future frame - at the start of each row of out_dev; *n_out (host) = their count (same for all rows, 0 is
 * normal for short pushes: the algorithmic latency is n_fft / 2 + 1 samples plus up to one hop).  se_stream_flush() ends
 * the stream: the remaining frames (reflected right edge, as the offline STFT) and samples; the concatenated outputs equal
 * se_enhance_batch() of the whole signal sample for sample (up to fp32 rounding of the differently tiled recurrence).
*   c_dev: the utterance scale c (se_rms_scale) cannot be known before the utterance ends; the caller provides one value
 *          per stream (e.g. from a calibration run), NULL = 1.0; se_stream_begin_running() below estimates it on the fly.  With the offline c the two paths
 *          agree exactly - that is what the tests check.
 *   max_chunk_frames: frames advanced per internal step (latency / efficiency trade-off, default 16).
 * Supported: SE_MODEL_CRN, SE_MODEL_LSTM, SE_MODEL_GCRN, SE_MODEL_DPCRN, SE_MODEL_DCCRN (whose decoder looks six frames ahead:
 * its output is final six frames later than the others'; with SE_CFG_DCCRN_CAUSAL_DEC - the DCCRN of DCCRN_SNR/ - it is final
 * with no extra frames of delay), and SE_MODEL_CTSNET / SE_MODEL_TAYLORSENET / SE_MODEL_G2NET when
 * loaded with the cumulative-LayerNorm weights of the `_new` directories (CTSNet_new/Step1_network.py:213-286 - with the
 * InstanceNorm weights of the base directories the network needs the whole utterance and se_stream_begin fails; the engine
 * then carries up to 128 history frames per dilated conv and the running cLN sums).  A stream ends at max_samples of se_config
 * at the latest (se_stream_push refuses the push that would pass it) unless the engine was created with
 * SE_CFG_STREAM_SLIDING: then it may run to 2^31 - 1 - max_samples samples, fed at most max_samples samples per push. */
int se_stream_begin(se_engine* e, int32_t batch, int32_t max_chunk_frames, const float* c_dev, void* stream);
/* The same, for a caller that has no scale to give: the stream runs on a RUNNING unit-RMS scale.  After every push
 * c = sqrt(samples so far / their sum of squares) - the decode scripts' `c = np.sqrt(len(x) / np.sum(x ** 2.0))`
 * (e.g. CRN/crn_decode_vb.py:34) over what has been heard; the frames that push releases are transformed under that c and
 * taken back by it in the iSTFT (the overlap-add mixes frames of different c, each divided by its own).  A single push of a
 * whole utterance followed by se_stream_flush() therefore equals se_enhance_batch(); piecewise, the first frames see the
 * scale of a short prefix - the price of not knowing the future - and the output tracks the offline decode as the
 * estimate settles (tests/test_gpu_streaming.py).  Scaling the input by k scales the output by k exactly as offline. */
int se_stream_begin_running(se_engine* e, int32_t batch, int32_t max_chunk_frames, void* stream);
/* A third way to start, for a live caller (additions: the ABI number stays): the stream runs on a TRACKING unit-RMS scale, an
 * exponentially forgetting estimate with one value per STFT frame.  Block k is the samples [k hop, (k + 1) hop) of a row, e_k their sum
 * of squares in float64, lambda = exp(-hop / tau_samples) (tau_samples == 0: lambda = 1, never forget), and
 *     E_k = lambda E_(k-1) + e_k      W_k = lambda W_(k-1) + hop      (E_(-1) = W_(-1) = 0, float64)
 * Frame t uses the blocks that end at or before its own last sample: K(t) = floor((t hop + n_fft / 2) / hop),
 *     c_t = sqrt(W_(K(t)-1) / E_(K(t)-1)),   c_t = 1 where E <= 1e-20 (digital silence, as the running scale).
 * Every block a frame needs has arrived when se_stream_push releases the frame (that needs sample t hop + n_fft / 2): the scale adds no
 * latency.  At se_stream_flush the n_total mod hop samples left are one last short block (E = lambda E + e, W = lambda W + r); frames
 * whose K(t) lies past the last block use the last state - the zeros a decode script pads behind the signal are not counted.  Frame t
 * is transformed under c_t and taken back by 1 / c_t in the overlap-add, both rounded from the same float64 value.
 *   - It follows the level: after a few tau the estimate is that of the recent signal, also in a SE_CFG_STREAM_SLIDING stream of hours.
 *   - It is a function of the signal, not of the pushes: a block is summed whole, in one fixed order, out of the stream's input
 *     window when the push that completes it arrives, so c_t is bit-identical for every split of the signal into pushes (the outputs
 *     then differ by the fp32 rounding of differently tiled chunks only).  The window keeps the head of an incomplete block as long
 *     as n_fft >= 2 hop - 2, also when it slides (csrc/stream_window.h); other front ends are refused.
 *   - Its state - (E, W) per row and the two per-frame rings - holds no absolute time: tracking streams are parked, selected,
 *     concatenated (equal tau_samples) and JOINED (se_stream_state_join below rotates the rings by the shift in frames).
 *   - Scaling the input by k scales every c_t by 1 / k and the output by k.  A signal of period hop has c_t = the offline c.
 * Needs what se_stream_begin_running needs.  Refused, each with its own reason: tau_samples negative, NaN or infinite; a model
 * without a frame-online mode (se_stream_begin's wording); n_fft < 2 hop - 2.
 *
 * se_stream_scale copies one float per row of the running stream to c_dev (device, `batch` floats): the scale of the most recently
 * released frame - se_stream_begin: the caller's c; the running scale: the current c; the tracking scale: c_t of the last frame
 * released; 1 before any frame.  The level read-out of a tracking stream.  Refused without a running stream. */
int se_stream_begin_tracking(se_engine* e, int32_t batch, int32_t max_chunk_frames, float tau_samples, void* stream);
int se_stream_scale(se_engine* e, float* c_dev, void* stream);
int se_stream_push(se_engine* e, const float* wav_dev, int64_t pitch, int32_t n_new, float* out_dev, int64_t out_pitch,
                   int32_t* n_out, void* stream);
int se_stream_flush(se_engine* e, float* out_dev, int64_t out_pitch, int32_t* n_out, void* stream);

/* Parking a frame-online stream and putting it back.  A handle carries ONE stream group; se_stream_begin for another group, and
 * se_enhance_long / se_enhance_long_ragged, end it for good.  se_stream_save copies everything the next se_stream_push or
 * se_stream_flush of the running stream reads into a library-owned object; se_stream_restore makes a saved stream the running
 * stream of a handle again, replacing whatever ran there as se_stream_begin does.  One engine can so serve more callers than
 * max_batch, or groups that began at different times, by turns: restore -> push -> save per group.
 *   CONTRACT: take any stream and any point between two calls on it - before its first frame is complete, after its last push.
 *   Save it.  Let anything else happen on the engine: other streams, offline decodes, se_enhance_long, nothing at all.  Restore
 *   it there, or on another engine of the same configuration and weights.  The outputs of every later se_stream_push and of
 *   se_stream_flush then equal those of the uninterrupted stream bit for bit, *n_out included.
 * The object holds a host record (the manifest: the engine's identity, the stream's counters, the size of every carried buffer)
 * and one device payload: the conv history, LSTM (h, c) and call-order state slots of the model, the scale(s) - under a running
 * scale also the sum of squares and the per-frame ring -, and the input samples a later frame or the flush's right-edge
 * reflection can still reach, rows back to back (less than n_fft + hop + 4 per row), so they find their place in an engine with
 * another max_samples.  The workspace is not part of it: the first window after a restore is zero-filled as after any decode.
 *   se_stream_state_create : an empty object; touches no device.  se_stream_state_destroy releases it (NULL: nothing).
 *   se_stream_state_bytes  : device memory of the payload (its window part sized for the most a stream keeps live, so the
 *                            figure does not move from save to save; of an imported image not restored yet: its payload); 0 = empty.
 *   se_stream_save   : needs a running stream on e ("... without se_stream_begin" otherwise); does not end or alter it.  One
 *                      kernel, enqueued on `stream`, ordered against the handle's last stream call as the entry points above.
 *                      The first save of a layout (model, batch, chunk size, slot set) allocates; saving again into an object
 *                      that holds the same layout allocates nothing and waits for nothing.
 *   se_stream_restore: e must be finalized, on the device the payload lives on, and match the engine the stream was saved on in:
 *                      model id; every se_config.flags bit except SE_CFG_GRAPHS and SE_CFG_STREAM_SLIDING; n_fft / hop / win;
 *                      p_in / p_out.  Further: max_batch >= the snapshot's batch; a workspace planned for its max_chunk_frames;
 *                      without SE_CFG_STREAM_SLIDING max_samples >= the samples the stream has received, with it a window that
 *                      holds the saved live samples; for a running-scale or tracking-scale stream a per-frame ring no longer than the snapshot's
 *                      (an engine planned for a larger max_samples may need a longer one).  Each mismatch is refused with its own
 *                      reason.  WEIGHTS ARE NOT COMPARED: the same weights on both engines are the caller's duty (weights of other
 *                      SHAPES are noticed - the state buffers differ in size - but only after the handle's stream has ended).
 *                      The same object may be restored any number of times and on more than one engine: that forks a stream.  An
 *                      engine that has not streamed yet gets its state buffers made here, the cLN networks' slots in the recorded
 *                      order and sizes; one that already holds the layout is copied into, one kernel and no allocation.
 *   se_stream_state_export / _import: the object as one byte string in HOST memory, for another device or process.  Synchronous:
 *                      the image is complete on return.  export with cap == 0 returns the size needed, else the size written
 *                      (-1: error - an empty object, a buffer too small).  import parses and validates the manifest and keeps the
 *                      bytes on the host - it runs, and refuses, without a GPU; the upload happens at the first restore, on that
 *                      engine's device.  It refuses a wrong magic or version, an image cut short, a segment table whose sizes do
 *                      not add up to the recorded payload, negative or overflowing sizes, and trailing bytes.
 * Errors of the calls that take an engine are read through that engine's se_last_error, of the others through se_last_error(NULL).
 * A refused call changes nothing: neither the object nor a stream running on the engine.  An object is not thread-safe, and like
 * a handle it orders calls made on different hipStreams behind one another. */
typedef struct se_stream_state se_stream_state;
int se_stream_state_create(se_stream_state** out);
int se_stream_state_destroy(se_stream_state* s);
int64_t se_stream_state_bytes(const se_stream_state* s);
int se_stream_save(se_engine* e, se_stream_state* s, void* stream);
int se_stream_restore(se_engine* e, const se_stream_state* s, void* stream);
int64_t se_stream_state_export(const se_stream_state* s, void* host_buf, int64_t cap);
int se_stream_state_import(se_stream_state* s, const void* host_buf, int64_t bytes);

/* Rows of parked groups (additions: the ABI number stays).  A snapshot holds `batch` rows that have advanced in lockstep; these two
 * make a new snapshot out of some rows of one, or out of all rows of several - to drop the callers that hung up, move some rows to
 * another device, fork a caller, or put two groups back into one.  The carried buffers keep the batch index in different places
 * (conv history [B][rows][HC], LSTM state [H][B], ...), so an engine supplies the layouts: `e` must be finalized and of the
 * snapshots' kind - the identity checks of se_stream_restore (model id, flags except SE_CFG_GRAPHS / SE_CFG_STREAM_SLIDING,
 * n_fft / hop / win, p_in / p_out), with its reasons.  The capacity checks (max_batch, max_samples, window, ring) are left to the
 * restore of the result.  Neither call touches the stream running on `e` or its workspace; both order themselves on `stream` as
 * se_stream_save does, run one kernel launch, and leave the result on e's device, where it exports like a saved snapshot.  An
 * imported image that has not been restored yet is uploaded to e's device first.  A `dst` that already holds the resulting layout
 * is reused without allocating.  A refused call changes nothing; the reason is read through se_last_error(e).
 *   select: dst = n_rows >= 1 rows of src, row j = row rows[j] (a host array; an index may repeat, which forks a caller; one outside
 *           0 .. batch - 1 is refused).  Every counter and mode is copied; batch becomes n_rows.  dst == src is refused.
 *   concat: dst = the rows of parts[0], then parts[1], ...  (n_parts >= 1; dst must be none of them).  The parts must agree in every
 *           manifest field except the batch - each differing field is refused with a reason that names it ("n_total 4160 vs 4000"):
 *           snapshots whose counters differ cannot be joined.
 * A snapshot taken before the model's state exists (before the first frame) holds the engine-level segments only and is handled.
 * A continued row decodes as it would have in its old group up to the fp32 rounding of kernels selected by batch size. */
int se_stream_state_select(se_engine* e, se_stream_state* dst, const se_stream_state* src, const int32_t* rows, int32_t n_rows,
                           void* stream);
int se_stream_state_concat(se_engine* e, se_stream_state* dst, const se_stream_state* const* parts, int32_t n_parts, void* stream);

/* Groups that began at different times (additions: the ABI number stays, and se_stream_state_concat keeps refusing differing counters
 * exactly as above).  Once a stream is past its left edge - no frame still to be transformed reads a reflected sample, no sample still
 * to be written lies under the deficient start of the overlap-add envelope - a decode step no longer depends on the stream's absolute
 * position, provided the position moves by whole hops.  A parked stream may then have its counters REBASED by a multiple of the hop,
 * and two parked groups whose counters differ by such a multiple be joined into one that advances in lockstep from then on, every
 * row getting what it would have got alone.
 *   join  : dst = the rows of parts[0], then parts[1], ... as concat, on the counters of parts[0]; every other part is rebased onto
 *           them.  `e`, `stream`, the upload of imported images, the reuse of `dst`, the single kernel launch and the untouched
 *           running stream are concat's; n_parts == 1 yields a copy.  A part is accepted when
 *             - every manifest field other than the positions (n_total, t_done, o_done, keep) agrees with parts[0] - concat's checks and
 *               wording ("parts[0] and parts[1] differ: max_chunk 16 vs 8");
 *             - it is in phase: the shift parts[0].n_total - n_total is a multiple of lcm(hop, 4) (the window origin `keep` is a multiple
 *               of 4 and stays one), and n_total - t_done * hop and n_total - o_done equal those of parts[0];
 *             - as soon as any shift is not 0, every part - parts[0] included - is past the left edge: t_done >= max(1,
 *               ceil(n_fft / 2 / hop), and where hop < n_fft / 2 ceil(n_fft / hop) - 1 + the model's frames of look-ahead), i.e. 1 for 320 / 160, 3 for
 *               512 / 128, 9 for the DCCRN whose decoder looks six frames ahead (csrc/stream_join.h has the derivation);
 *             - its state holds no absolute time: a running-scale stream is refused (its ring of 1 / c per frame is indexed by the
 *               absolute frame, and its sum by the absolute sample count; a TRACKING-scale stream is accepted - its (E, W) are relative,
 *               and its rings are rotated by shift / hop frames on the way, csrc/stream_join.h - with equal tau_samples), and so are the models whose state counts frames - CTSNet, TaylorSENet and G2Net with the cumulative
 *               LayerNorm, FullSubNet with the cumulative norm - unless the engine was created with SE_CFG_STREAM_ROW_ORIGINS: every
 *               row then carries its own frame origin, the join adds shift / hop to the origins of the rows it rebases, and these
 *               four configurations are accepted under the same phase and left-edge conditions (their state is per row, zero-initialised
 *               slots are the causal padding, and every model-side index is taken from the row's own origin).  CRN, LSTM, GCRN, DPCRN
 *               and DCCRN (complex or real LSTM core, either decoder) are accepted with or without the bit.
 *           Each failure is refused with its own reason, naming the field and both values.  Parts may have been saved with live input
 *           windows of different lengths; the result keeps, for every row, the samples from the highest rebased `keep` of any part.
 *           The capacity checks are left to the restore of the result: an engine without SE_CFG_STREAM_SLIDING restores it if
 *           parts[0].n_total fits its max_samples.  A joined row continues bit for bit as it would have alone at the same batch size;
 *           at another batch size up to the fp32 rounding of kernels selected by batch size, as after select and concat.
 *   counts: the host record a server needs to tell when a caller is in phase with a group - rows, samples received (n_total), frames
 *           transformed (t_done), samples emitted (o_done), the hop; any out-pointer may be NULL.  An empty object is an error
 *           (se_last_error(NULL)).  Works on an imported image without a GPU. */
int se_stream_state_join(se_engine* e, se_stream_state* dst, const se_stream_state* const* parts, int32_t n_parts, void* stream);
int se_stream_state_counts(const se_stream_state* s, int32_t* batch, int64_t* n_total, int64_t* t_done, int64_t* o_done, int32_t* hop);

/* se_enhance_batch for clips LONGER than max_samples (any length; shorter ones take the same path): `batch` equal-length clips
 * resident on the device, decoded in windows of max_chunk_frames frames through the frame-online machinery above - conv history,
 * TCM rings, LSTM (h, c) and the running norm sums carried from window to window - under the WHOLE clip's unit-RMS scale, so
 * the workspace stays the one planned for max_samples whatever n_samples is.  Row b of wav_out_dev receives
 * se_output_samples(e, n_samples) samples: what se_enhance_batch returns on an engine created with max_samples >= n_samples,
 * up to the fp32 rounding of the differently tiled recurrence (the streamed-vs-offline agreement of se_stream_flush).
 *   n_samples: n_fft ... 2^31 - 1 - n_fft - 32 hop (the position counters; independent of max_samples); batch <= max_batch.
 *   max_chunk_frames: frames per window; 0 = the largest the workspace was planned for (an offline caller wants large
 *                     windows, not the frame-online default of 16); larger values are clamped to that.
 * The input rows are read in place (pitch in_pitch, no copy, no stream window: SE_CFG_STREAM_SLIDING is not needed and the
 * buffers of se_stream_* are not allocated).  Only the models se_stream_begin accepts - a network that needs the whole
 * utterance (Uformer; FullSubNet with offline_laplace_norm or the GRU; CTSNet / G2Net / TaylorSENet with InstanceNorm weights)
 * is refused with the reason in se_last_error.  The call ENDS any stream running on the handle: a later se_stream_push /
 * se_stream_flush fails with "... without se_stream_begin" (a REFUSED call touches nothing: the stream goes on).  Ordered against frame-online calls on other hipStreams like the
 * other offline calls. */
int se_enhance_long(se_engine* e, const float* wav_in_dev, int64_t in_pitch, int32_t batch, int32_t n_samples,
                    int32_t max_chunk_frames, float* wav_out_dev, int64_t out_pitch, void* stream);

/* se_enhance_long for `batch` resident clips of DIFFERENT lengths, any of them longer than max_samples: one walk over the
 * windows of the longest row, every row under its own sizes.  `lengths` is a HOST array of `batch` sample counts, each in
 * n_fft ... 2^31 - 1 - n_fft - 32 hop (independent of max_samples; shorter clips take the same path).  Row b of wav_in_dev
 * holds lengths[b] valid samples and nothing past them is read; row b of wav_out_dev receives se_output_samples(e, lengths[b])
 * samples followed by zeros up to se_output_samples(e, max lengths).  Each row gets what se_enhance_long returns for that clip
 * alone, up to the fp32 rounding of the differently tiled recurrence: its own whole-clip unit-RMS scale, its own right-edge
 * reflection / tail pad and frame count (in whichever window holds its end), frames at or past its own last one transformed
 * to zeros and never overlap-added into its samples (every window's STFT / iSTFT launch sees the rows' frame counts clipped to the
 * frames that launch owns, derived on the device without a host synchronisation).  The networks are causal, so what a row's state holds after its end
 * never reaches a sample of it, and no operator on these paths reduces over the batch.  FullSubNet with the cumulative norm
 * looks two frames ahead at its input only and sees there the zero frames of the STFT, as it does when the row is decoded alone.
 * NOT accepted here by default: SE_MODEL_DCCRN with the look-ahead decoder (without SE_CFG_DCCRN_CAUSAL_DEC) - its decoder looks
 * one frame ahead per layer into tensors that are not zero behind a row's own last frame; the call refuses it with that reason
 * (se_enhance_long and se_enhance_ragged decode it as before).  An engine created with SE_CFG_DCCRN_ROW_ENDS is accepted: every
 * chunk then clears those tensors at or past each row's own end, layer by layer, and each row gets what se_enhance_long returns
 * for it alone, its last six frames included.
 *   max_chunk_frames: as se_enhance_long.  in_pitch >= max lengths (batch > 1), out_pitch >= se_output_samples(e, max lengths),
 *   batch <= max_batch.  Models, refusal reasons and the effect on a running stream: as se_enhance_long (a refused call
 *   touches nothing, an accepted one ends the stream). */
int se_enhance_long_ragged(se_engine* e, const float* wav_in_dev, int64_t in_pitch, int32_t batch, const int32_t* lengths,
                           int32_t max_chunk_frames, float* wav_out_dev, int64_t out_pitch, void* stream);

/* Stage hooks, so each oracle-pinned stage can be diffed alone (engine-internal spectrogram layout
 * [B][2][F][T] re/im planes, T contiguous, row pitch = T).
 *   se_stft     : torch.stft / librosa.stft call of the model's decode script, fused with x*c and |X|^p_in.
 *                 c_dev (may be NULL -> no scaling) holds one scale per utterance.
 *   se_istft    : torch.istft / librosa.istft (+ division by c when c_dev != NULL), n_out samples per row.
 *   se_rms_scale: c = sqrt(L / sum x^2).
 *   se_num_frames / se_num_bins: T and F for n_samples. */
int se_rms_scale(se_engine* e, const float* wav_dev, int64_t pitch, int32_t batch, int32_t n_samples, float* c_dev,
                 void* stream);
int se_stft(se_engine* e, const float* wav_dev, int64_t pitch, int32_t batch, int32_t n_samples,
            const float* c_dev, float p_in, float* spec_dev, void* stream);
int se_istft(se_engine* e, const float* spec_dev, int32_t batch, int32_t n_frames, const float* c_dev,
             float* wav_dev, int64_t pitch, int32_t n_out, void* stream);
int32_t se_num_frames(const se_engine* e, int32_t n_samples);
int32_t se_num_bins(const se_engine* e);

/* The two halves of a decode loop's body around `model(feat)` as stage hooks of their own (se_frontend /
 * se_backend), so that the front end and the mask / decompress stage can be diffed against the oracle alone.
 *   se_frontend: c = sqrt(L / sum x^2); x * c (+ the script's tail pad); STFT; |X|^p_in e^{j angle X} with the engine's p_in
 *                (e.g. DCCRN/dccrn_decode_vb.py:26-42, LSTM/lstm_decode_vb.py:33-38, GCRN/gcrn_decode_vb.py:35-46).
 *                wav_dev [batch][pitch] -> c_dev [batch], spec_dev [batch][2][F][T]  (T = se_num_frames(n_samples)).
 *   se_backend : network output -> estimated spectrum -> |S|^p_out e^{j angle S} (the engine's p_out) -> iSTFT -> / c.
 *                kind SE_BACKEND_RI   : est_dev [batch][2][F][T] IS the estimated spectrum (complex-mapping scripts:
 *                                       GCRN/gcrn_decode_vb.py:47-58, DCCRN/dccrn_decode_vb.py:45-62); spec_dev unused
 *                     SE_BACKEND_MAG  : est_dev [batch][F][T] is a magnitude, the phase is the noisy spectrum's
 *                                       (LSTM/lstm_decode_vb.py:47-52, CRN/crn_decode_vb.py:46-52)
 *                     SE_BACKEND_CMASK: est_dev [batch][2][F][T] is a complex ratio mask applied to spec_dev
 *                                       (FullSubNet/fullsubnet_sa_decode_vb.py:56-72, DPCRN/DPCRN.py:33-42)
 *                spec_dev: the front end's output (kinds MAG / CMASK); c_dev may be NULL (no division); n_out samples per row. */
#define SE_BACKEND_RI 0
#define SE_BACKEND_MAG 1
#define SE_BACKEND_CMASK 2
int se_frontend(se_engine* e, const float* wav_dev, int64_t pitch, int32_t batch, int32_t n_samples, float* c_dev,
                float* spec_dev, void* stream);
int se_backend(se_engine* e, int32_t kind, const float* est_dev, const float* spec_dev, int32_t batch, int32_t n_frames,
               const float* c_dev, float* wav_dev, int64_t pitch, int32_t n_out, void* stream);

/* Kernel time of the dominant kernel family (f32-MFMA implicit-GEMM convolution) inside the last
 * se_enhance_batch / se_forward, measured with HIP events on the stream each launch runs on (the caller's `stream` and the
 * engine's auxiliary streams: launches that overlap on two streams both count); enabled by se_set_profiling(e, 1).
 * Returns accumulated milliseconds and the launch count through the out-params. */
int se_set_profiling(se_engine* e, int32_t on);
int se_get_profile(se_engine* e, double* gemm_ms, int64_t* gemm_launches, double* gemm_flops);

/* The HBM-bound front / back-end kernels of the last profiled se_enhance_batch / se_enhance_ragged, per stage: accumulated
 * HIP-event milliseconds on `stream`, launch count, and the stage's ALGORITHMIC bytes (what it has to read and write once:
 * RMS 4L; STFT 4L + 8FT (+4FT magnitudes); mask apply / decompress 16-24 FT; iSTFT + overlap-add 8FT + 4L - per utterance,
 * SURVEY.md 8(d)).  bytes / ms against the HBM peak is the stage's roofline fraction (bench.py `roofline_stages`). */
enum se_stage { SE_STAGE_RMS = 0, SE_STAGE_STFT = 1, SE_STAGE_MASK = 2, SE_STAGE_ISTFT = 3 };
int se_get_stage_profile(se_engine* e, int32_t stage, double* ms, int64_t* launches, double* bytes);

/* Sample-rate conversion in front of the path: librosa.resample(y, sr_in, sr_out, fix=True, scale=False) as called at
 * DCCRN/dccrn_decode_vb.py:26 and LSTM/lstm_decode_vb.py:34 (VoiceBank+DEMAND ships at 48 kHz; the models run at 16 kHz).
 * Stateless (no engine handle; errors through se_last_error(NULL)).  Device pointers; `n_in` samples per row in,
 * se_resample_samples(n_in, sr_in, sr_out) = ceil(n_in * sr_out / sr_in) samples per row out.
 * Calls may be in flight on several hipStreams at once, at equal or different ratios, and may come from several threads: the
 * filter table and (for sr_in % sr_out != 0) the table of read positions are kept per ratio and device from the first call at
 * that ratio on, shared with se_resample_ragged, written once and then only read.  A later call at a known ratio waits for
 * nothing; a call waits for the device only when its row is longer than any seen at its ratio and the position table grows. */
int64_t se_resample_samples(int32_t n_in, int32_t sr_in, int32_t sr_out);
int se_resample(const float* in_dev, int64_t in_pitch, int32_t batch, int32_t n_in, int32_t sr_in, int32_t sr_out,
                float* out_dev, int64_t out_pitch, void* stream);

/* The same conversion for rows of DIFFERENT lengths in one call - the clips of a directory in front of se_enhance_ragged.  Stateless
 * like se_resample (no handle, errors through se_last_error(NULL), work enqueued on `stream`).
 *   in_dev  [batch][in_pitch] (elements): row b holds n_in[b] valid samples - float (SE_SAMPLES_F32), or int16 as a PCM_16 file
 *           stores them (SE_SAMPLES_S16: value / 32768, exact in fp32, as se_pcm16_decode).  n_in is a HOST array of `batch`
 *           entries, read before the call returns.  Nothing past a row's own length is read.
 *   out_dev [batch][out_pitch]: row b receives se_resample_samples(n_in[b], sr_in, sr_out) samples, then zeros up to
 *           se_resample_samples(max n_in, sr_in, sr_out) - the row convention of se_enhance_ragged, which takes the buffer as it
 *           is.  Nothing past that is written.
 *   CONTRACT: row b's samples equal, as numbers, what se_resample returns for that clip alone (for SE_SAMPLES_S16: se_pcm16_decode
 *   followed by se_resample) - the same float64 sum term by term at the same read positions, the fix_length zero tail included.
 *   sr_in == sr_out copies (and converts) the rows through.
 * The row lengths travel as kernel arguments, 64 rows a launch: a batch is ceil(batch / 64) launches and no copy.  The filter
 * table is kept per ratio and device from the first call at that ratio on.  For sr_in % sr_out == 0 a later call allocates nothing
 * and waits for nothing.  For other ratios the table of read positions (a function of the output index and the ratio alone) is
 * kept per ratio too, shared by all rows and long enough for the longest row seen: a call waits for the device only when that
 * table has to grow.  Calls may come from several threads and hipStreams.
 * Refused, each with its own reason and before anything is enqueued: a null pointer; batch < 1; an n_in[b] < 1 (named by index); a
 * format other than the two; rates <= 0 (or sr_out / sr_in below the filter table's resolution, 1 / 512); in_pitch below the
 * longest row or out_pitch below its output when batch > 1; a row whose output count passes 2^31 - 1. */
#define SE_SAMPLES_F32 0
#define SE_SAMPLES_S16 1
int se_resample_ragged(const void* in_dev, int32_t in_format, int64_t in_pitch, int32_t batch, const int32_t* n_in /* HOST */,
                       int32_t sr_in, int32_t sr_out, float* out_dev, int64_t out_pitch, void* stream);

/* The same conversion for a signal that arrives piecewise - in front of se_stream_*, whose 16 kHz input a live source delivers at
 * 48 / 44.1 / 32 kHz.  A stand-alone object next to the engine (no engine handle, errors through se_last_error(NULL)); one
 * object serves `batch` <= max_batch parallel rows that advance together, on the device that is current at create.  All device
 * memory (two history buffers of max_batch x 2 * reach floats, the filter table, for non-integer ratios a ring of read positions)
 * is allocated at create; push and flush allocate nothing.  A handle is not thread-safe.
 *   CONTRACT: for any split of a signal of n samples into pushes of 1 ... max_push samples, the outputs of the pushes followed by
 *   the output of the flush, concatenated, are the se_resample_samples(n, sr_in, sr_out) samples se_resample returns for the
 *   whole signal - equal as numbers, sample for sample (the same float64 sum in the same order at the same read positions),
 *   the zero tail of librosa's fix_length included.
 *   se_resampler_begin: starts (or restarts: all state is reset) a signal of `batch` rows.
 *   se_resampler_push : in_dev [batch][in_pitch], n_new new samples per row (0 ... max_push; 0 does nothing); the output samples
 *                       this push makes final - those whose filter taps have all arrived - go to the start of each row of out_dev
 *                       [batch][out_pitch].  *n_out (a HOST value, the same for all rows, 0 is normal) = their count =
 *                       se_resampler_ready_samples(after) - se_resampler_ready_samples(before), at most ceil(n_new * sr_out /
 *                       sr_in) + 1.  Pitches are ignored when batch == 1.
 *   se_resampler_flush: the signal has ended: the remaining outputs (right filter wing cut at the end, as offline) and the zero
 *                       tail, at most ceil((reach + 1) * sr_out / sr_in) + 2 per row; the object then waits for the next begin.
 *   sr_in == sr_out   : the input is copied through - n_out = n_new, flush returns 0.
 *   LATENCY: the filter looks floor(32769 / step) input samples ahead, step = floor(512 min(1, sr_out / sr_in)): 192 samples
 *   = 4 ms at 48 -> 16 kHz (128 at 32 -> 16 kHz, 177 at 44.1 -> 16 kHz, 64 when upsampling) - the algorithmic latency.  The
 *   release rule rounds it up and is one sample late: the output read at input position p is returned by the push that brings
 *   sample p + reach, reach = floor(32769 / step) + 1 (193 at 48 -> 16 kHz) - so a signal of up to reach samples comes out of
 *   the flush alone.
 *   WAITS: when sr_in is a multiple of sr_out (48 / 32 -> 16 kHz) a push enqueues one kernel and calls nothing that waits for the
 *   device.  Other ratios carry resampy's running float64 read position on the host and hand a push's positions to the device
 *   through a ring of 8 pinned slots; the host waits (hipEventSynchronize) only for the copy enqueued 8 pushes earlier.
 *   ERRORS (a refused call changes no state: the signal goes on): n_new above max_push; batch above max_batch; push or flush
 *   without begin; a total length beyond what se_resample accepts (2^31 - 1 samples, in or out); a row pitch below the row.
 * se_resampler_ready_samples is stateless and host-only: how many output samples are final once n_in input samples of a signal
 * that has not ended have arrived (-1: bad arguments).  For sr_in % sr_out != 0 it walks the running sum, O(n_in). */
typedef struct se_resampler se_resampler;
int se_resampler_create(int32_t sr_in, int32_t sr_out, int32_t max_batch, int32_t max_push, se_resampler** out);
int se_resampler_destroy(se_resampler* r);
int se_resampler_begin(se_resampler* r, int32_t batch, void* stream);
int se_resampler_push(se_resampler* r, const float* in_dev, int64_t in_pitch, int32_t n_new, float* out_dev, int64_t out_pitch,
                      int32_t* n_out, void* stream);
int se_resampler_flush(se_resampler* r, float* out_dev, int64_t out_pitch, int32_t* n_out, void* stream);
int64_t se_resampler_ready_samples(int64_t n_in, int32_t sr_in, int32_t sr_out);

/* Parking a source-rate signal and putting it back: what se_stream_save / se_stream_restore are to a handle's stream, for a
 * se_resampler.  Together they park a stream that is fed at the source's rate (a resampler in front of se_stream_push): save both,
 * restore both.  One object can so serve more signals than max_batch by turns: restore -> push -> save per signal.
 *   CONTRACT: take any signal on a se_resampler and any point between two calls on it - before its first push, after a push that
 *   released nothing, after its last push.  Save it.  Let anything else happen on the object: other signals, including ones that
 *   overwrite both history buffers, nothing at all.  Restore it there, or on another object created with the same sr_in / sr_out.
 *   The outputs of every later se_resampler_push and of se_resampler_flush then equal those of the uninterrupted signal bit for
 *   bit, *n_out included - so the concatenation still equals se_resample of the whole signal, sample for sample.
 * The object holds a host record (sr_in, sr_out, batch, the samples arrived, the first sample of the history, the next output and
 * the running float64 read position as its 8 bytes) and one device payload: the live history of every row, rows back to back, at
 * most 2 * reach floats per row.  Which of the two history buffers was current, the pinned position ring and the filter table are
 * not part of it: a push's read positions are re-derived from the record.  A pass-through object (sr_in == sr_out) saves counters
 * only: a payload of 0 bytes.
 *   se_resampler_state_create : an empty object; touches no device.  se_resampler_state_destroy releases it (NULL: nothing).
 *   se_resampler_state_bytes  : device memory of the payload (sized for the most a signal of that batch keeps, so the figure does
 *                               not move from save to save; of an imported image not restored yet: its payload); 0 = empty.
 *   se_resampler_state_counts : the host record - rates, rows, input samples arrived (n_in), output samples released (n_out); any
 *                               out-pointer may be NULL.  An empty object is an error.
 *   se_resampler_save   : needs an open signal on r ("... without se_resampler_begin" / "... after se_resampler_flush" otherwise);
 *                         does not end or alter it.  One kernel, enqueued on `stream`, ordered against the object's last call like
 *                         push and flush.  The first save into an object allocates its payload; saving again into an object that
 *                         holds the same (sr_in, sr_out, batch) allocates nothing, and no save waits for the device.
 *   se_resampler_restore: r must convert the same sr_in -> sr_out, have max_batch >= the snapshot's batch and live on the device the
 *                         payload lives on (an imported image goes anywhere); max_push may differ.  Each mismatch, and an empty
 *                         object, is refused with its own reason.  It replaces whatever signal is open on r, as se_resampler_begin
 *                         does.  One kernel into the current history buffer; the first restore of an imported image uploads its
 *                         payload once (synchronously).  The same object may be restored any number of times and on more than one
 *                         se_resampler: that forks a signal.
 *   se_resampler_state_export / _import: the object as one byte string in HOST memory, as se_stream_state_export / _import:
 *                         synchronous; export with cap == 0 returns the size needed, else the size written (-1: error).  import
 *                         parses and validates on the host - it runs, and refuses, without a GPU: a wrong magic or version, an
 *                         image cut short, a payload size that is not batch * (n_total - w0) * 4, negative or overflowing
 *                         counters, w0 > n_total, more history than 2 * reach of the recorded rates, and trailing bytes.
 * Errors are read through se_last_error(NULL).  A refused call changes nothing: neither the object nor the signal running on r.  An
 * object is not thread-safe, and like a se_resampler it orders calls made on different hipStreams behind one another. */
typedef struct se_resampler_state se_resampler_state;
int se_resampler_state_create(se_resampler_state** out);
int se_resampler_state_destroy(se_resampler_state* s);
int64_t se_resampler_state_bytes(const se_resampler_state* s);
int se_resampler_state_counts(const se_resampler_state* s, int32_t* sr_in, int32_t* sr_out, int32_t* batch, int64_t* n_in,
                              int64_t* n_out);
int se_resampler_save(se_resampler* r, se_resampler_state* s, void* stream);
int se_resampler_restore(se_resampler* r, const se_resampler_state* s, void* stream);
int64_t se_resampler_state_export(const se_resampler_state* s, void* host_buf, int64_t cap);
int se_resampler_state_import(se_resampler_state* s, const void* host_buf, int64_t bytes);
/* The same row operations on the resampler's half of a parked group: the payload is [batch][n_total - w0] floats, so no engine is
 * needed.  select: rows[j] of src (repeats allowed, dst != src, n_rows >= 1); concat: the parts' rows in order - sr_in / sr_out, the
 * samples in and out, the history origin and the 8 bytes of the read position must agree, each difference is refused by name.
 * Pass-through states hold counters only.  The result lives where the sources do: on their device, or on the host when every
 * source is an imported image that has not been restored yet.  Errors through se_last_error(NULL). */
int se_resampler_state_select(se_resampler_state* dst, const se_resampler_state* src, const int32_t* rows, int32_t n_rows, void* stream);
int se_resampler_state_concat(se_resampler_state* dst, const se_resampler_state* const* parts, int32_t n_parts, void* stream);

/* Source-rate signals that began at different times: what se_stream_state_join is to the engine's half of a parked group, for the
 * resampler's half (an addition: the ABI number stays, and se_resampler_state_concat keeps refusing differing counters exactly as
 * above).  For an integer decimation (sr_in % sr_out == 0, D = sr_in / sr_out) output t reads around input position t * D exactly and
 * every index a push forms is that position plus a constant; once the left filter wing no longer reaches position 0 a parked signal
 * may have its counters REBASED by a multiple of D (n_in and the history origin by s, n_out by s / D), and two parked groups whose
 * counters differ by such a multiple be joined into one that advances in lockstep (csrc/resampler_join.h has the derivation).
 *   join  : dst = the rows of parts[0], then parts[1], ... as concat, on the counters of parts[0]; every other part is rebased onto
 *           them.  n_parts == 1 yields a copy; n_parts < 1, a null entry, an empty object and dst among the parts are refused as
 *           concat refuses them.  A part is accepted when
 *             - sr_in and sr_out agree with parts[0] - concat's wording ("parts[0] and parts[1] differ: sr_in 48000 vs 44100");
 *             - the ratio is an integer decimation whose flush arithmetic has been walked over every length: D = 1 (pass-through),
 *               2, 3.  44.1 -> 16 kHz and any upsampling are refused ("the read position is a running float64 sum from the signal's
 *               start (sr_in % sr_out != 0)"), every other D by name;
 *             - it is in phase: the shift parts[0].n_in - n_in is a multiple of D, and n_in - n_out * D equals that of parts[0];
 *             - as soon as any shift is not 0, every part - parts[0] included - is past the left edge: n_out * D >= reach - 2, i.e.
 *               n_out >= 64 at 48 -> 16 kHz and at 32 -> 16 kHz (reach: LATENCY above); the refusal names n_out, the threshold and
 *               the rates;
 *             - the joined history origin lies inside the samples it holds.
 *           Parts may have been saved with histories of different lengths; the result keeps, for every row, the samples from the
 *           highest rebased origin of any part.  Its record is parts[0]'s counters with that origin and the read position n_out * D.
 *           Pass-through states hold counters only: any shift is accepted and the result has a payload of 0 bytes.  The result lives
 *           where the sources do: when every source is an imported image that has not been restored yet the join runs on the host and
 *           touches no device; imported parts among device parts are uploaded first.  A dst that already holds the layout is reused
 *           without allocating.  One kernel per 64 rows, enqueued on `stream` and ordered against the objects' last use as
 *           se_resampler_save is.  A refused call changes nothing; errors through se_last_error(NULL).
 *   CONTRACT: restore the result on any se_resampler of the same rates with max_batch >= its rows.  The outputs of every later
 *   se_resampler_push and of se_resampler_flush then equal, bit for bit and *n_out included, what each row's signal would have
 *   produced uninterrupted.  (The sum is per output and per row in float64, so the batch size does not enter.) */
int se_resampler_state_join(se_resampler_state* dst, const se_resampler_state* const* parts, int32_t n_parts, void* stream);

/* The two ends of `enhance(args)`: `feat_wav, orig_fs = sf.read(path)` hands out int16 / 32768 as floats, and
 * `sf.write(path, y, fs)` stores PCM_16 (soundfile's default subtype for .wav: round to nearest, clipped) - e.g.
 * DCCRN/dccrn_decode_vb.py:25,64.  Both conversions are exact in fp32, so they run on the device and the host moves raw
 * 2-byte samples only.  Stateless; rows of `n` samples, pitches in elements. */
int se_pcm16_decode(const int16_t* in_dev, int64_t in_pitch, int32_t batch, int32_t n, float* out_dev, int64_t out_pitch,
                    void* stream);
int se_pcm16_encode(const float* in_dev, int64_t in_pitch, int32_t batch, int32_t n, int16_t* out_dev, int64_t out_pitch,
                    void* stream);

/* ABI version of this header. */
int32_t se_abi_version(void);   /* 2: se_enhance_ragged, se_get_stage_profile, se_stream_*; 3: se_uformer_forward, se_pcm16_*; 4: se_stream_begin_running; 5: se_frontend, se_backend (+ the flag bits SE_CFG_DCCRN_CAUSAL_DEC, SE_CFG_STREAM_SLIDING: no new entry point, same number; + se_enhance_long, se_enhance_long_ragged: added entry points, nothing existing changes, same number; + se_resampler_*: likewise; + se_stream_state_*, se_stream_save, se_stream_restore: likewise; + se_resampler_state_*, se_resampler_save, se_resampler_restore: likewise; + se_resampler_state_join: likewise; + the flag bit SE_CFG_DCCRN_ROW_ENDS: no new entry point, same number; + the flag bit SE_CFG_STREAM_ROW_ORIGINS: likewise, and a snapshot segment kind only engines with the bit write; + the flag bits SE_CFG_FSN_GAUSSIAN, SE_CFG_FSN_CUM_LAYERNORM: no new entry point, same number; + the flag fields SE_CFG_FSN_LOOK_AHEAD, SE_CFG_FSN_FB_NEIGHBORS: likewise) */

#ifdef __cplusplus
}
#endif
#endif /* SE_ENGINE_H */
