// The resampler fed piecewise (se_resampler_* of include/se_engine.h; k_resample.hip): push / flush enqueue one launch each and
// return how many samples per row they wrote to the start of `out`; errors are thrown like everywhere else.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace se {

// The offline resampler (launch_resample of kernels.h) for rows of different lengths in one call (se_resample_ragged): row b holds
// n_in[b] (HOST array) float or PCM_16 samples (in_format: SE_SAMPLES_*) and gets what launch_resample gives it alone, then zeros up
// to the longest row's output; makes every check of the call itself (resample_ragged.h) before anything is enqueued
void launch_resample_ragged(const void* x, int in_format, long in_pitch, int batch, const int32_t* n_in, int sr_in, int sr_out, float* y,
                            long out_pitch, hipStream_t s);

class StreamResampler;
StreamResampler* stream_resampler_create(int sr_in, int sr_out, int max_batch, int max_push);
void stream_resampler_destroy(StreamResampler* r);
void stream_resampler_begin(StreamResampler* r, int batch, hipStream_t s);
int stream_resampler_push(StreamResampler* r, const float* in, long in_pitch, int n_new, float* out, long out_pitch, hipStream_t s);
int stream_resampler_flush(StreamResampler* r, float* out, long out_pitch, hipStream_t s);
// outputs that are final once n_in samples of a signal that has not ended have arrived (host arithmetic, resample_pos.h)
long resample_ready_samples(long n_in, int sr_in, int sr_out);

// A parked signal (se_resampler_state of include/se_engine.h): the host record of resampler_manifest.h + one device payload.
// save / restore enqueue one copy kernel; export is the one call that waits for the device; import touches none.
struct ResamplerState;
ResamplerState* resampler_state_create();
void resampler_state_destroy(ResamplerState* s);
int64_t resampler_state_bytes(const ResamplerState* s);
void resampler_state_counts(const ResamplerState* s, int32_t* sr_in, int32_t* sr_out, int32_t* batch, int64_t* n_in, int64_t* n_out);
void stream_resampler_save(StreamResampler* r, ResamplerState* s, hipStream_t st);
void stream_resampler_restore(StreamResampler* r, ResamplerState* s, hipStream_t st);
int64_t resampler_state_export(const ResamplerState* s, void* host_buf, int64_t cap);
void resampler_state_import(ResamplerState* s, const void* host_buf, int64_t bytes);
// rows of parked signals: dst <- rows[j] of src / the rows of parts[0], parts[1], ... (include/se_engine.h)
void resampler_state_select(ResamplerState* dst, ResamplerState* src, const int32_t* rows, int32_t n_rows, hipStream_t st);
void resampler_state_concat(ResamplerState* dst, ResamplerState* const* parts, int32_t n_parts, hipStream_t st);
// concat for parts that began at different times: every part rebased onto the counters of parts[0] (resampler_join.h)
void resampler_state_join(ResamplerState* dst, ResamplerState* const* parts, int32_t n_parts, hipStream_t st);

}  // namespace se
