// The resampler fed piecewise (se_resampler_* of include/se_engine.h; k_resample.hip): push / flush enqueue one launch each and
// return how many samples per row they wrote to the start of `out`; errors are thrown like everywhere else.
#pragma once
#include <hip/hip_runtime.h>

namespace se {

class StreamResampler;
StreamResampler* stream_resampler_create(int sr_in, int sr_out, int max_batch, int max_push);
void stream_resampler_destroy(StreamResampler* r);
void stream_resampler_begin(StreamResampler* r, int batch, hipStream_t s);
int stream_resampler_push(StreamResampler* r, const float* in, long in_pitch, int n_new, float* out, long out_pitch, hipStream_t s);
int stream_resampler_flush(StreamResampler* r, float* out, long out_pitch, hipStream_t s);
// outputs that are final once n_in samples of a signal that has not ended have arrived (host arithmetic, resample_pos.h)
long resample_ready_samples(long n_in, int sr_in, int sr_out);

}  // namespace se
