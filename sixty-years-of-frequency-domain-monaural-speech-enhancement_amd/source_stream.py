"""Frame-online decoding fed at the source's sample rate: a `StreamResampler` in front of `Engine.stream_begin` /
`stream_push` / `stream_flush`.

The engine streams at the models' 16 kHz; a microphone or a 48 kHz file reader delivers 48 / 44.1 / 32 kHz.  A push at `sr_in`
is resampled on the device - the samples `resample()` would give for the whole signal, as far as they are final - and those go
into the engine's stream; what comes back is the engine's 16 kHz output (the reference writes 16 kHz files: nothing is
converted back to `sr_in`).  The engine and its stream state are used as they are; on top of the engine's own latency the
resampler looks 192 input samples (4 ms) ahead at 48 -> 16 kHz.
"""
from .resample import StreamResampler


class SourceRateStream:
    """`SourceRateStream(model.engine, 48000)`: `begin(batch, ...)`, `push(x)` with x [batch, n <= max_push] at sr_in ->
    enhanced 16 kHz samples [batch, n_out] (n_out may be 0), `flush()` -> the rest.  `begin` takes what `Engine.stream_begin`
    takes: a per-stream scale `c` (of the 16 kHz signal, e.g. from a calibration run) or `running_rms=True`.
    Not covered by `Engine.stream_save` / `stream_restore`: the resampler in front carries state of its own (filter history, read
    position) that a StreamSnapshot does not hold, so a stream fed through this class cannot be parked and resumed."""

    def __init__(self, engine, sr_in, sr_out=16000, max_push=None):
        self.engine = engine
        self.resampler = StreamResampler(sr_in, sr_out, max_batch=engine.max_batch, max_push=max_push, device=engine.device)
        self._batch = 0

    def begin(self, batch, c=None, max_chunk_frames=16, running_rms=False):
        self._batch = 0
        self.engine.stream_begin(batch, c=c, max_chunk_frames=max_chunk_frames, running_rms=running_rms)
        self.resampler.begin(batch)
        self._batch = int(batch)

    def _empty(self, like):
        return like.new_empty((self._batch, 0))

    def push(self, x):
        y = self.resampler.push(x)
        if y.shape[1] == 0:                  # nothing final at 16 kHz yet: the engine is not called
            return self._empty(y)
        return self.engine.stream_push(y)

    def flush(self):
        import torch
        tail = self.resampler.flush()
        outs = [self.engine.stream_push(tail)] if tail.shape[1] else []
        outs.append(self.engine.stream_flush())
        self._batch = 0
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=1)

    def close(self):
        self.resampler.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
