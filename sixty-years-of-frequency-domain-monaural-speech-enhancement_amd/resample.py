"""`librosa.resample(y, orig_sr, target_sr, fix=True, scale=False)` on the GPU (csrc/k_resample.hip through the C ABI).

The reference decode scripts resample every clip to 16 kHz right after reading it (DCCRN/dccrn_decode_vb.py:26,
LSTM/lstm_decode_vb.py:34).  No CPU fallback: the call fails without the HIP library / a GPU.

`resample()` needs the whole clip; `StreamResampler` takes the same signal piecewise (a microphone, a 48 kHz file reader in
front of the frame-online engine) and returns, push by push, the very samples `resample()` gives for the whole of it.
"""
import math
import ctypes as C

from . import _lib


def resample_samples(n_in, sr_in, sr_out):
    return int(_lib.load().se_resample_samples(int(n_in), int(sr_in), int(sr_out)))


def resample(wav, sr_in, sr_out=16000):
    """wav: float32 cuda tensor [B, L] (or [L]) -> [B, ceil(L * sr_out / sr_in)]."""
    import torch
    lib = _lib.load()
    squeeze = wav.dim() == 1
    x = wav[None] if squeeze else wav
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    if sr_in == sr_out:
        return wav
    B, L = x.shape
    n_out = resample_samples(L, sr_in, sr_out)
    y = torch.empty((B, n_out), dtype=torch.float32, device=x.device)
    st = C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    rc = lib.se_resample(C.c_void_p(x.data_ptr()), x.stride(0) if B > 1 else L, B, L, int(sr_in), int(sr_out),
                         C.c_void_p(y.data_ptr()), n_out, st)
    if rc:
        raise RuntimeError(lib.se_last_error(None).decode())
    return y[0] if squeeze else y


def ready_samples(n_in, sr_in, sr_out):
    """Output samples that are final once n_in input samples of a signal that has not ended have arrived (host arithmetic)."""
    return int(_lib.load().se_resampler_ready_samples(int(n_in), int(sr_in), int(sr_out)))


class StreamResampler:
    """The stateful form of `resample()` (se_resampler_* of include/se_engine.h): `begin(batch)`, then `push(x)` with
    x [batch, 1..max_push] at sr_in -> the output samples [batch, n_out] that became final (n_out may be 0: the filter looks 192
    input samples ahead at 48 -> 16 kHz), then `flush()` -> the rest.  Concatenated they equal `resample()` of the whole signal
    sample for sample.  All device memory is allocated here, for max_batch rows and pushes of up to max_push samples
    (default: 100 ms at sr_in); the object lives on `device` (default: torch's current one)."""

    def __init__(self, sr_in, sr_out=16000, max_batch=1, max_push=None, device=None):
        self.sr_in, self.sr_out, self.max_batch = int(sr_in), int(sr_out), int(max_batch)
        self.max_push = int(max_push) if max_push is not None else max(1, self.sr_in // 10)
        self._h = C.c_void_p()
        self._batch = 0            # rows of the open signal (0 = none)
        self._n_in = self._n_out = 0
        self._lib = _lib.load()
        import torch
        self.device = torch.cuda.current_device() if device is None else int(device)
        with torch.cuda.device(self.device):
            if self._lib.se_resampler_create(self.sr_in, self.sr_out, self.max_batch, self.max_push, C.byref(self._h)):
                self._h = C.c_void_p()
                raise RuntimeError(self._lib.se_last_error(None).decode())

    def close(self):
        if getattr(self, '_h', None) is not None and self._h.value:
            self._lib.se_resampler_destroy(self._h)
            self._h = C.c_void_p()
            self._batch = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _check(self, rc):
        if rc:
            raise RuntimeError(self._lib.se_last_error(None).decode())

    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def begin(self, batch=1):
        """Start (or restart) a signal of `batch` rows; everything carried from an earlier signal is dropped."""
        self._check(self._lib.se_resampler_begin(self._h, int(batch), self._stream()))
        self._batch = int(batch)
        self._n_in = self._n_out = 0

    def push(self, x):
        """x: float32 cuda tensor [batch, n] (or [n] for a stream of one row) at sr_in -> [batch, n_out] (or [n_out]) at sr_out."""
        import torch
        squeeze = x.dim() == 1
        x = x[None] if squeeze else x
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1      # as resample()
        assert x.device.index == self.device, f"tensor on cuda:{x.device.index}, the resampler lives on cuda:{self.device}"
        B, n = x.shape
        if self._batch and B != self._batch:
            raise RuntimeError(f"push: {B} rows pushed into a signal of {self._batch}")
        cap = n if self.sr_in == self.sr_out else math.ceil(n * self.sr_out / self.sr_in) + 1
        y = torch.empty((B, max(cap, 1)), dtype=torch.float32, device=x.device)
        n_out = C.c_int32(0)
        self._check(self._lib.se_resampler_push(self._h, C.c_void_p(x.data_ptr()), x.stride(0) if B > 1 else max(n, 1), n,
                                                C.c_void_p(y.data_ptr()), y.stride(0), C.byref(n_out), self._stream()))
        self._n_in += n
        self._n_out += n_out.value
        y = y[:, :n_out.value]
        return y[0] if squeeze else y

    def flush(self):
        """End of the signal: the remaining samples [batch, n_out], `resample_samples(total)` in all with the pushes' outputs."""
        import torch
        if not self._batch:
            raise RuntimeError("flush without begin")
        rest = 0
        if self.sr_in != self.sr_out and self._n_in > 0:
            rest = resample_samples(self._n_in, self.sr_in, self.sr_out) - self._n_out
        y = torch.empty((self._batch, max(rest, 1)), dtype=torch.float32, device=torch.device('cuda', self.device))
        n_out = C.c_int32(0)
        self._check(self._lib.se_resampler_flush(self._h, C.c_void_p(y.data_ptr()), y.stride(0), C.byref(n_out), self._stream()))
        self._batch = 0
        return y[:, :n_out.value]
