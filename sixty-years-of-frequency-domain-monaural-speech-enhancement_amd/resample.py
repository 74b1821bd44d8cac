"""`librosa.resample(y, orig_sr, target_sr, fix=True, scale=False)` on the GPU (csrc/k_resample.hip through the C ABI).

The reference decode scripts resample every clip to 16 kHz right after reading it (DCCRN/dccrn_decode_vb.py:26,
LSTM/lstm_decode_vb.py:34).  No CPU fallback: the call fails without the HIP library / a GPU.

`resample()` needs the whole clip, and clips of one length; `resample_ragged()` takes whole clips of different lengths in one
call, float32 or raw PCM_16, and gives each the samples `resample()` gives it alone (the file driver's staged batch); `StreamResampler` takes the same signal piecewise (a microphone, a 48 kHz file reader in
front of the frame-online engine) and returns, push by push, the very samples `resample()` gives for the whole of it.
"""
import math
import ctypes as C

from . import _lib
from .engine import EngineError


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


SAMPLES_F32, SAMPLES_S16 = 0, 1            # SE_SAMPLES_* of include/se_engine.h


def resample_ragged(x, lengths, sr_in, sr_out=16000, out=None):
    """Rows of different lengths in one call (se_resample_ragged).  x: cuda tensor [B, pitch], float32 or int16 (PCM_16 samples as
    the file stores them: value / 32768); row b holds lengths[b] valid samples, nothing behind them is read.
    -> float32 [B, resample_samples(max(lengths))]: row b is `resample()` of that clip alone, sample for sample, then zeros - the rows
    `Engine.enhance_ragged` takes.  `out`: a float32 cuda tensor of at least that many columns to write into (the view of its first
    columns is returned; nothing behind them is written)."""
    import torch
    if not (isinstance(x, torch.Tensor) and x.dim() == 2):
        raise EngineError("resample_ragged: x has to be a tensor [B, pitch]")
    if x.dtype not in (torch.float32, torch.int16):
        raise EngineError(f"resample_ragged: x is {x.dtype}, the rows are float32 or int16")
    if x.stride(1) != 1:
        raise EngineError("resample_ragged: the samples of a row have to be contiguous")
    B, pitch = x.shape
    lengths = [int(n) for n in lengths]
    if len(lengths) != B:
        raise EngineError(f"resample_ragged: {len(lengths)} lengths for {B} rows")
    if B < 1:
        raise EngineError("resample_ragged: at least one row has to be given")
    for b, n in enumerate(lengths):
        if not 1 <= n <= pitch:
            raise EngineError(f"resample_ragged: lengths[{b}] = {n} outside 1..{pitch}, the samples a row of x holds")
    sr_in, sr_out = int(sr_in), int(sr_out)
    if sr_in <= 0 or sr_out <= 0:
        raise EngineError(f"resample_ragged: sample rates {sr_in} -> {sr_out} Hz: both have to be positive")
    if not x.is_cuda:
        raise EngineError("resample_ragged: x has to live on the GPU")
    n_out = resample_samples(max(lengths), sr_in, sr_out)
    if out is None:
        out = torch.empty((B, n_out), dtype=torch.float32, device=x.device)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == x.device and out.dtype == torch.float32 and out.dim() == 2
              and out.stride(1) == 1 and out.shape[0] == B and out.shape[1] >= n_out):
        raise EngineError(f"resample_ragged: out has to be a float32 tensor [{B}, >= {n_out}] on {x.device}")
    lib = _lib.load()
    arr = (C.c_int32 * B)(*lengths)
    with torch.cuda.device(x.device):
        st = C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
        rc = lib.se_resample_ragged(C.c_void_p(x.data_ptr()), SAMPLES_S16 if x.dtype == torch.int16 else SAMPLES_F32,
                                    x.stride(0) if B > 1 else pitch, B, arr, sr_in, sr_out, C.c_void_p(out.data_ptr()),
                                    out.stride(0) if B > 1 else out.shape[1], st)
    if rc:
        raise EngineError(lib.se_last_error(None).decode())
    return out[:, :n_out]


def ready_samples(n_in, sr_in, sr_out):
    """Output samples that are final once n_in input samples of a signal that has not ended have arrived (host arithmetic)."""
    return int(_lib.load().se_resampler_ready_samples(int(n_in), int(sr_in), int(sr_out)))


class ResamplerSnapshot:
    """A parked `StreamResampler` signal (se_resampler_state of include/se_engine.h): what `StreamResampler.save()` fills and
    `StreamResampler.restore()` puts back - on the same object or on another of the same sr_in / sr_out, any number of times.
    `to_bytes()` / `from_bytes()` move it through host memory (another device, another process)."""

    def __init__(self):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        self.device = None         # where a save put the payload (None: empty, or an imported image, which goes anywhere)
        if self._lib.se_resampler_state_create(C.byref(self._h)):
            self._h = C.c_void_p()
            raise EngineError(self._lib.se_last_error(None).decode())

    @property
    def closed(self):
        return getattr(self, '_h', None) is None or not self._h.value

    def close(self):
        if not self.closed:
            self._lib.se_resampler_state_destroy(self._h)
            self._h = C.c_void_p()

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

    @property
    def nbytes(self):
        """device memory of the payload (0 = empty, or a pass-through signal)"""
        if self.closed:
            raise EngineError("ResamplerSnapshot.nbytes: the snapshot is closed")
        return int(self._lib.se_resampler_state_bytes(self._h))

    def counts(self):
        """(sr_in, sr_out, batch, n_in, n_out) of the saved signal: the host record; an empty snapshot is an error"""
        if self.closed:
            raise EngineError("ResamplerSnapshot.counts: the snapshot is closed")
        sr_in, sr_out, batch, n_in, n_out = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int64(0), C.c_int64(0)
        if self._lib.se_resampler_state_counts(self._h, C.byref(sr_in), C.byref(sr_out), C.byref(batch), C.byref(n_in), C.byref(n_out)):
            raise EngineError(self._lib.se_last_error(None).decode())
        return sr_in.value, sr_out.value, batch.value, n_in.value, n_out.value

    def to_bytes(self):
        """the snapshot as one byte string (header + payload); synchronises with the save that filled it"""
        if self.closed:
            raise EngineError("ResamplerSnapshot.to_bytes: the snapshot is closed")
        n = int(self._lib.se_resampler_state_export(self._h, None, 0))
        if n < 0:
            raise EngineError(self._lib.se_last_error(None).decode())
        buf = C.create_string_buffer(n)
        if self._lib.se_resampler_state_export(self._h, C.cast(buf, C.c_void_p), n) != n:
            raise EngineError(self._lib.se_last_error(None).decode())
        return buf.raw

    @classmethod
    def from_bytes(cls, b):
        """a snapshot from `to_bytes()` output: validated here, on the host; uploaded by the first restore"""
        if not isinstance(b, (bytes, bytearray, memoryview)):
            raise EngineError(f"ResamplerSnapshot.from_bytes: expected bytes, got {type(b).__name__}")
        b = bytes(b)
        snap = cls()
        if snap._lib.se_resampler_state_import(snap._h, b, len(b)):
            snap.close()
            raise EngineError(snap._lib.se_last_error(None).decode())
        return snap

    # ---- rows of parked signals (se_resampler_state_select / se_resampler_state_concat): the payload is [batch][history] floats, so
    # no resampler object is needed.  The result lives where the sources do (imported images are cut on the host)
    @staticmethod
    def _stream_of(device):
        if device is None:
            return C.c_void_p(0)
        import torch
        return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)

    @staticmethod
    def _check_args(what, snaps):
        for s in snaps:
            if not isinstance(s, ResamplerSnapshot):
                raise EngineError(f"{what}: expected a ResamplerSnapshot, got {type(s).__name__}")
            if s.closed:
                raise EngineError(f"{what}: the snapshot is closed")

    def select(self, rows, out=None):
        """A snapshot of `len(rows)` rows: row j is row rows[j] of this one (an index may repeat)."""
        self._check_args('select', [self] + ([out] if out is not None else []))
        rows = [int(r) for r in rows]
        if not rows:
            raise EngineError("select: at least one row has to be selected")
        arr = (C.c_int32 * len(rows))(*rows)
        dst = out if out is not None else ResamplerSnapshot()
        if self._lib.se_resampler_state_select(dst._h, self._h, arr, len(rows), self._stream_of(self.device)):
            if out is None:
                dst.close()
            raise EngineError(self._lib.se_last_error(None).decode())
        dst.device = self.device
        return dst

    @classmethod
    def _gather(cls, what, parts, out):
        """concat / join: the rows of the parts, in order, through se_resampler_state_<what>"""
        parts = list(parts)
        cls._check_args(what, parts + ([out] if out is not None else []))
        if not parts:
            raise EngineError(f"{what}: at least one part has to be given")
        devices = {p.device for p in parts if p.device is not None}
        if len(devices) > 1:
            raise EngineError(f"{what}: the parts' payloads live on devices {sorted(devices)} (move them with to_bytes / from_bytes)")
        device = devices.pop() if devices else None
        arr = (C.c_void_p * len(parts))(*[p._h.value for p in parts])
        dst = out if out is not None else cls()
        if getattr(dst._lib, 'se_resampler_state_' + what)(dst._h, arr, len(parts), cls._stream_of(device)):
            if out is None:
                dst.close()
            raise EngineError(dst._lib.se_last_error(None).decode())
        dst.device = device
        return dst

    @classmethod
    def concat(cls, parts, out=None):
        """A snapshot of the rows of parts[0], then parts[1], ...: rates, sample counts and read position have to agree."""
        return cls._gather('concat', parts, out)

    @classmethod
    def join(cls, parts, out=None):
        """`concat` for signals that began at different times (se_resampler_state_join): the rows of parts[0], then parts[1], ..., on
        the counters of parts[0]; every other part is rebased onto them.  Integer decimations only (48 / 32 -> 16 kHz, pass-through);
        the parts must be in phase (their n_in differ by multiples of sr_in / sr_out) and past their left edge (64 outputs at
        48 -> 16 kHz); each refusal names its reason.  Every row then continues bit for bit as it would have alone."""
        return cls._gather('join', parts, out)


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

    def _closed(self):
        h = getattr(self, '_h', None)
        return h is None or not getattr(h, 'value', h)

    def _check_snapshot(self, what, snapshot):
        if not isinstance(snapshot, ResamplerSnapshot):
            raise EngineError(f"{what}: expected a ResamplerSnapshot, got {type(snapshot).__name__}")
        if snapshot.closed:
            raise EngineError(f"{what}: the snapshot is closed")
        if self._closed():
            raise EngineError(f"{what}: the resampler is closed")

    def save(self, snapshot=None):
        """Copy the open signal into `snapshot` (a new ResamplerSnapshot when None) without ending or altering it; returns the
        snapshot.  Saving again into the same object allocates nothing."""
        if snapshot is not None:
            self._check_snapshot('save', snapshot)
        elif self._closed():
            raise EngineError("save: the resampler is closed")
        snap = snapshot if snapshot is not None else ResamplerSnapshot()
        if self._lib.se_resampler_save(self._h, snap._h, self._stream()):
            if snapshot is None:
                snap.close()
            raise EngineError(self._lib.se_last_error(None).decode())
        snap.device = self.device
        return snap

    def check_restore(self, snapshot, what='restore'):
        """Everything `restore(snapshot)` can refuse, checked on the host without touching this object or the snapshot; returns
        the snapshot's (sr_in, sr_out, batch, n_in, n_out)."""
        self._check_snapshot(what, snapshot)
        counts = snapshot.counts()
        sr_in, sr_out, batch = counts[:3]
        if (sr_in, sr_out) != (self.sr_in, self.sr_out):
            raise EngineError(f"{what}: the snapshot was taken at {sr_in} -> {sr_out} Hz, this object converts {self.sr_in} -> {self.sr_out} Hz")
        if batch > self.max_batch:
            raise EngineError(f"{what}: snapshot of {batch} rows exceeds max_batch {self.max_batch} given at create")
        if snapshot.device not in (None, self.device) and snapshot.nbytes:
            raise EngineError(f"{what}: the payload lives on device {snapshot.device}, this object on device {self.device} "
                              f"(move it with to_bytes / from_bytes)")
        return counts

    def restore(self, snapshot):
        """Make the saved signal the open signal of this object (whatever ran here is replaced, as by begin): the outputs of every
        later push / flush equal those of the signal had it never been interrupted, bit for bit."""
        self._check_snapshot('restore', snapshot)
        if self._lib.se_resampler_restore(self._h, snapshot._h, self._stream()):
            raise EngineError(self._lib.se_last_error(None).decode())
        _, _, self._batch, self._n_in, self._n_out = snapshot.counts()      # flush() sizes its output from them
