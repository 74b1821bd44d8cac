"""Python handle over the C-ABI engine.  torch is used only for device memory and streams."""
import ctypes as C
import math

import numpy as np

from . import _lib


class EngineError(RuntimeError):
    pass


class StreamSnapshot:
    """A parked frame-online stream (se_stream_state of include/se_engine.h): what `Engine.stream_save()` fills and
    `Engine.stream_restore()` puts back - on the same engine or on another of the same configuration and weights, any number of
    times.  `to_bytes()` / `from_bytes()` move it through host memory (another device, another process)."""

    def __init__(self):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        self.batch = 0             # rows of the saved stream (0 = empty)
        if self._lib.se_stream_state_create(C.byref(self._h)):
            self._h = C.c_void_p()
            raise EngineError(self._lib.se_last_error(None).decode())

    @property
    def closed(self):
        return getattr(self, '_h', None) is None or not self._h.value

    def close(self):
        if not self.closed:
            self._lib.se_stream_state_destroy(self._h)
            self._h = C.c_void_p()
            self.batch = 0

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
        """device memory of the payload (0 = empty)"""
        if self.closed:
            raise EngineError("StreamSnapshot.nbytes: the snapshot is closed")
        return int(self._lib.se_stream_state_bytes(self._h))

    def to_bytes(self):
        """the snapshot as one byte string (manifest + payload); synchronises with the save that filled it"""
        if self.closed:
            raise EngineError("StreamSnapshot.to_bytes: the snapshot is closed")
        n = int(self._lib.se_stream_state_export(self._h, None, 0))
        if n < 0:
            raise EngineError(self._lib.se_last_error(None).decode())
        buf = C.create_string_buffer(n)
        if self._lib.se_stream_state_export(self._h, C.cast(buf, C.c_void_p), n) != n:
            raise EngineError(self._lib.se_last_error(None).decode())
        return buf.raw

    @classmethod
    def from_bytes(cls, b):
        """a snapshot from `to_bytes()` output: validated here, on the host; uploaded by the first stream_restore"""
        if not isinstance(b, (bytes, bytearray, memoryview)):
            raise EngineError(f"StreamSnapshot.from_bytes: expected bytes, got {type(b).__name__}")
        b = bytes(b)
        snap = cls()
        if snap._lib.se_stream_state_import(snap._h, b, len(b)):
            snap.close()
            raise EngineError(snap._lib.se_last_error(None).decode())
        snap.batch = int.from_bytes(b[28:32], 'little', signed=True)      # csrc/stream_manifest.h: the sixth int32 behind magic and version
        return snap

    # ---- rows of parked groups (se_stream_state_select / se_stream_state_concat): `engine` supplies the buffers' row layouts and
    # must be of the snapshots' kind; its own stream and workspace are not touched.  The result lives on the engine's device
    @staticmethod
    def _check_args(what, engine, snaps):
        if not isinstance(engine, Engine):
            raise EngineError(f"{what}: expected an Engine, got {type(engine).__name__}")
        for s in snaps:
            if not isinstance(s, StreamSnapshot):
                raise EngineError(f"{what}: expected a StreamSnapshot, got {type(s).__name__}")
            if s.closed:
                raise EngineError(f"{what}: the snapshot is closed")
        if not engine._h:
            raise EngineError(f"{what}: the engine is closed")

    def select(self, engine, rows, out=None):
        """A snapshot of `len(rows)` rows: row j is row rows[j] of this one (an index may repeat: a fork).  Every counter and mode
        is copied.  `out`: a snapshot to fill (one that already holds the resulting layout is reused without allocating)."""
        self._check_args('select', engine, [self] + ([out] if out is not None else []))
        rows = [int(r) for r in rows]
        if not rows:
            raise EngineError("select: at least one row has to be selected")
        arr = (C.c_int32 * len(rows))(*rows)
        dst = out if out is not None else StreamSnapshot()
        if engine._lib.se_stream_state_select(engine._h, dst._h, self._h, arr, len(rows), engine._stream()):
            if out is None:
                dst.close()
            raise EngineError(engine._lib.se_last_error(engine._h).decode())
        dst.batch = len(rows)
        return dst

    @classmethod
    def concat(cls, engine, parts, out=None):
        """A snapshot of the rows of parts[0], then parts[1], ...: groups that have advanced in lockstep (every counter equal)
        put back into one."""
        parts = list(parts)
        cls._check_args('concat', engine, parts + ([out] if out is not None else []))
        if not parts:
            raise EngineError("concat: at least one part has to be given")
        arr = (C.c_void_p * len(parts))(*[p._h.value for p in parts])
        dst = out if out is not None else cls()
        if engine._lib.se_stream_state_concat(engine._h, dst._h, arr, len(parts), engine._stream()):
            if out is None:
                dst.close()
            raise EngineError(engine._lib.se_last_error(engine._h).decode())
        dst.batch = sum(p.batch for p in parts)
        return dst

    @classmethod
    def join(cls, engine, parts, out=None):
        """`concat` for groups that began at different times (se_stream_state_join): the rows of parts[0], then parts[1], ..., on the
        counters of parts[0]; every other part is rebased onto them.  The parts must be in phase (their n_total differ by multiples
        of lcm(hop, 4) - `samples_until_joinable` tells how far a caller is from that), past their left edge, not on a running scale,
        and of a model whose state counts no frames (CRN, LSTM, GCRN, DPCRN, DCCRN); each refusal names its reason."""
        parts = list(parts)
        cls._check_args('join', engine, parts + ([out] if out is not None else []))
        if not parts:
            raise EngineError("join: at least one part has to be given")
        arr = (C.c_void_p * len(parts))(*[p._h.value for p in parts])
        dst = out if out is not None else cls()
        if engine._lib.se_stream_state_join(engine._h, dst._h, arr, len(parts), engine._stream()):
            if out is None:
                dst.close()
            raise EngineError(engine._lib.se_last_error(engine._h).decode())
        dst.batch = sum(p.batch for p in parts)
        return dst

    def counts(self):
        """(batch, n_total, t_done, o_done, hop): rows, samples received, frames transformed, samples emitted, the hop.  Host only."""
        if self.closed:
            raise EngineError("StreamSnapshot.counts: the snapshot is closed")
        b, hop = C.c_int32(), C.c_int32()
        n, t, o = C.c_int64(), C.c_int64(), C.c_int64()
        if self._lib.se_stream_state_counts(self._h, C.byref(b), C.byref(n), C.byref(t), C.byref(o), C.byref(hop)):
            raise EngineError(self._lib.se_last_error(None).decode())
        return b.value, n.value, t.value, o.value, hop.value


def samples_until_joinable(stream, group):
    """How many more samples the stream `stream` must receive before `StreamSnapshot.join` can put it into `group`: the smallest
    d >= 0 that makes the two n_total differ by a multiple of lcm(hop, 4) - less than one hop of buffering, and unchanged by
    whatever whole hops the group receives meanwhile.  Both arguments are `StreamSnapshot.counts()` records (or snapshots).  None if
    the two never can be joined: their hops differ.  Which of the two is ahead does not matter - a join rebases either way - and
    the left edge (the first frames of a stream) is the engine's to check: its refusal names the frame count."""
    a, g = (x.counts() if isinstance(x, StreamSnapshot) else tuple(int(v) for v in x) for x in (stream, group))
    if len(a) != 5 or len(g) != 5 or a[4] < 1 or g[4] < 1:
        raise EngineError("samples_until_joinable: expected two (batch, n_total, t_done, o_done, hop) records")
    if a[4] != g[4]:
        return None
    unit = a[4] * 4 // math.gcd(a[4], 4)
    return (g[1] - a[1]) % unit


class Engine:
    """One engine handle = one model replica on one GPU (one per rank)."""

    SE_CFG_STREAM_SLIDING = 1 << 17      # include/se_engine.h
    SE_CFG_DCCRN_ROW_ENDS = 1 << 18
    SE_CFG_STREAM_ROW_ORIGINS = 1 << 19

    def __init__(self, model, device=0, max_batch=1, max_samples=64000, p_in=1.0, p_out=1.0,
                 n_fft=0, hop=0, win=0, graphs=False, flags=0, sliding_stream=False, row_ends=False,
                 row_origins=False):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        self.model = model
        cfg = _lib.SeConfig(_lib.MODEL_IDS[model], device, max_batch, max_samples, p_in, p_out, n_fft, hop, win,
                            (1 if graphs else 0) | int(flags) | (self.SE_CFG_STREAM_SLIDING if sliding_stream else 0) |
                            (self.SE_CFG_DCCRN_ROW_ENDS if row_ends else 0) | (self.SE_CFG_STREAM_ROW_ORIGINS if row_origins else 0))
        # SE_CFG_GRAPHS | model-specific SE_CFG_* bits | SE_CFG_STREAM_SLIDING (frame-online streams may outlive max_samples) |
        # SE_CFG_DCCRN_ROW_ENDS (DCCRN's look-ahead decoder in enhance_long_ragged: rows cleared behind their own ends, layer by layer) |
        # SE_CFG_STREAM_ROW_ORIGINS (the cLN networks and FullSubNet with the cumulative norm: a frame origin per stream row, which
        # StreamSnapshot.join moves along - the join refuses these models without it)
        if self._lib.se_engine_create(C.byref(cfg), C.byref(self._h)):
            raise EngineError(self._lib.se_last_error(None).decode())
        self.device = device
        self.max_batch, self.max_samples = max_batch, max_samples
        self.sliding_stream = bool(cfg.flags & self.SE_CFG_STREAM_SLIDING)
        self.row_ends = bool(cfg.flags & self.SE_CFG_DCCRN_ROW_ENDS)
        self.row_origins = bool(cfg.flags & self.SE_CFG_STREAM_ROW_ORIGINS)
        self.finalized = False
        self._stream_batch = 0          # rows of the open frame-online stream (0 = none)

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc):
        if rc:
            raise EngineError(self._lib.se_last_error(self._h).decode())

    def close(self):
        if getattr(self, '_h', None) is not None and self._h.value:
            self._lib.se_engine_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        """torch's current stream of THIS engine's device (not of torch's current device)."""
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _check_tensor(self, t, what, dim=None):
        import torch
        if not (t.is_cuda and t.dtype == torch.float32):
            raise EngineError(f"{what}: expected a float32 cuda tensor, got {t.dtype} on {t.device}")
        if t.device.index != self.device:
            raise EngineError(f"{what}: tensor on cuda:{t.device.index} but the engine lives on cuda:{self.device}")
        if dim is not None and (t.dim() != dim or t.stride(-1) != 1):
            raise EngineError(f"{what}: expected a {dim}-D tensor with unit inner stride, got shape {tuple(t.shape)} "
                              f"strides {t.stride()}")

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, sd):
        """Strict load of a flat state dict (numpy arrays or torch tensors), then finalize."""
        for k, v in sd.items():
            a = v.detach().cpu().numpy() if hasattr(v, 'detach') else np.asarray(v)
            if a.dtype == np.int64:
                dt = 1
            else:
                a = np.ascontiguousarray(a, dtype=np.float32)
                dt = 0
            a = np.ascontiguousarray(a)
            shape = (C.c_int64 * max(a.ndim, 1))(*a.shape)
            self._check(self._lib.se_engine_set_tensor(self._h, k.encode(), a.ctypes.data_as(C.c_void_p), shape,
                                                       a.ndim, dt))
        self._check(self._lib.se_engine_finalize(self._h))
        self.finalized = True

    # ------------------------------------------------------------------ compute (torch tensors on the GPU)
    def forward(self, x, out_shape=None):
        import torch
        self._check_tensor(x, 'forward input')
        assert x.is_contiguous()
        out = torch.empty(out_shape or x.shape, dtype=torch.float32, device=x.device)
        shape = (C.c_int64 * x.dim())(*x.shape)
        self._check(self._lib.se_forward(self._h, C.c_void_p(x.data_ptr()), shape, x.dim(),
                                         C.c_void_p(out.data_ptr()), self._stream()))
        return out

    def uformer_forward(self, inputs, src=None, spectra=True):
        """`model(inputs, src)` of Uformer/uformer.py:172-287: (output, src_out, output_cplx, src_cplx); the source outputs
        are None without `src`, the spectra None with spectra=False."""
        import torch
        self._check_tensor(inputs, 'uformer_forward inputs', 2)
        if not inputs.is_contiguous():
            raise EngineError("uformer_forward inputs: expected dense rows")
        B, L = inputs.shape
        n_out, T, F = self.output_samples(L), self.num_frames(L), self.num_bins()
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=inputs.device)
        out = new(B, n_out)
        out_c = new(B, 2, F, T) if spectra else None
        src_o = src_c = None
        if src is not None:
            self._check_tensor(src, 'uformer_forward src', 2)
            if tuple(src.shape) != (B, L) or not src.is_contiguous():
                raise EngineError(f"uformer_forward src: expected a dense {(B, L)} tensor, got {tuple(src.shape)}")
            src_o = new(B, n_out)
            src_c = new(B, 2, F, T) if spectra else None
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        self._check(self._lib.se_uformer_forward(self._h, ptr(inputs), ptr(src), B, L, ptr(out), ptr(src_o), ptr(out_c),
                                                 ptr(src_c), self._stream()))
        return out, src_o, out_c, src_c

    def output_samples(self, n):
        return int(self._lib.se_output_samples(self._h, n))

    def num_frames(self, n):
        return int(self._lib.se_num_frames(self._h, n))

    def num_bins(self):
        return int(self._lib.se_num_bins(self._h))

    def _rows_call(self, what, wav, lengths, out, window=None):
        """The body of the four enhance_* wrappers: se_<what> on the rows of wav, all of wav.shape[1] samples (lengths None) or
        of `lengths`.  window: max_chunk_frames of the two windowed decodes, which also refuse a row count outside the engine's
        and rows that overlap before the library sees them."""
        import torch
        self._check_tensor(wav, f'{what} input', 2)
        B, W = wav.shape
        if window is not None and (B < 1 or B > self.max_batch):
            raise EngineError(f"{what} input: {B} rows outside 1..max_batch ({self.max_batch})")
        width = W
        if lengths is not None:
            lengths = [int(n) for n in lengths]
            if window is None:
                if len(lengths) != B or max(lengths) > W:
                    raise EngineError(f"{what}: {len(lengths)} lengths (max {max(lengths)}) for a {tuple(wav.shape)} batch")
            elif len(lengths) != B:
                raise EngineError(f"{what}: {len(lengths)} lengths for a batch of {B} rows")
            elif min(lengths) < 1 or max(lengths) > W:
                raise EngineError(f"{what}: lengths {min(lengths)}..{max(lengths)} outside rows of {W} samples")
            width = max(lengths)
        if window is not None:
            if B > 1 and wav.stride(0) < width:
                raise EngineError(f"{what} input: rows of {width} samples overlap (strides {wav.stride()})")
            window = int(window)
            if window < 0:
                raise EngineError(f"{what}: max_chunk_frames {window} is negative (0 = the largest window)")
        n_out = self.output_samples(width)
        if out is None:
            out = torch.empty((B, n_out), dtype=torch.float32, device=wav.device)
        else:
            self._check_tensor(out, f'{what} output', 2)
            if out.shape[0] != B or out.shape[1] < n_out:
                raise EngineError(f"{what} output: need [{B}, >= {n_out}], got {tuple(out.shape)}")
        # the stride of a size-1 dimension is arbitrary in torch / numpy: a single row's pitch is its width (of equal rows: the
        # samples decoded, of ragged rows: the tensor's)
        in_pitch = wav.stride(0) if B > 1 else W
        out_pitch = out.stride(0) if B > 1 else n_out if lengths is None else out.shape[1]
        n = (width if lengths is None else (C.c_int32 * B)(*lengths),) + (() if window is None else (window,))
        self._check(getattr(self._lib, 'se_' + what)(self._h, C.c_void_p(wav.data_ptr()), in_pitch, B, *n,
                                                     C.c_void_p(out.data_ptr()), out_pitch, self._stream()))
        return out

    def enhance_batch(self, wav, out=None):
        """wav [B, L] float32 cuda tensor -> [B, output_samples(L)]."""
        return self._rows_call('enhance_batch', wav, None, out)

    def enhance_ragged(self, wav, lengths, out=None):
        """wav [B, >= max(lengths)] float32 cuda tensor, lengths: B sample counts (host ints) ->
        [B, output_samples(max(lengths))]; row b holds output_samples(lengths[b]) samples, then zeros."""
        return self._rows_call('enhance_ragged', wav, lengths, out)

    def enhance_long(self, wav, out=None, max_chunk_frames=0):
        """wav [B, L] float32 cuda tensor, L of any length (max_samples does not bound it) -> [B, output_samples(L)]: the offline
        decode of the whole clips, run in windows of max_chunk_frames frames (0 = the largest the workspace holds) with the
        network state carried from window to window (se_enhance_long).  Models that stream only; ends a stream running on
        this engine."""
        return self._rows_call('enhance_long', wav, None, out, max_chunk_frames)

    def enhance_long_ragged(self, wav, lengths, max_chunk_frames=0, out=None):
        """wav [B, >= max(lengths)] float32 cuda tensor, lengths: B sample counts (host ints, each of any length from n_fft on) ->
        [B, output_samples(max(lengths))]: every row decoded in windows as enhance_long decodes it alone - its own unit-RMS
        scale, right edge and frame count - in ONE walk over the windows of the longest row (se_enhance_long_ragged).  Row b
        holds output_samples(lengths[b]) samples, then zeros; nothing past lengths[b] is read.  Models that stream only; ends a
        stream running on this engine."""
        return self._rows_call('enhance_long_ragged', wav, lengths, out, max_chunk_frames)

    # ------------------------------------------------------------------ frame-online decoding
    def stream_begin(self, batch, c=None, max_chunk_frames=16, running_rms=False, tracking_rms=None):
        """Start `batch` parallel streams; c: per-stream scale tensor (what rms_scale() returns offline) or None = 1.
        running_rms=True: no scale from the caller - the engine keeps a running unit-RMS estimate (se_stream_begin_running).
        tracking_rms=<seconds>: a unit-RMS estimate per frame that forgets with that time constant (se_stream_begin_tracking; the
        seconds are converted at 16 kHz, 0.0 = never forget, None = off) - what a live caller starts with: it follows the level, does
        not depend on how the signal is split into pushes, and such streams can be joined."""
        batch = int(batch)
        if not 1 <= batch <= self.max_batch:
            raise EngineError(f"stream_begin: batch {batch} outside 1..max_batch ({self.max_batch})")
        if c is not None:
            self._check_tensor(c, 'stream_begin c')
            if not c.is_contiguous() or c.numel() < batch:        # the engine copies `batch` floats from c
                raise EngineError(f"stream_begin c: need a contiguous tensor of >= {batch} scales, got shape {tuple(c.shape)}")
        if tracking_rms is not None:
            if c is not None:
                raise EngineError("stream_begin: tracking_rms and a caller-provided scale exclude each other")
            if running_rms:
                raise EngineError("stream_begin: tracking_rms and running_rms=True exclude each other")
            self._stream_batch = 0
            self._check(self._lib.se_stream_begin_tracking(self._h, batch, max_chunk_frames, float(tracking_rms) * 16000.0, self._stream()))
            self._stream_batch = batch
            return
        self._stream_batch = 0
        if running_rms:
            if c is not None:
                raise EngineError("stream_begin: running_rms=True and a caller-provided scale exclude each other")
            self._check(self._lib.se_stream_begin_running(self._h, batch, max_chunk_frames, self._stream()))
            self._stream_batch = batch
            return
        self._check(self._lib.se_stream_begin(self._h, batch, max_chunk_frames,
                                              C.c_void_p(c.data_ptr()) if c is not None else None, self._stream()))
        self._stream_batch = batch

    def stream_scale(self):
        """The scale of the most recently released frame of every stream, a float32 tensor [batch] (se_stream_scale): the caller's c,
        the running scale's current c, the tracking scale's c_t; 1 before any frame."""
        import torch
        if self._closed():
            raise EngineError("stream_scale: the engine is closed")
        # (room for max_batch rows: the engine copies the rows of ITS stream, and refuses by itself when it has none)
        out = torch.empty((self.max_batch,), dtype=torch.float32, device=torch.device('cuda', self.device))
        self._check(self._lib.se_stream_scale(self._h, C.c_void_p(out.data_ptr()), self._stream()))
        if not self._stream_batch:       # a stream this object did not begin (a begin that was refused leaves the engine's as it was)
            raise EngineError("stream_scale without stream_begin")
        return out[:self._stream_batch]

    def stream_push(self, wav):
        """wav [batch, n_new] -> the output samples that became final, [batch, n_out] (n_out may be 0)."""
        import torch
        self._check_tensor(wav, 'stream_push input', 2)
        B, n = wav.shape
        if not self._stream_batch:
            raise EngineError("stream_push without stream_begin")
        if B != self._stream_batch:      # the engine reads and writes exactly the stream's rows
            raise EngineError(f"stream_push: {B} rows pushed into a stream of {self._stream_batch}")
        if self.sliding_stream and n > self.max_samples:      # the stream window holds one push of max_samples behind its live tail
            raise EngineError(f"stream_push: {n} samples in one push, a sliding stream takes at most max_samples "
                              f"({self.max_samples}) at a time")
        out = torch.empty((B, n + 1024), dtype=torch.float32, device=wav.device)
        n_out = C.c_int32(0)
        pitch = wav.stride(0) if B > 1 else max(n, 1)
        self._check(self._lib.se_stream_push(self._h, C.c_void_p(wav.data_ptr()), pitch, n, C.c_void_p(out.data_ptr()),
                                             out.stride(0), C.byref(n_out), self._stream()))
        return out[:, :n_out.value]

    def stream_flush(self):
        """End of the streams: the remaining output samples, [batch, n_out]."""
        import torch
        if not self._stream_batch:
            raise EngineError("stream_flush without stream_begin")
        out = torch.empty((self._stream_batch, self.max_samples), dtype=torch.float32, device=torch.device('cuda', self.device))
        n_out = C.c_int32(0)
        self._check(self._lib.se_stream_flush(self._h, C.c_void_p(out.data_ptr()), out.stride(0), C.byref(n_out),
                                              self._stream()))
        self._stream_batch = 0
        return out[:, :n_out.value]

    def _closed(self):
        h = getattr(self, '_h', None)
        return h is None or not getattr(h, 'value', h)

    def _check_snapshot(self, what, snapshot):
        if not isinstance(snapshot, StreamSnapshot):
            raise EngineError(f"{what}: expected a StreamSnapshot, got {type(snapshot).__name__}")
        if snapshot.closed:
            raise EngineError(f"{what}: the snapshot is closed")
        if self._closed():
            raise EngineError(f"{what}: the engine is closed")

    def stream_save(self, snapshot=None):
        """Copy the running stream into `snapshot` (a new StreamSnapshot when None) without ending or altering it; returns the
        snapshot.  Saving again into the same object allocates nothing."""
        if snapshot is not None:
            self._check_snapshot('stream_save', snapshot)
        elif self._closed():
            raise EngineError("stream_save: the engine is closed")
        if not self._stream_batch:
            raise EngineError("stream_save without stream_begin")
        snap = snapshot if snapshot is not None else StreamSnapshot()
        try:
            self._check(self._lib.se_stream_save(self._h, snap._h, self._stream()))
        except EngineError:
            if snapshot is None:
                snap.close()
            raise
        snap.batch = self._stream_batch
        return snap

    def stream_restore(self, snapshot):
        """Make the saved stream the running stream of this engine (whatever ran here is replaced, as by stream_begin): the
        outputs of every later stream_push / stream_flush equal those of the stream had it never been interrupted, bit for bit."""
        self._check_snapshot('stream_restore', snapshot)
        self._check(self._lib.se_stream_restore(self._h, snapshot._h, self._stream()))
        self._stream_batch = snapshot.batch

    # ------------------------------------------------------------------ stage hooks
    def rms_scale(self, wav):
        import torch
        c = torch.empty(wav.shape[0], dtype=torch.float32, device=wav.device)
        self._check(self._lib.se_rms_scale(self._h, C.c_void_p(wav.data_ptr()), wav.stride(0), wav.shape[0],
                                           wav.shape[1], C.c_void_p(c.data_ptr()), self._stream()))
        return c

    def stft(self, wav, c=None, p_in=1.0):
        import torch
        B, L = wav.shape
        T, F = self.num_frames(L), self.num_bins()
        spec = torch.empty((B, 2, F, T), dtype=torch.float32, device=wav.device)
        self._check(self._lib.se_stft(self._h, C.c_void_p(wav.data_ptr()), wav.stride(0), B, L,
                                      C.c_void_p(c.data_ptr()) if c is not None else None, p_in,
                                      C.c_void_p(spec.data_ptr()), self._stream()))
        return spec

    def istft(self, spec, n_out, c=None):
        import torch
        B, _, F, T = spec.shape
        assert spec.is_contiguous()
        wav = torch.empty((B, n_out), dtype=torch.float32, device=spec.device)
        self._check(self._lib.se_istft(self._h, C.c_void_p(spec.data_ptr()), B, T,
                                       C.c_void_p(c.data_ptr()) if c is not None else None,
                                       C.c_void_p(wav.data_ptr()), wav.stride(0), n_out, self._stream()))
        return wav

    BACKEND_KINDS = {'ri': 0, 'mag': 1, 'cmask': 2}

    def frontend(self, wav):
        """se_frontend: (c [B], spec [B,2,F,T]) - unit-RMS scale, tail pad, STFT and |X|^p_in e^{j angle X} of the decode loop."""
        import torch
        B, L = wav.shape
        T, F = self.num_frames(L), self.num_bins()
        c = torch.empty(B, dtype=torch.float32, device=wav.device)
        spec = torch.empty((B, 2, F, T), dtype=torch.float32, device=wav.device)
        self._check(self._lib.se_frontend(self._h, C.c_void_p(wav.data_ptr()), wav.stride(0), B, L, C.c_void_p(c.data_ptr()),
                                          C.c_void_p(spec.data_ptr()), self._stream()))
        return c, spec

    def backend(self, kind, est, n_out, spec=None, c=None):
        """se_backend: the mask / decompress stage + iSTFT + / c alone.  kind 'ri' (est = estimated spectrum [B,2,F,T]),
        'mag' (est = magnitude [B,F,T], noisy phase from spec), 'cmask' (est = complex ratio mask [B,2,F,T] on spec)."""
        import torch
        assert est.is_contiguous() and (spec is None or spec.is_contiguous())
        B, T = est.shape[0], est.shape[-1]
        wav = torch.empty((B, n_out), dtype=torch.float32, device=est.device)
        self._check(self._lib.se_backend(self._h, self.BACKEND_KINDS[kind], C.c_void_p(est.data_ptr()),
                                         C.c_void_p(spec.data_ptr()) if spec is not None else None, B, T,
                                         C.c_void_p(c.data_ptr()) if c is not None else None, C.c_void_p(wav.data_ptr()),
                                         wav.stride(0), n_out, self._stream()))
        return wav

    # ------------------------------------------------------------------ profiling
    def set_profiling(self, on):
        self._check(self._lib.se_set_profiling(self._h, 1 if on else 0))

    def get_profile(self):
        ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
        self._check(self._lib.se_get_profile(self._h, C.byref(ms), C.byref(n), C.byref(fl)))
        return {'gemm_ms': ms.value, 'gemm_launches': n.value, 'gemm_flops': fl.value}

    STAGES = ('rms', 'stft', 'mask', 'istft')

    def get_stage_profile(self):
        """{stage: {'ms', 'launches', 'bytes'}} of the HBM-bound front / back-end kernels of the last profiled call."""
        out = {}
        for i, name in enumerate(self.STAGES):
            ms, n, by = C.c_double(), C.c_int64(), C.c_double()
            self._check(self._lib.se_get_stage_profile(self._h, i, C.byref(ms), C.byref(n), C.byref(by)))
            out[name] = {'ms': ms.value, 'launches': n.value, 'bytes': by.value}
        return out
