"""Frame-online decoding fed at the source's sample rate: a `StreamResampler` in front of `Engine.stream_begin` /
`stream_push` / `stream_flush`.

The engine streams at the models' 16 kHz; a microphone or a 48 kHz file reader delivers 48 / 44.1 / 32 kHz.  A push at `sr_in`
is resampled on the device - the samples `resample()` would give for the whole signal, as far as they are final - and those go
into the engine's stream; what comes back is the engine's 16 kHz output (the reference writes 16 kHz files: nothing is
converted back to `sr_in`).  The engine and its stream state are used as they are; on top of the engine's own latency the
resampler looks 192 input samples (4 ms) ahead at 48 -> 16 kHz.
"""
import math
import struct

from .engine import EngineError, StreamSnapshot
from .resample import ResamplerSnapshot, StreamResampler


class SourceStreamSnapshot:
    """A parked `SourceRateStream`: the pair (`engine`: StreamSnapshot, `resampler`: ResamplerSnapshot) that
    `SourceRateStream.save()` fills and `SourceRateStream.restore()` puts back.  `to_bytes()` is the two images, each behind its
    length (u64, little endian)."""

    def __init__(self, engine=None, resampler=None):
        self.engine = engine if engine is not None else StreamSnapshot()
        self.resampler = resampler if resampler is not None else ResamplerSnapshot()

    @property
    def closed(self):
        return self.engine.closed or self.resampler.closed

    def close(self):
        self.engine.close()
        self.resampler.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    @property
    def nbytes(self):
        """device memory of the two payloads"""
        return self.engine.nbytes + self.resampler.nbytes

    def to_bytes(self):
        e, r = self.engine.to_bytes(), self.resampler.to_bytes()
        return struct.pack('<Q', len(e)) + e + struct.pack('<Q', len(r)) + r

    @classmethod
    def from_bytes(cls, b):
        if not isinstance(b, (bytes, bytearray, memoryview)):
            raise EngineError(f"SourceStreamSnapshot.from_bytes: expected bytes, got {type(b).__name__}")
        b = bytes(b)
        parts, at = [], 0
        for name in ('engine', 'resampler'):
            if len(b) < at + 8:
                raise EngineError(f"SourceStreamSnapshot.from_bytes: truncated (no length in front of the {name} image)")
            n, = struct.unpack_from('<Q', b, at)
            at += 8
            if len(b) < at + n:
                raise EngineError(f"SourceStreamSnapshot.from_bytes: truncated ({name} image cut short)")
            parts.append(b[at:at + n])
            at += n
        if at != len(b):
            raise EngineError(f"SourceStreamSnapshot.from_bytes: {len(b) - at} trailing bytes behind the resampler image")
        eng = StreamSnapshot.from_bytes(parts[0])
        try:
            res = ResamplerSnapshot.from_bytes(parts[1])
        except EngineError:
            eng.close()
            raise
        return cls(eng, res)

    # ---- rows of parked groups: both halves, the resampler's - which needs no device to refuse - first
    def select(self, engine, rows):
        """The pair of `len(rows)` rows: row j is row rows[j] of this one, in both halves (StreamSnapshot.select,
        ResamplerSnapshot.select).  `engine`: an engine of the snapshot's kind."""
        if self.closed:
            raise EngineError("select: the snapshot is closed")
        rows = [int(r) for r in rows]
        batch = self.resampler.counts()[2]
        if batch != self.engine.batch:
            raise EngineError(f"select: the engine's half holds {self.engine.batch} rows, the resampler's {batch}")
        res = self.resampler.select(rows)
        try:
            eng = self.engine.select(engine, rows)
        except EngineError:
            res.close()
            raise
        return SourceStreamSnapshot(eng, res)

    @classmethod
    def concat(cls, engine, parts):
        """The pair of the rows of parts[0], then parts[1], ... in both halves."""
        parts = list(parts)
        for p in parts:
            if not isinstance(p, SourceStreamSnapshot):
                raise EngineError(f"concat: expected a SourceStreamSnapshot, got {type(p).__name__}")
            if p.closed:
                raise EngineError("concat: the snapshot is closed")
        res = ResamplerSnapshot.concat([p.resampler for p in parts])
        try:
            eng = StreamSnapshot.concat(engine, [p.engine for p in parts])
        except EngineError:
            res.close()
            raise
        return cls(eng, res)

    def counts(self):
        """Both halves' host records: (`StreamSnapshot.counts()`, `ResamplerSnapshot.counts()`) =
        ((batch, n_total, t_done, o_done, hop), (sr_in, sr_out, batch, n_in, n_out)).  Host only."""
        if self.closed:
            raise EngineError("counts: the snapshot is closed")
        return self.engine.counts(), self.resampler.counts()

    @classmethod
    def join(cls, engine, parts):
        """`concat` for source-rate groups that began at different times: the rows of parts[0], then parts[1], ... in both halves, on
        the counters of parts[0] (ResamplerSnapshot.join, then StreamSnapshot.join).  A caller is in phase with a group once
        `source_samples_until_joinable` says 0; both halves have to be past their left edge.  The two halves of every part have to
        tell one story - the engine has received what the resampler has released - which is checked here, on the host, first."""
        parts = list(parts)
        for p in parts:
            if not isinstance(p, SourceStreamSnapshot):
                raise EngineError(f"join: expected a SourceStreamSnapshot, got {type(p).__name__}")
            if p.closed:
                raise EngineError("join: the snapshot is closed")
        if not parts:
            raise EngineError("join: at least one part has to be given")
        recs = [p.counts() for p in parts]
        for k, (e, r) in enumerate(recs):
            if e[0] != r[2]:
                raise EngineError(f"join: parts[{k}]: the engine's half holds {e[0]} rows, the resampler's {r[2]}")
            if e[1] != r[4]:        # (equal in every part: the engine's shift is then the resampler's output shift as well)
                raise EngineError(f"join: parts[{k}]: the engine's half has received {e[1]} samples, the resampler's has released {r[4]}")
        res = ResamplerSnapshot.join([p.resampler for p in parts])
        try:
            eng = StreamSnapshot.join(engine, [p.engine for p in parts])
        except EngineError:
            res.close()
            raise
        return cls(eng, res)


JOIN_DECIMATIONS = (1, 2, 3)         # csrc/resampler_join.h RSJOIN_DECIMATIONS: the sr_in / sr_out se_resampler_state_join accepts


def source_samples_until_joinable(stream, group):
    """How many more samples at sr_in the source-rate stream `stream` must push before `SourceStreamSnapshot.join` can put it into
    `group`: the smallest d >= 0 that makes the two n_in differ by a multiple of D * lcm(hop, 4), D = sr_in / sr_out - the resampler's
    half rebases by multiples of D, the engine's by multiples of lcm(hop, 4) at sr_out: 480 samples at 48 kHz with hop 160, 384 with
    hop 128.  Unchanged by whatever whole hops the group receives meanwhile.  Both arguments are `SourceStreamSnapshot.counts()` records
    (or snapshots).  None if the two never can be joined: other rates, a ratio the join refuses (44.1 kHz, upsampling, a decimation
    other than 1, 2, 3), other hops.  The left edges are the library's to check: its refusals name the counts."""
    recs = []
    for x in (stream, group):
        e, r = x.counts() if isinstance(x, SourceStreamSnapshot) else x
        e, r = tuple(int(v) for v in e), tuple(int(v) for v in r)
        if len(e) != 5 or len(r) != 5 or e[4] < 1 or r[0] < 1 or r[1] < 1:
            raise EngineError("source_samples_until_joinable: expected two ((batch, n_total, t_done, o_done, hop), "
                              "(sr_in, sr_out, batch, n_in, n_out)) records")
        recs.append((e, r))
    (ea, ra), (eg, rg) = recs
    if ra[:2] != rg[:2] or ea[4] != eg[4]:
        return None
    sr_in, sr_out = ra[:2]
    if sr_in % sr_out or sr_in // sr_out not in JOIN_DECIMATIONS:
        return None
    unit = sr_in // sr_out * (ea[4] * 4 // math.gcd(ea[4], 4))
    return (rg[3] - ra[3]) % unit


class SourceRateStream:
    """`SourceRateStream(model.engine, 48000)`: `begin(batch, ...)`, `push(x)` with x [batch, n <= max_push] at sr_in ->
    enhanced 16 kHz samples [batch, n_out] (n_out may be 0), `flush()` -> the rest.  `begin` takes what `Engine.stream_begin`
    takes: a per-stream scale `c` (of the 16 kHz signal, e.g. from a calibration run) or `running_rms=True`, or `tracking_rms=<seconds>` (of 16 kHz time).
    `save()` / `restore()` park and resume the stream as `Engine.stream_save` / `stream_restore` do for a 16 kHz one: a
    `SourceStreamSnapshot` holds the engine's stream and the resampler's filter history and read position, so groups fed at the
    source's rate can share one engine and one `SourceRateStream` by turns (restore -> push -> save per group).  Parked groups of an
    integer decimation (48 / 32 kHz) that began at different times are put into one by `SourceStreamSnapshot.join`, once
    `source_samples_until_joinable` says the late caller is in phase."""

    def __init__(self, engine, sr_in, sr_out=16000, max_push=None):
        self.engine = engine
        self.resampler = StreamResampler(sr_in, sr_out, max_batch=engine.max_batch, max_push=max_push, device=engine.device)
        self._batch = 0

    def begin(self, batch, c=None, max_chunk_frames=16, running_rms=False, tracking_rms=None):
        self._batch = 0
        self.engine.stream_begin(batch, c=c, max_chunk_frames=max_chunk_frames, running_rms=running_rms, tracking_rms=tracking_rms)
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

    @staticmethod
    def _check_pair(what, snapshot):
        if not isinstance(snapshot, SourceStreamSnapshot):
            raise EngineError(f"{what}: expected a SourceStreamSnapshot, got {type(snapshot).__name__}")
        if snapshot.closed:
            raise EngineError(f"{what}: the snapshot is closed")

    def save(self, snapshot=None):
        """Copy the running stream - the engine's and the resampler's half - into `snapshot` (a new SourceStreamSnapshot when
        None) without ending or altering it; returns the snapshot."""
        if snapshot is not None:
            self._check_pair('save', snapshot)
        if not self._batch:
            raise EngineError("save without begin")
        snap = snapshot if snapshot is not None else SourceStreamSnapshot()
        try:
            self.engine.stream_save(snap.engine)
            self.resampler.save(snap.resampler)
        except EngineError:
            if snapshot is None:
                snap.close()
            raise
        return snap

    def restore(self, snapshot):
        """Make the saved stream the running one (whatever ran here is replaced, as by begin): every later push / flush gives the
        outputs of the stream had it never been interrupted, bit for bit.  A refused restore leaves both halves as they were:
        what the resampler can refuse is checked on the host before the engine's half is put back."""
        self._check_pair('restore', snapshot)
        _, _, batch, _, _ = self.resampler.check_restore(snapshot.resampler)
        if batch != snapshot.engine.batch:
            raise EngineError(f"restore: the engine's half holds {snapshot.engine.batch} rows, the resampler's {batch}")
        self.engine.stream_restore(snapshot.engine)
        self.resampler.restore(snapshot.resampler)
        self._batch = batch

    def close(self):
        self.resampler.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
