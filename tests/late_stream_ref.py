"""Moving a parked frame-online stream to a late position, for the tests of streams near the end of the counter range
(tests/test_late_stream_host.py, tests/test_gpu_late_stream.py).  Not a test module.

A stream that is past its left edge does not depend on its absolute position as long as the position moves by whole hops
(csrc/stream_join.h derives it; se_stream_state_join relies on it for moves of a few hops).  `rebase_image` applies that move to the host
image of a parked stream (csrc/stream_manifest.h) by any number of frames: n_total, o_done and keep move by frames * hop, t_done by frames,
and every row origin of a SNAP_ORIGIN segment by frames, so each row's own frame index stays what it was.  Nothing else in the image
changes.  The image is parsed here, in Python, from the documented layout alone:

    u32 magic 'SEST' | u32 version | i32 x 18 fields | f32 p_in | f32 p_out | i32 nseg | i32 0 | i64 payload bytes      (104 bytes)
    nseg x { i32 kind | i32 index | i64 bytes }
    payload: segment k at the sum of the 16 B rounded sizes before it
"""
import struct

import numpy as np

MAGIC, VERSION = 0x54534553, 1
HEAD = 104                           # bytes in front of the segment table
FIELDS = ('model', 'flags', 'n_fft', 'hop', 'win', 'batch', 'max_chunk', 'n_total', 't_done', 'o_done', 'keep', 'running', 'ring', 'first',
          'state_B', 'reserved0', 'reserved1', 'reserved2')
OFFSET = {name: 8 + 4 * k for k, name in enumerate(FIELDS)}      # n_total 36, t_done 40, o_done 44, keep 48, running 52, ring 56, first 60
NSEG_AT = 88
SNAP_HIST, SNAP_H, SNAP_CELL, SNAP_SLOT, SNAP_WINDOW, SNAP_ORIGIN = 4, 5, 6, 7, 8, 9
INT32_MAX = 2 ** 31 - 1


class RebaseRefused(ValueError):
    pass


def align16(n):
    return (n + 15) // 16 * 16


def left_edge_frames(n_fft, hop, lag):
    """csrc/stream_join.h stream_left_edge_frames: the smallest t_done from which a stream can be moved"""
    stft = (n_fft // 2 + hop - 1) // hop
    istft = 0 if hop >= n_fft // 2 else (n_fft + hop - 1) // hop - 1 + lag
    return max(1, stft, istft)


def sample_limit(max_samples, n_fft, hop):
    """csrc/stream_window.h stream_sample_limit: the longest stream of a sliding engine, in samples"""
    return INT32_MAX - max(max_samples, n_fft + 32 * hop)


def parse_image(image):
    """the header fields of a stream image by name, 'p_in' / 'p_out', and 'segs': [(kind, index, bytes, offset into the image)]"""
    image = bytes(image)
    if len(image) < HEAD:
        raise RebaseRefused('stream image shorter than its header')
    magic, version = struct.unpack_from('<II', image, 0)
    if magic != MAGIC or version != VERSION:
        raise RebaseRefused('not a version %d stream image' % VERSION)
    d = dict(zip(FIELDS, struct.unpack_from('<18i', image, 8)))
    d['p_in'], d['p_out'] = struct.unpack_from('<ff', image, 80)
    nseg, _, total = struct.unpack_from('<iiq', image, NSEG_AT)
    if nseg < 0 or len(image) < HEAD + 16 * nseg:
        raise RebaseRefused('segment table cut short')
    off, segs = HEAD + 16 * nseg, []
    for k in range(nseg):
        kind, index, n = struct.unpack_from('<iiq', image, HEAD + 16 * k)
        if n < 0 or n % 4:
            raise RebaseRefused('segment %d of a negative or odd size' % k)
        segs.append((kind, index, n, off))
        off += align16(n)
    if off != len(image) or off - (HEAD + 16 * nseg) != total:
        raise RebaseRefused('the segment sizes do not add up to the image')
    d['segs'] = segs
    return d


def origins(image):
    """the rows' frame origins (the SNAP_ORIGIN segment) as a tuple, or None for an image without one"""
    d = parse_image(image)
    for kind, _, n, off in d['segs']:
        if kind == SNAP_ORIGIN:
            if n != 4 * d['batch']:
                raise RebaseRefused('origin segment of %d bytes for %d rows' % (n, d['batch']))
            return tuple(int(v) for v in np.frombuffer(image, '<i4', d['batch'], off))
    return None


def payload_outside_origins(image):
    """the payload with the bytes of the origin entries cut out: what a move leaves as it is"""
    d = parse_image(image)
    out, pos = [], HEAD + 16 * len(d['segs'])
    for kind, _, n, off in d['segs']:
        if kind == SNAP_ORIGIN:
            out.append(bytes(image[pos:off]))
            pos = off + n
    out.append(bytes(image[pos:]))
    return b''.join(out)


def counters(image):
    """(n_total, t_done, o_done, keep) of an image"""
    d = parse_image(image)
    return d['n_total'], d['t_done'], d['o_done'], d['keep']


def first_counts(d):
    """whether the `first` field of a parsed image says anything: a model that keeps call-order slots (SNAP_SLOT segments) has no such
    flag and se_stream_save records a constant 1 for it (csrc/stream_join.h snap_join_plan, `first_counts`)"""
    return not any(kind == SNAP_SLOT for kind, _, _, _ in d['segs'])


def rebase_image(image, frames, lag=0, max_samples=0):
    """The image of the same stream `frames` frames later (earlier, if negative).  lag: the model's look-ahead in frames (it enters the left
    edge); max_samples: that of the engine the image goes to (it enters the stream limit; 0: the limit of the smallest engine).  Raises
    RebaseRefused where the move would not be position independent or leaves the counter range."""
    image = bytes(image)
    frames = int(frames)
    d = parse_image(image)
    n_fft, hop, batch = d['n_fft'], d['hop'], d['batch']
    if hop < 1 or n_fft < 2 or batch < 1:
        raise RebaseRefused('front end n_fft / hop %d / %d or batch %d out of range' % (n_fft, hop, batch))
    if first_counts(d) and d['first'] != 0:
        raise RebaseRefused('first %d: the first chunk of the stream is still to come' % d['first'])
    need = left_edge_frames(n_fft, hop, lag)
    if d['t_done'] < need or d['t_done'] + frames < need:
        raise RebaseRefused('short of the left edge: t_done %d (%d after the move), a stream can be moved from t_done %d on'
                            % (d['t_done'], d['t_done'] + frames, need))
    if d['running'] == 1:
        raise RebaseRefused('running 1: the whole-stream RMS divides by the position')
    if d['running'] not in (0, 2):
        raise RebaseRefused('unknown scale mode %d' % d['running'])
    shift = frames * hop
    if shift % 4:
        raise RebaseRefused('a move of %d samples is no multiple of 4: the window origin stays 16 B aligned' % shift)
    if d['ring'] > 1 and frames % d['ring']:
        raise RebaseRefused('a move of %d frames would rotate the per-frame rings of %d entries' % (frames, d['ring']))
    limit = sample_limit(max_samples, n_fft, hop)
    moved = {'n_total': d['n_total'] + shift, 'o_done': d['o_done'] + shift, 'keep': d['keep'] + shift, 't_done': d['t_done'] + frames}
    for name, v in moved.items():
        if v < 0 or v > limit:
            raise RebaseRefused('%s %d outside [0, %d], the stream limit' % (name, v, limit))
    out = bytearray(image)
    for name, v in moved.items():
        struct.pack_into('<i', out, OFFSET[name], v)
    for kind, _, n, off in d['segs']:
        if kind != SNAP_ORIGIN:
            continue
        if n != 4 * batch:
            raise RebaseRefused('origin segment of %d bytes for %d rows' % (n, batch))
        org = [int(v) + frames for v in struct.unpack_from('<%di' % batch, image, off)]
        if min(org) < -INT32_MAX - 1 or max(org) > INT32_MAX:
            raise RebaseRefused('a row origin leaves the int32 range')
        struct.pack_into('<%di' % batch, out, off, *org)
    return bytes(out)
