"""CPU: tests/late_stream_ref.py `rebase_image`, the move of a parked stream's host image (csrc/stream_manifest.h) to a late position
that tests/test_gpu_late_stream.py continues streams from.  Images are built here by a small writer of the documented layout - with and
without the frame-origin segment, with segments whose sizes are no multiples of 16 - and the moved images are read back by the library
itself: `StreamSnapshot.from_bytes` (se_stream_state_import validates every field) and se_stream_state_counts.  No device is needed."""
import struct

import numpy as np
import pytest

import se_amd  # noqa: F401
from se_amd.engine import StreamSnapshot

import late_stream_ref as LS
from late_stream_ref import RebaseRefused, rebase_image

ROW_ORIGINS = 1 << 19               # SE_CFG_STREAM_ROW_ORIGINS / SNAP_FLAG_ROW_ORIGINS


def _image(n_fft=320, hop=160, batch=2, n_total=5127, t_done=31, o_done=4800, keep=4800, running=0, ring=0, first=0, origin=None,
           slots=False, tracking=False, seed=0):
    """a well-formed stream image: c [batch] float (8 B for two rows: no multiple of 16), recurrent state or call-order slots of odd
    sizes, optionally the scale rings and the origin segment, the input window last; every payload byte is random, padding included"""
    rng = np.random.default_rng(seed)
    segs = [(1, 0, 4 * batch)]
    if tracking:
        running, ring = 2, ring or 64
        segs += [(2, 0, 16 * batch), (3, 0, 4 * batch * ring)]
    if slots:
        segs += [(7, 0, 36 * batch), (7, 1, 1028 * batch), (7, 2, 16 * batch)]
    else:
        segs += [(4, 0, 100 * batch), (5, 0, 52 * batch), (6, 0, 52 * batch), (4, 1, 64 * batch)]
    flags = 0
    if origin is not None:
        assert len(origin) == batch
        flags |= ROW_ORIGINS
        segs.append((9, 0, 4 * batch))
    segs.append((8, 0, 4 * batch * (n_total - keep)))
    payload = bytearray()
    for kind, _, n in segs:
        if kind == 9:
            body = struct.pack('<%di' % batch, *origin) + bytes(rng.integers(0, 256, LS.align16(n) - n, dtype=np.uint8))
        else:
            body = bytes(rng.integers(0, 256, LS.align16(n), dtype=np.uint8))
        payload += body
    head = struct.pack('<II18iffiiq', LS.MAGIC, LS.VERSION, 1, flags, n_fft, hop, n_fft, batch, 16, n_total, t_done, o_done, keep, running, ring,
                       1 if slots else first, batch, 0, 0, 0, 1.0, 1.0, len(segs), 0, len(payload))
    table = b''.join(struct.pack('<iiq', *s) for s in segs)
    return head + table + bytes(payload)


# (n_fft, hop, look-ahead, t_done, n_total, o_done, keep): streams a little past a first slide of a 4000-sample engine
CASES = {
    'crn': dict(n_fft=320, hop=160, n_total=5127, t_done=31, o_done=4800, keep=4800),
    'dccrn': dict(n_fft=512, hop=128, n_total=5127, t_done=39, o_done=3968, keep=4736),
    'fullsubnet': dict(n_fft=512, hop=256, n_total=5127, t_done=20, o_done=4352, keep=4864),
}
LAG = {'crn': 0, 'dccrn': 6, 'fullsubnet': 2}
VARIANTS = [('crn', {}), ('crn', dict(slots=True, origin=(0, 0))), ('crn', dict(slots=True, origin=(-3, 5))), ('crn', dict(tracking=True)),
            ('crn', dict(slots=True, tracking=True, origin=(7, -2))), ('dccrn', {}), ('dccrn', dict(batch=3)),
            ('fullsubnet', dict(origin=(0, -11))), ('fullsubnet', dict(batch=1, origin=(4,)))]


def test_the_header_offsets_are_the_documented_ones():
    assert [LS.OFFSET[k] for k in ('n_total', 't_done', 'o_done', 'keep', 'running', 'ring', 'first')] == [36, 40, 44, 48, 52, 56, 60]
    assert LS.NSEG_AT == 88 and LS.HEAD == 104
    img = _image(**CASES['crn'], origin=(1, 2), slots=True)
    d = LS.parse_image(img)
    assert (d['n_total'], d['t_done'], d['o_done'], d['keep'], d['hop'], d['batch']) == (5127, 31, 4800, 4800, 160, 2)
    assert [s[2] % 16 for s in d['segs']].count(0) < len(d['segs'])          # sizes that are no multiples of 16 are in
    assert d['segs'][0][3] == 104 + 16 * len(d['segs']) and d['segs'][1][3] == d['segs'][0][3] + 16
    with StreamSnapshot.from_bytes(img) as snap:                             # the writer's images are the library's images
        assert snap.counts() == (2, 5127, 31, 4800, 160)


def test_left_edge_and_limit_mirror_the_headers():
    # csrc/stream_join.h stream_left_edge_frames, the values csrc/tests/stream_join_check.cpp finds by walking a stream
    assert LS.left_edge_frames(320, 160, 0) == 1 and LS.left_edge_frames(512, 128, 6) == 9 and LS.left_edge_frames(512, 128, 0) == 3
    assert LS.left_edge_frames(512, 256, 2) == 1 and LS.left_edge_frames(400, 160, 0) == 2
    # csrc/stream_window.h stream_sample_limit, the formula tests/test_sliding_window_logic.py asserts of the library
    assert LS.sample_limit(4000, 320, 160) == 2 ** 31 - 1 - 5440 and LS.sample_limit(16000 * 300, 512, 128) == 2 ** 31 - 1 - 4800000


@pytest.mark.parametrize('name,kw', VARIANTS)
@pytest.mark.parametrize('where', ['one', 'across_2_24', 'limit'])
def test_a_moved_image_is_accepted_and_carries_the_moved_counters(name, kw, where):
    base = CASES[name]
    img = _image(**base, **kw, seed=len(kw) + 1)
    d = LS.parse_image(img)
    hop, unit = d['hop'], max(1, d['ring'])
    limit = LS.sample_limit(4000, d['n_fft'], hop)
    f = {'one': unit, 'across_2_24': -(-(2 ** 24 - d['n_total'] + 1) // (hop * unit)) * unit,
         'limit': (limit - d['n_total']) // (hop * unit) * unit}[where]
    out = rebase_image(img, f, lag=LAG[name], max_samples=4000)
    assert len(out) == len(img)
    with StreamSnapshot.from_bytes(out) as snap:
        assert snap.batch == d['batch']
        assert snap.counts() == (d['batch'], d['n_total'] + f * hop, d['t_done'] + f, d['o_done'] + f * hop, hop)
        assert snap.to_bytes() == out
    assert LS.counters(out) == (d['n_total'] + f * hop, d['t_done'] + f, d['o_done'] + f * hop, d['keep'] + f * hop)
    if where == 'across_2_24':
        assert d['n_total'] + f * hop > 2 ** 24 >= d['n_total'] + (f - unit) * hop
    if where == 'limit':
        assert limit - unit * hop < d['n_total'] + f * hop <= limit
    # nothing else moves: every header field but the four counters, the segment table, the payload outside the origin entries
    moved = {LS.OFFSET[k] for k in ('n_total', 't_done', 'o_done', 'keep')}
    table_end = LS.HEAD + 16 * len(d['segs'])
    for off in range(0, table_end, 4):
        assert off in moved or out[off:off + 4] == img[off:off + 4], off
    assert LS.payload_outside_origins(out) == LS.payload_outside_origins(img)
    want = kw.get('origin')
    assert LS.origins(out) == (None if want is None else tuple(o + f for o in want))
    # and back
    assert rebase_image(out, -f, lag=LAG[name], max_samples=4000) == img


def test_a_move_of_zero_frames_is_the_image_itself():
    img = _image(**CASES['dccrn'])
    assert rebase_image(img, 0, lag=6) == img


def test_refusals():
    crn = CASES['crn']
    ok = _image(**crn)
    assert rebase_image(ok, 5) != ok
    # the stream's first chunk is still to come (a model that keeps a StreamState); call-order slots record a constant 1 that says nothing
    with pytest.raises(RebaseRefused, match='first 1'):
        rebase_image(_image(**crn, first=1), 5)
    assert LS.parse_image(_image(**crn, slots=True))['first'] == 1
    rebase_image(_image(**crn, slots=True), 5)
    # short of the left edge: 512 / 128 with six frames of look-ahead can be moved from t_done 9 on
    early = dict(CASES['dccrn'], n_total=8 * 128 + 200, t_done=8, o_done=0, keep=768)
    with pytest.raises(RebaseRefused, match='short of the left edge: t_done 8'):
        rebase_image(_image(**early), 4, lag=6)
    rebase_image(_image(**early), 4, lag=0)                                   # (the causal decoder: from t_done 3 on)
    rebase_image(_image(**dict(early, n_total=9 * 128 + 200, t_done=9, keep=896)), 4, lag=6)
    with pytest.raises(RebaseRefused, match='short of the left edge'):       # ... and no move back below it
        rebase_image(_image(**CASES['dccrn']), -31, lag=6)
    with pytest.raises(RebaseRefused, match='short of the left edge: t_done 0'):
        rebase_image(_image(**dict(crn, n_total=100, t_done=0, o_done=0, keep=0)), 1)
    # the whole-stream RMS
    with pytest.raises(RebaseRefused, match='running 1'):
        rebase_image(_image(**crn, running=1, ring=64), 64)
    # a shift that is no multiple of 4 samples
    odd = dict(n_fft=6, hop=6, n_total=1003, t_done=160, o_done=950, keep=956)
    with StreamSnapshot.from_bytes(_image(**odd)) as snap:
        assert snap.counts()[4] == 6
    with pytest.raises(RebaseRefused, match='no multiple of 4'):
        rebase_image(_image(**odd), 1)
    with pytest.raises(RebaseRefused, match='no multiple of 4'):
        rebase_image(_image(**odd), 3)
    assert LS.counters(rebase_image(_image(**odd), 2)) == (1015, 162, 962, 968)
    # per-frame rings: whole turns only
    trk = _image(**crn, tracking=True)
    for f in (1, 63, 65, -16):
        with pytest.raises(RebaseRefused, match='rotate the per-frame rings of 64'):
            rebase_image(trk, f)
    rebase_image(trk, 128)
    # the stream limit: the last legal move ends at or below it, one more frame passes it
    limit = LS.sample_limit(4000, 320, 160)
    f = (limit - crn['n_total']) // 160
    assert limit - 160 < LS.counters(rebase_image(ok, f, max_samples=4000))[0] <= limit
    with pytest.raises(RebaseRefused, match='n_total .* the stream limit'):
        rebase_image(ok, f + 1, max_samples=4000)
    big = 16000 * 300
    assert f * 160 + crn['n_total'] > LS.sample_limit(big, 320, 160)
    with pytest.raises(RebaseRefused, match='the stream limit'):
        rebase_image(ok, f, max_samples=big)
    with pytest.raises(RebaseRefused, match='o_done -160 outside'):            # ... nor below zero
        rebase_image(_image(**dict(crn, o_done=4000)), -26)
    # not an image
    with pytest.raises(RebaseRefused):
        rebase_image(ok[:-16], 1)
    with pytest.raises(RebaseRefused):
        rebase_image(b'SESTnope' + ok[8:], 1)


def test_the_library_refuses_what_lies_past_the_helper():
    """the moved image is checked by the library's own parser, not by the helper alone: a keep moved without n_total is refused there"""
    img = bytearray(_image(**CASES['crn']))
    struct.pack_into('<i', img, LS.OFFSET['keep'], CASES['crn']['keep'] + 160 * 4)
    from se_amd.engine import EngineError
    with pytest.raises(EngineError, match='stream state image'):
        StreamSnapshot.from_bytes(bytes(img))
