"""GPU: rows of parked stream groups (se_stream_state_select / se_stream_state_concat, StreamSnapshot.select / .concat and the same
pair on the resampler's and the source-rate snapshot).

Models, weight seeds and the bar are those of tests/test_gpu_sliding_stream.py (`ALL`, `_make`, `_close`: identical shape and
rms(got - ref) < 1e-6 + 2e-5 rms(ref)); engines are made for max_samples = 4000 and 4 rows, clips are 3500 samples of
synth.synth_clip pushed in pieces of 700.  A selected row continues at another batch size, and kernel selection depends on the batch
(gc_select, the cooperative LSTM), so a continued row is held to the streamed bar, not to bit identity; the snapshots themselves are
copies and are compared byte for byte."""
import functools
import struct

import numpy as np
import pytest

import se_amd  # noqa: F401
from se_amd import synth
from se_amd.engine import EngineError, StreamSnapshot
from test_gpu_sliding_stream import ALL, _close, _make

pytestmark = pytest.mark.gpu

MS, B4, L, PIECE = 4000, 4, 3500, 700
STARTS = list(range(0, L, PIECE))
CUT = 2                          # the group is saved after this many pushes
HEAD = 104                       # csrc/stream_manifest.h: magic, version, 18 int32, p_in, p_out, nseg, pad, payload bytes
KIND_HIST, KIND_H, KIND_CELL = 4, 5, 6
RLSTM = 'dccrn_rlstm'            # DCCRN with real LSTMs (tests/test_gpu_dccrn_real_lstm.py: seed 24)


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _model(name, B, max_samples=MS, **kw):
    if name == RLSTM:
        from se_amd.models import DCCRN
        return DCCRN(rnn_units=256, masking_mode='E', kernel_num=[16, 32, 64, 128, 256, 256], max_batch=B, max_samples=max_samples,
                     **kw).load_synthetic(24)
    return _make(name, B, max_samples, **kw)


_ENGINES = {}


def _engine(name, B=B4, tag='', **kw):
    """one engine per (model, rows, kind) for the whole module: its streams follow one another on it, as a server's would"""
    key = (name, B, tag)
    if key not in _ENGINES:
        _ENGINES[key] = _model(name, B, **kw).engine
    return _ENGINES[key]


@pytest.fixture(scope='module', autouse=True)
def _release():
    yield
    for eng in _ENGINES.values():
        eng.close()
    _ENGINES.clear()
    _clean.cache_clear()
    _signal.cache_clear()


@functools.lru_cache(maxsize=None)
def _signal(n=L, rows=B4, seed=900):
    x = np.stack([synth.synth_clip(seed + b, 'speech' if b % 2 == 0 else 'white', n) for b in range(rows)])
    x.setflags(write=False)
    return x


def _begin(eng, rows, c, running):
    if running:
        eng.stream_begin(rows, running_rms=True)
    else:
        eng.stream_begin(rows, c=c)


def _push_all(eng, xt, first=0, starts=STARTS, piece=PIECE):
    """pushes pieces first.. of xt and flushes; the outputs of every call, flush last"""
    outs = [eng.stream_push(xt[:, p:p + piece].contiguous()).cpu().numpy() for p in starts[first:]]
    outs.append(eng.stream_flush().cpu().numpy())
    return outs


@functools.lru_cache(maxsize=None)
def _clean(name, running=False):
    """the group of 4 uninterrupted: (outputs per call, the image saved after CUT pushes, the rows' scales).  Computed once per
    model and mode, shared by every test, never written to"""
    torch = _torch()
    eng = _engine(name)
    xt = torch.from_numpy(_signal()).cuda()
    c = eng.rms_scale(xt)
    _begin(eng, B4, c, running)
    outs = [eng.stream_push(xt[:, p:p + PIECE].contiguous()).cpu().numpy() for p in STARTS[:CUT]]
    with eng.stream_save() as snap:
        img = snap.to_bytes()
    outs += _push_all(eng, xt, CUT)
    for o in outs:
        o.setflags(write=False)
    return outs, img, c.cpu().numpy()


def _check_rows(name, got, ref_outs, rows, what):
    """got: the outputs of the calls behind the cut for the selected rows; ref_outs: the uninterrupted group's, all rows"""
    ref = ref_outs[-len(got):]
    assert [o.shape[1] for o in got] == [o.shape[1] for o in ref], (name, what, 'n_out per call')
    g, r = np.concatenate(got, axis=1), np.concatenate(ref, axis=1)
    for j, b in enumerate(rows):
        ok, info = _close(g[j], r[b])
        print(name, what, 'row', b, '(shape, shape, rms err, rms ref)', info)
        assert ok and np.isfinite(g[j]).all(), (name, what, b, info)


def _segments(img):
    """[(kind, index, float32 view)] of an exported image"""
    nseg = struct.unpack_from('<i', img, HEAD - 16)[0]
    off, segs = HEAD + 16 * nseg, []
    for k in range(nseg):
        kind, index, n = struct.unpack_from('<iiq', img, HEAD + 16 * k)
        segs.append((kind, index, np.frombuffer(img, '<f4', n // 4, off)))
        off += (n + 15) // 16 * 16
    assert off == len(img)
    return segs


# ------------------------------------------------------------------------------------------------ 1. byte identity
@pytest.mark.parametrize('name', ALL)
def test_select_and_concat_are_copies(name):
    _torch()
    _, img, _ = _clean(name)
    eng = _engine(name)
    with StreamSnapshot.from_bytes(img) as src:
        with src.select(eng, [0, 1, 2, 3]) as same:
            assert same.batch == 4 and same.to_bytes() == img
        with src.select(eng, [0, 2]) as even, src.select(eng, [1, 3]) as odd:
            assert even.batch == odd.batch == 2
            with StreamSnapshot.concat(eng, [even, odd]) as joined:
                assert joined.batch == 4 and joined.to_bytes() != img
                with joined.select(eng, [0, 2, 1, 3]) as back:
                    assert back.to_bytes() == img
                # ... into an object that already holds the layout: no new payload (the device size stays), the same bytes
                n0 = even.nbytes
                assert joined.select(eng, [0, 1], out=even) is even and even.nbytes == n0
                with src.select(eng, [0, 2]) as again:
                    assert even.to_bytes() == again.to_bytes()


# ------------------------------------------------------------------------------------------------ 2. continuation
@pytest.mark.parametrize('name,running', [(n, False) for n in ALL] + [('crn', True), ('dccrn', True)])
def test_selected_rows_continue_as_in_their_group(name, running):
    torch = _torch()
    ref_outs, img, c = _clean(name, running)
    eng = _engine(name)
    rows = [3, 1]
    xt = torch.from_numpy(_signal()[rows]).cuda()
    with StreamSnapshot.from_bytes(img) as src, src.select(eng, rows) as part:
        eng.stream_restore(part)
        got = _push_all(eng, xt, CUT)
    _check_rows(name, got, ref_outs, rows, 'running scale' if running else 'given scale')


# ------------------------------------------------------------------------------------------------ 3. no row reaches another
@pytest.mark.parametrize('name', ['crn', 'dpcrn', 'dccrn', RLSTM, 'g2net_new', 'fullsubnet_cum'])
def test_no_row_reaches_another(name):
    """Rows 0 and 2 are fed NaN from the first sample, so everything they have written is NaN.  A wrong (outer, inner) of any buffer
    hands a clean row some of it, or leaves a NaN row something finite.  `Written by the row`: the state starts as zeros, so a float
    that is not zero in the clean group's snapshot of the same moment has been written."""
    torch = _torch()
    ref_outs, clean_img, c = _clean(name)
    eng = _engine(name)
    x = _signal().copy()
    x[[0, 2]] = np.nan
    xt = torch.from_numpy(x).cuda()
    eng.stream_begin(B4, c=torch.from_numpy(c).cuda())
    outs = [eng.stream_push(xt[:, p:p + PIECE].contiguous()).cpu().numpy() for p in STARTS[:CUT]]
    snap = eng.stream_save()
    outs += _push_all(eng, xt, CUT)
    whole = np.concatenate(outs, axis=1)
    assert np.isfinite(whole[[1, 3]]).all(), (name, 'a clean row of the uninterrupted group turned NaN')
    with snap, snap.select(eng, [1, 3]) as clean_rows, snap.select(eng, [0]) as nan_row, StreamSnapshot.from_bytes(clean_img) as cs, \
            cs.select(eng, [0]) as clean_row0:
        for kind, index, v in _segments(clean_rows.to_bytes()):
            assert np.isfinite(v).all(), (name, 'NaN in a clean row, segment', kind, index)
        written = 0
        for (kind, index, v), (_, _, w) in zip(_segments(nan_row.to_bytes()), _segments(clean_row0.to_bytes())):
            if kind in (KIND_HIST, KIND_H, KIND_CELL) and name in ('crn', 'dccrn', RLSTM):
                hit = w != 0
                written += int(hit.sum())
                assert np.isnan(v[hit]).all(), (name, 'a finite value in the NaN row, segment', kind, index, int((~np.isnan(v[hit])).sum()))
        assert written > 1000 or name not in ('crn', 'dccrn', RLSTM), (name, written)
        eng.stream_restore(clean_rows)
        got = _push_all(eng, torch.from_numpy(_signal()[[1, 3]]).cuda(), CUT)
    _check_rows(name, got, ref_outs, [1, 3], 'next to NaN rows')


# ------------------------------------------------------------------------------------------------ 4. concat, fork
@pytest.mark.parametrize('name', ['crn', 'g2net_new'])
def test_two_groups_joined_continue_as_on_their_own(name):
    torch = _torch()
    e4 = _engine(name)
    pair = [_engine(name, 2, 'a'), _engine(name, 2, 'b')]
    x = _signal()
    c = e4.rms_scale(torch.from_numpy(x).cuda())
    snaps, own = [], []
    for k, eng in enumerate(pair):
        xt = torch.from_numpy(x[2 * k:2 * k + 2]).cuda()
        eng.stream_begin(2, c=c[2 * k:2 * k + 2].contiguous())
        for p in STARTS[:CUT]:
            eng.stream_push(xt[:, p:p + PIECE].contiguous())
        snaps.append(eng.stream_save())
        own.append(_push_all(eng, xt, CUT))
    with snaps[0], snaps[1], StreamSnapshot.concat(e4, snaps) as joined:
        assert joined.batch == 4
        e4.stream_restore(joined)
        got = _push_all(e4, torch.from_numpy(x).cuda(), CUT)
    assert [o.shape[1] for o in got] == [o.shape[1] for o in own[0]] == [o.shape[1] for o in own[1]]
    g = np.concatenate(got, axis=1)
    want = np.concatenate([np.concatenate(o, axis=1) for o in own], axis=0)
    for b in range(4):
        ok, info = _close(g[b], want[b])
        print(name, 'joined row', b, info)
        assert ok, (name, b, info)


@pytest.mark.parametrize('name', ['crn', 'dccrn'])
def test_fork_gives_two_equal_rows(name):
    torch = _torch()
    ref_outs, img, _ = _clean(name)
    eng = _engine(name)
    xt = torch.from_numpy(_signal()[[1, 1]]).cuda()
    with StreamSnapshot.from_bytes(img) as src, src.select(eng, [1, 1]) as fork:
        eng.stream_restore(fork)
        got = np.concatenate(_push_all(eng, xt, CUT), axis=1)
    assert np.array_equal(got[0], got[1])
    _check_rows(name, [got], [np.concatenate(ref_outs[CUT:], axis=1)], [1, 1], 'fork')


# ------------------------------------------------------------------------------------------------ 5. before the first frame
@pytest.mark.parametrize('name', ['crn', 'g2net_new', 'dccrn'])
def test_select_before_the_first_frame(name):
    torch = _torch()
    eng = _engine(name)
    x = _signal()
    xt = torch.from_numpy(x).cuda()
    c = eng.rms_scale(xt)
    off = _model(name, 1, L)
    want = off.enhance_batch(xt[2:3].contiguous()).cpu().numpy()
    off.engine.close()
    eng.stream_begin(B4, c=c)
    first = eng.stream_push(xt[:, :100].contiguous())
    assert first.shape[1] == 0
    with eng.stream_save() as snap, snap.select(eng, [2]) as one:
        eng.stream_restore(one)
        outs = [eng.stream_push(xt[2:3, 100:PIECE].contiguous()).cpu().numpy()] + _push_all(eng, xt[2:3], 1)
    ok, info = _close(np.concatenate(outs, axis=1), want)
    print(name, 'selected before the first frame vs offline', info)
    assert ok, (name, info)


# ------------------------------------------------------------------------------------------------ 6. sliding engine
def test_select_after_a_slide():
    """a window that has slid: the window segment starts at keep > 0"""
    torch = _torch()
    eng = _engine('crn', B4, 'sliding', sliding_stream=True)
    n, piece = 9000, 1000
    starts = list(range(0, n, piece))
    x = _signal(n, B4, 930)
    xt = torch.from_numpy(x).cuda()
    c = eng.rms_scale(xt[:, :MS].contiguous())
    eng.stream_begin(B4, c=c)
    ref = [eng.stream_push(xt[:, p:p + piece].contiguous()).cpu().numpy() for p in starts[:6]]      # 6000 > 4480: it has slid
    snap = eng.stream_save()
    assert struct.unpack_from('<i', snap.to_bytes(), 8 + 10 * 4)[0] > 0                            # keep
    ref += _push_all(eng, xt, 6, starts, piece)
    rows = [3, 1]
    with snap, snap.select(eng, rows) as part:
        eng.stream_restore(part)
        got = _push_all(eng, torch.from_numpy(x[rows]).cuda(), 6, starts, piece)
    _check_rows('crn', got, ref, rows, 'sliding')


# ------------------------------------------------------------------------------------------------ 7. source-rate pair
def test_source_rate_pair():
    torch = _torch()
    from se_amd.source_stream import SourceRateStream
    eng = _engine('crn')
    n, piece, rows = 3 * L, 3 * PIECE, [2, 0]
    starts = list(range(0, n, piece))
    x = _signal(n, 3, 960)
    xt = torch.from_numpy(x).cuda()

    def run(srs, xs, first):
        ys, outs = [], []
        for p in starts[first:]:
            y = srs.resampler.push(xs[:, p:p + piece].contiguous())
            ys.append(y.cpu().numpy())
            outs.append(srs.engine.stream_push(y).cpu().numpy())
        tail = srs.resampler.flush()
        ys.append(tail.cpu().numpy())
        if tail.shape[1]:
            outs.append(srs.engine.stream_push(tail).cpu().numpy())
        outs.append(srs.engine.stream_flush().cpu().numpy())
        return ys, outs

    with SourceRateStream(eng, 48000, max_push=piece) as srs:
        srs.begin(3)
        head = []
        for p in starts[:CUT]:
            y = srs.resampler.push(xt[:, p:p + piece].contiguous())
            head.append(y.cpu().numpy())
            srs.engine.stream_push(y)
        snap = srs.save()
        ref_y, ref_out = run(srs, xt, CUT)
        with snap, snap.select(eng, rows) as part:
            assert part.engine.batch == 2 and part.resampler.counts()[2] == 2
            srs.restore(part)
            got_y, got_out = run(srs, torch.from_numpy(x[rows]).cuda(), CUT)
    assert len(got_y) == len(ref_y)
    for g, r in zip(got_y, ref_y):                                  # the resampler is row- and batch-independent: bit for bit
        assert g.shape[1] == r.shape[1] and np.array_equal(g, r[rows])
    _check_rows('crn', got_out, ref_out, rows, 'source rate')


# ------------------------------------------------------------------------------------------------ 8. refusals that need the device
def test_refusals_leave_the_running_stream_as_it_was():
    torch = _torch()
    ref_outs, img, c = _clean('crn')
    _, img_dccrn, _ = _clean('dccrn')
    _, img_snr, _ = _clean('dccrn_snr')
    eng, dccrn = _engine('crn'), _engine('dccrn')
    xt = torch.from_numpy(_signal()).cuda()
    eng.stream_begin(B4, c=torch.from_numpy(c).cuda())
    outs = [eng.stream_push(xt[:, p:p + PIECE].contiguous()).cpu().numpy() for p in STARTS[:CUT]]
    with StreamSnapshot.from_bytes(img) as src, StreamSnapshot.from_bytes(img_dccrn) as other, StreamSnapshot.from_bytes(img_snr) as snr, \
            StreamSnapshot() as empty:
        with pytest.raises(EngineError, match='se_stream_state_select: the snapshot was taken on model id'):
            other.select(eng, [0])
        with pytest.raises(EngineError, match='se_stream_state_concat: the snapshot was taken on model id'):
            StreamSnapshot.concat(eng, [other])
        with pytest.raises(EngineError, match='dst == src'):
            src.select(eng, [0], out=src)
        with pytest.raises(EngineError, match=r'dst == parts\[1\]'):
            StreamSnapshot.concat(eng, [other, src], out=src)
        with pytest.raises(EngineError, match=r'rows\[1\] = 4 outside 0 \.\. 3'):
            src.select(eng, [0, 4])
        with pytest.raises(EngineError, match='the stream state object is empty'):
            empty.select(eng, [0])
        with pytest.raises(EngineError, match=r'parts\[0\] and parts\[1\] differ: model'):
            StreamSnapshot.concat(eng, [src, other])
        assert src.to_bytes() == img
        # other flags: the look-ahead DCCRN's snapshot on ... the causal-decoder one's engine is a matter of se_config.flags
        with pytest.raises(EngineError, match='se_stream_state_select: se_config.flags differ'):
            snr.select(dccrn, [0])
        outs += _push_all(eng, xt, CUT)
    assert [o.shape for o in outs] == [o.shape for o in ref_outs]
    got, ref = np.concatenate(outs, axis=1), np.concatenate(ref_outs, axis=1)
    assert np.array_equal(got, ref)
    off = _model('crn', B4, L)
    ok, info = _close(got, off.enhance_batch(xt).cpu().numpy())
    off.engine.close()
    assert ok, info
