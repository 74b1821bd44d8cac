"""GPU: parked streams that began at different times joined into one group (se_stream_state_join, StreamSnapshot.join).

CRN, DPCRN (320 / 160), DCCRN with the decoder that looks six frames ahead and the causal-decoder DCCRN (512 / 128), with the models,
weight seeds and the bar of tests/test_gpu_sliding_stream.py (`_make`, `_close`: identical shape and rms(got - ref) < 1e-6 + 2e-5
rms(ref) - the continued-row bar of tests/test_gpu_stream_select.py).  Engines are sliding, for 3 rows and max_samples = 16000 (one
second); the late caller A streams 18001 samples, the group it joins is 5 hops ahead of it, so every continued stream slides once.
A rebased row that continues alone runs the kernels it ran before at the same batch size and is held to bit identity; rows that
continue in a larger group are held to the bar, against the offline decode of their whole signal."""
import functools
import struct

import numpy as np
import pytest

import se_amd  # noqa: F401
from se_amd import synth
from se_amd.engine import EngineError, StreamSnapshot
from test_gpu_sliding_stream import _close, _make

pytestmark = pytest.mark.gpu

MS, B3 = 16000, 3
MODELS = ['crn', 'dpcrn', 'dccrn', 'dccrn_snr']
GEOM = {'crn': (320, 160, 0), 'dpcrn': (320, 160, 0), 'dccrn': (512, 128, 6), 'dccrn_snr': (512, 128, 0)}      # n_fft, hop, look-ahead
LA = 18001                       # samples of the late caller: past the window of 16000 + n_fft + hop, no hop multiple
AHEAD = 5                        # hops the group is ahead of the late caller
L3, K3 = 5001, 17000             # test 3: the late caller's samples; the group is saved behind sample K3, right after its slide
HEAD = 104                       # csrc/stream_manifest.h: magic, version, 18 int32, p_in, p_out, nseg, pad, payload bytes
PIECES = (37, 1000, 3, 481, 2000, 4000)
SEED_A, SEED_G, SEED_H, SEED_G3 = 970, 971, 972, 973


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _threshold(name):
    """csrc/stream_join.h stream_left_edge_frames"""
    n_fft, hop, lag = GEOM[name]
    return max(1, -(-(n_fft // 2) // hop), 0 if hop >= n_fft // 2 else -(-n_fft // hop) - 1 + lag)


def _n_at(name, frames, extra=7):
    """samples after which exactly `frames` frames are transformed (+ a few that are no multiple of anything)"""
    n_fft, hop, _ = GEOM[name]
    return (frames - 1) * hop + n_fft // 2 + 1 + extra


_ENGINES, _OFFLINE = {}, {}


def _engine(name, B=B3, ms=MS):
    """one sliding engine per model for the whole module: its streams follow one another on it, as a server's would"""
    if (name, B, ms) not in _ENGINES:
        _ENGINES[(name, B, ms)] = _make(name, B, ms, sliding_stream=True).engine
    return _ENGINES[(name, B, ms)]


@pytest.fixture(scope='module', autouse=True)
def _release():
    yield
    for eng in _ENGINES.values():
        eng.close()
    for m in _OFFLINE.values():
        m.engine.close()
    _ENGINES.clear()
    _OFFLINE.clear()
    _ref.cache_clear()
    _alone.cache_clear()


@functools.lru_cache(maxsize=None)
def _ref(name, seed, L):
    """(signal, its offline decode, its unit-RMS scale), one row: computed once, shared, never written to"""
    torch = _torch()
    if name not in _OFFLINE:
        _OFFLINE[name] = _make(name, 1, 24000)
    m = _OFFLINE[name]
    x = synth.synth_clip(seed, 'speech' if seed % 2 == 0 else 'white', L)[None]
    xt = torch.from_numpy(x).cuda()
    ref = m.enhance_batch(xt).cpu().numpy()
    c = m.engine.rms_scale(xt).cpu().numpy()
    for a in (x, ref, c):
        a.setflags(write=False)
    return x, ref, c


def _cuts(n, pieces=PIECES):
    """[0, n) in uneven pieces (the last size repeats)"""
    pos, k, out = 0, 0, []
    while pos < n:
        m = min(pieces[min(k, len(pieces) - 1)], n - pos)
        out.append((pos, pos + m))
        pos += m
        k += 1
    return out


def _head(eng, x, c, n, **kw):
    """a one-row stream of x begun on eng and pushed to sample n; returns the output so far"""
    torch = _torch()
    eng.stream_begin(1, c=torch.from_numpy(c).cuda(), **kw)
    return eng.stream_push(torch.from_numpy(x[:, :n]).cuda().contiguous()).cpu().numpy()


def _tail(eng, rows):
    """pushes the rows' remaining samples - rows: [(signal, first sample)], equally many left in each - in uneven pieces and flushes; the
    outputs of every call, flush last"""
    torch = _torch()
    left = rows[0][0].shape[1] - rows[0][1]
    assert all(x.shape[1] - n0 == left for x, n0 in rows)
    xt = torch.from_numpy(np.concatenate([x[:, n0:] for x, n0 in rows])).cuda()
    outs = [eng.stream_push(xt[:, a:b].contiguous()).cpu().numpy() for a, b in _cuts(left)]
    outs.append(eng.stream_flush().cpu().numpy())
    return outs


@functools.lru_cache(maxsize=None)
def _alone(name):
    """The callers of tests 1, 2 and 4, each streamed alone at batch 1 on the module's engine and parked: A just past the left-edge
    threshold, G and H (other signals) AHEAD hops further on, in phase.  A's stream then runs on to its end: the uninterrupted
    reference.  Images and outputs are computed once and never written to."""
    eng = _engine(name)
    hop = GEOM[name][1]
    nA = _n_at(name, _threshold(name))
    nG = nA + AHEAD * hop
    d = {'nA': nA, 'nG': nG}
    for key, seed, L, n in (('G', SEED_G, LA + AHEAD * hop, nG), ('H', SEED_H, LA + AHEAD * hop, nG), ('A', SEED_A, LA, nA)):
        x, _, c = _ref(name, seed, L)
        d['out' + key] = _head(eng, x, c, n)
        with eng.stream_save() as snap:
            d['img' + key] = snap.to_bytes()
            d['cnt' + key] = snap.counts()
    d['restA'] = _tail(eng, [(_ref(name, SEED_A, LA)[0], nA)])
    return d


def _check_row(name, what, head, outs, row, ref):
    got = np.concatenate([head[0]] + [o[row] for o in outs])
    ok, info = _close(got, ref[0])
    print(name, what, 'row', row, '(shape, shape, rms err, rms ref)', info)
    assert ok and np.isfinite(got).all(), (name, what, row, info)


# ------------------------------------------------------------------------------------------------ 1. the rebase is exact
@pytest.mark.parametrize('name', MODELS)
def test_rebased_row_continues_bit_for_bit(name):
    _torch()
    d = _alone(name)
    eng = _engine(name)
    hop = GEOM[name][1]
    assert d['cntA'][2] == _threshold(name) and d['cntG'][1] - d['cntA'][1] == AHEAD * hop and d['cntA'][4] == hop
    xA = _ref(name, SEED_A, LA)[0]
    with StreamSnapshot.from_bytes(d['imgG']) as g, StreamSnapshot.from_bytes(d['imgA']) as a:
        with pytest.raises(EngineError, match=r'se_stream_state_concat: parts\[0\] and parts\[1\] differ: n_total %d vs %d' % (d['nG'], d['nA'])):
            StreamSnapshot.concat(eng, [g, a])
        with StreamSnapshot.join(eng, [g, a]) as j, j.select(eng, [1]) as one, j.select(eng, [0]) as zero:
            assert j.batch == 2 and j.counts() == (2,) + d['cntG'][1:]
            assert one.counts() == d['cntG'] and zero.to_bytes() == d['imgG']          # A on G's counters; G itself is a copy
            eng.stream_restore(one)
            got = _tail(eng, [(xA, d['nA'])])
    ref = d['restA']
    assert [o.shape for o in got] == [o.shape for o in ref], (name, 'n_out per call')
    for k, (o, r) in enumerate(zip(got, ref)):
        assert np.array_equal(o, r), (name, 'call', k, float(np.abs(o - r).max()))
    # one part: a copy
    with StreamSnapshot.from_bytes(d['imgA']) as a, StreamSnapshot.join(eng, [a]) as same:
        assert same.to_bytes() == d['imgA']


# ------------------------------------------------------------------------------------------------ 2. joined rows get their own result
@pytest.mark.parametrize('name', MODELS)
def test_joined_rows_get_their_own_result(name):
    _torch()
    d = _alone(name)
    eng = _engine(name)
    hop = GEOM[name][1]
    xA, refA, _ = _ref(name, SEED_A, LA)
    xG, refG, _ = _ref(name, SEED_G, LA + AHEAD * hop)
    with StreamSnapshot.from_bytes(d['imgG']) as g, StreamSnapshot.from_bytes(d['imgA']) as a, StreamSnapshot.join(eng, [g, a]) as j:
        eng.stream_restore(j)
        outs = _tail(eng, [(xG, d['nG']), (xA, d['nA'])])
    _check_row(name, 'joined', d['outG'], outs, 0, refG)
    _check_row(name, 'joined', d['outA'], outs, 1, refA)


# ------------------------------------------------------------------------------------------------ 3. windows of different live lengths
def _pad_window(img, cols):
    """the image of the same stream saved with a window that starts `cols` samples earlier, those samples NaN: keep is lowered, every
    window row gets `cols` NaN in front (the region behind the row's live samples)"""
    assert cols % 4 == 0
    f = list(struct.unpack_from('<18i', img, 8))
    batch, n_total, keep = f[5], f[7], f[10]
    nseg = struct.unpack_from('<i', img, HEAD - 16)[0]
    segs = [struct.unpack_from('<iiq', img, HEAD + 16 * k) for k in range(nseg)]
    assert segs[-1][0] == 8 and segs[-1][2] == batch * (n_total - keep) * 4
    fixed = sum((n + 15) // 16 * 16 for _, _, n in segs[:-1])
    pay = HEAD + 16 * nseg
    win = np.frombuffer(img, '<f4', batch * (n_total - keep), pay + fixed).reshape(batch, -1)
    new = np.concatenate([np.full((batch, cols), np.nan, '<f4'), win], axis=1).tobytes()
    new += bytes(-len(new) % 16)
    f[10] = keep - cols
    segs[-1] = (8, 0, batch * (n_total - keep + cols) * 4)
    return (img[:8] + struct.pack('<18i', *f) + img[80:HEAD - 8] + struct.pack('<q', fixed + len(new)) +
            b''.join(struct.pack('<iiq', *s) for s in segs) + img[pay:pay + fixed] + new)


def _window(img):
    f = struct.unpack_from('<18i', img, 8)
    n = f[5] * (f[7] - f[10])
    return np.frombuffer(img, '<f4', n, len(img) - (n * 4 + 15) // 16 * 16).reshape(f[5], -1)


@pytest.mark.parametrize('name', MODELS)
def test_windows_of_different_live_lengths(name):
    """G is saved right after its window has slid, A long before a slide.  The engine's window buffer cannot be reached from here, so
    the region behind each row's live window is filled with NaN in the saved images: the same streams saved with windows that start
    8 (G) and 20 (A) samples earlier, those samples NaN."""
    torch = _torch()
    eng = _engine(name)
    n_fft, hop, _ = GEOM[name]
    nA = _n_at(name, _threshold(name) + 2)
    shift = -(-(K3 - nA) // hop) * hop
    nG = nA + shift
    xA, refA, cA = _ref(name, SEED_A, L3)
    xG, refG, cG = _ref(name, SEED_G3, L3 + shift)
    eng.stream_begin(1, c=torch.from_numpy(cG).cuda())
    xt = torch.from_numpy(xG).cuda()
    headG = [eng.stream_push(xt[:, p:p + 4000].contiguous()).cpu().numpy() for p in range(0, MS, 4000)]
    assert nG - MS > n_fft + hop + 4                     # the window holds max_samples + n_fft + hop (+ 3): this push does not fit
    headG.append(eng.stream_push(xt[:, MS:nG].contiguous()).cpu().numpy())
    with eng.stream_save() as snap:
        imgG = snap.to_bytes()
    headA = _head(eng, xA, cA, nA)
    with eng.stream_save() as snap:
        imgA = snap.to_bytes()
    keepG, keepA = (struct.unpack_from('<i', i, 8 + 10 * 4)[0] for i in (imgG, imgA))
    assert keepG > MS - n_fft and keepA + shift == keepG
    with StreamSnapshot.from_bytes(_pad_window(imgG, 8)) as g, StreamSnapshot.from_bytes(_pad_window(imgA, 20)) as a, \
            StreamSnapshot.from_bytes(imgG) as g0, StreamSnapshot.from_bytes(imgA) as a0:
        assert np.isnan(_window(g.to_bytes())[:, :8]).all() and np.isnan(_window(a.to_bytes())[:, :20]).all()
        with StreamSnapshot.join(eng, [g0, a0]) as plain, StreamSnapshot.join(eng, [g0, a]) as trimmed:
            w = _window(plain.to_bytes())
            assert w.shape == (2, nG - keepG) and np.array_equal(w[0], xG[0, keepG:nG]) and np.array_equal(w[1], xA[0, keepA:nA])
            assert trimmed.to_bytes() == plain.to_bytes()                # A's 20 NaN columns are skipped: nothing of them arrives
        with StreamSnapshot.join(eng, [g, a]) as j:
            w = _window(j.to_bytes())
            assert w.shape == (2, nG - keepG + 8) and np.isnan(w[:, :8]).all()
            assert np.array_equal(w[0, 8:], xG[0, keepG:nG]) and np.array_equal(w[1, 8:], xA[0, keepA:nA])
            eng.stream_restore(j)
            outs = _tail(eng, [(xG, nG), (xA, nA)])
    assert all(np.isfinite(o).all() for o in outs)
    _check_row(name, 'after a slide', [np.concatenate(headG, axis=1)[0]], outs, 0, refG)
    _check_row(name, 'before a slide', headA, outs, 1, refA)


# ------------------------------------------------------------------------------------------------ 4. three parts, batch 3
@pytest.mark.parametrize('name', MODELS)
def test_three_parts_in_the_order_given(name):
    _torch()
    d = _alone(name)
    eng = _engine(name)
    hop = GEOM[name][1]
    rows = [('G', SEED_G, LA + AHEAD * hop, d['nG']), ('H', SEED_H, LA + AHEAD * hop, d['nG']), ('A', SEED_A, LA, d['nA'])]
    with StreamSnapshot.from_bytes(d['imgG']) as g, StreamSnapshot.from_bytes(d['imgH']) as h, StreamSnapshot.from_bytes(d['imgA']) as a, \
            StreamSnapshot.join(eng, [g, h, a]) as j:
        assert j.batch == 3 and j.counts() == (3,) + d['cntG'][1:]
        for r, key in enumerate('GH'):
            with j.select(eng, [r]) as one:
                assert one.to_bytes() == d['img' + key]
        eng.stream_restore(j)
        outs = _tail(eng, [(_ref(name, seed, L)[0], n) for _, seed, L, n in rows])
    for r, (key, seed, L, _) in enumerate(rows):
        _check_row(name, 'three parts', d['out' + key], outs, r, _ref(name, seed, L)[1])


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_leave_dst_and_the_running_stream_as_they_were():
    torch = _torch()
    d = _alone('crn')
    eng = _engine('crn')
    xA, _, cA = _ref('crn', SEED_A, LA)
    nA = d['nA']
    _head(eng, xA, cA, nA + 50)
    off_phase = eng.stream_save()
    _head(eng, xA, cA, nA, max_chunk_frames=8)
    chunk8 = eng.stream_save()
    eng.stream_begin(1, running_rms=True)
    eng.stream_push(torch.from_numpy(xA[:, :nA]).cuda().contiguous())
    running = eng.stream_save()
    # a DCCRN two frames into its stream, and one frame further: 512 / 128 can be rebased from frame 3 on
    snr = _engine('dccrn_snr')
    x3, _, c3 = _ref('dccrn_snr', SEED_A, LA)
    _head(snr, x3, c3, _n_at('dccrn_snr', 2))
    early = snr.stream_save()
    snr.stream_push(torch.from_numpy(x3[:, _n_at('dccrn_snr', 2):_n_at('dccrn_snr', 3)]).cuda().contiguous())
    later = snr.stream_save()
    assert early.counts()[2] == 2 and later.counts()[2] == 3
    head = _head(eng, xA, cA, nA)                        # the running stream: A, as in the uninterrupted reference
    assert np.array_equal(head, d['outA'])
    with off_phase, chunk8, running, early, later, StreamSnapshot.from_bytes(d['imgA']) as a, StreamSnapshot.from_bytes(d['imgG']) as g, \
            StreamSnapshot.from_bytes(d['imgA']) as dst:
        for parts, e, reason in [
                ([a, off_phase], eng, r'se_stream_state_join: parts\[0\] and parts\[1\] are out of phase: n_total %d vs %d, the shift -50 is not a '
                                      r'multiple of lcm\(hop, 4\) = 160' % (nA, nA + 50)),
                ([later, early], snr, r'parts\[1\] is short of the left edge: t_done 2, a stream can be rebased from t_done 3 on'),
                ([early, later], snr, r'parts\[0\] is short of the left edge: t_done 2'),
                ([g, running], eng, r'parts\[1\] is a running-scale stream'),
                ([g, chunk8], eng, r'parts\[0\] and parts\[1\] differ: max_chunk 16 vs 8'),
                ([g, dst], eng, r'dst == parts\[1\]: the rows are read while they are written'),
                ([g, early], eng, r'parts\[0\] and parts\[1\] differ: model'),
                ([early, later], eng, r'se_stream_state_join: the snapshot was taken on model id')]:
            with pytest.raises(EngineError, match=reason):
                StreamSnapshot.join(e, parts, out=dst)
            assert dst.to_bytes() == d['imgA'] and dst.batch == 1
        with pytest.raises(EngineError, match='the stream state object is empty'), StreamSnapshot() as empty:
            StreamSnapshot.join(eng, [g, empty], out=dst)
        with pytest.raises(EngineError, match=r'se_stream_state_concat: parts\[0\] and parts\[1\] differ: n_total'):
            StreamSnapshot.concat(eng, [g, a], out=dst)
        assert dst.to_bytes() == d['imgA']
        rest = _tail(eng, [(xA, nA)])
    assert [o.shape for o in rest] == [o.shape for o in d['restA']]
    assert all(np.array_equal(o, r) for o, r in zip(rest, d['restA']))


@pytest.mark.parametrize('name,counts', [('ctsnet_new', 'the cumulative LayerNorm divides its running sums by the number of frames'),
                                         ('fullsubnet_cum', 'the cumulative Laplace norm divides its running sums by the absolute frame index')])
def test_models_whose_state_counts_frames_are_refused(name, counts):
    torch = _torch()
    eng = _engine(name, 1, 4000)
    x = torch.from_numpy(synth.synth_clip(SEED_A, 'speech', 4000)[None]).cuda()
    eng.stream_begin(1)
    eng.stream_push(x[:, :2000].contiguous())
    with eng.stream_save() as first:
        ref = eng.stream_push(x[:, 2000:3280].contiguous()).cpu().numpy()          # 1280 samples: 8 hops of 160, 5 of 256
        with eng.stream_save() as second, StreamSnapshot.from_bytes(first.to_bytes()) as dst:
            img = dst.to_bytes()
            with pytest.raises(EngineError, match="se_stream_state_join: this model's stream state cannot be rebased: " + counts):
                StreamSnapshot.join(eng, [second, first], out=dst)
            assert dst.to_bytes() == img
            with pytest.raises(EngineError, match='cannot be rebased'):          # ... whatever the shift
                StreamSnapshot.join(eng, [first], out=dst)
            # the running stream goes on as the restored copy of itself does
            tail = [eng.stream_push(x[:, 3280:].contiguous()).cpu().numpy(), eng.stream_flush().cpu().numpy()]
            eng.stream_restore(first)
            again = [eng.stream_push(x[:, 2000:3280].contiguous()).cpu().numpy(), eng.stream_push(x[:, 3280:].contiguous()).cpu().numpy(),
                     eng.stream_flush().cpu().numpy()]
    assert all(np.array_equal(a, b) for a, b in zip([ref] + tail, again))
