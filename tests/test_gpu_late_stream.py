"""GPU: frame-online streams late in life.  A sliding stream is promised 2^31 - 1 - max(max_samples, n_fft + 32 hop) samples (37 hours at
16 kHz), and csrc/stream_join.h derives that nothing a push launches depends on the absolute position once the stream is past its left
edge.  Streaming a day of audio is not needed to get to the far end of the counters: a parked stream is a host image, and
tests/late_stream_ref.py `rebase_image` moves one by any number of frames (n_total, o_done, keep, t_done and every row origin; the
helper is pinned on the CPU by tests/test_late_stream_host.py).  Every case here parks a stream after its window has slid, continues it
twice - run A from the image as it is, run B from the moved image - and holds B to A BIT FOR BIT: the number of samples every push and
the flush return, every sample (np.array_equal, no tolerance anywhere in this file), the payload of a second save outside the origin
entries, and the counters and origins of B, which are exactly those of A moved.  An index that wraps or loses exactness at the far end
shows as a difference.

Per network three moves, smallest first (a network whose smaller move fails does not run its larger ones):
  smallest     f = ring (1 without per-frame rings), the smallest legal move
  across 2^24  the smallest legal f that puts n_total above 2^24 samples during run B (and, where 2^24 frames fit under the limit, a
               fourth move that puts t_done above 2^24 frames: none of the streamable front ends - hops 160, 128, 256 - allows it)
  limit        the largest legal f; run B's last accepted push ends exactly at the stream limit, one more sample is refused with the
               engine's own message, and the stream goes on to flush what A flushes
Engines are sliding, max_samples = 4000, batch 2 ('speech' and 'white' rows), with a caller-supplied scale."""
import functools

import numpy as np
import pytest

import se_amd  # noqa: F401
from se_amd import synth
from se_amd.engine import EngineError, StreamSnapshot
from test_gpu_sliding_stream import FSN_KW, _make

import late_stream_ref as LS

pytestmark = pytest.mark.gpu

MS, B = 4000, 2
HEAD_PUSHES = 32                  # 10 ms pieces before the stream is parked: 5120 samples, past every window of max_samples + n_fft + hop
RMIN = 10001                      # samples after the park: at least 2.5 x max_samples, so the window slides twice more
PIECES = (37, 1000, 3, 481, 2000, 4000)      # the uneven pushes of the streaming suites; the last size repeats
REFUSAL = r'sliding stream longer than 2\^31 - 1 - max_samples samples'
# name: (how the engine is made, look-ahead in frames); the cLN networks and FullSubNet's cumulative norms run with row origins
NETS = {
    'crn': ({}, 0), 'lstm': ({}, 0), 'gcrn': ({}, 0), 'dpcrn': ({}, 0), 'dccrn': ({}, 6), 'dccrn_rlstm': ({}, 6), 'dccrn_snr': ({}, 6),
    'ctsnet_new': (dict(row_origins=True), 0), 'taylorsenet_new': (dict(row_origins=True), 0), 'g2net_new': (dict(row_origins=True), 0),
    'fullsubnet_cum': (dict(row_origins=True), 2), 'fullsubnet_cln': (dict(row_origins=True), 2),
}
MOVES = ('smallest', 'across_2_24', 'limit')
_ENGINES, _BROKEN, _ERRORS = {}, set(), []


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _engine(name):
    """one sliding engine per network for the whole module"""
    if name not in _ENGINES:
        kw = dict(NETS[name][0], sliding_stream=True)
        if name == 'dccrn_rlstm':          # DCCRN-E with the real LSTM (tests/test_gpu_dccrn_real_lstm.py)
            from se_amd.models import DCCRN
            m = DCCRN(rnn_units=256, masking_mode='E', kernel_num=[16, 32, 64, 128, 256, 256], max_batch=B, max_samples=MS, **kw).load_synthetic(24)
        elif name == 'fullsubnet_cln':     # tests/test_gpu_fullsubnet_norms.py
            from se_amd.models import Model
            m = Model(max_batch=B, max_samples=MS, p_in=0.5, p_out=2.0, norm_type='cumulative_layer_norm', **FSN_KW, **kw).load_synthetic(15)
        else:
            m = _make(name, B, MS, **kw)
        _ENGINES[name] = m.engine
    return _ENGINES[name]


@pytest.fixture(scope='module', autouse=True)
def _release():
    yield
    for eng in _ENGINES.values():
        eng.close()
    _ENGINES.clear()
    _parked.cache_clear()
    _run_a.cache_clear()
    _joined.cache_clear()


def _cuts(n):
    pos, k, out = 0, 0, []
    while pos < n:
        m = min(PIECES[min(k, len(PIECES) - 1)], n - pos)
        out.append((pos, pos + m))
        pos += m
        k += 1
    return out


def _plan(img, lag):
    """from the parked image alone: the move unit, the stream limit, the three moves and the samples R both runs push behind the park -
    the limit move is the largest legal one that leaves at least RMIN samples, and R is what then ends exactly at the limit"""
    d = LS.parse_image(img)
    hop, unit = d['hop'], max(1, d['ring'])
    assert hop % 4 == 0 and d['t_done'] >= LS.left_edge_frames(d['n_fft'], hop, lag) and d['keep'] > 0
    limit = LS.sample_limit(MS, d['n_fft'], hop)
    assert limit == 2 ** 31 - 1 - max(MS, d['n_fft'] + 32 * hop)                 # the formula tests/test_sliding_window_logic.py asserts
    f_lim = (limit - d['n_total'] - RMIN) // (hop * unit) * unit
    R = limit - d['n_total'] - f_lim * hop
    assert RMIN <= R < RMIN + hop * unit and R >= 2.5 * MS
    f_24 = -(-(2 ** 24 + 1 - d['n_total'] - R) // (hop * unit)) * unit            # the smallest legal f with n_total + R + f hop > 2^24
    assert d['n_total'] + f_24 * hop <= 2 ** 24 < d['n_total'] + R + f_24 * hop
    moves = {'smallest': unit, 'across_2_24': f_24, 'limit': f_lim}
    t_end = d['t_done'] + R // hop + 2
    if (2 ** 24 + unit + 1) * hop + d['n_total'] + R <= limit:                   # t_done above 2^24 frames: where the hop allows it
        moves['frames_2_24'] = -(-(2 ** 24 + 1 - t_end) // unit) * unit
    return dict(hop=hop, unit=unit, limit=limit, R=R, moves=moves, n0=d['n_total'])


@functools.lru_cache(maxsize=None)
def _parked(name, tracking=False):
    """the stream of `name` begun, pushed in 10 ms pieces until its window has slid, and parked: (image, plan, rest of the signal, scale)"""
    torch = _torch()
    eng = _engine(name)
    n0 = HEAD_PUSHES * 160
    # the signal is made before its length is known: R < RMIN + hop * ring <= RMIN + 256 * 1024
    x = np.stack([synth.synth_clip(880 + b, 'speech' if b == 0 else 'white', n0 + RMIN + 256 * 1024) for b in range(B)])
    xt = torch.from_numpy(x).cuda()
    if tracking:
        eng.stream_begin(B, tracking_rms=0.5)
    else:
        eng.stream_begin(B, c=eng.rms_scale(xt[:, :n0 + RMIN].contiguous()))
    for k in range(HEAD_PUSHES):
        eng.stream_push(xt[:, 160 * k:160 * (k + 1)].contiguous())
    with eng.stream_save() as snap:
        img = snap.to_bytes()
    plan = _plan(img, NETS[name][1])
    assert plan['n0'] == n0 > MS + LS.parse_image(img)['n_fft'] + plan['hop'] + 4          # the window has slid at least once
    assert LS.parse_image(img)['running'] == (2 if tracking else 0)
    rest = x[:, n0:n0 + plan['R']].copy()
    rest.setflags(write=False)
    return img, plan, rest


def _continue(eng, img, rest, at_limit=False):
    """restores img and pushes `rest` in uneven pieces; a second save; the flush.  (the outputs of every call, flush last; the image of
    the second save).  at_limit: the last push has ended at the stream limit - one more sample is refused, and the stream goes on"""
    torch = _torch()
    xt = torch.from_numpy(np.array(rest)).cuda()              # (a copy: `rest` is shared and read-only)
    with StreamSnapshot.from_bytes(img) as snap:
        eng.stream_restore(snap)
    outs = [eng.stream_push(xt[:, a:b].contiguous()).cpu().numpy() for a, b in _cuts(rest.shape[1])]
    if at_limit:
        with pytest.raises(EngineError, match=REFUSAL):
            eng.stream_push(xt[:, :1].contiguous())
    with eng.stream_save() as snap:
        img2 = snap.to_bytes()
        cnt2 = snap.counts()
    assert cnt2[1:4] == LS.counters(img2)[:3]
    outs.append(eng.stream_flush().cpu().numpy())
    return outs, img2


@functools.lru_cache(maxsize=None)
def _run_a(name, tracking=False):
    img, plan, rest = _parked(name, tracking)
    outs, img2 = _continue(_engine(name), img, rest)
    for o in outs:
        o.setflags(write=False)
    assert sum(o.shape[1] for o in outs) > plan['R'] - 2 * 512 and all(np.isfinite(o).all() for o in outs)
    return outs, img2


def _same_but_moved(what, img_a, img_b, f, hop):
    """image B is image A moved by f frames: counters, origins, and nothing else"""
    ca, cb = LS.counters(img_a), LS.counters(img_b)
    assert cb == (ca[0] + f * hop, ca[1] + f, ca[2] + f * hop, ca[3] + f * hop), (what, 'counters', ca, cb, f)
    oa, ob = LS.origins(img_a), LS.origins(img_b)
    assert (oa is None and ob is None) or ob == tuple(o + f for o in oa), (what, 'origins', oa, ob, f)
    assert len(img_a) == len(img_b), (what, 'image sizes')
    da, db = LS.parse_image(img_a), LS.parse_image(img_b)
    for k in LS.FIELDS:
        assert k in ('n_total', 't_done', 'o_done', 'keep') or da[k] == db[k], (what, 'header field', k, da[k], db[k])
    assert [s[:3] for s in da['segs']] == [s[:3] for s in db['segs']], (what, 'segment table')
    pa, pb = LS.payload_outside_origins(img_a), LS.payload_outside_origins(img_b)
    if pa != pb:
        bad = [(kind, index) for kind, index, n, off in da['segs'] if kind != LS.SNAP_ORIGIN and img_a[off:off + n] != img_b[off:off + n]]
        raise AssertionError((what, 'the payloads of the second save differ in segments (kind, index)', bad))


def _check_b(what, eng, img, rest, plan, f, ref, lag, at_limit):
    ref_outs, ref_img2 = ref
    moved = LS.rebase_image(img, f, lag=lag, max_samples=MS)
    n_end = LS.counters(moved)[0] + rest.shape[1]
    assert n_end <= plan['limit'] and (n_end == plan['limit']) == at_limit
    outs, img2 = _continue(eng, moved, rest, at_limit=at_limit)
    print(what, 'f', f, 'n_total of run B', LS.counters(moved)[0], '..', n_end, 'limit', plan['limit'], 'origins', LS.origins(moved))
    assert [o.shape for o in outs] == [o.shape for o in ref_outs], (what, 'samples returned per call', [o.shape for o in outs], [o.shape for o in ref_outs])
    for k, (o, r) in enumerate(zip(outs, ref_outs)):
        assert np.array_equal(o, r), (what, 'call', k, 'of', len(outs), 'differs: max |B - A|', float(np.abs(o - r).max()),
                                      'first at sample', int(np.argmax((o != r).any(axis=0))))
    _same_but_moved(what, ref_img2, img2, f, plan['hop'])
    assert LS.counters(img2)[0] == n_end


def _guarded(key, body):
    """a network whose smaller move failed does not run a larger one; after anything but a failed assertion - an error of the engine or of
    the device - no later case of this file starts work on the GPU at all"""
    assert not _ERRORS, ('an earlier case ended in an error, not in a failed assertion: nothing more is started on the device', _ERRORS)
    assert key not in _BROKEN, (key, 'a smaller move of this network has failed: the larger one is not run')
    try:
        body()
    except (AssertionError, pytest.fail.Exception):
        _BROKEN.add(key)
        raise
    except BaseException as ex:
        _BROKEN.add(key)
        _ERRORS.append((key, type(ex).__name__))
        raise


def _moves_of(plan):
    return [m for m in ('smallest', 'across_2_24', 'frames_2_24', 'limit') if m in plan['moves']]


# ------------------------------------------------------------------------------------------------ 1. every streamable network
@pytest.mark.parametrize('name,move', [(n, m) for n in NETS for m in MOVES])
def test_rebased_stream_continues_bit_for_bit(name, move):
    def body():
        eng = _engine(name)
        img, plan, rest = _parked(name)
        assert eng.row_origins == (LS.origins(img) is not None) and (LS.origins(img) in (None, (0, 0)))
        ref = _run_a(name)
        for m in ([move] if move != 'across_2_24' else ['across_2_24', 'frames_2_24']):
            if m in plan['moves']:
                _check_b((name, m), eng, img, rest, plan, plan['moves'][m], ref, NETS[name][1], m == 'limit')
    _guarded(name, body)


# ------------------------------------------------------------------------------------------------ 2. the tracking scale
@pytest.mark.parametrize('name,move', [(n, m) for n in ('crn', 'g2net_new') for m in MOVES])
def test_tracking_scale_stream_continues_bit_for_bit(name, move):
    """se_stream_begin_tracking: c_t and 1 / c_t of frame t live in rings at position t & (ring - 1), t the GROUP frame, so every move is a
    multiple of the ring length (no ring is rotated) - and the kernels that form the ring position do so from a late frame index"""
    def body():
        eng = _engine(name)
        img, plan, rest = _parked(name, True)
        assert plan['unit'] == LS.parse_image(img)['ring'] >= 64 and all(f % plan['unit'] == 0 for f in plan['moves'].values())
        _check_b((name, 'tracking', move), eng, img, rest, plan, plan['moves'][move], _run_a(name, True), NETS[name][1], move == 'limit')
    _guarded((name, 'tracking'), body)


# ------------------------------------------------------------------------------------------------ 3. origins of either sign
@functools.lru_cache(maxsize=None)
def _joined():
    """g2net_new: three one-row streams parked 3 hops ahead of, at, and 2 hops behind one position; two joins put the first and the last
    into one group on the counters of the middle one, with origins -3 and +2"""
    torch = _torch()
    name = 'g2net_new'
    eng = _engine(name)
    imgs = {}
    for key, pushes, seed in (('mid', HEAD_PUSHES, 890), ('old', HEAD_PUSHES + 3, 891), ('young', HEAD_PUSHES - 2, 892)):
        x = torch.from_numpy(synth.synth_clip(seed, 'speech' if seed % 2 == 0 else 'white', 160 * pushes)[None]).cuda()
        eng.stream_begin(1, c=eng.rms_scale(x))
        for k in range(pushes):
            eng.stream_push(x[:, 160 * k:160 * (k + 1)].contiguous())
        with eng.stream_save() as snap:
            imgs[key] = snap.to_bytes()
    with StreamSnapshot.from_bytes(imgs['mid']) as mid, StreamSnapshot.from_bytes(imgs['old']) as old, \
            StreamSnapshot.from_bytes(imgs['young']) as young, StreamSnapshot.join(eng, [mid, old]) as j1, j1.select(eng, [1]) as one, \
            StreamSnapshot.join(eng, [one, young]) as j2:
        img = j2.to_bytes()
    assert LS.origins(img) == (-3, 2) and LS.counters(img)[0] == 160 * HEAD_PUSHES
    plan = _plan(img, 0)
    rest = np.stack([synth.synth_clip(893 + b, 'speech' if b == 0 else 'white', plan['R']) for b in range(B)])
    rest.setflags(write=False)
    outs, img2 = _continue(eng, img, rest)
    assert LS.origins(img2) == (-3, 2)
    return img, plan, rest, (outs, img2)


@pytest.mark.parametrize('move', MOVES)
def test_rows_with_origins_of_either_sign_continue_bit_for_bit(move):
    def body():
        img, plan, rest, ref = _joined()
        f = plan['moves'][move]
        _check_b(('g2net_new', 'joined', move), _engine('g2net_new'), img, rest, plan, f, ref, 0, move == 'limit')
        assert LS.origins(LS.rebase_image(img, f, max_samples=MS)) == (f - 3, f + 2)
    _guarded(('g2net_new', 'joined'), body)
