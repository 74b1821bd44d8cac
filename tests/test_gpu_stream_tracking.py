"""GPU: frame-online streams on the tracking unit-RMS scale (se_stream_begin_tracking, include/se_engine.h): an exponentially forgetting
estimate with one value per STFT frame, defined on whole hop blocks of the input.  It is a function of the signal and not of the
pushes, it follows the level, and its state holds no absolute time, so such streams are parked, selected, concatenated and joined.

The end-to-end bound is the project's streamed-versus-offline bound of tests/test_gpu_streaming.py, 1e-6 + 2e-5 rms(ref): the runs
compared differ in their chunk tilings (and, after select / concat / join, in kernels selected by batch size).  Scales are compared
with the float64 restatement of tests/tracking_ref.py to 1e-6 relative (one float32 rounding of a float64 value, with slack)."""
import functools

import numpy as np
import pytest

import se_amd  # noqa: F401
from se_amd import synth
from se_amd.engine import EngineError, StreamSnapshot, samples_until_joinable
from conftest import rms
from test_gpu_sliding_stream import _make
import tracking_ref as TR

pytestmark = pytest.mark.gpu
GEOM = {'crn': (320, 160), 'dccrn': (512, 128)}
L = 12000
_M = {}


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _model(name, B, ms, **kw):
    key = (name, B, ms, tuple(sorted(kw.items())))
    if key not in _M:
        _M[key] = _make(name, B, ms, **kw)
    return _M[key]


@pytest.fixture(scope='module', autouse=True)
def _release():
    yield
    for m in _M.values():
        m.engine.close()
    _M.clear()


def _bound(ref):
    return 1e-6 + 2e-5 * rms(ref)


def _cuts(n, pieces, start=0):
    pos, k, out = start, 0, []
    while pos < n:
        m = min(pieces[min(k, len(pieces) - 1)], n - pos)
        out.append((pos, pos + m))
        pos += m
        k += 1
    return out


def _feed(eng, xt, cuts, flush=True, scales=None):
    """pushes xt[:, a:b] for the cuts, then flushes; the concatenated output (scales: a list that gets stream_scale() after every push)"""
    outs = []
    for a, b in cuts:
        outs.append(eng.stream_push(xt[:, a:b].contiguous()).cpu().numpy())
        if scales is not None:
            scales.append(eng.stream_scale().cpu().numpy())
    if flush:
        outs.append(eng.stream_flush().cpu().numpy())
    return np.concatenate(outs, axis=1)


def _close(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    e = rms(got - ref)
    print(what, 'rms err', e, 'bound', _bound(ref), 'rms ref', rms(ref))
    assert np.isfinite(got).all() and e < _bound(ref), (what, e, _bound(ref))


# ------------------------------------------------------------------------------------------------ 2. the anchor to the offline decode
@pytest.mark.parametrize('name', ['crn', 'dccrn'])
def test_periodic_signal_equals_offline_decode(name):
    """x[n] = g_b p[n mod hop] has the same energy in every block: W_k / E_k = hop / e for every k and lambda, so every c_t is the offline
    sqrt(L / sum x^2) (L a multiple of hop) and the tracking stream in 10 ms pushes is the pinned offline decode."""
    torch = _torch()
    n_fft, hop = GEOM[name]
    Lp = (L // (5 * hop)) * 5 * hop
    rng = np.random.default_rng(3)
    p = rng.standard_normal(hop)
    x = (np.array([[0.3], [0.011]]) * np.tile(p, Lp // hop)[None]).astype(np.float32)
    tau = 0.1
    lam = TR.lam_of(tau * 16000.0, hop)
    T = 1 + Lp // hop
    c = TR.frame_scales(x, n_fft, hop, lam, Lp, True, T)
    c_off = np.sqrt(Lp / (x.astype(np.float64) ** 2).sum(-1))
    # (frame 0 of a front end with n_fft / 2 == hop lies in front of the first block only where D == 0; here D >= 1)
    assert np.abs(c / c_off[:, None] - 1).max() < 1e-12
    m = _model(name, 2, Lp)
    xt = torch.from_numpy(x).cuda()
    ref = m.enhance_batch(xt).cpu().numpy()
    eng = m.engine
    eng.stream_begin(2, max_chunk_frames=4, tracking_rms=tau)
    sc = []
    got = _feed(eng, xt, _cuts(Lp, [160]), scales=sc)
    _close(got, ref, name + ' periodic, tracking vs offline')
    np.testing.assert_allclose(sc[-1], c_off, rtol=1e-6)


# ------------------------------------------------------------------------------------------------ 3. split independence
def _step_signal(B, n, seed):
    x = np.stack([synth.synth_clip(seed + b, 'speech', n) for b in range(B)])
    x[:, n // 2:] *= 8.0
    return x.astype(np.float32)


SPLITS = {'10ms': [160], 'uneven': [37, 1000, 3, 481, 2000], 'one': [L]}


def test_output_does_not_depend_on_the_split():
    torch = _torch()
    m = _model('crn', 2, L)
    eng = m.engine
    xt = torch.from_numpy(_step_signal(2, L, 820)).cuda()
    out = {}
    for mode in ('tracking', 'running'):
        for k, pieces in SPLITS.items():
            kw = dict(tracking_rms=0.5) if mode == 'tracking' else dict(running_rms=True)
            eng.stream_begin(2, max_chunk_frames={'10ms': 1, 'uneven': 4, 'one': 8}[k], **kw)
            out[mode, k] = _feed(eng, xt, _cuts(L, pieces))
    keys = list(SPLITS)
    for i in range(3):
        for j in range(i + 1, 3):
            a, b = out['tracking', keys[i]], out['tracking', keys[j]]
            _close(a, b, 'tracking %s vs %s' % (keys[i], keys[j]))
            ra, rb = out['running', keys[i]], out['running', keys[j]]
            e = rms(ra - rb)
            print('running', keys[i], keys[j], 'rms diff', e, '10 x bound', 10 * _bound(rb))
            assert e > 10 * _bound(rb), 'the running scale no longer depends on the split: this test would not catch per-push scaling'


# ------------------------------------------------------------------------------------------------ 4. homogeneity
def test_scaling_the_input_scales_the_output():
    torch = _torch()
    m = _model('crn', 2, L)
    eng = m.engine
    x = _step_signal(2, L, 830)
    res = {}
    for g in (1.0, 0.25):
        eng.stream_begin(2, max_chunk_frames=4, tracking_rms=0.5)
        sc = []
        res[g] = (_feed(eng, torch.from_numpy(x * np.float32(g)).cuda(), _cuts(L, [480]), scales=sc), np.stack(sc))
    _close(res[0.25][0], 0.25 * res[1.0][0], 'input x 0.25')
    assert (res[0.25][1] == 4.0 * res[1.0][1]).all(), 'stream_scale() is not exactly 4 x'


# ------------------------------------------------------------------------------------------------ 5. forgetting
@pytest.mark.parametrize('tau', [0.25, 0.0])
def test_scale_follows_a_level_step(tau):
    """White noise at level a for 2 s, then a / 8.  With tau = 0.25 s the old level still weighs 63 e^-8 = 2.1 % in E after 2 s, i.e. - 1.05 %
    in c, and the estimate of white noise over an effective 0.5 s scatters by about 1 % more: whether the float64 reference itself ends
    within 1 % of 8 x its value at 2 s depends on the noise.  The seed is one for which it does, with margin (0.2 %; found on the CPU
    from the reference alone), and the test asserts that first; what the engine is held to is the reference, to 1e-6 after every push."""
    torch = _torch()
    n_fft, hop = GEOM['crn']
    n = 64000
    rng = np.random.default_rng(28)
    x = (rng.standard_normal((2, n)) * np.array([[0.2], [0.03]])).astype(np.float32)
    x[:, n // 2:] /= 8.0
    lam = TR.lam_of(tau * 16000.0, hop)
    cuts = _cuts(n, [160])                    # 10 ms pushes: the read-out after every one of them
    # (the scale of a frame depends on whole blocks in front of it only, so the scales of the whole signal hold for every prefix)
    c_all = TR.frame_scales(x, n_fft, hop, lam, n, False, TR.frames_released(n, n_fft, hop))
    ref = np.stack([c_all[:, TR.frames_released(b, n_fft, hop) - 1] if TR.frames_released(b, n_fft, hop) else np.ones(2) for a, b in cuts])
    half = n // 2 // 160 - 1
    if tau > 0:
        assert np.abs(ref[-1] / (8 * ref[half]) - 1).max() < 0.01, 'the reference itself does not settle'
    else:
        assert (ref[-1] < 2 * ref[half]).all()
    m = _model('crn', 2, 16000, sliding_stream=True)
    eng = m.engine
    eng.stream_begin(2, max_chunk_frames=8, tracking_rms=tau)
    sc = []
    _feed(eng, torch.from_numpy(x).cuda(), cuts, scales=sc)
    sc = np.stack(sc)
    np.testing.assert_allclose(sc, ref, rtol=1e-6)
    if tau > 0:
        assert np.abs(sc[-1] / (8 * sc[half]) - 1).max() < 0.01
    else:
        assert (sc[-1] < 2 * sc[half]).all()


# ------------------------------------------------------------------------------------------------ 6. parking
@functools.lru_cache(maxsize=None)
def _uninterrupted(name, tau):
    """(signal, output of the uninterrupted tracking stream, scales after every push): computed once, never written to"""
    torch = _torch()
    m = _model(name, 2, L)
    x = _step_signal(2, L, 840)
    eng = m.engine
    eng.stream_begin(2, max_chunk_frames=4, tracking_rms=tau)
    sc = []
    out = _feed(eng, torch.from_numpy(x).cuda(), _cuts(L, [400]), scales=sc)
    for a in (x, out):
        a.setflags(write=False)
    return x, out, sc


@pytest.mark.parametrize('name', ['crn', 'dccrn'])
@pytest.mark.parametrize('via_bytes', [False, True])
def test_save_restore_continues_bit_for_bit(name, via_bytes):
    torch = _torch()
    x, ref, _ = _uninterrupted(name, 0.5)
    m = _model(name, 2, L)
    eng = m.engine
    xt = torch.from_numpy(x).cuda()
    cuts = _cuts(L, [400])
    k = len(cuts) // 2 + 1
    eng.stream_begin(2, max_chunk_frames=4, tracking_rms=0.5)
    head = _feed(eng, xt, cuts[:k], flush=False)
    snap = eng.stream_save()
    if via_bytes:
        img = snap.to_bytes()
        snap.close()
        snap = StreamSnapshot.from_bytes(img)
        assert snap.counts()[:2] == (2, cuts[k - 1][1])
    m.enhance_batch(xt)                                           # other work on the engine
    eng.stream_begin(1, max_chunk_frames=8, running_rms=True)     # ... another stream, of another mode
    eng.stream_push(xt[:1, :3000].contiguous())
    eng.stream_restore(snap)
    tail = _feed(eng, xt, cuts[k:])
    snap.close()
    got = np.concatenate([head, tail], axis=1)
    assert got.shape == ref.shape and got.tobytes() == ref.tobytes(), rms(got - ref)


def test_select_and_concat_continue_and_differing_tau_is_named():
    torch = _torch()
    x, ref, _ = _uninterrupted('crn', 0.5)
    m = _model('crn', 2, L)
    eng = m.engine
    xt = torch.from_numpy(x).cuda()
    cuts = _cuts(L, [400])
    k = len(cuts) // 2
    eng.stream_begin(2, max_chunk_frames=4, tracking_rms=0.5)
    head = _feed(eng, xt, cuts[:k], flush=False)
    snap = eng.stream_save()
    one = snap.select(eng, [1])
    eng.stream_restore(one)
    got = np.concatenate([head[1:], _feed(eng, xt[1:], cuts[k:])], axis=1)
    _close(got, ref[1:], 'select row 1')
    r1, r0 = snap.select(eng, [1]), snap.select(eng, [0])
    both = StreamSnapshot.concat(eng, [r1, r0])
    eng.stream_restore(both)
    got = np.concatenate([head[::-1], _feed(eng, xt.flip(0), cuts[k:])], axis=1)
    _close(got, ref[::-1], 'concat rows 1, 0')
    eng.stream_begin(1, max_chunk_frames=4, tracking_rms=0.25)
    _feed(eng, xt[:1], cuts[:k], flush=False)
    other = eng.stream_save()
    with pytest.raises(EngineError, match='tau_samples'):
        StreamSnapshot.concat(eng, [r0, other])
    for s in (snap, one, r1, r0, both, other):
        s.close()


# ------------------------------------------------------------------------------------------------ 7. join
@pytest.mark.parametrize('name', ['crn', 'dccrn'])
def test_join_of_streams_that_began_at_different_times(name):
    """Group A (two rows) has streamed 3 s, caller B 0.5 s, both on the tracking scale with tau 0.5 s; B is brought in phase, the two are
    joined, and every row continues to its end as it does alone."""
    torch = _torch()
    n_fft, hop = GEOM[name]
    REST, NA, NB = 4000, 48000, 8000
    m = _model(name, 3, 16000, sliding_stream=True)
    eng = m.engine
    xa = _step_signal(2, NA + REST, 850)
    eng.stream_begin(2, max_chunk_frames=8, tracking_rms=0.5)
    xat = torch.from_numpy(xa).cuda()
    _feed(eng, xat, _cuts(NA, [1600]), flush=False)
    snap_a = eng.stream_save()
    eng.stream_begin(1, max_chunk_frames=8, tracking_rms=0.5)
    xb_full = _step_signal(1, NB + hop + REST, 860)
    xbt = torch.from_numpy(xb_full).cuda()
    _feed(eng, xbt, _cuts(NB, [1600]), flush=False)
    d = samples_until_joinable(eng.stream_save(), snap_a)
    assert 0 <= d < hop * 4
    if d:
        eng.stream_push(xbt[:, NB:NB + d].contiguous())
    nb = NB + d
    snap_b = eng.stream_save()
    xbt = xbt[:, :nb + REST]
    # alone
    solo = {}
    for key, snap, xt, n0 in (('a', snap_a, xat, NA), ('b', snap_b, xbt, nb)):
        eng.stream_restore(snap)
        sc = []
        solo[key] = (_feed(eng, xt, _cuts(n0 + REST, [160, 1000, 37], start=n0), scales=sc), np.stack(sc))
    # joined
    joined = StreamSnapshot.join(eng, [snap_a, snap_b])
    eng.stream_restore(joined)
    sc = []
    rest = torch.cat([xat[:, NA:], xbt[:, nb:]], 0).contiguous()
    got = _feed(eng, rest, _cuts(REST, [160, 1000, 37]), scales=sc)
    sc = np.stack(sc)
    _close(got[:2], solo['a'][0], name + ' joined rows of A')
    _close(got[2:], solo['b'][0], name + ' joined row B')
    assert sc[:, :2].tobytes() == solo['a'][1].tobytes() and sc[:, 2:].tobytes() == solo['b'][1].tobytes(), 'scales differ from the solo runs'
    # a tracking part with a fixed-scale part; a part short of the left edge
    eng.stream_begin(1, max_chunk_frames=8)
    _feed(eng, xbt, _cuts(nb, [1600]), flush=False)
    fixed = eng.stream_save()
    with pytest.raises(EngineError, match='running 2 vs 0'):
        StreamSnapshot.join(eng, [snap_a, fixed])
    # (CRN can be rebased from its first frame on, and a stream without a frame cannot be in phase with one that has some - its
    # n_total - o_done is clamped - so for 320 / 160 the left-edge refusal is reachable only in the host check program)
    if name == 'dccrn':      # in phase with A after eight frames; its look-ahead decoder can be rebased from nine on (csrc/stream_join.h)
        eng.stream_begin(1, max_chunk_frames=8, tracking_rms=0.5)
        short = 7 * hop + n_fft // 2 + 1 + (NA - n_fft // 2 - 1) % hop
        eng.stream_push(xbt[:, :short].contiguous())
        with eng.stream_save() as early:
            assert early.counts()[2] == 8
            with pytest.raises(EngineError, match='short of the left edge'):
                StreamSnapshot.join(eng, [snap_a, early])
    for s in (snap_a, snap_b, joined, fixed):
        s.close()


# ------------------------------------------------------------------------------------------------ 8. refusals that need an engine
def test_refused_arguments_and_the_scale_of_the_other_modes():
    torch = _torch()
    m = _model('crn', 2, L)
    eng = m.engine
    for bad in (-1.0, float('nan'), float('inf')):
        with pytest.raises(EngineError, match='tau_samples'):
            eng.stream_begin(2, tracking_rms=bad)
    c = torch.ones(2, device='cuda')
    with pytest.raises(EngineError, match='tracking_rms and a caller-provided scale'):
        eng.stream_begin(2, c=c, tracking_rms=0.5)
    with pytest.raises(EngineError, match='tracking_rms and running_rms'):
        eng.stream_begin(2, running_rms=True, tracking_rms=0.5)
    # (the refused begins above left whatever stream an earlier test had on the engine: the wrapper's refusal or the engine's)
    with pytest.raises(EngineError, match='stream_scale without (se_)?stream_begin'):
        eng.stream_scale()
    eng.stream_begin(2, tracking_rms=0.5)
    eng.stream_push(torch.zeros(2, 400, device='cuda'))
    eng.stream_flush()
    with pytest.raises(EngineError, match='se_stream_scale without se_stream_begin'):      # the engine's own, once its stream has ended
        eng.stream_scale()
    from test_gpu_ragged import _make as _make_any
    u = _make_any('ctsnet', 1, 8000)          # InstanceNorm weights: statistics over the whole utterance
    with pytest.raises(EngineError, match='no frame-online mode'):
        u.engine.stream_begin(1, tracking_rms=0.5)
    u.engine.close()
    # the read-out in the other modes: the caller's c; 1 before any frame
    cc = torch.tensor([0.5, 3.0], device='cuda')
    eng.stream_begin(2, c=cc)
    assert (eng.stream_scale().cpu().numpy() == np.array([0.5, 3.0], np.float32)).all()
    eng.stream_begin(2, tracking_rms=0.0)
    assert (eng.stream_scale().cpu().numpy() == 1.0).all()
    eng.stream_push(torch.zeros(2, 100, device='cuda'))
    assert (eng.stream_scale().cpu().numpy() == 1.0).all()


def _tracking_image(hop, ring=64, tau=8000.0):
    """a well-formed image (csrc/stream_manifest.h) of a one-row CRN stream on the tracking scale before its first sample"""
    import struct
    tau_bits = struct.unpack('<i', struct.pack('<f', tau))[0]
    segs = [(1, 0, 4), (2, 0, 16), (3, 0, ring * 4), (3, 1, ring * 4), (8, 0, 0)]
    pay = sum((b + 15) // 16 * 16 for _, _, b in segs)
    img = struct.pack('<II18iffiiq', 0x54534553, 1, 2, 0, 320, hop, 320, 1, 4, 0, 0, 0, 0, 2, ring, 1, 0, tau_bits, 0, 0, 1.0, 1.0, len(segs), 0, pay)
    return img + b''.join(struct.pack('<iiq', *sg) for sg in segs) + bytes(pay)


def test_front_end_that_drops_the_head_of_a_block_is_refused():
    """n_fft 320 with hop 162: 320 < 2 * 162 - 2, the stream window may drop samples of the incomplete hop block.  se_stream_begin_tracking
    and the restore of a tracking-scale image refuse it, each by name; the same engine begins a fixed-scale stream."""
    from se_amd.engine import Engine
    from se_amd.models import MODEL_CLASSES
    eng = Engine('crn', 0, 1, 8000, 1.0, 1.0, n_fft=320, hop=162, win=320)
    eng.load_state_dict(synth.synth_state_dict(MODEL_CLASSES['crn'].state_dict_schema(), 12))
    try:
        with pytest.raises(EngineError, match=r'se_stream_begin_tracking: n_fft 320 < 2 hop - 2 \(hop 162\)'):
            eng.stream_begin(1, max_chunk_frames=4, tracking_rms=0.5)
        with StreamSnapshot.from_bytes(_tracking_image(162)) as snap:
            with pytest.raises(EngineError, match=r'se_stream_restore: n_fft < 2 hop - 2'):
                eng.stream_restore(snap)
        eng.stream_begin(1, max_chunk_frames=4)
    finally:
        eng.close()
    # with the project's hop the same image passes that check; a ring shorter than the engine needs is refused under the mode's own name
    m = _model('crn', 2, L)
    with StreamSnapshot.from_bytes(_tracking_image(160, ring=16)) as snap:
        with pytest.raises(EngineError, match='the snapshot of a tracking-scale stream keeps 1 / c of 16 frames'):
            m.engine.stream_restore(snap)


# ------------------------------------------------------------------------------------------------ 7b. the source-rate pair
@pytest.mark.parametrize('name', ['crn', 'dccrn'])
def test_source_rate_pair_joins_on_the_tracking_scale(name):
    """Two groups fed at 48 kHz through SourceRateStream, both begun with tracking_rms: the late caller is brought in phase with
    source_samples_until_joinable, the pair is joined by SourceStreamSnapshot.join, and every row continues to the flush as it does
    alone - the output within the bound (another batch size), stream_scale() after every push bit for bit."""
    torch = _torch()
    from se_amd.source_stream import SourceRateStream, SourceStreamSnapshot, source_samples_until_joinable
    SR, NG, NA0, REST = 48000, 60007, 15000, 24000
    eng = _model(name, 3, 16000, sliding_stream=True).engine
    xg = np.stack([synth.synth_clip(870 + b, 'speech', NG + REST, fs=SR) for b in range(2)]).astype(np.float32)
    xa = synth.synth_clip(873, 'speech', NA0 + 1000 + REST, fs=SR)[None].astype(np.float32)
    xg[:, NG // 2:] *= 4.0
    tg, ta = torch.from_numpy(xg).cuda(), torch.from_numpy(xa).cuda()

    def push(src, xt, cuts, scales=None):
        outs = []
        for a, b in cuts:
            outs.append(src.push(xt[:, a:b].contiguous()).cpu().numpy())
            if scales is not None:
                scales.append(eng.stream_scale().cpu().numpy())
        return outs

    with SourceRateStream(eng, SR, max_push=4800) as src:
        src.begin(2, tracking_rms=0.5, max_chunk_frames=8)
        push(src, tg, _cuts(NG, [4800, 37, 1000]))
        snap_g = src.save()
        src.begin(1, tracking_rms=0.5, max_chunk_frames=8)
        push(src, ta, _cuts(NA0, [4800]))
        with src.save() as s0:
            d = source_samples_until_joinable(s0, snap_g)
        assert d is not None and 0 <= d < 1000
        push(src, ta, [(NA0, NA0 + d)] if d else [])
        na = NA0 + d
        snap_a = src.save()
        assert source_samples_until_joinable(snap_a, snap_g) == 0
        ta = ta[:, :na + REST]
        solo = {}
        for key, snap, xt, n0 in (('g', snap_g, tg, NG), ('a', snap_a, ta, na)):
            src.restore(snap)
            sc = []
            outs = push(src, xt, _cuts(n0 + REST, [480, 3000, 111], start=n0), scales=sc) + [src.flush().cpu().numpy()]
            solo[key] = (np.concatenate(outs, axis=1), np.stack(sc))
        with SourceStreamSnapshot.join(eng, [snap_g, snap_a]) as j:
            src.restore(j)
            sc = []
            rest = torch.cat([tg[:, NG:], ta[:, na:]], 0).contiguous()
            outs = push(src, rest, _cuts(REST, [480, 3000, 111]), scales=sc) + [src.flush().cpu().numpy()]
        got, sc = np.concatenate(outs, axis=1), np.stack(sc)
        snap_g.close()
        snap_a.close()
    _close(got[:2], solo['g'][0], name + ' source-rate pair, rows of the group')
    _close(got[2:], solo['a'][0], name + ' source-rate pair, the late caller')
    assert sc[:, :2].tobytes() == solo['g'][1].tobytes() and sc[:, 2:].tobytes() == solo['a'][1].tobytes(), 'scales differ from the solo runs'
    assert len(np.unique(sc[:, 0])) > 5, 'the read-out does not move'
