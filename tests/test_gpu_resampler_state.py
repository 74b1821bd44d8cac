"""GPU: parking and resuming source-rate signals (se_resampler_save / se_resampler_restore, StreamResampler.save / restore,
SourceRateStream.save / restore).  The contract is bit identity: a signal saved at any point between two calls, with anything
else run on the object in between, continues after the restore with the outputs of the uninterrupted signal, push by push, the
counts included - so every comparison here is np.array_equal, never a tolerance.  The uninterrupted runs are computed once per
rate and never written to; `resample()` of the whole signal is what they in turn have to equal."""
import numpy as np
import pytest

import se_amd  # noqa: F401
from se_amd import synth
from se_amd.engine import EngineError

pytestmark = pytest.mark.gpu

B, N = 2, 5003                         # rows, samples at sr_in: 13 histories of 48 -> 16 kHz, no multiple of any push
PIECES = [1, 7, 193, 480, 1000]        # then 1000s: pushes that release nothing, pushes shorter and longer than a history
RATES = [(48000, 16000), (32000, 16000), (44100, 16000), (16000, 48000), (16000, 16000)]
CUTS = ['start', 'unreleased', 'odd', 'even', 'end']
CASES = [(i, o, c) for i, o in RATES for c in CUTS if not (i == o and c == 'unreleased')]      # pass-through releases every sample at once

_cache = {}


def _sizes(n=N):
    out, pos = [], 0
    while pos < n:
        out.append(min(PIECES[min(len(out), len(PIECES) - 1)], n - pos))
        pos += out[-1]
    return out


def _signal(seed=700, n=N, rows=B):
    import torch
    key = ('x', seed, n, rows)
    if key not in _cache:
        x = np.stack([synth.synth_clip(seed + b, 'speech' if b % 2 == 0 else 'white', n, fs=48000) for b in range(rows)])
        _cache[key] = torch.from_numpy(x).cuda()
    return _cache[key]


def _push_from(rs, xt, sizes, first):
    """pushes first .. of `sizes` -> their outputs as host arrays"""
    pos = sum(sizes[:first])
    outs = []
    for m in sizes[first:]:
        outs.append(rs.push(xt[:, pos:pos + m]).cpu().numpy())
        pos += m
    return outs


def _rest(rs, xt, sizes, first):
    """the pushes from `first` on and the flush"""
    return _push_from(rs, xt, sizes, first) + [rs.flush().cpu().numpy()]


def _alone(sr_in, sr_out, seed=700, n=N):
    """the uninterrupted signal: every push's output and the flush's, checked once against resample() of the whole"""
    from se_amd import resample as HR
    key = ('alone', sr_in, sr_out, seed, n)
    if key not in _cache:
        xt = _signal(seed, n)
        with HR.StreamResampler(sr_in, sr_out, max_batch=B, max_push=1000) as rs:
            rs.begin(B)
            outs = _rest(rs, xt, _sizes(n), 0)
        want = HR.resample(xt, sr_in, sr_out).cpu().numpy()
        assert np.array_equal(np.concatenate(outs, axis=1), want)
        for o in outs:
            o.setflags(write=False)
        _cache[key] = outs
    return _cache[key]


def _cut(sr_in, sr_out, name):
    """pushes made before the save, chosen from se_resampler_ready_samples"""
    from se_amd import resample as HR
    sizes = _sizes()
    ready = [HR.ready_samples(sum(sizes[:k]), sr_in, sr_out) for k in range(len(sizes) + 1)]
    if name == 'start':
        return 0
    if name == 'end':
        return len(sizes)
    if name == 'unreleased':        # the most pushes that together are shorter than the reach: nothing has been released
        k = max(k for k in range(1, len(sizes)) if ready[k] == 0)
        assert k >= 1 and ready[k + 1] > 0
        return k
    odd = min(k for k in range(1, len(sizes), 2) if ready[k] > 0)
    if name == 'odd':
        return odd
    even = min(k for k in range(2, len(sizes), 2) if k > odd)
    assert 0 < ready[odd] < ready[even] and even < len(sizes)
    return even


def _same(got, want, what=''):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape, (what, k, g.shape, w.shape)          # *n_out of push k
        assert np.array_equal(g, w), (what, k, float(np.abs(g - w).max()))


def _disturb(rs):
    """another whole signal on the object: other rows, NaN samples, pushes that rewrite both history buffers"""
    import torch
    junk = torch.full((3, 1000), float('nan'), dtype=torch.float32, device='cuda')
    rs.begin(3)
    for n in (1000, 999, 1000, 5):
        rs.push(junk[:, :n])
    rs.flush()


@pytest.mark.parametrize('sr_in,sr_out,cut', CASES)
def test_save_another_signal_restore(sr_in, sr_out, cut):
    from se_amd import resample as HR
    xt, sizes, want = _signal(), _sizes(), _alone(sr_in, sr_out)
    k = _cut(sr_in, sr_out, cut)
    with HR.StreamResampler(sr_in, sr_out, max_batch=3, max_push=1000) as rs:
        rs.begin(B)
        outs = _push_from(rs, xt, sizes[:k], 0)
        with rs.save() as snap:
            assert snap.counts() == (sr_in, sr_out, B, sum(sizes[:k]), sum(o.shape[1] for o in outs))
            assert (snap.nbytes == 0) == (sr_in == sr_out)
            _disturb(rs)
            rs.restore(snap)
            outs += _rest(rs, xt, sizes, k)
    _same(outs, want, cut)                    # so the concatenation is resample() of the whole signal (_alone)
    assert not np.isnan(np.concatenate(outs, axis=1)).any()


@pytest.mark.parametrize('sr_in,sr_out,cut', CASES)
def test_restore_on_another_object_that_has_never_run(sr_in, sr_out, cut):
    from se_amd import resample as HR
    xt, sizes, want = _signal(), _sizes(), _alone(sr_in, sr_out)
    k = _cut(sr_in, sr_out, cut)
    with HR.StreamResampler(sr_in, sr_out, max_batch=B, max_push=1000) as rs, \
            HR.StreamResampler(sr_in, sr_out, max_batch=5, max_push=1111) as other:
        rs.begin(B)
        outs = _push_from(rs, xt, sizes[:k], 0)
        with rs.save() as snap:
            rs.begin(1)                       # the source object moves on to something else
            other.restore(snap)
            outs += _rest(other, xt, sizes, k)
    _same(outs, want, cut)


@pytest.mark.parametrize('sr_in,sr_out', RATES)
def test_a_save_disturbs_nothing_and_one_snapshot_forks(sr_in, sr_out):
    from se_amd import resample as HR
    xt, sizes, want = _signal(), _sizes(), _alone(sr_in, sr_out)
    k = _cut(sr_in, sr_out, 'odd')
    with HR.StreamResampler(sr_in, sr_out, max_batch=B, max_push=1000) as rs:
        rs.begin(B)
        outs = _push_from(rs, xt, sizes[:k], 0)
        with rs.save() as snap:
            _same(outs + _rest(rs, xt, sizes, k), want, 'the signal that goes on')
            for fork in range(2):
                rs.restore(snap)
                _same(_rest(rs, xt, sizes, k), want[k:], f'fork {fork}')


@pytest.mark.parametrize('sr_in,sr_out,cut', CASES)
def test_byte_round_trip(sr_in, sr_out, cut):
    from se_amd import resample as HR
    xt, sizes, want = _signal(), _sizes(), _alone(sr_in, sr_out)
    k = _cut(sr_in, sr_out, cut)
    with HR.StreamResampler(sr_in, sr_out, max_batch=B, max_push=1000) as rs:
        rs.begin(B)
        _push_from(rs, xt, sizes[:k], 0)
        with rs.save() as snap:
            img = snap.to_bytes()
            counts = snap.counts()
    with HR.ResamplerSnapshot.from_bytes(img) as snap, HR.StreamResampler(sr_in, sr_out, max_batch=B, max_push=1000) as fresh:
        reach2 = 0 if sr_in == sr_out else 2 * (32769 // int(512 * min(1.0, sr_out / sr_in)) + 1)
        assert snap.counts() == counts and snap.nbytes == len(img) - 64 == B * min(sum(sizes[:k]), reach2) * 4
        fresh.restore(snap)
        assert snap.to_bytes() == img         # the upload changed nothing
        _same(_rest(fresh, xt, sizes, k), want[k:], cut)


def test_two_signals_take_turns_on_one_object():
    """restore -> push -> save per push, two signals of different lengths on one 44100 -> 16000 object: each equals its own run
    alone, and a snapshot's device memory does not move from save to save"""
    from se_amd import resample as HR
    sigs = [(_signal(700, N), _sizes(N), _alone(44100, 16000, 700, N)), (_signal(720, 3001), _sizes(3001), _alone(44100, 16000, 720, 3001))]
    with HR.StreamResampler(44100, 16000, max_batch=B, max_push=1000) as rs:
        snaps, outs, sizes_seen = [], [[], []], [set(), set()]
        for g in range(2):
            rs.begin(B)
            snaps.append(rs.save())
            sizes_seen[g].add(snaps[g].nbytes)
        for k in range(max(len(s[1]) for s in sigs)):
            for g, (xt, sizes, _) in enumerate(sigs):
                if k >= len(sizes):
                    continue
                rs.restore(snaps[g])
                outs[g] += _push_from(rs, xt, sizes[:k + 1], k)
                assert rs.save(snaps[g]) is snaps[g]
                sizes_seen[g].add(snaps[g].nbytes)
        for g in range(2):
            rs.restore(snaps[g])
            outs[g].append(rs.flush().cpu().numpy())
            _same(outs[g], sigs[g][2], f'signal {g}')
            assert sizes_seen[g] == {B * 2 * 178 * 4}, sizes_seen[g]          # batch x 2 * reach floats (a multiple of 4: the pitch)
            snaps[g].close()


def test_refusals_carry_their_reason_and_leave_the_signal_as_it_was():
    from se_amd import resample as HR
    xt, sizes, want = _signal(), _sizes(), _alone(48000, 16000)
    x3 = _signal(700, N, rows=3)
    with HR.StreamResampler(48000, 16000, max_batch=B, max_push=1000) as rs, \
            HR.StreamResampler(44100, 16000, max_batch=B, max_push=1000) as r44, \
            HR.StreamResampler(48000, 16000, max_batch=3, max_push=1000) as r3, HR.ResamplerSnapshot() as empty:
        with pytest.raises(EngineError, match='se_resampler_save without se_resampler_begin'):
            rs.save()
        with pytest.raises(EngineError, match='se_resampler_save without se_resampler_begin'):
            rs.save(empty)
        assert empty.nbytes == 0
        r44.begin(B)
        r44.push(xt[:, :900])
        r3.begin(3)
        r3.push(x3[:, :900])
        closed = r3.save()
        closed.close()
        rs.begin(B)
        outs = _push_from(rs, xt, sizes[:4], 0)
        with r44.save() as other_rate, r3.save() as three_rows, rs.save() as mine:
            img = mine.to_bytes()
            with pytest.raises(EngineError, match='se_resampler_restore: the resampler state object is empty'):
                rs.restore(empty)
            with pytest.raises(EngineError, match='taken at 44100 -> 16000 Hz, this object converts 48000 -> 16000 Hz'):
                rs.restore(other_rate)
            with pytest.raises(EngineError, match='snapshot of 3 rows exceeds max_batch 2'):
                rs.restore(three_rows)
            with pytest.raises(EngineError, match='restore: the snapshot is closed'):
                rs.restore(closed)
            with pytest.raises(EngineError, match='save: the snapshot is closed'):
                rs.save(closed)
            with pytest.raises(EngineError, match='max_batch'):
                rs.check_restore(three_rows)
            # neither the signal ...
            outs += _rest(rs, xt, sizes, 4)
            _same(outs, want)
            # ... nor an object: a save refused after the flush leaves the snapshot it was given as it was
            with pytest.raises(EngineError, match='se_resampler_save after se_resampler_flush'):
                rs.save(mine)
            assert mine.to_bytes() == img
            rs.restore(mine)
            _same(_rest(rs, xt, sizes, 4), want[4:], 'after the refusals')


# ---- SourceRateStream on CRN: the engine's stream and the resampler's signal parked and resumed together

L48, PUSH = 24000, 480                 # 0.5 s at 48 kHz, 10 ms pushes: one STFT frame each


def _crn():
    if 'crn' not in _cache:
        from se_amd.models import MODEL_CLASSES
        _cache['crn'] = MODEL_CLASSES['crn'](max_batch=B, max_samples=16000).load_synthetic(12)
    return _cache['crn']


def _begin(src, eng, xt, running):
    from se_amd import resample as HR
    if running:
        src.begin(B, max_chunk_frames=4, running_rms=True)
    else:
        src.begin(B, c=eng.rms_scale(HR.resample(xt, 48000, 16000)), max_chunk_frames=4)


@pytest.mark.parametrize('running', [False, True], ids=['given_c', 'running_rms'])
def test_source_rate_groups_take_turns_on_crn(running):
    import torch
    from se_amd import resample as HR
    from se_amd.source_stream import SourceRateStream, SourceStreamSnapshot
    eng = _crn().engine
    xs = [torch.from_numpy(np.stack([synth.synth_clip(seed + b, 'speech' if b % 2 == 0 else 'white', L48, fs=48000)
                                     for b in range(B)])).cuda() for seed in (760, 780)]
    starts = list(range(0, L48, PUSH))
    alone = []
    for xt in xs:                             # each group pushed alone through an uninterrupted SourceRateStream
        with SourceRateStream(eng, 48000, max_push=PUSH) as src:
            _begin(src, eng, xt, running)
            alone.append([src.push(xt[:, p:p + PUSH]).cpu().numpy() for p in starts] + [src.flush().cpu().numpy()])
    assert alone[0][0].shape == (B, 0) and sum(o.shape[1] for o in alone[0]) > 7000
    assert not np.array_equal(np.concatenate(alone[0], axis=1), np.concatenate(alone[1], axis=1))
    with SourceRateStream(eng, 48000, max_push=PUSH) as src, HR.StreamResampler(44100, 16000, max_batch=B, max_push=PUSH) as r44:
        snaps, outs = [], [[], []]
        for xt in xs:
            _begin(src, eng, xt, running)
            snaps.append(src.save())
        for i, p in enumerate(starts):
            for g, xt in enumerate(xs):
                src.restore(snaps[g])
                outs[g].append(src.push(xt[:, p:p + PUSH]).cpu().numpy())
                assert src.save(snaps[g]) is snaps[g]
            if i == len(starts) // 2:         # group 0 goes through host memory once, mid-stream
                img = snaps[0].to_bytes()
                snaps[0].close()
                snaps[0] = SourceStreamSnapshot.from_bytes(img)
                assert snaps[0].to_bytes() == img and snaps[0].engine.batch == B
        src.restore(snaps[0])
        outs[0].append(src.flush().cpu().numpy())
        src.restore(snaps[1])
        # a refused restore - the resampler half of another rate beside a valid engine half (group 0's, mid-stream) - leaves the
        # engine's stream and the resampler as they were: group 1 flushes as if nothing had been tried
        r44.begin(B)
        r44.push(xs[0][:, :PUSH])
        bad = SourceStreamSnapshot(engine=snaps[0].engine, resampler=r44.save())
        with pytest.raises(EngineError, match='taken at 44100 -> 16000 Hz'):
            src.restore(bad)
        outs[1].append(src.flush().cpu().numpy())
        bad.close()
        for sn in snaps:
            sn.close()
    for g in range(2):
        _same(outs[g], alone[g], f'group {g}')
