"""GPU: parked source-rate streams that began at different times joined into one group (se_resampler_state_join,
ResamplerSnapshot.join, SourceStreamSnapshot.join).

The resampler's half is held to its own contract: head + tail of every row equals `resample()` of its whole signal under
np.array_equal, and every call releases what the uninterrupted stream releases - no tolerance.  The pair (a SourceRateStream at 48 kHz
in front of CRN, 320 / 160, and of the DCCRN that looks six frames ahead, 512 / 128) is held to the bar of
tests/test_gpu_sliding_stream.py (`_make`, `_close`: identical shape and rms(got - ref) < 1e-6 + 2e-5 rms(ref)) against the offline
decode of the resampled whole signal, and a rebased row that continues alone at batch 1 to bit identity with itself never interrupted.
Engines are sliding, for 3 rows and max_samples = 16000, as in tests/test_gpu_stream_join.py, whose piece sizes are reused."""
import functools

import numpy as np
import pytest

import se_amd  # noqa: F401
from se_amd import synth
from se_amd.engine import EngineError
from se_amd.resample import ResamplerSnapshot, StreamResampler, resample
from se_amd.source_stream import SourceRateStream, SourceStreamSnapshot, source_samples_until_joinable
from test_gpu_sliding_stream import _close, _make

pytestmark = pytest.mark.gpu

MS, B3 = 16000, 3
PIECES = (37, 1000, 3, 481, 2000, 4000)          # tests/test_gpu_stream_join.py
AHEAD = 5                                        # hops of 160 output samples the group is ahead of the late caller
SR = 48000
HOP = {'crn': 160, 'dccrn': 128}
N_G, N_A0, REST = 12007, 5000, 42000             # test 3 / 4, at 48 kHz: the group's save point, the late caller's first, samples left
SEED_A, SEED_G, SEED_H = 980, 981, 982


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _cuts(n, pieces=PIECES, start=0):
    """[start, start + n) in uneven pieces (the last size repeats)"""
    pos, k, out = 0, 0, []
    while pos < n:
        m = min(pieces[min(k, len(pieces) - 1)], n - pos)
        out.append((start + pos, start + pos + m))
        pos += m
        k += 1
    return out


def _clip(seed, L, fs):
    return synth.synth_clip(seed, 'speech' if seed % 2 == 0 else 'white', L, fs=fs)[None]


# ------------------------------------------------------------------------------------------------ 1, 2. the resampler alone
def _push_all(rs, xt, cuts):
    return [rs.push(xt[:, a:b].contiguous()).cpu().numpy() for a, b in cuts]


@pytest.mark.parametrize('via_bytes', [False, True], ids=['device', 'bytes'])
@pytest.mark.parametrize('sr_in', [48000, 32000])
def test_resampler_rows_joined_continue_bit_for_bit(sr_in, via_bytes):
    """The late caller is saved with the first n_in that is past the left edge (64 outputs released): its history still starts at
    sample 0 and is shorter than 2 * reach, so rebased it starts later than the group's own.  The first piece after the join is one
    sample: the history origin must not move back."""
    torch = _torch()
    D = sr_in // 16000
    reach = 32769 // (512 // D) + 1
    shift = AHEAD * D * 160
    nA = 63 * D + reach + 1
    nG, rest = nA + shift, 9001
    xA = _clip(SEED_A, nA + rest, sr_in)
    xG = np.concatenate([_clip(SEED_G, nG + rest, sr_in), _clip(SEED_H, nG + rest, sr_in)])
    tA, tG = torch.from_numpy(xA).cuda(), torch.from_numpy(xG).cuda()
    ref = {'A': resample(tA, sr_in).cpu().numpy(), 'G': resample(tG, sr_in).cpu().numpy()}
    tail_pieces = (1,) + PIECES
    with StreamResampler(sr_in, max_batch=B3, max_push=4000) as rs:
        # the uninterrupted streams: what every call releases
        alone = {}
        for key, xt, n in (('A', tA, nA), ('G', tG, nG)):
            rs.begin(xt.shape[0])
            outs = _push_all(rs, xt, _cuts(n) + _cuts(rest, tail_pieces, n)) + [rs.flush().cpu().numpy()]
            assert np.array_equal(np.concatenate(outs, axis=1), ref[key])
            alone[key] = [o.shape[1] for o in outs]
        assert alone['A'][len(_cuts(nA)):] == alone['G'][len(_cuts(nG)):]          # in phase: the tails release alike
        # the parked heads
        heads, snaps = {}, {}
        for key, xt, n in (('G', tG, nG), ('A', tA, nA)):
            rs.begin(xt.shape[0])
            heads[key] = np.concatenate(_push_all(rs, xt, _cuts(n)), axis=1)
            snaps[key] = rs.save()
        assert snaps['A'].counts() == (sr_in, 16000, 1, nA, 64) and snaps['G'].counts()[3:] == (nG, 64 + AHEAD * 160)
        if via_bytes:                                       # a host-side join; the upload happens at the restore
            images = {k: s.to_bytes() for k, s in snaps.items()}
            for s in snaps.values():
                s.close()
            snaps = {k: ResamplerSnapshot.from_bytes(b) for k, b in images.items()}
        with snaps['G'] as g, snaps['A'] as a:
            with pytest.raises(EngineError, match=r'se_resampler_state_concat: parts\[0\] and parts\[1\] differ: n_in %d vs %d' % (nG, nA)):
                ResamplerSnapshot.concat([g, a])
            with ResamplerSnapshot.join([g, a]) as j:
                assert j.counts() == (sr_in, 16000, 3, nG, 64 + AHEAD * 160)
                assert (j.device is None) == via_bytes
                if via_bytes:
                    assert g.to_bytes() == images['G'] and a.to_bytes() == images['A']
                rs.restore(j)
                x3 = torch.cat([tG[:, nG:], tA[:, nA:]])
                outs = _push_all(rs, x3, _cuts(rest, tail_pieces)) + [rs.flush().cpu().numpy()]
    assert [o.shape[1] for o in outs] == alone['A'][len(_cuts(nA)):], 'n_out per call'
    tail = np.concatenate(outs, axis=1)
    assert np.array_equal(np.concatenate([heads['G'], tail[:2]], axis=1), ref['G'])
    assert np.array_equal(np.concatenate([heads['A'], tail[2:]], axis=1), ref['A'])


@pytest.mark.parametrize('imported, ahead', [('A', 1), ('G', 2)], ids=['late-imported', 'group-imported'])
def test_resampler_join_of_an_imported_and_a_resident_part(imported, ahead):
    """One part is an imported image, the other lives on the device: the join uploads the image there and gathers both in one launch.
    One row each, `ahead` hops apart, parked as in the test above - the group's packed history starts before the joined origin, so its
    row is read from a nonzero column (2 * reach - nA = 3 floats at 48 kHz).  Each row continues, call by call, bit for bit as it
    does alone after its save."""
    torch = _torch()
    D = SR // 16000
    reach = 32769 // (512 // D) + 1
    nA = 63 * D + reach + 1
    n = {'A': nA, 'G': nA + ahead * D * 160}
    assert 2 * reach - nA > 0
    rest, tail_pieces = 1201, (1, 37, 481)
    x = {k: torch.from_numpy(_clip(seed, n[k] + rest, SR)).cuda() for k, seed in (('A', SEED_A), ('G', SEED_G))}
    with StreamResampler(SR, max_batch=2, max_push=4000) as rs:
        snaps, alone = {}, {}
        for key in ('G', 'A'):
            rs.begin(1)
            _push_all(rs, x[key], _cuts(n[key]))
            snaps[key] = rs.save()
            alone[key] = _push_all(rs, x[key], _cuts(rest, tail_pieces, n[key])) + [rs.flush().cpu().numpy()]
        image = snaps[imported].to_bytes()
        snaps[imported].close()
        snaps[imported] = ResamplerSnapshot.from_bytes(image)
        with snaps['G'] as g, snaps['A'] as a:
            assert (g.device is None, a.device is None) == (imported == 'G', imported == 'A')
            with ResamplerSnapshot.join([g, a]) as j:
                assert j.device is not None and j.counts() == (SR, 16000, 2, n['G'], 64 + ahead * 160)
                rs.restore(j)
                x2 = torch.cat([x['G'][:, n['G']:], x['A'][:, n['A']:]])
                outs = _push_all(rs, x2, _cuts(rest, tail_pieces)) + [rs.flush().cpu().numpy()]
    for i, key in enumerate(('G', 'A')):
        assert [o.shape[1] for o in outs] == [o.shape[1] for o in alone[key]], 'n_out per call'
        assert all(np.array_equal(o[i:i + 1], r) for o, r in zip(outs, alone[key])), key


# ------------------------------------------------------------------------------------------------ 3, 4. the pair
_ENGINES, _OFFLINE = {}, {}


def _engine(name):
    if name not in _ENGINES:
        _ENGINES[name] = _make(name, B3, MS, sliding_stream=True).engine
    return _ENGINES[name]


@pytest.fixture(scope='module', autouse=True)
def _release():
    yield
    for eng in _ENGINES.values():
        eng.close()
    for m in _OFFLINE.values():
        m.engine.close()
    _ENGINES.clear()
    _OFFLINE.clear()
    _pair.cache_clear()


def _n_a(name):
    """the late caller's save point: N_A0, then the samples that put it in phase with the group (D * lcm(hop, 4) at 48 kHz)"""
    unit = 3 * HOP[name]
    return N_A0 + (N_G - N_A0) % unit


def _offline(name, x48):
    """(offline decode, unit-RMS scale) of the resampled whole signal, one row"""
    torch = _torch()
    if name not in _OFFLINE:
        _OFFLINE[name] = _make(name, 1, 24000)
    m = _OFFLINE[name]
    y = resample(torch.from_numpy(x48).cuda(), SR)
    return m.enhance_batch(y).cpu().numpy(), m.engine.rms_scale(y).cpu().numpy()


def _src_push(src, xt, cuts):
    return [src.push(xt[:, a:b].contiguous()).cpu().numpy() for a, b in cuts]


@functools.lru_cache(maxsize=None)
def _pair(name):
    """The callers of tests 3 and 4 on the module's engine, each behind one SourceRateStream: the group G (two rows) parked N_G source
    samples in; the late caller A parked at N_A0 and again once it is in phase; A's stream then runs on to its end at batch 1: the
    uninterrupted reference.  Computed once, never written to."""
    torch = _torch()
    eng = _engine(name)
    nA = _n_a(name)
    d = {'nA': nA}
    d['xA'] = _clip(SEED_A, nA + REST, SR)
    d['xG'] = np.concatenate([_clip(SEED_G, N_G + REST, SR), _clip(SEED_H, N_G + REST, SR)])
    offA = _offline(name, d['xA'])
    offG = [_offline(name, d['xG'][r:r + 1]) for r in range(2)]
    d['refA'], d['refG'] = offA[0], np.concatenate([o[0] for o in offG])
    cA, cG = torch.from_numpy(offA[1]).cuda(), torch.from_numpy(np.concatenate([o[1] for o in offG])).cuda()
    d['cA'] = offA[1]
    tA, tG = torch.from_numpy(d['xA']).cuda(), torch.from_numpy(d['xG']).cuda()
    with SourceRateStream(eng, SR, max_push=4800) as src:
        src.begin(2, c=cG)
        d['headG'] = np.concatenate(_src_push(src, tG, _cuts(N_G)), axis=1)
        with src.save() as snap:
            d['imgG'], d['cntG'] = snap.to_bytes(), snap.counts()
        src.begin(1, c=cA)
        head = _src_push(src, tA, _cuts(N_A0))
        with src.save() as snap:
            d['cntA0'] = snap.counts()
        head += _src_push(src, tA, [(N_A0, nA)] if nA > N_A0 else [])
        d['headA'] = np.concatenate(head, axis=1)
        with src.save() as snap:
            d['imgA'], d['cntA'] = snap.to_bytes(), snap.counts()
        d['restA'] = _src_push(src, tA, _cuts(REST, start=nA)) + [src.flush().cpu().numpy()]
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _check_row(name, what, got, ref):
    ok, info = _close(got, ref)
    print(name, what, '(shape, shape, rms err, rms ref)', info)
    assert ok and np.isfinite(got).all(), (name, what, info)


@pytest.mark.parametrize('name', ['crn', 'dccrn'])
def test_late_source_rate_caller_joins_a_running_group(name):
    torch = _torch()
    d = _pair(name)
    eng = _engine(name)
    nA, unit = d['nA'], 3 * HOP[name]
    assert source_samples_until_joinable(d['cntA0'], d['cntG']) == nA - N_A0 and 0 < nA - N_A0 < unit
    assert source_samples_until_joinable(d['cntA'], d['cntG']) == 0 and (N_G - nA) % unit == 0 and N_G > nA
    tA, tG = torch.from_numpy(d['xA']).cuda(), torch.from_numpy(d['xG']).cuda()
    with SourceRateStream(eng, SR, max_push=4800) as src, SourceStreamSnapshot.from_bytes(d['imgG']) as g, \
            SourceStreamSnapshot.from_bytes(d['imgA']) as a:
        with pytest.raises(EngineError, match=r'se_resampler_state_concat: parts\[0\] and parts\[1\] differ: n_in %d vs %d' % (N_G, nA)):
            SourceStreamSnapshot.concat(eng, [g, a])
        with SourceStreamSnapshot.join(eng, [g, a]) as j:
            assert j.counts() == ((3,) + d['cntG'][0][1:], d['cntG'][1][:2] + (3,) + d['cntG'][1][3:])
            src.restore(j)
            x3 = torch.cat([tG[:, N_G:], tA[:, nA:]])
            outs = _src_push(src, x3, _cuts(REST)) + [src.flush().cpu().numpy()]
            tail = np.concatenate(outs, axis=1)
            for r in range(2):
                _check_row(name, f'joined, group row {r}', np.concatenate([d['headG'][r], tail[r]]), d['refG'][r])
            _check_row(name, 'joined, the late caller', np.concatenate([d['headA'][0], tail[2]]), d['refA'][0])
            # the late row alone, on the group's counters, at batch 1: what it ran before, bit for bit
            with j.select(eng, [2]) as one:
                assert one.counts() == ((1,) + d['cntG'][0][1:], d['cntG'][1][:2] + (1,) + d['cntG'][1][3:])
                src.restore(one)
                got = _src_push(src, tA, _cuts(REST, start=nA)) + [src.flush().cpu().numpy()]
    assert [o.shape for o in got] == [o.shape for o in d['restA']], (name, 'n_out per call')
    for k, (o, r) in enumerate(zip(got, d['restA'])):
        assert np.array_equal(o, r), (name, 'call', k, float(np.abs(o - r).max()))


def test_refused_pair_join_leaves_the_running_stream_as_it_was():
    torch = _torch()
    name = 'crn'
    d = _pair(name)
    eng = _engine(name)
    nA = d['nA']
    tA = torch.from_numpy(d['xA']).cuda()
    cA = torch.from_numpy(d['cA']).cuda()
    x441 = torch.from_numpy(_clip(SEED_A, 9000, 44100)).cuda()
    with SourceRateStream(eng, 44100, max_push=4800) as s441, SourceRateStream(eng, SR, max_push=4800) as src:
        s441.begin(1, c=cA)
        s441.push(x441[:, :4410].contiguous())
        p441 = s441.save()
        s441.push(x441[:, 4410:8820].contiguous())
        q441 = s441.save()
        off = {}
        for extra in (1, 3):                                # one sample out of phase; in phase for the resampler, not for the engine
            src.begin(1, c=cA)
            _src_push(src, tA, _cuts(N_A0) + [(N_A0, nA + extra)])
            off[extra] = src.save()
        src.begin(1, c=cA)                                  # the running stream: A, as in the uninterrupted reference
        head = np.concatenate(_src_push(src, tA, _cuts(N_A0) + ([(N_A0, nA)] if nA > N_A0 else [])), axis=1)
        assert np.array_equal(head, d['headA'])
        with p441, q441, off[1], off[3], SourceStreamSnapshot.from_bytes(d['imgG']) as g:
            for parts, reason in [
                    ([q441, p441], r'se_resampler_state_join: 44100 -> 16000 Hz cannot be rebased: the read position is a running float64 sum'),
                    ([g, off[1]], r'se_resampler_state_join: parts\[0\] and parts\[1\] are out of phase: n_in %d vs %d, the shift %d is not a '
                                  r'multiple of sr_in / sr_out = 3' % (N_G, nA + 1, N_G - nA - 1)),
                    ([g, off[3]], r'se_stream_state_join: parts\[0\] and parts\[1\] are out of phase'),
                    ([g, p441], r'se_resampler_state_join: parts\[0\] and parts\[1\] differ: sr_in 48000 vs 44100')]:
                with pytest.raises(EngineError, match=reason):
                    SourceStreamSnapshot.join(eng, parts)
            assert g.to_bytes() == d['imgG']
        rest = _src_push(src, tA, _cuts(REST, start=nA)) + [src.flush().cpu().numpy()]
    assert [o.shape for o in rest] == [o.shape for o in d['restA']]
    assert all(np.array_equal(o, r) for o, r in zip(rest, d['restA']))
