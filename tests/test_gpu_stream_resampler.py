"""GPU: the stateful resampler (se_resampler_*, se_amd.resample.StreamResampler) - a signal fed in pushes of any sizes and
then flushed must give the very samples `resample()` (se_resample) gives for the whole signal: equal as numbers, the fix_length
zero tail included.  se_resample itself is pinned to oracle/resample.py by tests/test_resample.py; the streamed result is held
to the same bound here.  Then SourceRateStream: the resampler in front of the engine's frame-online stream."""
import numpy as np
import pytest

import se_amd  # noqa: F401
from se_amd import synth
from conftest import rms

pytestmark = pytest.mark.gpu

N = 4801                 # more than twice the two-sided reach (2 x 193 at 48 -> 16 kHz), not a multiple of 3
PITCH = N + 59           # batch 3: rows further apart than they are long
ORACLE_BOUND = 2e-7      # tests/test_resample.py::test_hip_resampler_matches_oracle: fp32 output of a float64 accumulation
RATES = [(48000, 16000), (32000, 16000), (44100, 16000), (16000, 48000)]
SCHEDULES = {'sevens': [7], '480s': [480], 'whole': [N], 'ragged': [1, 191, 2, 1000, N]}

_cache = {}


def _signal(B):
    """[B, N] float32 on the device, rows PITCH apart when B > 1"""
    import torch
    if B not in _cache:
        x = np.stack([synth.synth_clip(700 + b, 'speech' if b % 2 == 0 else 'white', N, fs=48000) for b in range(B)])
        buf = torch.zeros((B, PITCH if B > 1 else N), dtype=torch.float32, device='cuda')
        buf[:, :N] = torch.from_numpy(x).cuda()
        _cache[B] = (x, buf[:, :N])
    return _cache[B]


def _offline(B, sr_in, sr_out):
    """resample() of the whole signal (computed once per case, never written to) and the oracle's float64 result"""
    from se_amd import resample as HR
    from oracle import resample as R
    key = (B, sr_in, sr_out)
    if key not in _cache:
        x, xt = _signal(B)
        y = HR.resample(xt, sr_in, sr_out).cpu().numpy()
        ref = np.stack([R.librosa_resample(x[b].astype(np.float64), sr_in, sr_out) for b in range(B)])
        assert y.shape == ref.shape and np.abs(y - ref).max() < ORACLE_BOUND
        y.setflags(write=False)
        ref.setflags(write=False)
        _cache[key] = (y, ref)
    return _cache[key]


def _streamed(rs, xt, pieces, B=None):
    """begin, the pushes (the last size repeats), flush -> (concatenated output, the pushes' output counts, the flush's count)"""
    B = xt.shape[0] if B is None else B
    n = xt.shape[1]
    rs.begin(B)
    outs, pos, k = [], 0, 0
    while pos < n:
        m = min(pieces[min(k, len(pieces) - 1)], n - pos)
        outs.append(rs.push(xt[:, pos:pos + m]).cpu().numpy())
        pos += m
        k += 1
    tail = rs.flush().cpu().numpy()
    return np.concatenate(outs + [tail], axis=1), [o.shape[1] for o in outs], tail.shape[1]


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('sched', sorted(SCHEDULES))
@pytest.mark.parametrize('sr_in,sr_out', RATES)
def test_pushes_and_flush_equal_the_offline_call(sr_in, sr_out, sched, B):
    from se_amd import resample as HR
    pieces = SCHEDULES[sched]
    x, xt = _signal(B)
    want, ref = _offline(B, sr_in, sr_out)
    with HR.StreamResampler(sr_in, sr_out, max_batch=B, max_push=max(pieces)) as rs:
        got, counts, _ = _streamed(rs, xt, pieces)
    assert got.shape == want.shape == (B, HR.resample_samples(N, sr_in, sr_out))
    for b in range(B):
        assert np.array_equal(got[b], want[b]), (b, np.abs(got[b] - want[b]).max())
        assert np.abs(got[b] - ref[b]).max() < ORACLE_BOUND
    # each push returns what became final: the stateless count, before and after
    fed = done = 0
    for i, c in enumerate(counts):
        fed += min(pieces[min(i, len(pieces) - 1)], N - fed)
        assert done + c == HR.ready_samples(fed, sr_in, sr_out)
        done += c


def test_one_sample_pushes_48k():
    from se_amd import resample as HR
    x, xt = _signal(1)
    want, _ = _offline(1, 48000, 16000)
    with HR.StreamResampler(48000, 16000, max_batch=1, max_push=1) as rs:
        got, counts, n_tail = _streamed(rs, xt, [1])
    assert got.shape == want.shape and np.array_equal(got, want)
    assert counts[:193] == [0] * 193 and counts[193] == 1          # output 0 comes with sample 193, then one output per 3 inputs
    assert counts[193:202] == [1, 0, 0] * 3 and set(counts[193:]) == {0, 1} and n_tail == want.shape[1] - sum(counts)


@pytest.mark.parametrize('sr_in,sr_out,n', [(48000, 16000, 100), (48000, 16000, 193), (44100, 16000, 100), (44100, 16000, 178)])
def test_signals_below_and_at_the_look_ahead(sr_in, sr_out, n):
    """100 samples, below the filter's reach, and exactly the reach (193 at 48 kHz, 178 at 44.1 kHz): every push returns 0
    samples, the flush returns all of them (right wing cut at the end)"""
    from se_amd import resample as HR
    _, xt = _signal(3)
    xt = xt[:, :n]
    want = HR.resample(xt, sr_in, sr_out).cpu().numpy()
    with HR.StreamResampler(sr_in, sr_out, max_batch=3, max_push=64) as rs:
        got, counts, n_tail = _streamed(rs, xt, [64, 30, 64])
    assert len(counts) >= 2 and counts == [0] * len(counts) and n_tail == want.shape[1] == HR.resample_samples(n, sr_in, sr_out)
    assert got.shape == want.shape and np.array_equal(got, want)


def test_begin_resets_everything():
    from se_amd import resample as HR
    _, xt = _signal(3)
    want, _ = _offline(3, 44100, 16000)
    with HR.StreamResampler(44100, 16000, max_batch=3, max_push=1000) as rs:
        rs.begin(3)
        rs.push(xt[:, 1000:2000])                    # a signal that is abandoned mid-way
        rs.push(xt[:, 7:500])
        got, _, _ = _streamed(rs, xt, [1000])        # begins again
        assert np.array_equal(got, want)
        got, _, _ = _streamed(rs, xt[:1], [333], B=1)       # and again after a flush, with fewer rows
        assert np.array_equal(got[0], want[0])


def test_two_objects_on_two_streams_share_nothing():
    import torch
    from se_amd import resample as HR
    _, xt = _signal(3)
    want48, _ = _offline(3, 48000, 16000)
    want44, _ = _offline(3, 44100, 16000)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with HR.StreamResampler(48000, 16000, max_batch=3, max_push=480) as a, \
            HR.StreamResampler(44100, 16000, max_batch=3, max_push=441) as b:
        with torch.cuda.stream(s1):
            a.begin(3)
        with torch.cuda.stream(s2):
            b.begin(3)
        oa, ob = [], []
        for k in range(0, N, 480):                   # interleaved: one push each, turn by turn
            with torch.cuda.stream(s1):
                oa.append(a.push(xt[:, k:k + 480]))
            j = k // 480 * 441
            with torch.cuda.stream(s2):
                ob.append(b.push(xt[:, j:min(j + 441, N)]))
        with torch.cuda.stream(s2):                  # 10 pushes of 441 and one of 391: all of it
            ob.append(b.flush())
        with torch.cuda.stream(s1):
            oa.append(a.flush())
        torch.cuda.synchronize()
        assert np.array_equal(torch.cat(oa, dim=1).cpu().numpy(), want48)
        assert np.array_equal(torch.cat(ob, dim=1).cpu().numpy(), want44)


def test_equal_rates_pass_through():
    import torch
    from se_amd import resample as HR
    x, xt = _signal(3)
    with HR.StreamResampler(16000, 16000, max_batch=3, max_push=1000) as rs:
        rs.begin(3)
        outs = [rs.push(xt[:, p:p + 1000]) for p in range(0, N, 1000)]
        assert [o.shape[1] for o in outs] == [1000, 1000, 1000, 1000, 801]
        assert rs.flush().shape == (3, 0)
        assert np.array_equal(torch.cat(outs, dim=1).cpu().numpy(), x)


def test_refusals_leave_the_stream_as_it_was():
    import ctypes as C
    import torch
    from se_amd import resample as HR, _lib
    _, xt = _signal(3)
    want, _ = _offline(3, 48000, 16000)
    with HR.StreamResampler(48000, 16000, max_batch=3, max_push=1000) as rs:
        with pytest.raises(RuntimeError, match='without se_resampler_begin'):
            rs.push(xt[:, :10])
        with pytest.raises(RuntimeError, match='without begin'):
            rs.flush()
        with pytest.raises(RuntimeError, match='max_batch'):
            rs.begin(4)
        with pytest.raises(RuntimeError, match='without se_resampler_begin'):      # the refused begin started nothing
            rs.push(xt[:, :10])
        rs.begin(3)
        outs = [rs.push(xt[:, :1000])]
        with pytest.raises(RuntimeError, match='max_push'):
            rs.push(xt[:, 1000:2001])
        with pytest.raises(RuntimeError, match='rows'):
            rs.push(xt[:2, 1000:2000])
        # an output row pitch below the samples the push releases: refused by the library itself
        small, n_out = torch.empty((3, 8), dtype=torch.float32, device='cuda'), C.c_int32(-1)
        piece = xt[:, 1000:2000]
        assert rs._lib.se_resampler_push(rs._h, C.c_void_p(piece.data_ptr()), piece.stride(0), 1000, C.c_void_p(small.data_ptr()),
                                         small.stride(0), C.byref(n_out), rs._stream()) != 0
        assert b'pitch' in _lib.load().se_last_error(None) and n_out.value == -1
        # the stream goes on as if none of these had been tried
        outs += [rs.push(xt[:, p:p + 1000]) for p in range(1000, N, 1000)]
        outs.append(rs.flush())
        assert np.array_equal(torch.cat(outs, dim=1).cpu().numpy(), want)
    # a total length beyond the int range of se_resample
    with HR.StreamResampler(48000, 16000, max_batch=1, max_push=2 ** 31 - 1) as rs:
        # one push that is within max_push but carries the total past 2^31 - 1: refused before anything is read
        rs.begin(1)
        out = rs.push(xt[:1, :1000])
        n_out = C.c_int32(-1)
        assert rs._lib.se_resampler_push(rs._h, C.c_void_p(xt.data_ptr()), 2 ** 31 - 1, 2 ** 31 - 1000, C.c_void_p(small.data_ptr()),
                                         8, C.byref(n_out), rs._stream()) != 0
        assert b'pass' in _lib.load().se_last_error(None) and n_out.value == -1
        rest = [rs.push(xt[:1, p:p + 1000]) for p in range(1000, N, 1000)] + [rs.flush()]
        assert np.array_equal(torch.cat([out] + rest, dim=1).cpu().numpy()[0], want[0])


def test_source_rate_stream_on_crn():
    """48 kHz pushes of 10 ms through SourceRateStream against the offline decode of the offline-resampled signal.  The 16 kHz
    samples that enter the engine are identical (the tests above), so what remains is the engine's own streamed-versus-offline
    rounding: the bound of tests/test_gpu_streaming.py::test_streamed_output_equals_offline."""
    import torch
    from se_amd import resample as HR
    from se_amd.models import MODEL_CLASSES
    from se_amd.source_stream import SourceRateStream
    B, L48 = 2, 28801                                 # 0.6 s at 48 kHz, not a multiple of 3 or of a push
    x48 = np.stack([synth.synth_clip(760 + b, 'speech' if b % 2 == 0 else 'white', L48, fs=48000) for b in range(B)])
    xt = torch.from_numpy(x48).cuda()
    x16 = HR.resample(xt, 48000, 16000)
    assert x16.shape == (B, 9601)
    m = MODEL_CLASSES['crn'](max_batch=B, max_samples=16000).load_synthetic(12)
    ref = m.enhance_batch(x16).cpu().numpy()
    eng = m.engine
    for running in (False, True):
        with SourceRateStream(eng, 48000, max_push=480) as src:
            if running:
                src.begin(B, max_chunk_frames=4, running_rms=True)       # se_stream_begin_running
            else:
                src.begin(B, c=eng.rms_scale(x16), max_chunk_frames=4)   # se_stream_begin, given c
            outs = [src.push(xt[:, p:p + 480]) for p in range(0, L48, 480)]
            outs.append(src.flush())
        assert outs[0].shape == (B, 0)                # the first 96 samples at 16 kHz are not yet a frame
        got = torch.cat(outs, dim=1).cpu().numpy()
        assert got.shape == ref.shape, (got.shape, ref.shape)
        if running:
            # the running scale sees a short prefix first (tests/test_gpu_streaming.py): the stream runs and ends at the same
            # length with finite samples; the numbers are the given-c case's business
            assert np.isfinite(got).all()
            continue
        e = rms(got - ref)
        print('crn at 48 kHz, streamed vs offline rms err', e, 'rms ref', rms(ref))
        assert e < 1e-6 + 2e-5 * rms(ref), (e, rms(ref))
