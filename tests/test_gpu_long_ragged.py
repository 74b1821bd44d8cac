"""GPU: se_enhance_long_ragged (`Engine.enhance_long_ragged`) - resident clips of DIFFERENT lengths, any of them longer than the
engine's max_samples, decoded in ONE walk over the windows of the longest row, each row under its own sizes.

The yardstick of a row is `Engine.enhance_long` of that clip alone on the same engine with the same window size (that path is pinned
to the offline decode by tests/test_gpu_long_decode.py) under the project's streamed-vs-offline bar: identical shape and
rms(got - ref) < 1e-6 + 2e-5 rms(ref).  The fixture cases compare with the reference's own decodes of a 10 s and a 15 s clip under
the bars of tests/test_gpu_long_decode.py.  Models and weight seeds are those of tests/test_gpu_sliding_stream.py; the engines are
made for max_samples = 4000 and three rows.

The `_vb` DCCRN (look-ahead decoder) is refused by this entry point - its decoder looks ahead behind the input layer, see
include/se_engine.h - so its cases are a refusal test here; the causal-decoder DCCRN (`dccrn_snr`) stands where `dccrn` would."""
import ctypes as C
import functools
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import se_amd  # noqa: F401
from se_amd import synth, schemas, wavio, decode
from conftest import rms
from test_gpu_sliding_stream import ALL, MS, FSN_KW, _make, _close, _torch
from test_gpu_long_clips import _fixture
from test_gpu_b256_fixture import make as make_fixture_model

pytestmark = pytest.mark.gpu

# 14001: a multiple of no hop; 8960 = 128 * 70 = 160 * 56 = 256 * 35: the row's end on a frame boundary of every front end;
# 3333: shorter than max_samples, the row ends in the first windows
LENS = (14001, 8960, 3333)
B = len(LENS)


def _rows_of(lens, seed0=820):
    """[len(lens), max(lens)] float32: row b = a clip of lens[b] samples, zeros behind it"""
    x = np.zeros((len(lens), max(lens)), dtype=np.float32)
    for b, L in enumerate(lens):
        x[b, :L] = synth.synth_clip(seed0 + b, 'speech' if b % 2 == 0 else 'white', L)
    x.setflags(write=False)
    return x


_ENGINES = {}


def _engine(name):
    if name not in _ENGINES:
        _ENGINES[name] = _make(name, B, MS).engine
    return _ENGINES[name]


@functools.lru_cache(maxsize=None)
def _alone(name, chunk, lens=LENS):
    """row b -> enhance_long of that clip alone on the shared engine: computed once per (model, window), shared, never written to"""
    torch = _torch()
    x = _rows_of(lens)
    eng = _engine(name)
    refs = []
    for b, L in enumerate(lens):
        y = eng.enhance_long(torch.from_numpy(x[b:b + 1, :L].copy()).cuda(), max_chunk_frames=chunk).cpu().numpy()[0]
        y.setflags(write=False)
        refs.append(y)
    return tuple(refs)


@pytest.fixture(scope='module', autouse=True)
def _release_shared_engines():
    yield
    for eng in _ENGINES.values():
        eng.close()
    _ENGINES.clear()
    _alone.cache_clear()


def _check_rows(eng, got, refs, lens, tag):
    n_max = eng.output_samples(max(lens))
    assert got.shape == (len(lens), n_max), (tag, got.shape, n_max)
    for b, L in enumerate(lens):
        n = eng.output_samples(L)
        ok, info = _close(got[b, :n], refs[b])
        print(tag, 'row', b, 'L', L, 'vs the row alone (shape, shape, rms err, rms ref)', info)
        assert ok and np.isfinite(got[b]).all(), (tag, b, info)
        assert not got[b, n:].any(), (tag, b, 'samples behind the row\'s own output are not zero')


# ------------------------------------------------------------------------------------------------ 1. each row = its own windowed decode
MODELS = [n for n in ALL if n != 'dccrn']           # (the look-ahead DCCRN: refused, test below)


@pytest.mark.parametrize('name', MODELS)
@pytest.mark.parametrize('chunk', [0, 1, 7])
def test_each_row_equals_its_own_windowed_decode(name, chunk):
    torch = _torch()
    eng = _engine(name)
    got = eng.enhance_long_ragged(torch.from_numpy(_rows_of(LENS)).cuda(), LENS, max_chunk_frames=chunk).cpu().numpy()
    _check_rows(eng, got, _alone(name, chunk), LENS, f'{name} chunk {chunk}')


# ------------------------------------------------------------------------------------------------ 2. equal rows among ragged ones
@pytest.mark.parametrize('name', ['crn', 'dccrn_snr'])
def test_equal_rows_agree_with_the_equal_length_call(name):
    torch = _torch()
    lens = (14001, 14001, 5000)
    x = _rows_of(lens, 830)
    eng = _engine(name)
    ref = eng.enhance_long(torch.from_numpy(x[:2].copy()).cuda()).cpu().numpy()
    got = eng.enhance_long_ragged(torch.from_numpy(x).cuda(), lens).cpu().numpy()
    ok, info = _close(got[:2], ref)
    print(name, 'two equal rows of a ragged call vs enhance_long of the two (shape, shape, rms err, rms ref)', info)
    assert ok, (name, info)
    short = eng.enhance_long(torch.from_numpy(x[2:, :5000].copy()).cuda()).cpu().numpy()[0]
    ok, info = _close(got[2, :eng.output_samples(5000)], short)
    assert ok and not got[2, eng.output_samples(5000):].any(), (name, info)


# ------------------------------------------------------------------------------------------------ 3. against the reference itself
@pytest.mark.parametrize('name', ['crn', 'lstm', 'gcrn', 'dpcrn', 'ctsnet_new', 'g2net_new', 'taylorsenet_new'])
def test_long_fixtures_decoded_together_match_reference(name):
    torch = _torch()
    c10, r10 = _fixture('10', name)
    c15, r15 = _fixture('15', name)
    lens = (len(c10), len(c15))
    x = np.zeros((2, max(lens)), dtype=np.float32)
    x[0, :lens[0]], x[1, :lens[1]] = c10, c15
    m = make_fixture_model(name, 2, 16000)
    y = m.enhance_long_ragged(torch.from_numpy(x).cuda(), lens).cpu().numpy()
    m.engine.close()
    for b, (ref, tag) in enumerate(((r10, '10 s'), (r15, '15 s'))):
        got = y[b, :len(ref)]
        assert got.shape == ref.shape and not y[b, len(ref):].any(), (name, tag, y.shape, ref.shape)
        e = rms(got - ref)
        print(name, tag, 'in a batch of two through a 1 s engine: rms err vs reference', e, 'rms ref', rms(ref))
        assert np.isfinite(got).all() and e < 1e-4 and e < 5e-4 * max(rms(ref), 1e-3), (name, tag, e, rms(ref))


# ------------------------------------------------------------------------------------------------ 4. nothing past a row's length
@pytest.mark.parametrize('name', ['crn', 'dccrn_snr', 'g2net_new', 'fullsubnet_cum'])
def test_nothing_past_a_rows_length_is_read_or_written(name):
    torch = _torch()
    eng = _engine(name)
    x = _rows_of(LENS)
    clean = eng.enhance_long_ragged(torch.from_numpy(x).cuda(), LENS).cpu().numpy()
    xp = x.copy()
    for b, L in enumerate(LENS):
        xp[b, L:] = np.nan
    n_max = eng.output_samples(max(LENS))
    out = torch.full((B, n_max + 64), float('nan'), dtype=torch.float32, device='cuda')
    eng.enhance_long_ragged(torch.from_numpy(xp).cuda(), LENS, out=out)
    got = out.cpu().numpy()
    assert np.isnan(got[:, n_max:]).all(), (name, 'the call wrote past se_output_samples(longest row)')
    for b, L in enumerate(LENS):
        n = eng.output_samples(L)
        assert np.isfinite(got[b, :n]).all(), (name, b)
        ok, info = _close(got[b, :n], clean[b, :n])
        print(name, 'row', b, 'poisoned vs clean (shape, shape, rms err, rms ref)', info)
        assert ok, (name, b, info)
        assert (got[b, n:n_max] == 0).all(), (name, b, 'not exactly zero behind the row\'s output')


# ------------------------------------------------------------------------------------------------ 4b. a window launch owns its own frames only
@pytest.mark.parametrize('name', ['crn', 'dccrn_snr', 'g2net_new', 'fullsubnet_cum'])
@pytest.mark.parametrize('chunk', [1, 7, 0])
def test_one_row_is_bit_identical_to_the_equal_length_call(name, chunk):
    """A batch of ONE row through the ragged entry point enqueues the launches of enhance_long with the same shapes and operands:
    every window's STFT / iSTFT must see the bound an equal-length launch has (t0 + n, t_fin), not the row's whole-clip frame count -
    else the forward transform pairs a window's last frame with a frame of the next window and the inverse transforms columns past
    the window (odd windows: chunks 1 and 7), and the samples carry rounding noise of unrelated data.  Same arithmetic, same bits."""
    torch = _torch()
    eng = _engine(name)
    L = LENS[0]
    x = torch.from_numpy(_rows_of(LENS)[:1, :L].copy()).cuda()
    ref = eng.enhance_long(x, max_chunk_frames=chunk).cpu().numpy()
    got = eng.enhance_long_ragged(x, [L], max_chunk_frames=chunk).cpu().numpy()
    diff = int((got != ref).sum()) if got.shape == ref.shape else -1
    print(name, 'chunk', chunk, 'samples that differ from enhance_long', diff, 'of', ref.size)
    assert got.shape == ref.shape and np.array_equal(got, ref), (name, chunk, diff)


POISON_SCRIPT = r'''
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
import se_amd
from se_amd import synth, models_new
from se_amd.models import MODEL_CLASSES
LENS = (14001, 8960, 3333)
x = np.zeros((3, LENS[0]), dtype=np.float32)
for b, L in enumerate(LENS):
    x[b, :L] = synth.synth_clip(820 + b, 'speech' if b % 2 == 0 else 'white', L)
xt = torch.from_numpy(x).cuda()
for name, seed in (('crn', 12), ('g2net_new', 20)):
    eng = MODEL_CLASSES[name](max_batch=3, max_samples=4000).load_synthetic(seed).engine
    for chunk in (1, 7, 0):                                   # every chunk size re-carves (and so poisons) the workspace
        got = eng.enhance_long_ragged(xt, LENS, max_chunk_frames=chunk).cpu().numpy()
        assert np.isfinite(got).all(), (name, chunk)
        for b, L in enumerate(LENS):
            ref = eng.enhance_long(xt[b:b + 1, :L].contiguous(), max_chunk_frames=chunk).cpu().numpy()[0]
            n = ref.shape[0]
            e = float(np.sqrt(np.mean((got[b, :n] - ref) ** 2)))
            print(name, chunk, 'row', b, 'rms err', e)
            assert e < 1e-6 + 2e-5 * float(np.sqrt(np.mean(ref ** 2))) and not got[b, n:].any(), (name, chunk, b, e)
    eng.close()
print('POISON-OK')
'''


def test_poisoned_workspace_never_reaches_a_row():
    """SE_ARENA_POISON=1 fills the workspace with NaN patterns at every re-carve: a window launch that reads a column nobody wrote,
    or past the end of the estimate, shows up as NaN in a row"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SE_ARENA_POISON='1')
    r = subprocess.run([sys.executable, '-c', POISON_SCRIPT, root], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'POISON-OK' in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


# ------------------------------------------------------------------------------------------------ 5. contract
def test_models_that_need_the_whole_utterance_are_refused_with_the_reason():
    torch = _torch()
    from se_amd import models
    from se_amd.engine import EngineError
    x = torch.from_numpy(synth.synth_clip(800, 'speech', 8000)[None]).cuda()
    cases = [(lambda: models.MODEL_CLASSES['uformer'](max_batch=1, max_samples=MS).load_synthetic(21), 'Uformer attends'),
             (lambda: models.CTSNet(max_batch=1, max_samples=MS).load_synthetic(17, 18), 'InstanceNorm'),
             (lambda: models.Model(max_batch=1, max_samples=MS, norm_type='offline_laplace_norm', **FSN_KW).load_synthetic(15),
              'offline_laplace_norm'),
             (lambda: models.Model(max_batch=1, max_samples=MS, norm_type='cumulative_laplace_norm',
                                   **{**FSN_KW, 'sequence_model': 'GRU'}).load_synthetic(15), 'GRU FullSubNet')]
    for build, why in cases:
        m = build()
        with pytest.raises(EngineError, match=why):
            m.enhance_long_ragged(x, [8000])
        with pytest.raises(EngineError) as long_err:
            m.enhance_long(x)
        # the same reason text as se_enhance_long gives
        with pytest.raises(EngineError) as rag_err:
            m.enhance_long_ragged(x, [8000])
        tail = lambda ex: str(ex.value).split('causal end to end: ', 1)[1]
        assert tail(rag_err) == tail(long_err), (str(rag_err.value), str(long_err.value))
        m.engine.close()


def test_the_look_ahead_dccrn_is_refused_with_the_reason_and_decodes_alone_as_before():
    torch = _torch()
    from se_amd.engine import EngineError
    m = _make('dccrn', 2, MS)
    x = torch.from_numpy(_rows_of((8000, 5000), 840)).cuda()
    with pytest.raises(EngineError, match='look-ahead decoder'):
        m.enhance_long_ragged(x, [8000, 5000])
    assert m.enhance_long(x).shape == (2, m.engine.output_samples(8000))
    m.engine.close()


def _raw(eng, x, lens, batch=None, out_pitch=None):
    torch = _torch()
    out = torch.empty((x.shape[0], eng.output_samples(max(lens))), device='cuda')
    arr = (C.c_int32 * len(lens))(*lens)
    rc = eng._lib.se_enhance_long_ragged(eng._h, C.c_void_p(x.data_ptr()), x.stride(0), batch or len(lens), arr, 0,
                                         C.c_void_p(out.data_ptr()), out_pitch or out.stride(0), eng._stream())
    return rc, eng._lib.se_last_error(eng._h)


def test_bad_shapes_are_refused_and_a_running_stream_goes_on():
    torch = _torch()
    from se_amd.engine import EngineError
    eng = _engine('crn')
    x = torch.from_numpy(np.stack([synth.synth_clip(800 + b, 'speech', 8000) for b in range(B)])).cuda()
    short = x[:, :MS].contiguous()
    want = eng.enhance_batch(short).cpu().numpy()
    eng.stream_begin(B, c=eng.rms_scale(short), max_chunk_frames=4)
    outs = [eng.stream_push(x[:, :2000].contiguous()).cpu().numpy()]
    rc, err = _raw(eng, x, [8000, 319, 8000])                                    # n_fft - 1
    assert rc != 0 and b'lengths[1] shorter than one FFT frame' in err, err
    with pytest.raises(EngineError, match='shorter than one FFT frame'):
        eng.enhance_long_ragged(x, [8000, 8000, 319])
    rc, err = _raw(eng, x, [8000] * (B + 1), batch=B + 1)
    assert rc != 0 and b'max_batch' in err, err
    rc, err = _raw(eng, x, [8000, 4000, 4000], out_pitch=eng.output_samples(8000) - 1)     # the pitch is checked against the longest row
    assert rc != 0 and b'output row pitch smaller' in err, err
    rc, err = _raw(eng, x, [8000, 2 ** 31 - 1 - 320 - 32 * 160 + 1, 8000])
    assert rc != 0 and b'position bound' in err, err                            # (refused before anything is read)
    with pytest.raises(EngineError, match='need'):
        eng.enhance_long_ragged(x, [8000, 5000, 4000], out=torch.empty((B, 100), device='cuda'))
    # every refusal left the stream as it was
    outs.append(eng.stream_push(x[:, 2000:MS].contiguous()).cpu().numpy())
    outs.append(eng.stream_flush().cpu().numpy())
    ok, info = _close(np.concatenate(outs, axis=1), want)
    assert ok, info


def test_an_accepted_call_ends_a_running_stream():
    torch = _torch()
    from se_amd.engine import EngineError
    eng = _engine('crn')
    xt = torch.from_numpy(_rows_of(LENS)).cuda()
    eng.stream_begin(B, max_chunk_frames=4)
    eng.stream_push(xt[:, :2000].contiguous())
    got = eng.enhance_long_ragged(xt, LENS).cpu().numpy()
    _check_rows(eng, got, _alone('crn', 0), LENS, 'crn behind a stream')
    with pytest.raises(EngineError, match='without se_stream_begin'):
        eng.stream_push(xt[:, 2000:3000].contiguous())
    short = xt[:, :MS].contiguous()                                             # a new stream starts as ever
    eng.stream_begin(B, c=eng.rms_scale(short), max_chunk_frames=4)
    outs = [eng.stream_push(short).cpu().numpy(), eng.stream_flush().cpu().numpy()]
    assert _close(np.concatenate(outs, axis=1), eng.enhance_batch(short).cpu().numpy())[0]


# ------------------------------------------------------------------------------------------------ 6. the file driver
def test_driver_groups_the_clips_above_max_seconds(tmp_path):
    _torch()
    mix, grouped, single = str(tmp_path / 'noisy'), str(tmp_path / 'grouped'), str(tmp_path / 'single')
    lengths = [4000, 40000, 6000, 44001, 70000, 41000]           # four above 2 s: three of similar length, one that fits no group
    os.makedirs(mix)
    names = []
    for i, L in enumerate(lengths):
        names.append(f'p{232 + i}_{i:03d}.wav')
        wavio.write_wav_pcm16(os.path.join(mix, names[-1]), synth.synth_clip(70 + i, 'speech', L), 16000)
    sd = synth.synth_state_dict(schemas.crn_schema(), 12)
    ns = lambda out: types.SimpleNamespace(mix_file_path=mix, esti_clean_file_path=out, fs=16000)
    st4, st1 = {}, {}
    assert decode.enhance(ns(grouped), 'crn', state_dict=sd, max_batch=4, verbose=False, stats=st4, max_seconds=2,
                          long_batch=4) == len(lengths)
    assert decode.enhance(ns(single), 'crn', state_dict=sd, max_batch=4, verbose=False, stats=st1, max_seconds=2,
                          long_batch=1) == len(lengths)
    assert st4['long_clips'] == st1['long_clips'] == 4 and st4['long_audio_s'] == st1['long_audio_s']
    assert st1['long_calls'] == 4 and st4['long_calls'] == 2, (st1, st4)
    assert sorted(os.listdir(grouped)) == sorted(os.listdir(single)) == sorted(names)
    for name, L in zip(names, lengths):
        a, fa = wavio.read_wav(os.path.join(grouped, name))
        b, fb = wavio.read_wav(os.path.join(single, name))
        assert fa == fb == 16000 and len(a) == len(b) == L, (name, len(a), len(b))
        lsb = np.abs(np.round(a * 32768.0).astype(np.int64) - np.round(b * 32768.0).astype(np.int64))
        print(name, 'PCM_16 samples that differ between grouped and one at a time', int((lsb != 0).sum()), 'max', int(lsb.max()))
        assert lsb.max() <= 1, (name, int(lsb.max()))
