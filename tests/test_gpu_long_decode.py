"""GPU: se_enhance_long (`Engine.enhance_long`) - the OFFLINE decode of clips longer than the engine's max_samples, run in windows
through the frame-online machinery (csrc/engine.hip stream_process) under the whole clip's unit-RMS scale, reading the caller's
resident rows in place.

The yardstick of the windowed-vs-offline cases is the offline decode of the whole signal on a second engine with max_samples = L
(the existing tests pin that decode to the reference) under the project's streamed-vs-offline bar: identical shape and
rms(got - ref) < 1e-6 + 2e-5 rms(ref).  The long10 cases compare with the reference's own decode of a 10 s clip
(tests/golden/long10_<name>.npz) under the bars of tests/test_gpu_long_clips.py.  Models, seeds and row counts are those of
tests/test_gpu_sliding_stream.py; the bounded engines are made for max_samples = 4000 WITHOUT the sliding-stream flag."""
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
from test_gpu_sliding_stream import ALL, MS, FSN_KW, _make, _rows, _close, _torch
from test_gpu_long_clips import _fixture
from test_gpu_b256_fixture import make as make_fixture_model

pytestmark = pytest.mark.gpu

L_LONG = 14001                  # 3.5 x max_samples, a multiple of no hop: reflection and tail pad fall into the last window


@functools.lru_cache(maxsize=None)
def _offline(name, L):
    """(signal, its offline decode) from an engine with max_samples = L: computed once per model, shared, never written to"""
    torch = _torch()
    B = _rows(name)
    x = np.stack([synth.synth_clip(800 + b, 'speech' if b % 2 == 0 else 'white', L) for b in range(B)])
    m = _make(name, B, L)
    ref = m.enhance_batch(torch.from_numpy(x).cuda()).cpu().numpy()
    m.engine.close()
    for a in (x, ref):
        a.setflags(write=False)
    return x, ref


_ENGINES = {}


def _bounded(name):
    """one engine of max_samples = 4000 per model for the whole module, created without `sliding_stream`"""
    if name not in _ENGINES:
        _ENGINES[name] = _make(name, _rows(name), MS).engine
        assert not _ENGINES[name].sliding_stream
    return _ENGINES[name]


@pytest.fixture(scope='module', autouse=True)
def _release_shared_engines():
    yield
    for eng in _ENGINES.values():
        eng.close()
    _ENGINES.clear()
    _offline.cache_clear()


# ------------------------------------------------------------------------------------------------ 1. windowed = offline
@pytest.mark.parametrize('name', ALL)
@pytest.mark.parametrize('chunk', [0, 1, 7])
def test_windowed_equals_offline(name, chunk):
    torch = _torch()
    x, ref = _offline(name, L_LONG)
    got = _bounded(name).enhance_long(torch.from_numpy(x).cuda(), max_chunk_frames=chunk).cpu().numpy()
    ok, info = _close(got, ref)
    print(name, 'chunk', chunk, 'enhance_long vs offline (shape, shape, rms err, rms ref)', info)
    assert ok and np.isfinite(got).all(), (name, chunk, info)


# ------------------------------------------------------------------------------------------------ 2. clips that would have fitted
@pytest.mark.parametrize('name', ['crn', 'dccrn'])
def test_short_clip_takes_the_same_path(name):
    torch = _torch()
    L = 3333
    eng = _bounded(name)
    x = torch.from_numpy(np.stack([synth.synth_clip(810 + b, 'speech' if b % 2 == 0 else 'white', L) for b in range(2)])).cuda()
    ref = eng.enhance_batch(x).cpu().numpy()
    got = eng.enhance_long(x).cpu().numpy()
    ok, info = _close(got, ref)
    print(name, 'L', L, 'enhance_long vs the same engine\'s enhance_batch (shape, shape, rms err, rms ref)', info)
    assert ok, (name, info)


# ------------------------------------------------------------------------------------------------ 3. against the reference itself
@pytest.mark.parametrize('name', ['crn', 'lstm', 'gcrn', 'dpcrn', 'dccrn', 'ctsnet_new', 'g2net_new', 'taylorsenet_new'])
def test_long10_fixture_matches_reference(name):
    torch = _torch()
    clip, ref = _fixture('10', name)
    m = make_fixture_model(name, 1, 16000)
    y = m.enhance_long(torch.from_numpy(clip[None]).cuda()).cpu().numpy()[0]
    m.engine.close()
    assert y.shape == ref.shape, (name, y.shape, ref.shape)
    e = rms(y - ref)
    print(name, '10 s through a 1 s engine: rms err vs reference', e, 'rms ref', rms(ref))
    assert np.isfinite(y).all() and e < 1e-4 and e < 5e-4 * max(rms(ref), 1e-3), (name, e, rms(ref))


# ------------------------------------------------------------------------------------------------ 4. contract
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
                                   **{**FSN_KW, 'sequence_model': 'GRU'}).load_synthetic(15), 'GRU FullSubNet'),
             (lambda: models.MODEL_CLASSES['g2net'](max_batch=1, max_samples=MS).load_synthetic(20), 'InstanceNorm'),
             (lambda: models.MODEL_CLASSES['taylorsenet'](max_batch=1, max_samples=MS).load_synthetic(19), 'InstanceNorm')]
    for build, why in cases:
        m = build()
        with pytest.raises(EngineError, match=why):
            m.enhance_long(x)
        m.engine.close()


def test_bad_shapes_are_refused():
    torch = _torch()
    from se_amd.engine import EngineError
    eng = _bounded('crn')
    x = torch.from_numpy(np.stack([synth.synth_clip(800 + b, 'speech', 8000) for b in range(2)])).cuda()
    with pytest.raises(EngineError, match='shorter than one FFT frame'):
        eng.enhance_long(x[:, :319].contiguous())                                   # n_fft - 1
    n_out = eng.output_samples(8000)
    with pytest.raises(EngineError, match='need'):
        eng.enhance_long(x, out=torch.empty((2, n_out - 1), device='cuda'))         # refused by the wrapper ...
    out = torch.empty((2, n_out), device='cuda')
    rc = eng._lib.se_enhance_long(eng._h, C.c_void_p(x.data_ptr()), x.stride(0), 2, 8000, 0, C.c_void_p(out.data_ptr()),
                                  n_out - 1, eng._stream())
    assert rc != 0 and b'output row pitch smaller' in eng._lib.se_last_error(eng._h)       # ... and by the library itself
    rc = eng._lib.se_enhance_long(eng._h, C.c_void_p(x.data_ptr()), x.stride(0), 3, 8000, 0, C.c_void_p(out.data_ptr()),
                                  n_out, eng._stream())
    assert rc != 0 and b'max_batch' in eng._lib.se_last_error(eng._h)
    rc = eng._lib.se_enhance_long(eng._h, C.c_void_p(x.data_ptr()), x.stride(0), 1, 2 ** 31 - 1 - 320 - 32 * 160 + 1, 0,
                                  C.c_void_p(out.data_ptr()), 2 ** 31 - 1, eng._stream())
    assert rc != 0 and b'position bound' in eng._lib.se_last_error(eng._h)          # (refused before anything is read)
    ok, info = _close(eng.enhance_long(x).cpu().numpy(), _make_ref('crn', x))
    assert ok, info                                                                 # the handle is as it was


def _make_ref(name, x):
    m = _make(name, x.shape[0], x.shape[1])
    ref = m.enhance_batch(x).cpu().numpy()
    m.engine.close()
    return ref


def test_enhance_long_ends_a_running_stream():
    torch = _torch()
    from se_amd.engine import EngineError
    x, ref = _offline('crn', L_LONG)
    xt = torch.from_numpy(x).cuda()
    eng = _bounded('crn')
    eng.stream_begin(2, max_chunk_frames=4)
    eng.stream_push(xt[:, :2000].contiguous())
    ok, info = _close(eng.enhance_long(xt).cpu().numpy(), ref)
    assert ok, info
    with pytest.raises(EngineError, match='without se_stream_begin'):
        eng.stream_push(xt[:, 2000:3000].contiguous())
    eng.stream_begin(2, c=eng.rms_scale(xt[:, :MS].contiguous()), max_chunk_frames=4)        # a new stream starts as ever
    outs = [eng.stream_push(xt[:, :MS].contiguous()).cpu().numpy(), eng.stream_flush().cpu().numpy()]
    assert _close(np.concatenate(outs, axis=1), eng.enhance_batch(xt[:, :MS].contiguous()).cpu().numpy())[0]


def test_a_refused_enhance_long_leaves_a_running_stream_alone():
    torch = _torch()
    from se_amd.engine import EngineError
    x, ref = _offline('crn', L_LONG)
    xt = torch.from_numpy(x).cuda()
    eng = _bounded('crn')
    short = xt[:, :MS].contiguous()
    want = eng.enhance_batch(short).cpu().numpy()
    eng.stream_begin(2, c=eng.rms_scale(short), max_chunk_frames=4)
    outs = [eng.stream_push(xt[:, :2000].contiguous()).cpu().numpy()]
    with pytest.raises(EngineError, match='shorter than one FFT frame'):
        eng.enhance_long(xt[:, :319].contiguous())
    with pytest.raises(EngineError, match='need'):
        eng.enhance_long(xt, out=torch.empty((2, 100), device='cuda'))
    outs.append(eng.stream_push(xt[:, 2000:MS].contiguous()).cpu().numpy())
    outs.append(eng.stream_flush().cpu().numpy())
    ok, info = _close(np.concatenate(outs, axis=1), want)
    assert ok, info


@pytest.mark.parametrize('name', ['crn', 'dccrn'])
def test_enhance_batch_around_an_enhance_long_is_bit_identical(name):
    torch = _torch()
    x, ref = _offline(name, L_LONG)
    xt = torch.from_numpy(x).cuda()
    eng = _bounded(name)
    short = xt[:, :MS].contiguous()
    before = eng.enhance_batch(short).cpu().numpy()
    assert _close(eng.enhance_long(xt, max_chunk_frames=5).cpu().numpy(), ref)[0]
    assert np.array_equal(eng.enhance_batch(short).cpu().numpy(), before)


# ------------------------------------------------------------------------------------------------ 5. poisoned arena
POISON_SCRIPT = r'''
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
import se_amd
from se_amd import synth, models_new
from se_amd.models import MODEL_CLASSES
L, B = 14001, 2
x = np.stack([synth.synth_clip(800 + b, 'speech' if b % 2 == 0 else 'white', L) for b in range(B)])
xt = torch.from_numpy(x).cuda()
for name, seed in (('crn', 12), ('g2net_new', 20)):
    m = MODEL_CLASSES[name](max_batch=B, max_samples=L).load_synthetic(seed)
    ref = m.enhance_batch(xt).cpu().numpy()
    m.engine.close()
    assert np.isfinite(ref).all(), name
    eng = MODEL_CLASSES[name](max_batch=B, max_samples=4000).load_synthetic(seed).engine
    for chunk in (0, 1, 7):                                   # the windows are re-carved per chunk size; the last one is shorter
        got = eng.enhance_long(xt, max_chunk_frames=chunk).cpu().numpy()
        assert got.shape == ref.shape and np.isfinite(got).all(), (name, chunk)
        e = float(np.sqrt(np.mean((got - ref) ** 2)))
        print(name, chunk, 'rms err', e)
        assert e < 1e-6 + 2e-5 * float(np.sqrt(np.mean(ref ** 2))), (name, chunk, e)
    eng.close()
print('POISON-OK')
'''


def test_poisoned_arena_never_reaches_a_windowed_output():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SE_ARENA_POISON='1')
    r = subprocess.run([sys.executable, '-c', POISON_SCRIPT, root], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'POISON-OK' in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


# ------------------------------------------------------------------------------------------------ 6. the file driver
def _write_clips(d, lengths, seed0):
    os.makedirs(d, exist_ok=True)
    names = []
    for i, L in enumerate(lengths):
        names.append(f'p{232 + i}_{i:03d}.wav')
        wavio.write_wav_pcm16(os.path.join(d, names[-1]), synth.synth_clip(seed0 + i, 'speech', L), 16000)
    return names


def test_driver_decodes_clips_above_max_seconds_in_windows(tmp_path):
    _torch()
    mix, bounded, whole = str(tmp_path / 'noisy'), str(tmp_path / 'bounded'), str(tmp_path / 'whole')
    lengths = [4000, 6000, 4000, 144000, 5001]                   # one clip of 9 s among short ones
    names = _write_clips(mix, lengths, 40)
    sd = synth.synth_state_dict(schemas.crn_schema(), 12)
    ns = lambda out: types.SimpleNamespace(mix_file_path=mix, esti_clean_file_path=out, fs=16000)
    st = {}
    assert decode.enhance(ns(bounded), 'crn', state_dict=sd, max_batch=2, verbose=False, stats=st, max_seconds=2) == len(lengths)
    assert sorted(os.listdir(bounded)) == sorted(names)
    assert st['long_clips'] == 1 and st['long_audio_s'] == 9.0 and st['engine_samples'] == 32000 and st['decoded'] == len(lengths)
    st0 = {}
    assert decode.enhance(ns(whole), 'crn', state_dict=sd, max_batch=2, verbose=False, stats=st0) == len(lengths)
    assert 'long_clips' not in st0
    for name, L in zip(names, lengths):
        a, fa = wavio.read_wav(os.path.join(bounded, name))
        b, fb = wavio.read_wav(os.path.join(whole, name))
        assert fa == fb == 16000 and len(a) == len(b) == L, (name, len(a), len(b))
        lsb = np.abs(np.round(a * 32768.0).astype(np.int64) - np.round(b * 32768.0).astype(np.int64))
        print(name, 'PCM_16 samples that differ from the unbounded driver\'s', int((lsb != 0).sum()), 'max', int(lsb.max()))
        assert lsb.max() <= 1, (name, int(lsb.max()))


def test_driver_refuses_long_clips_of_a_model_that_needs_the_whole_utterance(tmp_path):
    _torch()
    mix, out = str(tmp_path / 'noisy'), str(tmp_path / 'enh')
    names = _write_clips(mix, [4000, 40000], 60)
    sd1 = synth.synth_state_dict(schemas.SCHEMAS['cts_step1'](), 17)
    sd2 = synth.synth_state_dict(schemas.SCHEMAS['cts_step2'](), 18)
    args = types.SimpleNamespace(mix_file_path=mix, esti_file_path=out, fs=16000)
    with pytest.raises(ValueError, match=names[1]):
        decode.enhance(args, 'ctsnet', state_dict=(sd1, sd2), max_batch=2, verbose=False, max_seconds=2)
    assert not os.path.isdir(out) or not os.listdir(out)
