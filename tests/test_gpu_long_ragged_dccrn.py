"""GPU: the `_vb` DCCRN (look-ahead decoder) in se_enhance_long_ragged, on engines created with SE_CFG_DCCRN_ROW_ENDS
(`row_ends=True`): every chunk of the window walk clears the encoder outputs, the core output and each decoder layer's output at or
past each row's own last frame, so each of the six decoder layers sees behind a row's end the zeros it sees when the clip is decoded
alone.

The yardstick of a row is `Engine.enhance_long` of that clip alone on the same flagged engine with the same window size (that path
is pinned to the offline decode and the reference fixtures by tests/test_gpu_long_decode.py), under the project's streamed-vs-offline
bar as `_close` applies it: identical shape and rms(got - ref) < 1e-6 + 2e-5 rms(ref).  A missing cut only damages the last six
frames of a row, so every row is also held to the same bar on its TAIL alone - its last 6 * 128 + 512 output samples, rms(ref) taken
over that tail - where a whole-row rms would dilute the error by more than ten.  Helpers, weight seeds and signals are those of
tests/test_gpu_sliding_stream.py and tests/test_gpu_long_ragged.py; engines of max_samples = 4000 and three rows."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import se_amd  # noqa: F401
from se_amd import synth, schemas, wavio, decode
from test_gpu_sliding_stream import MS, _make, _close, _torch
from test_gpu_long_ragged import _rows_of

pytestmark = pytest.mark.gpu

LENS = (14001, 8960, 3333)            # 111, 71 and 28 frames (tests/test_gpu_long_ragged.py)
TAIL = 6 * 128 + 512                  # the samples the six look-ahead frames of a row reach
DCCRN_CL = dict(rnn_units=256, use_clstm=True, kernel_num=[32, 64, 128, 256, 256, 256])

_ENGINES = {}


def _engine(kind='cl'):
    """one flagged engine of max_samples = 4000 and three rows per variant for the whole module"""
    from se_amd import models
    if kind not in _ENGINES:
        if kind == 'cl':            # the decode script's DCCRN-CL, 'E' mask (weights: seed 14, as everywhere)
            m = _make('dccrn', 3, MS, row_ends=True)
        elif kind == 'cl_plain':    # the same network and weights without the bit
            m = _make('dccrn', 3, MS)
        elif kind == 'real':        # use_clstm=False: the real-LSTM core
            m = models.DCCRN(use_clstm=False, rnn_units=256, max_batch=3, max_samples=MS, p_in=0.5, p_out=2.0, row_ends=True).load_synthetic(14)
        elif kind == 'mask_c':
            m = models.DCCRN(masking_mode='C', **DCCRN_CL, max_batch=3, max_samples=MS, p_in=0.5, p_out=2.0, row_ends=True).load_synthetic(14)
        _ENGINES[kind] = m.engine
        assert _ENGINES[kind].row_ends == (kind != 'cl_plain')
    return _ENGINES[kind]


@pytest.fixture(scope='module', autouse=True)
def _release_shared_engines():
    yield
    for eng in _ENGINES.values():
        eng.close()
    _ENGINES.clear()


def _alone(eng, x, lens, chunk):
    torch = _torch()
    return [eng.enhance_long(torch.from_numpy(x[b:b + 1, :L].copy()).cuda(), max_chunk_frames=chunk).cpu().numpy()[0]
            for b, L in enumerate(lens)]


def _check_rows(eng, got, refs, lens, tag):
    n_max = eng.output_samples(max(lens))
    assert got.shape == (len(lens), n_max), (tag, got.shape, n_max)
    bad = []
    for b, L in enumerate(lens):
        n = eng.output_samples(L)
        ok, info = _close(got[b, :n], refs[b])
        ok_t, info_t = _close(got[b, n - TAIL:n], refs[b][n - TAIL:])
        print(tag, 'row', b, 'L', L, 'vs the row alone (shape, shape, rms err, rms ref): whole', info, 'tail', info_t)
        if not (ok and ok_t and np.isfinite(got[b]).all()):
            bad.append((b, info, info_t))
        assert not got[b, n:].any(), (tag, b, 'samples behind the row\'s own output are not zero')
    assert not bad, (tag, bad)


def _ragged_case(kind, lens, chunk, seed0=820):
    torch = _torch()
    eng = _engine(kind)
    x = _rows_of(lens, seed0)
    got = eng.enhance_long_ragged(torch.from_numpy(x).cuda(), lens, max_chunk_frames=chunk).cpu().numpy()
    _check_rows(eng, got, _alone(eng, x, lens, chunk), lens, f'dccrn {kind} {lens} chunk {chunk}')


# ------------------------------------------------------------------------------------------------ 1. each row = its own windowed decode
@pytest.mark.parametrize('chunk', [0, 1, 7])
def test_each_row_equals_its_own_windowed_decode(chunk):
    _ragged_case('cl', LENS, chunk)


def test_real_lstm_core_takes_the_same_cuts():
    _ragged_case('real', LENS, 7)


def test_masking_mode_c():
    _ragged_case('mask_c', LENS, 0)


def test_rows_that_end_inside_the_last_chunks_extension():
    """108 and 109 frames beside 111: the rows end 3 and 2 frames before the longest, inside the six frames whose decoder columns
    only the chunk that ends the walk computes"""
    for chunk in (0, 7):
        _ragged_case('cl', (14001, 13617, 13745), chunk, 850)


def test_a_row_that_ends_on_a_window_edge():
    """70 frames: the row's last frame (69) is the last frame of a 7-frame window, every one of its look-ahead columns lies in later
    windows; 71 frames: its last frame (70) is the first frame of the next window"""
    _ragged_case('cl', (14001, 8832, 8960), 7, 860)


def test_nothing_past_a_rows_length_is_read_or_written():
    torch = _torch()
    eng = _engine('cl')
    x = _rows_of(LENS)
    clean = eng.enhance_long_ragged(torch.from_numpy(x).cuda(), LENS, max_chunk_frames=7).cpu().numpy()
    xp = x.copy()
    for b, L in enumerate(LENS):
        xp[b, L:] = np.nan
    n_max = eng.output_samples(max(LENS))
    out = torch.full((len(LENS), n_max + 64), float('nan'), dtype=torch.float32, device='cuda')
    eng.enhance_long_ragged(torch.from_numpy(xp).cuda(), LENS, max_chunk_frames=7, out=out)
    got = out.cpu().numpy()
    assert np.isnan(got[:, n_max:]).all(), 'the call wrote past se_output_samples(longest row)'
    for b, L in enumerate(LENS):
        n = eng.output_samples(L)
        assert np.isfinite(got[b, :n]).all(), b
        ok, info = _close(got[b, :n], clean[b, :n])
        print('row', b, 'poisoned vs clean (shape, shape, rms err, rms ref)', info)
        assert ok, (b, info)
        assert (got[b, n:n_max] == 0).all(), (b, 'not exactly zero behind the row\'s output')


# ------------------------------------------------------------------------------------------------ 2. what must not change
@pytest.mark.parametrize('chunk', [1, 7, 0])
def test_one_row_is_bit_identical_to_the_equal_length_call(chunk):
    """one row never ends inside a window of its own walk: every cut is the whole window, the zero-tail launches return at once"""
    torch = _torch()
    eng = _engine('cl')
    L = LENS[0]
    x = torch.from_numpy(_rows_of(LENS)[:1, :L].copy()).cuda()
    ref = eng.enhance_long(x, max_chunk_frames=chunk).cpu().numpy()
    got = eng.enhance_long_ragged(x, [L], max_chunk_frames=chunk).cpu().numpy()
    assert got.shape == ref.shape and np.array_equal(got, ref), (chunk, int((got != ref).sum()))


def test_equal_rows_and_streams_are_those_of_an_engine_without_the_bit():
    torch = _torch()
    flagged, plain = _engine('cl'), _engine('cl_plain')
    x = torch.from_numpy(np.stack([synth.synth_clip(870 + b, 'speech', 9000) for b in range(3)])).cuda()
    for chunk in (7, 0):
        a = flagged.enhance_long(x, max_chunk_frames=chunk).cpu().numpy()
        b = plain.enhance_long(x, max_chunk_frames=chunk).cpu().numpy()
        assert a.shape == b.shape and np.array_equal(a, b), ('enhance_long', chunk, int((a != b).sum()))
    short = x[:, :MS].contiguous()
    outs = []
    for eng in (flagged, plain):
        eng.stream_begin(3, c=eng.rms_scale(short), max_chunk_frames=4)
        parts = [eng.stream_push(short[:, :1500].contiguous()).cpu().numpy(), eng.stream_push(short[:, 1500:].contiguous()).cpu().numpy(),
                 eng.stream_flush().cpu().numpy()]
        outs.append(np.concatenate(parts, axis=1))
    assert outs[0].shape == outs[1].shape and np.array_equal(outs[0], outs[1]), int((outs[0] != outs[1]).sum())


POISON_SCRIPT = r'''
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
import se_amd
from se_amd import synth
from se_amd.models import MODEL_CLASSES
LENS = (14001, 8960, 3333)
x = np.zeros((3, LENS[0]), dtype=np.float32)
for b, L in enumerate(LENS):
    x[b, :L] = synth.synth_clip(820 + b, 'speech' if b % 2 == 0 else 'white', L)
xt = torch.from_numpy(x).cuda()
eng = MODEL_CLASSES['dccrn'](max_batch=3, max_samples=4000, row_ends=True).load_synthetic(14).engine
for chunk in (1, 7, 0):                                   # every chunk size re-carves (and so poisons) the workspace
    got = eng.enhance_long_ragged(xt, LENS, max_chunk_frames=chunk).cpu().numpy()
    assert np.isfinite(got).all(), chunk
    for b, L in enumerate(LENS):
        ref = eng.enhance_long(xt[b:b + 1, :L].contiguous(), max_chunk_frames=chunk).cpu().numpy()[0]
        n = ref.shape[0]
        for lo in (0, n - 1280):
            e = float(np.sqrt(np.mean((got[b, lo:n] - ref[lo:]) ** 2)))
            print(chunk, 'row', b, 'from', lo, 'rms err', e)
            assert e < 1e-6 + 2e-5 * float(np.sqrt(np.mean(ref[lo:] ** 2))), (chunk, b, lo, e)
        assert not got[b, n:].any(), (chunk, b)
eng.close()
print('POISON-OK')
'''


def test_poisoned_workspace_never_reaches_a_row():
    """SE_ARENA_POISON=1 fills the workspace with NaN patterns at every re-carve: a cut that leaves a column behind a row's end as it
    found it, or a layer that reads a column nobody wrote, shows up as NaN in a row"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SE_ARENA_POISON='1')
    r = subprocess.run([sys.executable, '-c', POISON_SCRIPT, root], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'POISON-OK' in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


# ------------------------------------------------------------------------------------------------ 3. contract
def test_the_bit_is_refused_for_other_models_and_for_the_causal_decoder():
    from se_amd import models
    from se_amd.engine import Engine, EngineError
    assert Engine.SE_CFG_DCCRN_ROW_ENDS == 1 << 18 == decode.LONG_RAGGED_FLAGS['dccrn']
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'se_engine.h')).read()
    assert '#define SE_CFG_DCCRN_ROW_ENDS (1 << 18)' in hdr
    with pytest.raises(EngineError, match='SE_CFG_DCCRN_ROW_ENDS is a bit of SE_MODEL_DCCRN'):
        models.MODEL_CLASSES['crn'](max_batch=1, max_samples=MS, row_ends=True).load_synthetic(12)
    with pytest.raises(EngineError, match='does not combine with SE_CFG_DCCRN_CAUSAL_DEC'):
        models.DCCRN_SNR(**DCCRN_CL, max_batch=1, max_samples=MS, row_ends=True).load_synthetic(14)
    # without the bit: refused as ever, and the reason names the bit
    torch = _torch()
    x = torch.from_numpy(_rows_of((8000, 5000), 840)).cuda()
    with pytest.raises(EngineError, match='look-ahead decoder.*SE_CFG_DCCRN_ROW_ENDS'):
        _engine('cl_plain').enhance_long_ragged(x, [8000, 5000])


# ------------------------------------------------------------------------------------------------ 4. the file driver
def test_driver_groups_the_long_dccrn_clips(tmp_path):
    _torch()
    mix, grouped, single = str(tmp_path / 'noisy'), str(tmp_path / 'grouped'), str(tmp_path / 'single')
    lengths = [4000, 40000, 6000, 44001, 70000, 41000]           # four above 2 s: three of similar length, one that fits no group
    os.makedirs(mix)
    names = []
    for i, L in enumerate(lengths):
        names.append(f'p{232 + i}_{i:03d}.wav')
        wavio.write_wav_pcm16(os.path.join(mix, names[-1]), synth.synth_clip(70 + i, 'speech', L), 16000)
    sd = synth.synth_state_dict(schemas.SCHEMAS['dccrn'](), 14)
    ns = lambda out: types.SimpleNamespace(mix_file_path=mix, esti_clean_file_path=out, fs=16000)
    st4, st1 = {}, {}
    assert decode.enhance(ns(grouped), 'dccrn', state_dict=sd, max_batch=4, verbose=False, stats=st4, max_seconds=2,
                          long_batch=4) == len(lengths)
    assert decode.enhance(ns(single), 'dccrn', state_dict=sd, max_batch=4, verbose=False, stats=st1, max_seconds=2,
                          long_batch=1) == len(lengths)
    assert st4['long_clips'] == st1['long_clips'] == 4 and st4['long_audio_s'] == st1['long_audio_s']
    assert st1['long_calls'] == 4 and st4['long_calls'] == 2, (st1, st4)
    assert sorted(os.listdir(grouped)) == sorted(os.listdir(single)) == sorted(names)
    worst = []
    for name in names:
        a, fa = wavio.read_wav(os.path.join(grouped, name))
        b, fb = wavio.read_wav(os.path.join(single, name))
        assert fa == fb == 16000 and len(a) == len(b), (name, len(a), len(b))
        lsb = np.abs(np.round(a * 32768.0).astype(np.int64) - np.round(b * 32768.0).astype(np.int64))
        print(name, 'PCM_16 samples that differ between grouped and one at a time', int((lsb != 0).sum()), 'max', int(lsb.max()))
        worst.append(int(lsb.max()))
    assert max(worst) <= 1, worst
