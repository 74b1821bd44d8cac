"""GPU: DCCRN's real-LSTM forms (`use_clstm=False`: DCCRN-E / -R / -C, DCCRN/DCCRN_cprs.py:95-102; SE_CFG_DCCRN_REAL_LSTM) against
the fixtures of tools/gen_golden_dccrn_rlstm.py, and the engine's own paths against each other: batch 1 - 16 (one GEMM + cell
launch per step), 17+ (lstm_coop16_kernel<256>, one launch per layer), ragged batches, the frame-online mode."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import se_amd  # noqa: F401
from se_amd import synth, schemas
from conftest import load_golden, rms

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 24                    # tools/gen_golden_dccrn_rlstm.py
DEFAULT_KN = [16, 32, 64, 128, 256, 256]
CONFIGS = {'dccrn_rlstm': (256, DEFAULT_KN), 'dccrn_rlstm128': (128, DEFAULT_KN),
           'dccrn_rlstm_w32': (256, [32, 64, 128, 256, 256, 256])}


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _model(tag='dccrn_rlstm', mode='E', **kw):
    from se_amd.models import DCCRN
    units, kn = CONFIGS[tag]
    return DCCRN(rnn_units=units, masking_mode=mode, kernel_num=kn, **kw).load_synthetic(SEED)


def _wave_ok(y, ref):
    e = rms(y - ref)
    return e < 1e-4 and e < 5e-4 * max(rms(ref), 1e-3), (e, rms(ref))


@pytest.mark.parametrize('tag', list(CONFIGS))
@pytest.mark.parametrize('mode', ['E', 'C', 'R'])
def test_forward_and_decodes_match_reference_fixture(tag, mode):
    torch = _torch()
    G = load_golden(tag)
    m = _model(tag, mode, max_batch=2, max_samples=4000)
    y = m(torch.from_numpy(G['x']).cuda()).cpu().numpy()
    ref = G['y_' + mode]
    assert y.shape == ref.shape and rms(y - ref) < 1e-5 * max(rms(ref), 1.0), (rms(y - ref), rms(ref))
    wav = torch.from_numpy(np.stack([G['wav'], G['wav'][::-1].copy()])).cuda()
    for (p_in, p_out), key in (((1.0, 1.0), 'enh_'), ((0.5, 2.0), 'enh_cprs_')):
        m2 = _model(tag, mode, max_batch=2, max_samples=4000, p_in=p_in, p_out=p_out)
        out = m2.enhance_batch(wav).cpu().numpy()
        assert out.shape[1] == G[key + mode].shape[0]
        ok, info = _wave_ok(out[0], G[key + mode])
        assert ok, (key, info)


@pytest.fixture(scope='module')
def big():
    """DCCRN-E (rnn_units=256, default widths) for 256 clips of 4 s, and the fixture's clip."""
    _torch()
    F = load_golden('full_dccrn_rlstm')
    m = _model(max_batch=256, max_samples=int(F['n']), p_in=0.5, p_out=2.0)
    return m, synth.synth_clip(int(F['seed']), 'speech', int(F['n'])), F['enh4_cprs']


def test_full_clip_alone_and_in_batches(big):
    """batch 1 (per-step launches), 20 and 64 (lstm_coop16_kernel<256>, one and four 16-sequence tiles per workgroup), 256: the
    4 s fixture clip as row 0 of each agrees with the reference and with the other batches."""
    torch = _torch()
    m, x, ref = big
    outs = {}
    for B in (1, 20, 64, 256):
        rows = np.concatenate([x[None], synth.synth_batch(B - 1, 'speech', len(x), seed0=300)]) if B > 1 else x[None]
        outs[B] = m.enhance_batch(torch.from_numpy(rows.astype(np.float32)).cuda()).cpu().numpy()
        ok, info = _wave_ok(outs[B][0, :len(ref)], ref)
        assert ok, (B, info)
    for B in (20, 64, 256):
        assert rms(outs[B][0] - outs[1][0]) < 2e-5 * rms(outs[1][0]), B
    assert rms(outs[256][1:20] - outs[20][1:20]) < 2e-5 * rms(outs[20][1:20])


def test_ragged_rows_equal_per_clip_decodes():
    torch = _torch()
    for tag in ('dccrn_rlstm', 'dccrn_rlstm128'):
        m = _model(tag, max_batch=20, max_samples=16000, p_in=0.5, p_out=2.0)
        lengths = [16000, 4000, 9001, 12345] + [16000 - 333 * i for i in range(16)]
        wav = np.zeros((len(lengths), 16000), np.float32)
        for i, L in enumerate(lengths):
            wav[i, :L] = synth.synth_clip(400 + i, 'speech', L)
        out = m.enhance_ragged(torch.from_numpy(wav).cuda(), lengths).cpu().numpy()
        for i in (0, 1, 2, 3, 19):
            L = lengths[i]
            one = m.enhance_batch(torch.from_numpy(wav[i:i + 1, :L].copy()).cuda()).cpu().numpy()[0]
            assert rms(out[i, :len(one)] - one) < 1e-6 + 2e-5 * rms(one), (tag, i, L)


@pytest.mark.parametrize('tag', ['dccrn_rlstm', 'dccrn_rlstm128'])
@pytest.mark.parametrize('chunk', [1, 4, 16])
def test_streamed_equals_offline(tag, chunk):
    torch = _torch()
    m = _model(tag, max_batch=2, max_samples=20000, p_in=0.5, p_out=2.0)
    x = synth.synth_batch(2, 'speech', 160 + 37 + 1000 + 3 + 7777, seed0=70)
    wav = torch.from_numpy(x).cuda()
    off = m.enhance_batch(wav).cpu().numpy()
    eng = m.engine
    eng.stream_begin(2, c=eng.rms_scale(wav), max_chunk_frames=chunk)
    outs, p = [], 0
    for n in (160, 37, 1000, 3, 7777):
        outs.append(eng.stream_push(wav[:, p:p + n].contiguous()).cpu().numpy())
        p += n
    outs.append(eng.stream_flush().cpu().numpy())
    got = np.concatenate(outs, axis=1)
    assert got.shape == off.shape and rms(got - off) < 1e-6 + 2e-5 * rms(off), (rms(got - off), rms(off))


def test_running_rms_and_long_stream():
    """se_stream_begin_running, and a 10 s stream in 100 ms pushes against the offline decode of the same clip."""
    torch = _torch()
    m = _model(max_batch=1, max_samples=160000)
    x = synth.synth_batch(1, 'speech', 160000, seed0=90)
    wav = torch.from_numpy(x).cuda()
    off = m.enhance_batch(wav).cpu().numpy()
    eng = m.engine
    eng.stream_begin(1, c=eng.rms_scale(wav), max_chunk_frames=16)
    got = np.concatenate([eng.stream_push(wav[:, p:p + 1600].contiguous()).cpu().numpy() for p in range(0, 160000, 1600)]
                         + [eng.stream_flush().cpu().numpy()], axis=1)
    assert got.shape == off.shape and rms(got - off) < 1e-6 + 2e-5 * rms(off), (rms(got - off), rms(off))
    eng.stream_begin(1, max_chunk_frames=16, running_rms=True)
    run = np.concatenate([eng.stream_push(wav[:, p:p + 1600].contiguous()).cpu().numpy() for p in range(0, 160000, 1600)]
                         + [eng.stream_flush().cpu().numpy()], axis=1)
    assert run.shape == off.shape and np.isfinite(run).all() and 0.1 * rms(off) < rms(run) < 10 * rms(off)


_CHILD = r'''
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
import se_amd
from se_amd import synth
from se_amd.models import DCCRN
m = DCCRN(rnn_units=256, masking_mode='E', max_batch=48, max_samples=16000, p_in=0.5, p_out=2.0).load_synthetic(24)
x = synth.synth_batch(48, 'speech', 16000, seed0=500)
np.save(sys.argv[2], m.enhance_batch(torch.from_numpy(x).cuda()).cpu().numpy())
'''


def test_coop256_equals_per_step_path(tmp_path):
    """lstm_coop16_kernel<256> (default from 17 sequences on) vs the per-step GEMM + cell launches (SE_LSTM_COOP256=0, read once
    per process: a child process each) on the same 48 clips."""
    outs = []
    for on in ('1', '0'):
        f = str(tmp_path / f'coop{on}.npy')
        r = subprocess.run([sys.executable, '-c', _CHILD, ROOT, f], env=dict(os.environ, SE_LSTM_COOP256=on), cwd=ROOT,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append(np.load(f))
    assert np.isfinite(outs[0]).all()
    assert rms(outs[0] - outs[1]) < 2e-5 * rms(outs[1]), (rms(outs[0] - outs[1]), rms(outs[1]))


def test_decode_driver_real_lstm_checkpoint(tmp_path):
    """tools/decode_vb.py --model dccrn --checkpoint <DCCRN-E .npz>: the driver recognises the real-LSTM keys."""
    torch = _torch()
    from se_amd import decode, wavio
    sd = synth.synth_state_dict(schemas.SCHEMAS['dccrn_rlstm'](), SEED)
    ck = str(tmp_path / 'dccrn_e.npz')
    np.savez(ck, **sd)
    mix, out = str(tmp_path / 'noisy'), str(tmp_path / 'enh')
    os.makedirs(mix)
    clips = {}
    for i, L in enumerate((4000, 6000, 5000)):
        name = f'p{232 + i}_{i:03d}.wav'
        wavio.write_wav_pcm16(os.path.join(mix, name), synth.synth_clip(60 + i, 'speech', L), 16000)
        clips[name] = wavio.read_wav(os.path.join(mix, name))[0]
    args = types.SimpleNamespace(mix_file_path=mix, esti_clean_file_path=out, fs=16000)
    assert decode.enhance(args, 'dccrn', checkpoint=ck, max_batch=2) == 3
    m = _model(max_batch=1, max_samples=6000)
    for name, x in clips.items():
        y = wavio.read_wav(os.path.join(out, name))[0]
        ref = m.enhance_batch(torch.from_numpy(np.asarray(x, np.float32)[None].copy()).cuda()).cpu().numpy()[0]
        n = min(len(y), len(ref))
        assert n >= len(x) - 128 and rms(y[:n] - ref[:n]) < 1e-4 + 5e-4 * rms(ref), (name, rms(y[:n] - ref[:n]))
