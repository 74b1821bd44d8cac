"""GPU: the DCCRN of `DCCRN_SNR/` (DCCRN_SNR/DCCRN.py:9-183; SE_CFG_DCCRN_CAUSAL_DEC: the decoder keeps `out[..., :-1]`, :159) against
the fixtures of tools/gen_golden_dccrn_snr.py - forward and decode of both cores, ragged batches, a fixture row in a batch of 256,
the frame-online mode against the offline decode, the number of samples every push returns (no look-ahead: 6 x 128 samples
earlier than the `_vb` DCCRN), and the three decode paths over a poisoned arena.

Bars are the existing DCCRN tests': forward 1e-5 of the signal (test_gpu_dccrn.py), waveform 1e-4 RMS and 5e-4 rms(reference)
(test_gpu_dccrn.py / test_gpu_b256_fixture.py), ragged rows 1e-4 and 2e-5 rms(batch-1 decode) (test_gpu_ragged.py), streamed
1e-6 + 2e-5 rms(offline) (test_gpu_streaming.py).  DCCRN parity is unpinned at the `complexnn` boundary, here as there."""
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
CAUSAL = 1 << 16
CL = dict(rnn_units=256, use_clstm=True, kernel_num=[32, 64, 128, 256, 256, 256])       # dccrn_decode_snr.py:12
# core tag -> (constructor arguments, weight seed of the fixture)
CORES = {'clstm': (CL, 14), 'rlstm128': (dict(rnn_units=128), 24), 'rlstm256': (dict(rnn_units=256), 24)}
N_FFT, HOP = 512, 128


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _model(core='clstm', **kw):
    from se_amd.models import DCCRN_SNR
    ctor, seed = CORES[core]
    return DCCRN_SNR(**ctor, **kw).load_synthetic(seed)


def _wave_ok(y, ref):
    e = rms(y - ref)
    return e < 1e-4 and e < 5e-4 * max(rms(ref), 1e-3), (e, rms(ref))


# ------------------------------------------------------------------------------------------------ forward / decode parity
def test_forward_matches_reference_fixture_and_is_causal():
    torch = _torch()
    G = load_golden('dccrn_snr')
    m = _model('clstm', max_batch=2)
    y = m(torch.from_numpy(G['x']).cuda()).cpu().numpy()
    err = rms(y - G['y'])
    print('dccrn_snr forward rms err', err, 'rms ref', rms(G['y']))
    assert y.shape == G['y'].shape and err < 1e-5 * max(rms(G['y']), 1.0), (err, rms(G['y']))
    # not the look-ahead network: same weights and input as tests/golden/dccrn.npz
    assert rms(y - load_golden('dccrn')['y']) > 1e-2 * rms(G['y'])
    # the fixture's second forward (frames >= t_keep replaced): matched too, and the frames before t_keep did not move
    yf = m(torch.from_numpy(G['x_future']).cuda()).cpu().numpy()
    k = int(G['t_keep'])
    assert rms(yf - G['y_future']) < 1e-5 * max(rms(G['y_future']), 1.0)
    assert rms(yf[..., :k] - y[..., :k]) < 1e-6 * rms(y) and rms(yf[..., k:] - y[..., k:]) > 1e-2 * rms(y)


@pytest.mark.parametrize('units', [128, 256])
def test_real_lstm_forward_matches_reference_fixture(units):
    torch = _torch()
    G = load_golden('dccrn_snr_rlstm')
    m = _model(f'rlstm{units}', max_batch=2)
    y = m(torch.from_numpy(G['x']).cuda()).cpu().numpy()
    ref = G[f'y_{units}']
    err = rms(y - ref)
    print('dccrn_snr real-LSTM', units, 'forward rms err', err, 'rms ref', rms(ref))
    assert y.shape == ref.shape and err < 1e-5 * max(rms(ref), 1.0), (err, rms(ref))


@pytest.mark.parametrize('core', list(CORES))
@pytest.mark.parametrize('p_in,p_out,key', [(1.0, 1.0, 'enh'), (0.5, 2.0, 'enh_cprs')])
def test_decode_matches_reference_fixture(core, p_in, p_out, key):
    """dccrn_decode_snr.py:31-67 on the 4 000-sample clip: 4 000 samples back (the `_vb` script: 4 096), both rows of a batch."""
    torch = _torch()
    if core == 'clstm':
        G = load_golden('dccrn_snr')
        ref = G[key]
    else:
        G = load_golden('dccrn_snr_rlstm')
        ref = G[key + '_' + core[5:]]
    m = _model(core, p_in=p_in, p_out=p_out, max_batch=2, max_samples=4000)
    wav = torch.from_numpy(np.stack([G['wav'], G['wav']])).cuda()
    y = m.enhance_batch(wav).cpu().numpy()
    assert y.shape == (2, len(G['wav'])) and ref.shape == (len(G['wav']),)
    for b in range(2):
        ok, info = _wave_ok(y[b], ref)
        print('dccrn_snr', core, key, 'row', b, 'rms err, rms ref', info)
        assert ok, (core, key, b, info)


def test_full_clip_matches_reference_fixture():
    torch = _torch()
    F = load_golden('full_dccrn_snr')
    L = int(F['n'])
    m = _model('clstm', p_in=0.5, p_out=2.0, max_batch=2, max_samples=L)
    x = np.stack([synth.synth_clip(int(F['seed']), 'speech', L), synth.synth_clip(301, 'white', L)])
    y = m.enhance_batch(torch.from_numpy(x).cuda()).cpu().numpy()
    assert y.shape == (2, L) and np.isfinite(y).all()
    ok, info = _wave_ok(y[0], F['enh4_cprs'])
    print('dccrn_snr 4 s clip rms err, rms ref', info)
    assert ok, info


def test_output_samples_and_engine_refuses_other_masks():
    """se_output_samples(n) = n with the bit (the `_vb` DCCRN: the hop-padded length); the frame count is the same; MASK_C / _R
    + the causal decoder fail at se_engine_create with a message that names the bits."""
    _torch()
    from se_amd.engine import Engine, EngineError
    from se_amd.models import DCCRN
    snr = _model('clstm', max_samples=20000).engine
    vb = DCCRN(masking_mode='E', **CL, max_samples=20000).load_synthetic(14).engine
    for n in (512, 4000, 4096, 9001, 12345, 20000):
        pad = -(-n // HOP) * HOP
        assert snr.output_samples(n) == n and vb.output_samples(n) == pad
        assert snr.num_frames(n) == vb.num_frames(n) == 1 + pad // HOP
    for bits in (32, 64):
        with pytest.raises(EngineError, match='SE_CFG_DCCRN_CAUSAL_DEC'):
            Engine('dccrn', flags=CAUSAL | bits)


# ------------------------------------------------------------------------------------------------ ragged, batch row
@pytest.mark.parametrize('core', ['clstm', 'rlstm256'])
def test_ragged_rows_equal_per_clip_decodes(core):
    torch = _torch()
    lengths = [6000, 3217, 9000, 4801, 7777, 5120, 8191, 3999]
    kinds = ('speech', 'white', 'speech', 'gap')
    clips = [synth.synth_clip(1300 + i, kinds[i % 4], n) for i, n in enumerate(lengths)]
    x = np.zeros((len(lengths), max(lengths)), np.float32)
    for i, c in enumerate(clips):
        x[i, :len(c)] = c
        x[i, len(c):] = 0.25 * np.sin(0.01 * np.arange(max(lengths) - len(c)))     # junk past the end must be ignored
    m = _model(core, max_batch=len(lengths), max_samples=max(lengths), p_in=0.5, p_out=2.0)
    y = m.enhance_ragged(torch.from_numpy(x).cuda(), lengths).cpu().numpy()
    one = _model(core, max_batch=1, max_samples=max(lengths), p_in=0.5, p_out=2.0)
    assert y.shape == (len(lengths), max(lengths))
    for i, c in enumerate(clips):
        ref = one.enhance_batch(torch.from_numpy(c[None]).cuda()).cpu().numpy()[0]
        n = len(ref)
        assert n == lengths[i] == m.engine.output_samples(lengths[i])
        e = rms(y[i, :n] - ref)
        print('dccrn_snr', core, 'ragged row', i, lengths[i], 'rms err', e, 'rms ref', rms(ref))
        assert np.isfinite(y[i]).all()
        assert e < 1e-4 and e < 2e-5 * max(rms(ref), 1e-3), (core, i, lengths[i], e, rms(ref))
        assert not y[i, n:].any(), (core, i, 'samples past the row\'s own output length must be zero')


def test_fixture_row_at_batch_256():
    """The 4 s fixture clip in a middle row of 256 (the tiles, chunkings and the three-product layers a small batch never launches),
    against the reference's own decode of it; two more rows against a batch-of-2 engine."""
    torch = _torch()
    L, B = 64000, 256
    F = load_golden('full_dccrn_snr')
    base = synth.synth_batch(16, 'speech', L, seed0=700)
    x = np.tile(base, (B // 16, 1)).copy()
    x[3::16] = synth.synth_clip(77, 'white', L)
    x[1::16] *= 0.37
    row = 5 + 16 * ((B // 16) // 2)
    x[row] = synth.synth_clip(int(F['seed']), 'speech', L)
    big = _model('clstm', max_batch=B, max_samples=L, p_in=0.5, p_out=2.0)
    xt = torch.from_numpy(x).cuda()
    y = big.enhance_batch(xt)
    assert bool(torch.isfinite(y).all()) and tuple(y.shape) == (B, L)
    ok, info = _wave_ok(y[row].cpu().numpy(), F['enh4_cprs'])
    print('dccrn_snr B 256 fixture row', row, 'rms err, rms ref', info)
    assert ok, info
    small = _model('clstm', max_batch=2, max_samples=L, p_in=0.5, p_out=2.0)
    for k in (0, B - 2):
        ys = small.enhance_batch(xt[k:k + 2])
        for j in (0, 1):
            r = ys[j].cpu().numpy()
            assert rms(y[k + j].cpu().numpy() - r) < 2e-5 * max(rms(r), 1e-4), k + j


# ------------------------------------------------------------------------------------------------ frame-online
def _push_all(eng, xt, pieces, L):
    """Push `pieces` (then the rest in pieces of the last size), flush; -> (the per-call outputs, samples fed after each push)."""
    outs, fed, pos = [], [], 0
    k = 0
    while pos < L:
        n = min(pieces[min(k, len(pieces) - 1)], L - pos)
        outs.append(eng.stream_push(xt[:, pos:pos + n].contiguous()).cpu().numpy())
        pos += n
        fed.append(pos)
        k += 1
    outs.append(eng.stream_flush().cpu().numpy())
    return outs, fed


def _final_samples(n_total, lag):
    """Samples that are final once n_total have arrived: frame t is complete when sample t * hop + n_fft / 2 is there, an estimate
    frame is final `lag` frames later, a sample when every frame that covers it is (engine.hip: se_stream_push)."""
    t_avail = (n_total - N_FFT // 2 - 1) // HOP + 1 if n_total > N_FFT // 2 else 0
    return max(0, min(n_total, (t_avail - lag) * HOP - N_FFT // 2))


@pytest.mark.parametrize('core', list(CORES))
@pytest.mark.parametrize('pieces,chunk', [([160], 1), ([37, 1000, 3, 481, 2000], 4), ([4000], 16), ([7777, 160], 5)])
def test_streamed_output_equals_offline(core, pieces, chunk):
    torch = _torch()
    L, B = 12000, 2
    m = _model(core, max_batch=B, max_samples=L)
    x = np.stack([synth.synth_clip(800 + b, 'speech' if b % 2 == 0 else 'white', L) for b in range(B)])
    xt = torch.from_numpy(x).cuda()
    ref = m.enhance_batch(xt).cpu().numpy()
    eng = m.engine
    eng.stream_begin(B, c=eng.rms_scale(xt), max_chunk_frames=chunk)
    outs, fed = _push_all(eng, xt, pieces, L)
    got = np.concatenate(outs, axis=1)
    assert got.shape == ref.shape == (B, L), (got.shape, ref.shape)
    e = rms(got - ref)
    print('dccrn_snr', core, pieces, chunk, 'streamed vs offline rms err', e, 'rms ref', rms(ref))
    assert e < 1e-6 + 2e-5 * rms(ref), (core, e, rms(ref))
    done = 0
    for n_total, o in zip(fed, outs):           # every push returns exactly what is final without look-ahead
        want = max(done, _final_samples(n_total, 0))
        assert o.shape[1] == want - done, (n_total, o.shape[1], want - done)
        done = want


def test_compressed_exponents_ragged_end_and_second_stream():
    """Exponents 0.5 / 2.0, a length that is no hop multiple (the script zero-pads the tail and cuts the result back to the clip,
    dccrn_decode_snr.py:37-40,66), three rows; then a second stream on the same engine starts from zero state again."""
    torch = _torch()
    L, B = 9001, 3
    m = _model('clstm', max_batch=B, max_samples=L, p_in=0.5, p_out=2.0)
    x = np.stack([synth.synth_clip(800 + b, 'speech' if b % 2 == 0 else 'white', L) for b in range(B)])
    xt = torch.from_numpy(x).cuda()
    ref = m.enhance_batch(xt).cpu().numpy()
    eng = m.engine
    for pieces, chunk in (([1234], 8), ([4000, 37, 3], 3)):
        eng.stream_begin(B, c=eng.rms_scale(xt), max_chunk_frames=chunk)
        outs, _ = _push_all(eng, xt, pieces, L)
        got = np.concatenate(outs, axis=1)
        assert got.shape == ref.shape == (B, L) and rms(got - ref) < 1e-6 + 2e-5 * rms(ref), (pieces, rms(got - ref), rms(ref))


@pytest.mark.parametrize('core', ['clstm', 'rlstm256'])
def test_long_stream_equals_offline(core):
    """10 s (T = 1251) in 40 ms pushes: the four history columns of every tensor are rewritten 300 times."""
    torch = _torch()
    L = 160000
    m = _model(core, max_batch=1, max_samples=L)
    xt = torch.from_numpy(synth.synth_clip(880, 'speech', L)[None]).cuda()
    ref = m.enhance_batch(xt).cpu().numpy()
    eng = m.engine
    eng.stream_begin(1, c=eng.rms_scale(xt), max_chunk_frames=4)
    outs, _ = _push_all(eng, xt, [640], L)
    got = np.concatenate(outs, axis=1)
    assert got.shape == ref.shape == (1, L)
    e = rms(got - ref)
    print('dccrn_snr', core, '10 s stream vs offline rms err', e, 'rms ref', rms(ref))
    assert e < 1e-6 + 2e-5 * rms(ref)


@pytest.mark.parametrize('pieces,chunk', [([160], 1), ([37, 1000, 3, 481, 2000], 4), ([128], 16)])
def test_no_look_ahead_samples_arrive_six_frames_earlier(pieces, chunk):
    """After every push the engine returns min(n_total, t_avail hop - n_fft / 2) - o_done samples with lag 0; the `_vb` DCCRN
    (DCCRN_cprs.py:199: one frame of look-ahead per decoder layer) returns the same with t_avail - 6.  Both counted side by side on
    the same pushes: from the point on where the `_vb` engine has returned anything, this one is 6 x 128 samples ahead."""
    torch = _torch()
    from se_amd.models import DCCRN
    L, B = 8000, 2
    x = np.stack([synth.synth_clip(800 + b, 'speech', L) for b in range(B)])
    xt = torch.from_numpy(x).cuda()
    snr = _model('clstm', max_batch=B, max_samples=L).engine
    vb = DCCRN(masking_mode='E', **CL, max_batch=B, max_samples=L).load_synthetic(14).engine
    assert snr.output_samples(L) == L and vb.output_samples(L) == -(-L // HOP) * HOP
    counts = {}
    for name, eng in (('snr', snr), ('vb', vb)):
        eng.stream_begin(B, c=eng.rms_scale(xt), max_chunk_frames=chunk)
        outs, fed = _push_all(eng, xt, pieces, L)
        counts[name] = (np.cumsum([o.shape[1] for o in outs[:-1]]), fed, outs[-1].shape[1])
    (c_snr, fed, fl_snr), (c_vb, fed_vb, fl_vb) = counts['snr'], counts['vb']
    assert fed == fed_vb
    ahead = 0
    for n_total, a, b in zip(fed, c_snr, c_vb):
        assert a == _final_samples(n_total, 0), (n_total, a, _final_samples(n_total, 0))
        assert b == _final_samples(n_total, 6), (n_total, b, _final_samples(n_total, 6))
        if b > 0:
            assert a - b == 6 * HOP, (n_total, a, b)
            ahead += 1
    assert ahead > 0
    assert c_snr[-1] + fl_snr == L and c_vb[-1] + fl_vb == vb.output_samples(L)
    # the latency that is left: a sample is final when the last frame that covers it is complete - half a window ahead of it,
    # up to one hop for that frame's position and up to one hop until its last sample has arrived
    assert all(n - a <= N_FFT // 2 + 2 * HOP for n, a in zip(fed, c_snr) if n >= N_FFT)


# ------------------------------------------------------------------------------------------------ poisoned arena, driver
_POISON = r'''
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
import se_amd
from se_amd import synth
from se_amd.models import DCCRN_SNR
L, B = 12000, 2
rms = lambda a: float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))
x = np.stack([synth.synth_clip(860 + b, 'speech', L) for b in range(B)])
xt = torch.from_numpy(x).cuda()
for ctor, seed in ((dict(rnn_units=256, use_clstm=True, kernel_num=[32, 64, 128, 256, 256, 256]), 14), (dict(rnn_units=128), 24)):
    m = DCCRN_SNR(**ctor, max_batch=B, max_samples=L).load_synthetic(seed)
    ref = m.enhance_batch(xt).cpu().numpy()                                    # offline
    assert ref.shape == (B, L) and np.isfinite(ref).all(), ctor
    lengths = [L, 9001]                                                        # ragged: another carve of the same arena
    rag = m.enhance_ragged(xt, lengths).cpu().numpy()
    assert np.isfinite(rag).all(), ctor
    one = m.enhance_batch(xt[1:2, :9001].contiguous()).cpu().numpy()[0]
    assert np.isfinite(one).all(), ctor
    assert rms(rag[0] - ref[0]) < 1e-4 and rms(rag[0] - ref[0]) < 2e-5 * rms(ref[0]), (ctor, rms(rag[0] - ref[0]))
    assert rms(rag[1, :9001] - one) < 1e-4 and rms(rag[1, :9001] - one) < 2e-5 * rms(one) and not rag[1, 9001:].any(), ctor
    eng = m.engine
    for chunk in (1, 16):                                                      # thin and MFMA paths, windows re-carved
        eng.stream_begin(B, c=eng.rms_scale(xt), max_chunk_frames=chunk)
        outs = [eng.stream_push(xt[:, p:p + 4000].contiguous()).cpu().numpy() for p in range(0, L, 4000)]
        outs.append(eng.stream_flush().cpu().numpy())
        got = np.concatenate(outs, axis=1)
        assert got.shape == ref.shape and np.isfinite(got).all(), (ctor, chunk)
        assert rms(got - ref) < 1e-6 + 2e-5 * rms(ref), (ctor, chunk, rms(got - ref))
print('POISON-OK')
'''


def test_poisoned_arena_never_reaches_an_output():
    """SE_ARENA_POISON=1 (tests/test_gpu_poison.py): one offline, one ragged and one streamed decode of both cores - a stale column
    of the four-column history window, or a tail nobody zeroes any more, would come out as NaN."""
    env = dict(os.environ, SE_ARENA_POISON='1')
    r = subprocess.run([sys.executable, '-c', _POISON, ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'POISON-OK' in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_decode_driver_grid_cell(tmp_path):
    """se_amd.decode.enhance(args, 'dccrn_snr'): <mix>/<noise_type>/<seen>/<snr>/ in, the same sub-tree out (dccrn_decode_snr.py:
    20-27), every file as long as its clip (:66) and equal to the engine's decode of it; clips of three lengths share calls."""
    torch = _torch()
    from se_amd import decode, wavio
    mix, out = tmp_path / 'mix', tmp_path / 'esti'
    cell = os.path.join('cafe', 'seen', '-5')
    os.makedirs(str(mix / cell))
    clips = {}
    for i, L in enumerate((4000, 6001, 5000)):
        name = f'utt_{i:03d}.wav'
        wavio.write_wav_pcm16(str(mix / cell / name), synth.synth_clip(60 + i, 'speech', L), 16000)
        clips[name] = wavio.read_wav(str(mix / cell / name))[0]
    sd = synth.synth_state_dict(schemas.SCHEMAS['dccrn_snr'](), 14)
    args = types.SimpleNamespace(mix_file_path=str(mix), esti_clean_file_path=str(out), fs=16000, noise_type='cafe', seen='seen',
                                 snr='-5')
    assert decode.enhance(args, 'dccrn_snr', state_dict=sd, max_batch=4, max_pad=0.5) == 3
    assert sorted(os.listdir(str(out / cell))) == sorted(clips)
    m = _model('clstm', max_batch=1, max_samples=6001)
    for name, x in clips.items():
        y = wavio.read_wav(str(out / cell / name))[0]
        ref = m.enhance_batch(torch.from_numpy(np.asarray(x, np.float32)[None].copy()).cuda()).cpu().numpy()[0]
        assert len(y) == len(x) == len(ref)
        assert rms(y - ref) < 1e-4 + 5e-4 * rms(ref), (name, rms(y - ref))
