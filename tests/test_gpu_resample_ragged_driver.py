"""GPU: the file -> file driver (se_amd/decode.py) resamples a staged call, and a group of long clips, of one rate with ONE
se_resample_ragged call straight from the uploaded samples - and writes the bytes it wrote when it resampled clip by clip.  The
reference files are made here from the project's own pieces, one clip at a time: se_pcm16_decode + se_resample, then the engine call
the driver makes for the same rows and se_pcm16_encode.  The calls are counted by wrapping the library's functions."""
import ctypes as C
import os
import types

import numpy as np
import pytest

import se_amd  # noqa: F401
from se_amd import _lib, decode, resample, schemas, synth, wavio

pytestmark = pytest.mark.gpu

COUNTED = ('se_resample_ragged', 'se_resample', 'se_pcm16_decode')


def _write_dir(mix, clips):
    os.makedirs(mix)
    for k, (n, rate) in enumerate(clips):
        wavio.write_wav_pcm16(os.path.join(mix, f'p{232 + k}_{k:03d}.wav'), synth.synth_clip(140 + k, 'speech', n), rate)


def _counted(fn):
    """run fn() with the library's resampling entry points wrapped: -> (its result, calls per entry point)"""
    lib = _lib.load()
    calls = {name: 0 for name in COUNTED}
    orig = {name: getattr(lib, name) for name in COUNTED}

    def wrap(name):
        def f(*a):
            calls[name] += 1
            return orig[name](*a)
        return f

    for name in COUNTED:
        setattr(lib, name, wrap(name))
    try:
        return fn(), calls
    finally:
        for name in COUNTED:
            setattr(lib, name, orig[name])


def _pieces(mix, out_dir, max_batch, max_seconds=None, long_batch=1):
    """The directory decoded from the project's pieces, every clip resampled alone: the plan, the engine and the engine calls are the
    driver's (decode.plan_*), so the files differ from the driver's only if the resampled rows do."""
    import torch
    lib = _lib.load()
    dev = torch.device('cuda', torch.cuda.current_device())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    os.makedirs(out_dir)
    files = os.listdir(mix)
    info = [wavio.wav_info(os.path.join(mix, f)) for f in files]
    native, rates = [i[0] for i in info], [i[1] for i in info]
    lengths = [n if fs == 16000 else resample.resample_samples(n, fs, 16000) for n, fs in zip(native, rates)]
    own = decode.shard_clips(lengths, 0, 1)
    eng_samples, fit, over = decode.plan_long([lengths[i] for i in own], max_seconds)
    long_own, short_own = [own[k] for k in over], [own[k] for k in fit]
    groups = [[long_own[k] for k in g] for g in decode.plan_long_groups([lengths[i] for i in long_own], min(long_batch, max_batch))]
    mine = [[short_own[k] for k in b] for b in decode.plan_batches([lengths[i] for i in short_own], max_batch, max_batch * 64000, True)]
    eng_len = max(lengths[i] for b in mine for i in b)
    sd = synth.synth_state_dict(schemas.crn_schema(), 12)
    eng = decode._build('crn', None, sd, device=dev.index, max_batch=max(len(b) for b in mine + groups),
                        max_samples=max(eng_samples if long_own else eng_len, 512), p_in=None, p_out=None).engine

    def clip16k(i, raw):
        """clip i at 16 kHz: raw PCM_16 -> se_pcm16_decode (or the host's floats, as the long path reads them) -> se_resample"""
        path = os.path.join(mix, files[i])
        if raw:
            q = torch.from_numpy(np.fromfile(path, dtype='<i2', count=native[i], offset=info[i][5]).copy()).to(dev)
            nat = torch.empty(native[i], dtype=torch.float32, device=dev)
            assert lib.se_pcm16_decode(p(q), native[i], 1, native[i], p(nat), native[i], st) == 0
        else:
            nat = torch.from_numpy(np.ascontiguousarray(wavio.read_wav(path)[0], dtype=np.float32)).to(dev)
        if rates[i] == 16000:
            return nat
        wav = torch.empty(lengths[i], dtype=torch.float32, device=dev)
        assert lib.se_resample(p(nat), native[i], 1, native[i], rates[i], 16000, p(wav), lengths[i], st) == 0
        return wav

    def finish(b, out):
        nb, n = out.shape
        q = torch.empty((nb, n), dtype=torch.int16, device=dev)
        assert lib.se_pcm16_encode(p(out), n, nb, n, p(q), n, st) == 0
        q = q.cpu().numpy()
        for r, i in enumerate(b):
            decode._write_clip(os.path.join(out_dir, files[i]), q[r, :eng.output_samples(lengths[i])], 16000)

    for raw, calls in ((True, mine), (False, groups)):
        for b in calls:
            lens = [lengths[i] for i in b]
            rows = torch.zeros((len(b), max(lens)), dtype=torch.float32, device=dev)
            for r, i in enumerate(b):
                rows[r, :lengths[i]] = clip16k(i, raw)
            if not raw:
                finish(b, eng.enhance_long(rows) if len(b) == 1 else eng.enhance_long_ragged(rows, lens))
            else:
                finish(b, eng.enhance_batch(rows) if min(lens) == max(lens) else eng.enhance_ragged(rows, lens))
    torch.cuda.synchronize()
    return len(mine), len(groups)


def _same_files(a, b, count):
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) and len(os.listdir(a)) == count
    for f in os.listdir(a):
        assert open(os.path.join(a, f), 'rb').read() == open(os.path.join(b, f), 'rb').read(), f


def _drive(mix, out, **kw):
    sd = synth.synth_state_dict(schemas.crn_schema(), 12)
    args = types.SimpleNamespace(mix_file_path=mix, esti_clean_file_path=out, fs=16000)
    stats = {}
    (n, calls) = _counted(lambda: decode.enhance(args, 'crn', state_dict=sd, verbose=False, stats=stats, **kw))
    return n, calls, stats


@pytest.mark.parametrize('rate,natives', [(48000, [14403, 12000, 17999, 12001, 15000]), (44100, [11025, 9001, 13000, 9002])])
def test_a_directory_of_one_rate_makes_one_ragged_call_per_staged_batch(tmp_path, rate, natives):
    mix, out, ref = str(tmp_path / 'noisy'), str(tmp_path / 'enh'), str(tmp_path / 'ref')
    _write_dir(mix, [(n, rate) for n in natives])
    n, calls, stats = _drive(mix, out, max_batch=3)
    assert n == len(natives) and stats['raw_pcm16'] and stats['calls_rank'] >= 2
    # one call per staged batch, from the 2-byte samples: no clip-by-clip call and no float copy in front of it
    assert calls == {'se_resample_ragged': stats['calls_rank'], 'se_resample': 0, 'se_pcm16_decode': 0}, (calls, stats)
    assert _pieces(mix, ref, max_batch=3) == (stats['calls_rank'], 0)
    _same_files(out, ref, len(natives))


def test_a_call_that_mixes_rates_keeps_the_clip_by_clip_path(tmp_path):
    mix, out, ref = str(tmp_path / 'noisy'), str(tmp_path / 'enh'), str(tmp_path / 'ref')
    _write_dir(mix, [(4000, 16000), (12300, 48000), (4200, 16000), (12900, 48000)])      # 4000 ... 4300 samples at 16 kHz: one call
    n, calls, stats = _drive(mix, out, max_batch=4)
    assert n == 4 and stats['calls_rank'] == 1
    assert calls == {'se_resample_ragged': 0, 'se_resample': 2, 'se_pcm16_decode': 1}, calls
    assert _pieces(mix, ref, max_batch=4) == (1, 0)
    _same_files(out, ref, 4)


def test_a_group_of_long_clips_of_one_rate_is_resampled_by_one_call(tmp_path):
    mix, out, ref = str(tmp_path / 'noisy'), str(tmp_path / 'enh'), str(tmp_path / 'ref')
    _write_dir(mix, [(12000, 48000), (120000, 48000), (14403, 48000), (126001, 48000)])    # two above 2 s: 40000 and 42001 at 16 kHz
    n, calls, stats = _drive(mix, out, max_batch=2, max_seconds=2, long_batch=2)
    assert n == 4 and stats['long_clips'] == 2 and stats['long_calls'] == 1 and stats['calls_rank'] == 1, stats
    assert calls == {'se_resample_ragged': 2, 'se_resample': 0, 'se_pcm16_decode': 0}, calls
    assert _pieces(mix, ref, max_batch=2, max_seconds=2, long_batch=2) == (1, 1)
    _same_files(out, ref, 4)
