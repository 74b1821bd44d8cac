"""GPU: se_resample_ragged (include/se_engine.h; csrc/k_resample.hip, csrc/resample_ragged.h) - rows of different lengths resampled in
one call.  The contract is equality: row b of the call holds, bit for bit, what se_resample returns for that clip alone (for PCM_16
input: se_pcm16_decode followed by se_resample), then zeros up to the longest row's output; nothing past a row's length is read and
nothing past the longest row's output is written.  The row lengths are the smallest at which the kernel can go wrong: the first
samples, both filter wings clamped, the zero tail present and absent, the edges of an output block and of a launch's rows."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

import se_amd  # noqa: F401
from se_amd import _lib
from se_amd import resample as HR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HDR = open(os.path.join(ROOT, 'sixty-years-of-frequency-domain-monaural-speech-enhancement_amd', 'csrc', 'resample_ragged.h')).read()
ROWS = int(re.search(r'RS_RAGGED_ROWS = (\d+)', _HDR).group(1))        # rows one launch carries
BLOCK = int(re.search(r'RS_RAGGED_BLOCK = (\d+)', _HDR).group(1))      # outputs one block computes
RATES = [48000, 32000, 44100, 22050, 8000, 16000]
FORMATS = ['f32', 's16']
SENTINEL = 12345                                                       # behind an int16 row, where NaN cannot be stored


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _reach(sr):
    """the taps one filter wing can span (csrc/resample_pos.h): 193 at 48 -> 16 kHz"""
    step = int(min(1.0, 16000.0 / sr) * 512)
    return (64 * 512 + 1) // step + 1


def _n_out(n, sr):
    return n if sr == 16000 else int(math.ceil(n * (16000.0 / sr)))


def _with_outputs(sr, want, below=False):
    """the shortest row whose output has `want` samples; where no row has (8 -> 16 kHz makes even counts only) the nearest count
    above, or below, it"""
    n = max(1, int(want * sr / 16000.0) - 3)
    while _n_out(n, sr) < want:
        n += 1
    return n - 1 if below and _n_out(n, sr) > want else n


def _lengths(sr):
    r = _reach(sr)
    q = sr // math.gcd(sr, 16000)                      # rows of k * q samples have no zero tail
    tile = BLOCK * int(math.ceil(sr / 16000.0)) + 2 * r      # the input span of one block of outputs
    return [1, 2, 3, 4, r - 1, r, r + 1, 2 * r + 1, 5 * q, 5 * q + 1, _with_outputs(sr, 2 * BLOCK - 1, below=True), _with_outputs(sr, 2 * BLOCK + 1),
            _with_outputs(sr, BLOCK), 2 * tile + 7]


def _row(n, fmt):
    """the samples of a row of n, a function of n alone (so every test that meets the row meets the same reference)"""
    rng = np.random.default_rng(1000 + n)
    if fmt == 'f32':
        return (0.1 * rng.standard_normal(n)).astype(np.float32)
    x = rng.integers(-32768, 32768, n, dtype=np.int16)
    x[0] = -32768
    x[-1] = 32767 if n > 1 else x[-1]
    return x


@functools.lru_cache(maxsize=None)
def _alone(sr, n, fmt):
    """se_resample of the row alone (PCM_16: behind se_pcm16_decode): computed once, shared, never written to"""
    torch = _torch()
    lib = _lib.load()
    x = torch.from_numpy(_row(n, fmt)).cuda()
    if fmt == 's16':
        f = torch.empty(n, dtype=torch.float32, device='cuda')
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert lib.se_pcm16_decode(C.c_void_p(x.data_ptr()), n, 1, n, C.c_void_p(f.data_ptr()), n, st) == 0
        x = f
    y = HR.resample(x, sr, 16000).cpu().numpy().copy()
    assert y.shape == (_n_out(n, sr),)
    y.setflags(write=False)
    return y


def _pack(lens, fmt, poison=True, extra=5):
    """[B, max + extra] rows, poisoned (or zero) behind every row's length"""
    pitch = max(lens) + extra
    if fmt == 'f32':
        x = np.full((len(lens), pitch), np.nan if poison else 0.0, dtype=np.float32)
    else:
        x = np.full((len(lens), pitch), SENTINEL if poison else 0, dtype=np.int16)
    for b, n in enumerate(lens):
        x[b, :n] = _row(n, fmt)
    return x


def _check_rows(y, lens, sr, fmt):
    top = _n_out(max(lens), sr)
    assert y.shape == (len(lens), top)
    for b, n in enumerate(lens):
        ref = _alone(sr, n, fmt)
        assert np.array_equal(y[b, :len(ref)], ref), (sr, fmt, b, n, np.abs(y[b, :len(ref)] - ref).max())
        assert not y[b, len(ref):].any() and not np.signbit(y[b, len(ref):]).any(), (sr, fmt, b, n)      # exact zeros up to the bound


def _ragged(x, lens, sr, **kw):
    torch = _torch()
    return HR.resample_ragged(torch.from_numpy(x).cuda(), lens, sr, 16000, **kw).cpu().numpy()


@pytest.mark.parametrize('fmt', FORMATS)
@pytest.mark.parametrize('where', ['first', 'middle', 'last'])
@pytest.mark.parametrize('sr', RATES)
def test_every_row_equals_resample_of_the_row_alone(sr, where, fmt):
    lens = _lengths(sr)
    longest = max(lens)
    lens.remove(longest)
    lens.insert({'first': 0, 'middle': len(lens) // 2, 'last': len(lens)}[where], longest)
    _check_rows(_ragged(_pack(lens, fmt), lens, sr), lens, sr, fmt)


@pytest.mark.parametrize('fmt', FORMATS)
@pytest.mark.parametrize('sr', RATES)
def test_batches_of_one_three_and_one_more_than_a_launch(sr, fmt):
    base = _lengths(sr)
    for lens in ([base[0]], [base[-1]], [base[9]], base[7:10], [base[k % len(base)] for k in range(ROWS + 1)]):
        _check_rows(_ragged(_pack(lens, fmt), lens, sr), lens, sr, fmt)
    # the row behind the launch's last is a row of its own: the longest of the call, alone in the second launch
    lens = [base[k % 8] for k in range(ROWS)] + [base[-1]]
    _check_rows(_ragged(_pack(lens, fmt), lens, sr), lens, sr, fmt)


@pytest.mark.parametrize('sr', RATES)
def test_every_row_within_2e_7_of_the_oracle(sr):
    from oracle import resample as R
    lens = _lengths(sr)
    y = _ragged(_pack(lens, 'f32'), lens, sr)
    for b, n in enumerate(lens):
        ref = R.librosa_resample(_row(n, 'f32').astype(np.float64), sr, 16000)
        err = np.abs(y[b, :len(ref)] - ref).max()
        assert len(ref) == _n_out(n, sr) and err < 2e-7, (sr, n, err)       # the bar tests/test_resample.py sets for se_resample


@pytest.mark.parametrize('fmt', FORMATS)
@pytest.mark.parametrize('sr', [48000, 44100, 16000])
def test_nothing_past_a_row_is_read_and_nothing_past_the_bound_is_written(sr, fmt):
    torch = _torch()
    lens = _lengths(sr)[4:]
    clean = _ragged(_pack(lens, fmt, poison=False), lens, sr)
    poisoned = _ragged(_pack(lens, fmt, poison=True), lens, sr)
    assert clean.tobytes() == poisoned.tobytes() and np.isfinite(poisoned).all()
    top = _n_out(max(lens), sr)
    out = torch.full((len(lens), top + 300), float('nan'), dtype=torch.float32, device='cuda')
    got = HR.resample_ragged(torch.from_numpy(_pack(lens, fmt)).cuda(), lens, sr, 16000, out=out)
    assert got.data_ptr() == out.data_ptr() and got.shape == (len(lens), top)
    full = out.cpu().numpy()
    assert np.isnan(full[:, top:]).all()
    _check_rows(full[:, :top], lens, sr, fmt)          # (the zeros between a row's output and the bound included)


def _call(lib, x, fmt, in_pitch, batch, lens, sr_in, sr_out, out, out_pitch):
    torch = _torch()
    arr = (C.c_int32 * len(lens))(*lens) if lens is not None else None
    rc = lib.se_resample_ragged(C.c_void_p(x.data_ptr()) if x is not None else None, fmt, in_pitch, batch, arr, sr_in, sr_out,
                                C.c_void_p(out.data_ptr()) if out is not None else None, out_pitch,
                                C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, lib.se_last_error(None).decode()


def test_every_refusal_has_its_reason_and_leaves_the_output_alone():
    torch = _torch()
    lib = _lib.load()
    lens = [100, 4801, 7]
    x = torch.from_numpy(_pack(lens, 'f32', extra=0)).cuda()
    out = torch.full((3, 1601), 7.0, dtype=torch.float32, device='cuda')
    ok = (x, 0, 4801, 3, lens, 48000, 16000, out, 1601)

    def refused(reason, **kw):
        a = dict(zip(('x', 'fmt', 'in_pitch', 'batch', 'lens', 'sr_in', 'sr_out', 'out', 'out_pitch'), ok))
        a.update(kw)
        rc, err = _call(lib, a['x'], a['fmt'], a['in_pitch'], a['batch'], a['lens'], a['sr_in'], a['sr_out'], a['out'], a['out_pitch'])
        assert rc != 0 and 'se_resample_ragged: ' + reason in err, (reason, rc, err)

    refused('null argument', x=None)
    refused('null argument', out=None)
    refused('null argument', lens=None)
    refused('batch 0', batch=0)
    refused('batch -2', batch=-2)
    refused('n_in[2] = 0', lens=[100, 4801, 0])
    refused('n_in[0] = -5', lens=[-5, 4801, 7])
    refused('in_format 2', fmt=2)
    refused('in_format -1', fmt=-1)
    refused('sample rates 0 -> 16000', sr_in=0)
    refused('sample rates 48000 -> -1', sr_out=-1)
    refused('in_pitch 4800 is below the longest row (4801', in_pitch=4800)
    refused("out_pitch 1600 is below the longest row's output (1601", out_pitch=1600)
    refused('n_in[0] = 1073741824: the row\'s output would pass 2147483647', batch=1, lens=[2 ** 30], sr_in=8000)
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    rc, err = _call(lib, *ok)                              # the same arguments, none bent: accepted
    assert rc == 0, err
    _check_rows(out.cpu().numpy(), lens, 48000, 'f32')


def test_two_hip_streams_while_the_position_table_grows_and_se_resample_is_unchanged():
    """44.1 kHz: the table of read positions is shared by every call at the ratio.  The second call, on another hipStream, is longer than
    anything this module resamples at the rate, so the table is replaced while the first call may still be running."""
    torch = _torch()
    la, lb = [30011, 2000, 17], [5, 90001, 44100, 64007]
    x9 = torch.from_numpy(_row(9001, 'f32')).cuda()
    before = HR.resample(x9, 44100)
    xa, xb = torch.from_numpy(_pack(la, 'f32')).cuda(), torch.from_numpy(_pack(lb, 's16')).cuda()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        ya = HR.resample_ragged(xa, la, 44100)
    with torch.cuda.stream(s2):
        yb = HR.resample_ragged(xb, lb, 44100)
    with torch.cuda.stream(s1):
        ya2 = HR.resample_ragged(xa, la, 44100)            # behind the growth: the longer table, the same positions
    torch.cuda.synchronize()
    assert torch.equal(ya, ya2)
    _check_rows(ya.cpu().numpy(), la, 44100, 'f32')
    _check_rows(yb.cpu().numpy(), lb, 44100, 's16')
    assert torch.equal(HR.resample(x9, 44100), before)             # se_resample gives what it gave before the ragged calls


def test_the_output_feeds_enhance_ragged_as_it_is():
    torch = _torch()
    from se_amd import decode, schemas, synth
    native = [14403, 12000, 17999]
    lens = [_n_out(n, 48000) for n in native]
    sd = synth.synth_state_dict(schemas.crn_schema(), 12)
    eng = decode._build('crn', None, sd, device=torch.cuda.current_device(), max_batch=3, max_samples=max(lens), p_in=None, p_out=None).engine
    x = np.zeros((3, max(native)), dtype=np.float32)
    for b, n in enumerate(native):
        x[b, :n] = synth.synth_clip(95 + b, 'speech', n)
    xt = torch.from_numpy(x).cuda()
    together = HR.resample_ragged(xt, native, 48000)
    one_by_one = torch.full((3, max(lens)), float('nan'), dtype=torch.float32, device='cuda')
    for b, n in enumerate(native):
        one_by_one[b, :lens[b]] = HR.resample(xt[b, :n].contiguous(), 48000)
    a = eng.enhance_ragged(together, lens).cpu().numpy()
    b = eng.enhance_ragged(one_by_one, lens).cpu().numpy()
    assert np.isfinite(a).all() and a.any() and a.tobytes() == b.tobytes()
