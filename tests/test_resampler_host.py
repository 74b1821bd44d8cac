"""Host side of the stateful resampler (se_resampler_*, no GPU): `se_resampler_ready_samples` - how many output samples are
final once n_in input samples of a signal that has not ended have arrived - against a brute-force count made here from the
oracle's read positions (oracle.resample.time_registers) and the filter's tap reach ceil(32769 / index_step): output t, read at
position treg[t], is final when its position lies before n_in - reach, i.e. when sample int(treg[t]) + reach has arrived (so a
signal of `reach` samples releases nothing before it ends).  Plus what the Python layer decides before
the library is called: the binding lists the new entry points, StreamResampler refuses CPU tensors and wrong dtypes."""
import math

import numpy as np
import pytest

import se_amd  # noqa: F401
from se_amd import _lib
from se_amd import resample as HR
from oracle import resample as R

RATIOS = [(48000, 16000), (32000, 16000), (44100, 16000), (16000, 48000), (16000, 16000)]
LENGTHS = [0, 1, 192, 193, 194, 579, 4801]
NEW_SYMBOLS = ['se_resampler_create', 'se_resampler_destroy', 'se_resampler_begin', 'se_resampler_push', 'se_resampler_flush',
               'se_resampler_ready_samples']


def _reach(sr_in, sr_out):
    ratio = float(sr_out) / sr_in
    index_step = int(min(1.0, ratio) * 2 ** R.PRECISION)
    nwin = R.NUM_ZEROS * 2 ** R.PRECISION + 1
    assert nwin == 32769
    return math.ceil(nwin / index_step)


def _brute_ready(n_in, sr_in, sr_out):
    """outputs whose position lies before n_in - reach, and the positions (for the caller's own checks)"""
    if sr_in == sr_out:
        return n_in, None
    ratio = float(sr_out) / sr_in
    treg = R.time_registers(int(n_in * ratio) + 2, ratio)
    final = treg.astype(np.int64) + _reach(sr_in, sr_out) < n_in
    return int(final.sum()), treg


def test_binding_declares_the_entry_points():
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS
    lib = _lib.load()
    assert len(lib.se_resampler_create.argtypes) == 5 and len(lib.se_resampler_push.argtypes) == 8
    assert len(lib.se_resampler_flush.argtypes) == 5 and len(lib.se_resampler_ready_samples.argtypes) == 3
    assert lib.se_abi_version() == 5


def test_reach_at_the_rates_a_live_source_has():
    assert _reach(48000, 16000) == 193 and _reach(32000, 16000) == 129 and _reach(44100, 16000) == 178
    assert _reach(16000, 48000) == 65


@pytest.mark.parametrize('sr_in,sr_out', RATIOS)
def test_ready_samples_against_brute_force(sr_in, sr_out):
    ratio = float(sr_out) / sr_in
    for n_in in LENGTHS:
        want, treg = _brute_ready(n_in, sr_in, sr_out)
        got = HR.ready_samples(n_in, sr_in, sr_out)
        assert got == want, (sr_in, sr_out, n_in, got, want)
        assert got <= int(n_in * ratio)
        if treg is not None and got:
            # reached exactly by n_in - reach: the last final output reads before it, the next one at it or behind it
            reach = _reach(sr_in, sr_out)
            assert int(treg[got - 1]) < n_in - reach <= int(treg[got])
        if treg is not None and n_in <= _reach(sr_in, sr_out):
            assert got == 0


@pytest.mark.parametrize('sr_in,sr_out', RATIOS)
def test_ready_samples_is_monotone(sr_in, sr_out):
    ratio = float(sr_out) / sr_in
    got = [HR.ready_samples(n, sr_in, sr_out) for n in range(0, 1200)]
    assert all(b >= a for a, b in zip(got, got[1:]))
    assert all(g <= int(n * ratio) for n, g in enumerate(got))
    want = [_brute_ready(n, sr_in, sr_out)[0] for n in range(0, 1200, 37)]
    assert got[::37] == want
    # one more input sample releases at most ceil(ratio) + 1 outputs
    assert max(b - a for a, b in zip(got, got[1:])) <= math.ceil(ratio) + 1


def test_ready_samples_refuses_bad_arguments():
    assert HR.ready_samples(-1, 48000, 16000) == -1
    assert HR.ready_samples(10, 0, 16000) == -1 and HR.ready_samples(10, 48000, 0) == -1


def _bare_resampler():
    """a StreamResampler that never reached the library: what push() decides on its own must not need one"""
    r = object.__new__(HR.StreamResampler)
    r.sr_in, r.sr_out, r.max_batch, r.max_push, r.device = 48000, 16000, 1, 480, 0
    r._batch, r._n_in, r._n_out, r._h = 1, 0, 0, None

    class _NoLib:
        def __getattr__(self, name):
            raise AssertionError(f'the library was called ({name}) with a tensor push() has to refuse')
    r._lib = _NoLib()
    return r


def test_stream_resampler_refuses_cpu_tensors_and_wrong_dtypes():
    import torch
    r = _bare_resampler()
    with pytest.raises(AssertionError, match='^$'):              # the plain assert of resample(), not the library's
        r.push(torch.zeros(1, 480))                              # CPU tensor
    with pytest.raises(AssertionError, match='^$'):
        r.push(torch.zeros(480))
    with pytest.raises(AssertionError, match='^$'):
        HR.resample(torch.zeros(1, 480), 48000)                  # the rule it follows

    class _FakeCuda:                                             # a cuda tensor as far as the checks look
        is_cuda = True

        def __init__(self, dtype, shape, strides):
            self.dtype, self.shape, self._st = dtype, shape, strides

        def dim(self):
            return len(self.shape)

        def stride(self, i=None):
            return self._st if i is None else self._st[i]
    for bad in (_FakeCuda(torch.float64, (1, 480), (480, 1)), _FakeCuda(torch.int16, (1, 480), (480, 1)),
                _FakeCuda(torch.float32, (1, 480), (960, 2)), _FakeCuda(torch.float32, (1, 2, 480), (960, 480, 1))):
        with pytest.raises(AssertionError, match='^$'):
            r.push(bad)
