"""CPU: what Engine.enhance_batch / enhance_ragged / enhance_long / enhance_long_ragged hand to the library - the row pitches, the
row count, the sample count or the lengths, the window - and every refusal they make before the library is called.  The library
is a recording stand-in, the tensors are stand-ins with a shape, strides and an address (tests/test_long_decode_host.py)."""
import ctypes as C
import re

import pytest
import torch

import se_amd  # noqa: F401
from se_amd.engine import Engine, EngineError

STREAM = 0x5712EA


class _FakeCuda:
    """what the wrappers look at of a float32 cuda tensor, with an address"""
    is_cuda, dtype = True, torch.float32
    _next = [0x10000]

    def __init__(self, shape, strides=None, index=0, dtype=torch.float32):
        self.shape = tuple(shape)
        self._strides = tuple(strides) if strides is not None else (self.shape[1], 1)
        self.device = torch.device('cuda', index)
        self.dtype = dtype
        self._ptr = self._next[0]
        self._next[0] += 0x10000

    def dim(self):
        return len(self.shape)

    def stride(self, i=None):
        return self._strides if i is None else self._strides[i]

    def data_ptr(self):
        return self._ptr


class _Recorder:
    """stands where the loaded library would: se_output_samples answers n, the four decodes record their arguments"""
    DECODES = ('se_enhance_batch', 'se_enhance_ragged', 'se_enhance_long', 'se_enhance_long_ragged')

    def __init__(self):
        self.calls = []

    def se_output_samples(self, h, n):
        return n

    def __getattr__(self, name):
        if name not in self.DECODES:
            raise AssertionError(f'the wrapper called {name}')

        def call(*args):
            self.calls.append((name,) + tuple(self._plain(a) for a in args))
            return 0
        return call

    @staticmethod
    def _plain(a):
        if isinstance(a, C.c_void_p):
            return a.value
        if isinstance(a, C.Array):
            return list(a)
        return a


@pytest.fixture
def eng(monkeypatch):
    e = Engine.__new__(Engine)
    e._lib, e._h = _Recorder(), 'handle'
    e.device, e.max_batch, e.max_samples = 0, 3, 4000
    e._stream = lambda: C.c_void_p(STREAM)
    e.made = []

    def empty(shape, dtype=None, device=None):
        assert dtype == torch.float32 and device == torch.device('cuda', 0)
        e.made.append(_FakeCuda(shape))
        return e.made[-1]
    monkeypatch.setattr(torch, 'empty', empty)
    return e


ONE = lambda: _FakeCuda((1, 5000), (77, 1))            # (the stride of a size-1 dimension is arbitrary)
THREE = lambda: _FakeCuda((3, 5000))
VIEW = lambda: _FakeCuda((3, 5000), (6000, 1))         # rows of a wider buffer
L1, L3 = [4000], [5000, 4000, 4500]


def _run(eng, method, wav, out, lengths, mcf):
    args = [wav] if lengths is None else [wav, lengths]
    kw = {'out': out}
    if mcf is not None:
        kw['max_chunk_frames'] = mcf
    got = getattr(eng, method)(*args, **kw)
    assert got is (out if out is not None else eng.made[-1])
    assert len(eng._lib.calls) == 1
    call = eng._lib.calls[0]
    assert call[0] == 'se_' + method and call[1] == 'handle' and call[2] == wav.data_ptr()
    assert call[-3] == got.data_ptr() and call[-1] == STREAM
    # (in_pitch, batch, n or lengths, max_chunk_frames, out_pitch)
    return (call[3], call[4], call[5], call[6] if len(call) == 10 else None, call[-2]), got


# the tuples are today's, written out: one row passes (L, n_out) from the equal-length wrappers and (wav.shape[1], out.shape[1])
# from the ragged ones, more rows pass the tensors' row strides
@pytest.mark.parametrize('method,mcf', [('enhance_batch', None), ('enhance_long', 0), ('enhance_long', 7)])
@pytest.mark.parametrize('wav,out,want', [
    (ONE, None, (5000, 1, 5000, 5000)),
    (ONE, lambda: _FakeCuda((1, 5000)), (5000, 1, 5000, 5000)),
    (ONE, lambda: _FakeCuda((1, 5600), (9999, 1)), (5000, 1, 5000, 5000)),
    (THREE, None, (5000, 3, 5000, 5000)),
    (THREE, lambda: _FakeCuda((3, 5000)), (5000, 3, 5000, 5000)),
    (THREE, lambda: _FakeCuda((3, 5600)), (5000, 3, 5000, 5600)),
    (VIEW, None, (6000, 3, 5000, 5000)),
    (VIEW, lambda: _FakeCuda((3, 5600), (7000, 1)), (6000, 3, 5000, 7000)),
])
def test_equal_length_wrappers_pass_these_arguments(eng, method, mcf, wav, out, want):
    got, res = _run(eng, method, wav(), out() if out else None, None, mcf)
    assert got == (want[0], want[1], want[2], mcf, want[3])
    if out is None:
        assert res.shape == (want[1], 5000)


@pytest.mark.parametrize('method,mcf', [('enhance_ragged', None), ('enhance_long_ragged', 0), ('enhance_long_ragged', 7)])
@pytest.mark.parametrize('wav,lengths,out,want', [
    (ONE, L1, None, (5000, 1, L1, 4000)),
    (ONE, L1, lambda: _FakeCuda((1, 4000)), (5000, 1, L1, 4000)),
    (ONE, L1, lambda: _FakeCuda((1, 5600), (9999, 1)), (5000, 1, L1, 5600)),
    (THREE, L3, None, (5000, 3, L3, 5000)),
    (THREE, L3, lambda: _FakeCuda((3, 5000)), (5000, 3, L3, 5000)),
    (THREE, L3, lambda: _FakeCuda((3, 5600)), (5000, 3, L3, 5600)),
    (VIEW, L3, None, (6000, 3, L3, 5000)),
    (VIEW, [4800, 4000, 4500], None, (6000, 3, [4800, 4000, 4500], 4800)),
    (VIEW, L3, lambda: _FakeCuda((3, 5600), (7000, 1)), (6000, 3, L3, 7000)),
])
def test_ragged_wrappers_pass_these_arguments(eng, method, mcf, wav, lengths, out, want):
    got, res = _run(eng, method, wav(), out() if out else None, lengths, mcf)
    assert got == (want[0], want[1], want[2], mcf, want[3])
    if out is None:
        assert res.shape == (want[1], max(lengths))


def test_lengths_may_be_any_integers(eng):
    import numpy as np
    got, _ = _run(eng, 'enhance_ragged', THREE(), None, np.array(L3, dtype=np.int64), None)
    assert got == (5000, 3, L3, None, 5000)


METHODS = ('enhance_batch', 'enhance_ragged', 'enhance_long', 'enhance_long_ragged')


def _refused(eng, method, message, wav, lengths=None, **kw):
    args = [wav] if method in ('enhance_batch', 'enhance_long') else [wav, L3 if lengths is None else lengths]
    with pytest.raises(EngineError, match='^' + re.escape(message) + '$'):
        getattr(eng, method)(*args, **kw)
    assert eng._lib.calls == []


@pytest.mark.parametrize('method', METHODS)
def test_every_wrapper_refuses_a_bad_input_tensor(eng, method):
    _refused(eng, method, f'{method} input: expected a float32 cuda tensor, got torch.float32 on cpu', torch.zeros(3, 5000))
    _refused(eng, method, f'{method} input: expected a float32 cuda tensor, got torch.float16 on cuda:0',
             _FakeCuda((3, 5000), dtype=torch.float16))
    _refused(eng, method, f'{method} input: tensor on cuda:1 but the engine lives on cuda:0', _FakeCuda((3, 5000), index=1))
    _refused(eng, method, f'{method} input: expected a 2-D tensor with unit inner stride, got shape (5000,) strides (1,)',
             _FakeCuda((5000,), (1,)))
    _refused(eng, method, f'{method} input: expected a 2-D tensor with unit inner stride, got shape (3, 5000) strides (1, 3)',
             _FakeCuda((3, 5000), (1, 3)))


@pytest.mark.parametrize('method', METHODS)
def test_every_wrapper_refuses_a_bad_output_tensor(eng, method):
    _refused(eng, method, f'{method} output: expected a float32 cuda tensor, got torch.float32 on cpu', THREE(), out=torch.zeros(3, 5000))
    _refused(eng, method, f'{method} output: tensor on cuda:1 but the engine lives on cuda:0', THREE(),
             out=_FakeCuda((3, 5000), index=1))
    _refused(eng, method, f'{method} output: expected a 2-D tensor with unit inner stride, got shape (3, 5000) strides (10000, 2)',
             THREE(), out=_FakeCuda((3, 5000), (10000, 2)))
    _refused(eng, method, f'{method} output: need [3, >= 5000], got (2, 5000)', THREE(), out=_FakeCuda((2, 5000)))
    _refused(eng, method, f'{method} output: need [3, >= 5000], got (3, 4999)', THREE(), out=_FakeCuda((3, 4999)))


def test_enhance_ragged_refuses_lengths_that_do_not_fit_the_batch(eng):
    _refused(eng, 'enhance_ragged', 'enhance_ragged: 2 lengths (max 5000) for a (3, 5000) batch', THREE(), [5000, 4000])
    _refused(eng, 'enhance_ragged', 'enhance_ragged: 3 lengths (max 5001) for a (3, 5000) batch', THREE(), [5001, 4000, 4500])


@pytest.mark.parametrize('method', ('enhance_long', 'enhance_long_ragged'))
def test_the_long_wrappers_refuse_rows_window_and_overlap(eng, method):
    _refused(eng, method, f'{method} input: 4 rows outside 1..max_batch (3)', _FakeCuda((4, 5000)), [5000] * 4)
    _refused(eng, method, f'{method} input: 0 rows outside 1..max_batch (3)', _FakeCuda((0, 5000)), [])
    _refused(eng, method, f'{method} input: rows of 5000 samples overlap (strides (4999, 1))', _FakeCuda((3, 5000), (4999, 1)))
    _refused(eng, method, f'{method} input: rows of 5000 samples overlap (strides (0, 1))', _FakeCuda((3, 5000), (0, 1)))
    _refused(eng, method, f'{method}: max_chunk_frames -1 is negative (0 = the largest window)', THREE(), max_chunk_frames=-1)


def test_enhance_long_ragged_refuses_lengths_that_do_not_fit_the_batch(eng):
    m = 'enhance_long_ragged'
    _refused(eng, m, f'{m}: 2 lengths for a batch of 3 rows', THREE(), [5000, 4000])
    _refused(eng, m, f'{m}: lengths 4000..5001 outside rows of 5000 samples', THREE(), [5001, 4000, 4500])
    _refused(eng, m, f'{m}: lengths 0..5000 outside rows of 5000 samples', THREE(), [5000, 0, 4500])
    # rows may overlap past the longest length, not below it
    _refused(eng, m, f'{m} input: rows of 4500 samples overlap (strides (4499, 1))', _FakeCuda((3, 5000), (4499, 1)), [4500, 4000, 4500])
    got, _ = _run(eng, m, _FakeCuda((3, 5000), (4500, 1)), None, [4500, 4000, 4500], 0)
    assert got == (4500, 3, [4500, 4000, 4500], 0, 4500)
