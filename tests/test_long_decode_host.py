"""CPU: the host side of the windowed decode of long clips (se_enhance_long) - the Python wrappers refuse bad tensors before the
library is called, the driver's plan splits the clip list at the bound, `--max-seconds` parses."""
import pytest
import torch

import se_amd  # noqa: F401
from se_amd import _lib, decode
from se_amd.engine import Engine, EngineError


class _NoLibrary:
    """stands where the loaded library would: any call through it fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f'the wrapper called the library ({name}) with a tensor it should have refused')


class _FakeCuda:
    """what the wrappers look at of a float32 cuda tensor (there is no GPU here to make a real one on)"""
    is_cuda, dtype = True, torch.float32

    def __init__(self, shape, strides, index=0):
        self.shape, self._strides = tuple(shape), tuple(strides)
        self.device = torch.device('cuda', index)

    def dim(self):
        return len(self.shape)

    def stride(self, i=None):
        return self._strides if i is None else self._strides[i]

    def data_ptr(self):
        raise AssertionError('the wrapper took the address of a tensor it should have refused')


def _engine(max_batch=2, max_samples=4000):
    eng = Engine.__new__(Engine)                 # no handle: nothing here may reach the library
    eng._lib, eng._h = _NoLibrary(), None
    eng.device, eng.max_batch, eng.max_samples = 0, max_batch, max_samples
    return eng


@pytest.mark.parametrize('wav,why', [
    (torch.zeros(2, 9000), 'float32 cuda tensor'),                           # a host tensor
    (_FakeCuda((9000,), (1,)), '2-D tensor'),                                # one dimension short
    (_FakeCuda((1, 2, 9000), (18000, 9000, 1)), '2-D tensor'),               # one too many
    (_FakeCuda((2, 9000), (18000, 2)), 'unit inner stride'),                 # every other sample: not contiguous along time
    (_FakeCuda((2, 9000), (1, 2)), 'unit inner stride'),                     # a transposed view
    (_FakeCuda((2, 9000), (0, 1)), 'overlap'),                               # an expanded row
    (_FakeCuda((3, 9000), (9000, 1)), 'max_batch'),                          # more rows than the engine was made for
    (_FakeCuda((2, 9000), (9000, 1), index=1), 'cuda:1'),                    # another device
])
def test_enhance_long_refuses_bad_input_before_calling_the_library(wav, why):
    with pytest.raises(EngineError, match=why):
        _engine().enhance_long(wav)


def test_enhance_long_refuses_a_negative_window():
    with pytest.raises(EngineError, match='max_chunk_frames'):
        _engine().enhance_long(_FakeCuda((2, 9000), (9000, 1)), max_chunk_frames=-1)


def test_model_wrappers_pass_enhance_long_through():
    from se_amd import models, models_new
    seen = []

    class _Eng:
        def enhance_long(self, wav, out=None, max_chunk_frames=0):
            seen.append((wav, out, max_chunk_frames))
            return 'y'

    for net in (models.crn_net(), models.CTSNet(), models_new.CTSNet()):
        net.engine = _Eng()
        assert net.enhance_long('x', max_chunk_frames=7) == 'y' and seen[-1] == ('x', None, 7)


def test_binding_declares_the_entry_point():
    assert 'se_enhance_long' in _lib.SYMBOLS
    lib = _lib.load()
    assert len(lib.se_enhance_long.argtypes) == 9


def test_plan_puts_clips_above_the_bound_in_the_long_list():
    lens = [64000, 16000, 28_800_000, 32000, 32001, 40000]                   # 30 minutes among clips of seconds
    size, short, long_ = decode.plan_long(lens, 2)
    assert size == 32000 and short == [1, 3] and long_ == [0, 2, 4, 5]
    size, short, long_ = decode.plan_long(lens, 2.5)                         # fractions of a second
    assert size == 40000 and short == [1, 3, 4, 5] and long_ == [0, 2]
    size, short, long_ = decode.plan_long(lens, 3600)                        # a bound above every clip: the longest sizes the engine
    assert size == 28_800_000 and short == list(range(6)) and long_ == []
    size, short, long_ = decode.plan_long(lens, None)                        # no option: as before
    assert size == 28_800_000 and short == list(range(6)) and long_ == []
    assert decode.plan_long([], 2) == (0, [], [])
    with pytest.raises(ValueError):
        decode.plan_long(lens, 0)
    # the batched calls are planned over the clips that fit only
    plan = decode.plan_batches([lens[i] for i in short], 4, 4 * 64000, True)
    assert sorted(i for b in plan for i in b) == list(range(len(short)))


def test_models_the_driver_decodes_in_windows():
    assert decode.LONG_MODELS <= set(decode.MODELS)
    assert {'crn', 'dccrn', 'ctsnet_new'} <= decode.LONG_MODELS
    assert not decode.LONG_MODELS & {'uformer', 'fullsubnet', 'ctsnet', 'g2net', 'taylorsenet'}


def test_max_seconds_argument_parses():
    base = ['--mix_file_path', 'a', '--esti_clean_file_path', 'b']
    p = decode.build_parser()
    assert p.parse_args(base).max_seconds is None
    assert p.parse_args(base + ['--max-seconds', '30']).max_seconds == 30.0
    assert p.parse_args(base + ['--max_seconds', '2.5']).max_seconds == 2.5
    with pytest.raises(SystemExit):
        p.parse_args(base + ['--max-seconds', 'long'])
