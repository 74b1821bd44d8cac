"""CPU: the host side of se_resample_ragged (include/se_engine.h).  The planning - row sizes, the split of the rows over launches, the
refusals - is host code alone (csrc/resample_ragged.h) and runs under the host sanitizers in a stand-alone program
(csrc/tests/resample_ragged_check.cpp); the sizes it plans are the ones se_resample_samples names; the Python wrapper refuses what it
can see before the library is called."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import se_amd  # noqa: F401
from se_amd import _lib
from se_amd import resample as HR
from se_amd.engine import EngineError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'sixty-years-of-frequency-domain-monaural-speech-enhancement_amd', 'csrc')


@pytest.fixture(scope='module')
def check_program(tmp_path_factory):
    src = open(os.path.join(CSRC, 'resample_ragged.h')).read()
    assert not [line for line in src.split('\n') if line.startswith('#include') and 'hip' in line.lower()]
    cxx = shutil.which(os.environ.get('CXX', 'g++')) or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('ragged') / 'resample_ragged_check')
    subprocess.run([cxx, '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                    os.path.join(CSRC, 'tests', 'resample_ragged_check.cpp'), '-o', exe], check=True)
    return exe


def test_planner_is_host_only_and_clean_under_the_host_sanitizers(check_program):
    """row sizes against whole-number arithmetic, the row split around the per-launch bound, every refusal: a program of its own"""
    r = subprocess.run([check_program], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


@pytest.mark.parametrize('sr_in,sr_out', [(48000, 16000), (32000, 16000), (44100, 16000), (22050, 16000), (8000, 16000), (16000, 16000),
                                          (16000, 48000)])
def test_planned_sizes_are_the_ones_se_resample_samples_names(check_program, sr_in, sr_out):
    lens = list(range(1, 400)) + [4799, 4800, 4801, 44100, 57601, 470401]
    r = subprocess.run([check_program, 'sizes', str(sr_in), str(sr_out)] + [str(n) for n in lens], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    rows = [tuple(int(v) for v in line.split()) for line in r.stdout.split('\n') if line]
    assert len(rows) == len(lens)
    for n, (n_calc, n_out) in zip(lens, rows):
        assert n_out == HR.resample_samples(n, sr_in, sr_out), (n, n_out)
        assert n_calc == (n if sr_in == sr_out else int(n * (float(sr_out) / sr_in))) and 0 <= n_out - n_calc <= 1, (n, n_calc, n_out)


def test_binding_declares_the_entry_point_and_the_abi_stays_5():
    assert 'se_resample_ragged' in _lib.SYMBOLS
    hdr = open(os.path.join(ROOT, 'include', 'se_engine.h')).read()
    assert 'int se_resample_ragged(' in hdr and '#define SE_SAMPLES_F32 0' in hdr and '#define SE_SAMPLES_S16 1' in hdr
    lib = _lib.load()
    assert len(lib.se_resample_ragged.argtypes) == 10
    assert (HR.SAMPLES_F32, HR.SAMPLES_S16) == (0, 1)
    assert lib.se_abi_version() == 5


def test_wrapper_refuses_what_it_can_see_before_the_library_is_called(monkeypatch):
    import torch

    class NoLib:
        def __getattr__(self, name):
            raise AssertionError(f'the library was called ({name}) by a wrapper that has to refuse first')

    monkeypatch.setattr(_lib, 'load', lambda: NoLib())
    x = torch.zeros((3, 100), dtype=torch.float32)
    with pytest.raises(EngineError, match=r'lengths\[1\] = 101 outside 1..100'):
        HR.resample_ragged(x, [100, 101, 5], 48000)
    with pytest.raises(EngineError, match=r'lengths\[2\] = 0 outside 1..100'):
        HR.resample_ragged(x, [100, 1, 0], 48000)
    with pytest.raises(EngineError, match='2 lengths for 3 rows'):
        HR.resample_ragged(x, [100, 50], 48000)
    with pytest.raises(EngineError, match='4 lengths for 3 rows'):
        HR.resample_ragged(x, [1, 2, 3, 4], 48000)
    for dtype in (torch.float64, torch.int32, torch.float16, torch.uint8):
        with pytest.raises(EngineError, match='the rows are float32 or int16'):
            HR.resample_ragged(x.to(dtype), [100, 50, 5], 48000)
    with pytest.raises(EngineError, match=r'tensor \[B, pitch\]'):
        HR.resample_ragged(x[0], [100], 48000)
    with pytest.raises(EngineError, match=r'tensor \[B, pitch\]'):
        HR.resample_ragged(np.zeros((3, 100), dtype=np.float32), [100, 50, 5], 48000)
    with pytest.raises(EngineError, match='contiguous'):
        HR.resample_ragged(x[:, ::2], [50, 50, 5], 48000)
    with pytest.raises(EngineError, match='sample rates 0 -> 16000'):
        HR.resample_ragged(x, [100, 50, 5], 0)
    with pytest.raises(EngineError, match='has to live on the GPU'):       # (accepted so far: int16 rows, lengths within the pitch)
        HR.resample_ragged(x.to(torch.int16), [100, 50, 5], 48000)
