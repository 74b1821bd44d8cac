"""CPU: the host side of decoding the `_vb` DCCRN's long clips of different lengths in one window walk (SE_CFG_DCCRN_ROW_ENDS of
include/se_engine.h, `row_ends=True` on Engine and the model classes, decode.LONG_RAGGED_FLAGS).  The decode itself needs a device;
what decides which columns of a chunk are cleared - window_cut() of csrc/window_rows.h - is plain arithmetic that the kernel and the
host share, and runs in a stand-alone program under the host sanitizers (csrc/tests/window_cut_check.cpp)."""
import inspect
import os
import shutil
import subprocess

import se_amd  # noqa: F401
from se_amd import _lib, decode
from se_amd.engine import Engine
from se_amd import models

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'sixty-years-of-frequency-domain-monaural-speech-enhancement_amd', 'csrc')


def test_the_bit_is_declared_everywhere_and_the_abi_stays_5():
    hdr = open(os.path.join(ROOT, 'include', 'se_engine.h')).read()
    assert '#define SE_CFG_DCCRN_ROW_ENDS (1 << 18)' in hdr and '#define SE_CFG_STREAM_SLIDING (1 << 17)' in hdr
    assert 'SE_CFG_DCCRN_ROW_ENDS: no new entry point, same number' in hdr
    assert Engine.SE_CFG_DCCRN_ROW_ENDS == 1 << 18
    assert _lib.load().se_abi_version() == 5
    assert inspect.signature(Engine.__init__).parameters['row_ends'].default is False
    assert inspect.signature(models._EngineModule.__init__).parameters['row_ends'].default is False
    m = models.MODEL_CLASSES['dccrn'](row_ends=True, sliding_stream=True)
    assert m._flags == (1 << 18) | (1 << 17)
    assert models.MODEL_CLASSES['dccrn']()._flags == 0


def test_the_driver_keeps_its_table_and_adds_one():
    assert decode.LONG_RAGGED_FLAGS == {'dccrn': Engine.SE_CFG_DCCRN_ROW_ENDS}
    assert 'dccrn' not in decode.LONG_RAGGED_MODELS and 'dccrn' in decode.LONG_MODELS
    assert set(decode.LONG_RAGGED_FLAGS) == decode.LONG_MODELS - decode.LONG_RAGGED_MODELS      # every long model groups, one way or the other


def test_window_cut_is_host_arithmetic_and_clean_under_the_host_sanitizers(tmp_path):
    """window_rows.h compiles without HIP (its launchers are declared for the HIP compiler only); the stand-alone check program, built
    with -fsanitize=address,undefined and run directly, walks window_cut over every (row length 1..80, window origin, chunk size 1, 7,
    16) of a decode with 12 history columns against the brute-force statement - column c is kept if and only if frame t0 - HC + c lies
    below the row's frame count - and over the frame counts of the position bound 2^31 - 1 - n_fft - 32 hop, where nothing may overflow."""
    src = open(os.path.join(CSRC, 'window_rows.h')).read()
    assert 'SE_WINDOW_HD inline int window_cut(int tlen, int t0, int HC, int Tw)' in src
    cxx = shutil.which(os.environ.get('CXX', 'g++')) or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'window_cut_check')
    subprocess.run([cxx, '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                    os.path.join(CSRC, 'tests', 'window_cut_check.cpp'), '-o', exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), (r.returncode, r.stdout, r.stderr)
