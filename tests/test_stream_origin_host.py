"""CPU: the host side of per-row frame origins (SE_CFG_STREAM_ROW_ORIGINS of include/se_engine.h; `row_origins=True` on Engine and the
model classes).  What a snapshot carries for them - the SNAP_ORIGIN segment of csrc/stream_manifest.h - how select, concat and join
treat it, and the join plan of the four configurations whose state counts frames are pure functions of host headers; they run in a
stand-alone program under the host sanitizers (csrc/tests/stream_origin_check.cpp).  The import of an image is host code too and is
called here through the library."""
import inspect
import os
import shutil
import struct
import subprocess

import pytest

import se_amd  # noqa: F401
from se_amd import _lib
from se_amd import models, models_new
from se_amd.engine import Engine, EngineError, StreamSnapshot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'sixty-years-of-frequency-domain-monaural-speech-enhancement_amd', 'csrc')
BIT = 1 << 19


def _image(flags, segs, batch=3, n_total=3700, keep=3600, model=7):
    """a stream image (csrc/stream_manifest.h) of `batch` rows with the segments (kind, index, bytes) and a zero payload"""
    pay = sum((n + 15) // 16 * 16 for _, _, n in segs)
    return (struct.pack('<II18iffiiq', 0x54534553, 1, model, flags, 320, 160, 320, batch, 16, n_total, 22, 3000, keep, 0, 0, 0, batch, 0, 0, 0,
                        0.5, 2.0, len(segs), 0, pay) + b''.join(struct.pack('<iiq', *s) for s in segs) + bytes(pay))


def test_the_bit_is_declared_in_every_host_layer_and_the_abi_stays_5():
    hdr = open(os.path.join(ROOT, 'include', 'se_engine.h')).read()
    assert '#define SE_CFG_STREAM_ROW_ORIGINS (1 << 19)' in hdr
    assert Engine.SE_CFG_STREAM_ROW_ORIGINS == BIT
    assert inspect.signature(Engine.__init__).parameters['row_origins'].default is False
    assert inspect.signature(models._EngineModule.__init__).parameters['row_origins'].default is False
    for make in (lambda **kw: models_new.CTSNet(**kw), models_new._taylor, models_new._g2net):
        m = make(row_origins=True, max_batch=2, max_samples=4000)
        flags = m._kw.get('row_origins') if hasattr(m, '_kw') else m._flags & BIT
        assert flags, make
    fsn = models.Model(norm_type='cumulative_laplace_norm', row_origins=True)
    assert fsn._flags & BIT and fsn._flags & models.Model.SE_CFG_FSN_CUMULATIVE
    assert not models._EngineModule()._flags & BIT
    assert _lib.load().se_abi_version() == 5
    src = open(os.path.join(CSRC, 'stream_manifest.h')).read()
    assert 'SNAP_ORIGIN = 9' in src and 'SNAP_VERSION = 1;' in src


def test_import_validates_the_origin_segment():
    win = 3 * 100 * 4
    good = _image(BIT, [(1, 0, 12), (7, 0, 48), (9, 0, 12), (8, 0, win)])
    with StreamSnapshot.from_bytes(good) as snap:
        assert snap.batch == 3 and snap.to_bytes() == good
    for img, why in [
            (_image(BIT, [(1, 0, 12), (7, 0, 48), (9, 0, 16), (8, 0, win)]), 'frame origin segment of 16 bytes, 3 rows keep 12'),
            (_image(BIT, [(1, 0, 12), (9, 0, 12), (7, 0, 48), (8, 0, win)]), 'frame origin segment misplaced'),
            (_image(BIT, [(1, 0, 12), (7, 0, 48), (8, 0, win), (9, 0, 12)]), 'misplaced'),
            (_image(BIT, [(1, 0, 12), (7, 0, 48), (8, 0, win)]), 'no frame origin segment in a snapshot of an engine with SE_CFG_STREAM_ROW_ORIGINS'),
            (_image(0, [(1, 0, 12), (7, 0, 48), (9, 0, 12), (8, 0, win)]),
             'a frame origin segment in a snapshot of an engine without SE_CFG_STREAM_ROW_ORIGINS'),
            (_image(BIT, [(1, 0, 12), (10, 0, 12), (8, 0, win)]), 'segment 1 of unknown kind')]:
        with pytest.raises(EngineError, match='se_stream_state_import: stream state image: .*' + why):
            StreamSnapshot.from_bytes(img)
    # without the bit and without the segment: the images of before
    plain = _image(0, [(1, 0, 12), (7, 0, 48), (8, 0, win)])
    with StreamSnapshot.from_bytes(plain) as snap:
        assert snap.to_bytes() == plain


def test_origin_arithmetic_is_host_only_and_clean_under_the_host_sanitizers(tmp_path):
    """csrc/tests/stream_origin_check.cpp, built with -fsanitize=address,undefined and run directly: a manifest round trip with a
    SNAP_ORIGIN segment; the refusals (wrong size, behind the window, the bit without the segment, the segment without the bit); the row
    arithmetic of select, concat and join on origins, accumulation and negative values included; the plan accepting each of the four
    configurations with the bit and refusing a manifest without it in the parent's words; the left-edge refusal in its exact words for
    each of the four (in-phase counters with t_done 0; a set `first` flag, which counts for FullSubNet and not for the slot models)."""
    for h in ('stream_manifest.h', 'stream_rows.h', 'stream_join.h'):
        assert '#include <hip' not in open(os.path.join(CSRC, h)).read()
    assert 'stream_origin_check:' in open(os.path.join(CSRC, 'Makefile')).read()
    cxx = shutil.which(os.environ.get('CXX', 'g++')) or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'stream_origin_check')
    subprocess.run([cxx, '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                    os.path.join(CSRC, 'tests', 'stream_origin_check.cpp'), '-o', exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), (r.returncode, r.stdout, r.stderr)
