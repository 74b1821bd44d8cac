"""CPU: the host side of selecting and joining rows of parked streams (se_stream_state_select / _concat and
se_resampler_state_select / _concat of include/se_engine.h).  The engine's pair needs an engine - a device - to be called at all;
what it computes on the host, the scaled segment sizes and offsets of a result and every refusal that needs no device, are pure
functions of csrc/stream_rows.h and run in a stand-alone program under the host sanitizers (csrc/tests/stream_select_check.cpp).  The
resampler's pair needs no engine: images that have not been restored yet are cut on the host, so it is exercised here in full, on
images built from the layout csrc/resampler_manifest.h documents."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import se_amd  # noqa: F401
from se_amd import _lib
from se_amd.engine import EngineError, StreamSnapshot
from se_amd.resample import ResamplerSnapshot
from se_amd.source_stream import SourceStreamSnapshot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'sixty-years-of-frequency-domain-monaural-speech-enhancement_amd', 'csrc')
NEW_SYMBOLS = ['se_stream_state_select', 'se_stream_state_concat', 'se_resampler_state_select', 'se_resampler_state_concat']
HEAD = 64                       # resampler image: magic, version, sr_in, sr_out, batch, pad | n_total, w0, t, acc, payload bytes
KEEP = 2 * 193                  # 48 -> 16 kHz: the most history a row keeps (2 * reach)


def _image(rows, sr_in=48000, sr_out=16000, n_total=5003, t=1603, acc=4809.0, keep=KEEP):
    """a well-formed resampler image whose row b holds the value rows[b] + j / 1024 at history sample j"""
    pay = np.stack([r + np.arange(keep, dtype=np.float32) / 1024 for r in rows]).astype('<f4') if keep else np.zeros((len(rows), 0), '<f4')
    head = struct.pack('<II4iqqqdq', 0x53524553, 1, sr_in, sr_out, len(rows), 0, n_total, n_total - keep, t, acc, pay.nbytes)
    assert len(head) == HEAD
    return head + pay.tobytes()


def _rows_of(snap):
    b = snap.to_bytes()
    batch = struct.unpack_from('<i', b, 16)[0]
    return np.frombuffer(b[HEAD:], '<f4').reshape(batch, -1)


def test_binding_declares_the_entry_points_and_the_abi_stays_5():
    hdr = open(os.path.join(ROOT, 'include', 'se_engine.h')).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS
        assert name + '(' in hdr
    lib = _lib.load()
    assert len(lib.se_stream_state_select.argtypes) == 6 and len(lib.se_stream_state_concat.argtypes) == 5
    assert len(lib.se_resampler_state_select.argtypes) == 5 and len(lib.se_resampler_state_concat.argtypes) == 4
    assert lib.se_abi_version() == 5
    for cls in (StreamSnapshot, ResamplerSnapshot, SourceStreamSnapshot):
        assert callable(cls.select) and callable(cls.concat)


def test_engine_pair_without_an_engine_is_an_error_not_a_crash():
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.se_stream_state_create(C.byref(h)) == 0
    rows = (C.c_int32 * 1)(0)
    assert lib.se_stream_state_select(None, h, h, rows, 1, None) != 0
    assert lib.se_stream_state_concat(None, h, (C.c_void_p * 1)(h.value), 1, None) != 0
    lib.se_stream_state_destroy(h)
    snap = StreamSnapshot()
    with pytest.raises(EngineError, match='^select: expected an Engine, got NoneType$'):
        snap.select(None, [0])
    with pytest.raises(EngineError, match='^concat: expected an Engine, got str$'):
        StreamSnapshot.concat('engine', [snap])
    snap.close()


def test_resampler_select_cuts_an_imported_image_on_the_host():
    src = ResamplerSnapshot.from_bytes(_image([10, 20, 30, 40]))
    with src.select([3, 1, 1]) as got:
        assert got.counts() == (48000, 16000, 3, 5003, 1603)
        assert got.to_bytes() == _image([40, 20, 20])
    with src.select([0, 1, 2, 3]) as same:
        assert same.to_bytes() == src.to_bytes()
    # into an object that is in use: replaced, and again
    out = ResamplerSnapshot.from_bytes(_image([7]))
    assert src.select([2], out=out) is out and out.to_bytes() == _image([30])
    assert src.select([0, 3], out=out) is out and out.to_bytes() == _image([10, 40])
    out.close()
    src.close()


def test_resampler_concat_joins_rows_in_order_and_select_undoes_it():
    a, b = ResamplerSnapshot.from_bytes(_image([1, 2])), ResamplerSnapshot.from_bytes(_image([3]))
    with ResamplerSnapshot.concat([a, b, a]) as j:
        assert j.counts()[2] == 5
        assert np.array_equal(_rows_of(j)[:, 0], [1, 2, 3, 1, 2])
        assert j.to_bytes() == _image([1, 2, 3, 1, 2])
        with j.select([2]) as back:
            assert back.to_bytes() == b.to_bytes()
    with ResamplerSnapshot.concat([b]) as one:
        assert one.to_bytes() == b.to_bytes()
    a.close()
    b.close()


def test_resampler_pass_through_states_have_only_counters():
    img = lambda batch: _image([0] * batch, sr_in=16000, sr_out=16000, n_total=900, t=900, acc=0.0, keep=0)      # noqa: E731
    src = ResamplerSnapshot.from_bytes(img(3))
    with src.select([2, 2, 0, 1]) as got:
        assert got.counts() == (16000, 16000, 4, 900, 900) and got.nbytes == 0 and got.to_bytes() == img(4)
        with ResamplerSnapshot.concat([got, src]) as j:
            assert j.to_bytes() == img(7)
    src.close()


@pytest.mark.parametrize('rows,reason', [([4], r'rows\[0\] = 4 outside 0 \.\. 3'), ([0, -1], r'rows\[1\] = -1 outside 0 \.\. 3'),
                                         ([1, 2, 9, 0], r'rows\[2\] = 9 outside 0 \.\. 3')])
def test_resampler_select_refuses_a_bad_row_index_and_changes_nothing(rows, reason):
    src = ResamplerSnapshot.from_bytes(_image([10, 20, 30, 40]))
    out = ResamplerSnapshot.from_bytes(_image([7]))
    with pytest.raises(EngineError, match=reason):
        src.select(rows, out=out)
    assert out.to_bytes() == _image([7]) and src.to_bytes() == _image([10, 20, 30, 40])
    src.close()
    out.close()


def test_resampler_select_refuses_no_rows_an_empty_source_and_itself():
    lib = _lib.load()
    src = ResamplerSnapshot.from_bytes(_image([10, 20]))
    empty = ResamplerSnapshot()
    rows = (C.c_int32 * 1)(0)
    err = lambda: lib.se_last_error(None).decode()      # noqa: E731
    assert lib.se_resampler_state_select(empty._h, src._h, rows, 0, None) != 0 and 'n_rows 0' in err()
    assert lib.se_resampler_state_select(empty._h, src._h, None, 1, None) != 0 and 'null' in err()
    assert lib.se_resampler_state_select(src._h, src._h, rows, 1, None) != 0 and 'dst == src' in err()
    assert lib.se_resampler_state_select(None, src._h, rows, 1, None) != 0 and 'null' in err()
    with pytest.raises(EngineError, match='at least one row'):
        src.select([])
    with pytest.raises(EngineError, match='the resampler state object is empty'):
        empty.select([0])
    with pytest.raises(EngineError, match='dst == src'):
        src.select([0], out=src)
    assert src.to_bytes() == _image([10, 20])
    with pytest.raises(EngineError, match='^select: expected a ResamplerSnapshot, got bytes$'):
        src.select([0], out=b'x')
    closed = ResamplerSnapshot()
    closed.close()
    with pytest.raises(EngineError, match='^select: the snapshot is closed$'):
        closed.select([0])
    src.close()
    empty.close()


@pytest.mark.parametrize('kw,reason', [
    (dict(sr_in=32000, keep=100), 'sr_in 48000 vs 32000'),
    (dict(sr_out=8000, keep=100), 'sr_out 16000 vs 8000'),
    (dict(n_total=5004), 'n_in 5003 vs 5004'),
    (dict(t=1602), 'n_out 1603 vs 1602'),
    (dict(keep=KEEP - 1), 'w0 4617 vs 4618'),
    (dict(acc=4809.5), 'read position'),
])
def test_resampler_concat_refuses_parts_that_differ_in_one_field(kw, reason):
    a = ResamplerSnapshot.from_bytes(_image([1, 2]))
    b = ResamplerSnapshot.from_bytes(_image([3], **kw))
    out = ResamplerSnapshot.from_bytes(_image([7]))
    with pytest.raises(EngineError, match='parts.0. and parts.1. differ: ' + reason):
        ResamplerSnapshot.concat([a, b], out=out)
    assert out.to_bytes() == _image([7])
    for s in (a, b, out):
        s.close()


def test_resampler_concat_refuses_no_parts_an_empty_part_and_its_own_destination():
    lib = _lib.load()
    a = ResamplerSnapshot.from_bytes(_image([1, 2]))
    empty = ResamplerSnapshot()
    err = lambda: lib.se_last_error(None).decode()      # noqa: E731
    assert lib.se_resampler_state_concat(empty._h, (C.c_void_p * 1)(a._h.value), 0, None) != 0 and 'n_parts 0' in err()
    assert lib.se_resampler_state_concat(empty._h, None, 1, None) != 0 and 'null' in err()
    assert lib.se_resampler_state_concat(empty._h, (C.c_void_p * 2)(a._h.value, None), 2, None) != 0 and 'parts[1] is null' in err()
    with pytest.raises(EngineError, match='at least one part'):
        ResamplerSnapshot.concat([])
    with pytest.raises(EngineError, match=r'parts\[1\]: the resampler state object is empty'):
        ResamplerSnapshot.concat([a, empty])
    with pytest.raises(EngineError, match=r'dst == parts\[1\]'):
        ResamplerSnapshot.concat([ResamplerSnapshot.from_bytes(_image([5])), a], out=a)
    assert a.to_bytes() == _image([1, 2])
    a.close()
    empty.close()


def test_source_pair_checks_the_resamplers_half_first():
    """rows the resampler's half does not have are refused on the host, before an engine is looked at"""
    eng_img = struct.pack('<II18iffiiq', 0x54534553, 1, 5, 0, 512, 128, 512, 2, 16, 3700, 26, 3000, 3600, 0, 0, 1, 0, 0, 0, 0,
                          0.5, 2.0, 1, 0, 800) + struct.pack('<iiq', 8, 0, 800) + bytes(800)
    pair = SourceStreamSnapshot(StreamSnapshot.from_bytes(eng_img), ResamplerSnapshot.from_bytes(_image([1, 2])))
    with pytest.raises(EngineError, match=r'rows\[0\] = 2 outside 0 \.\. 1'):
        pair.select(object(), [2])
    three = SourceStreamSnapshot(StreamSnapshot.from_bytes(eng_img), ResamplerSnapshot.from_bytes(_image([1, 2, 3])))
    with pytest.raises(EngineError, match="the engine's half holds 2 rows, the resampler's 3"):
        three.select(object(), [0])
    with pytest.raises(EngineError, match='n_in 5003 vs 5004'):
        SourceStreamSnapshot.concat(object(), [pair, SourceStreamSnapshot(StreamSnapshot.from_bytes(eng_img),
                                                                          ResamplerSnapshot.from_bytes(_image([1], n_total=5004)))])
    pair.close()
    three.close()


def test_row_arithmetic_is_host_only_and_clean_under_the_host_sanitizers(tmp_path):
    """stream_rows.h includes no HIP; its stand-alone check program, built with -fsanitize=address,undefined, checks the scaled sizes
    and offsets of select / concat results for a manifest with all eight segment kinds, a gather written out index by index, and the
    refusals: a bad row index, n_rows == 0, layouts that do not fit, parts that differ in each single field."""
    src = open(os.path.join(CSRC, 'stream_rows.h')).read()
    assert 'hip' not in src.replace('no HIP', '').lower()
    cxx = shutil.which(os.environ.get('CXX', 'g++')) or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'stream_select_check')
    subprocess.run([cxx, '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                    os.path.join(CSRC, 'tests', 'stream_select_check.cpp'), '-o', exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), (r.returncode, r.stdout, r.stderr)
