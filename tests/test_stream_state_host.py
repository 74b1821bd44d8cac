"""CPU: the host side of parking and resuming frame-online streams (se_stream_state_*, se_stream_save, se_stream_restore of
include/se_engine.h).  The object is created, queried and destroyed without a device; se_stream_state_import parses, validates
and refuses on the host; the Python wrappers refuse a closed snapshot, a closed engine and a wrong type before the library is
called.  Images are built here from the layout csrc/stream_manifest.h documents - there is no GPU to export one from.  The
manifest code itself runs under the host sanitizers in a stand-alone program (csrc/tests/stream_manifest_check.cpp)."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import pytest

import se_amd  # noqa: F401
from se_amd import _lib
from se_amd.engine import Engine, EngineError, StreamSnapshot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'sixty-years-of-frequency-domain-monaural-speech-enhancement_amd', 'csrc')
NEW_SYMBOLS = ['se_stream_state_create', 'se_stream_state_destroy', 'se_stream_state_bytes', 'se_stream_save', 'se_stream_restore',
               'se_stream_state_export', 'se_stream_state_import']
HEAD = 104                      # magic, version, 18 int32, p_in, p_out, nseg, pad, payload bytes
KIND_HIST, KIND_WINDOW = 4, 8


def _image(seg_bytes=(48, 20, 0), batch=2, n_total=3700, keep=3600):
    """a well-formed image: len(seg_bytes) history segments and the input window of batch x (n_total - keep) floats"""
    segs = [(KIND_HIST, i, n) for i, n in enumerate(seg_bytes)] + [(KIND_WINDOW, 0, batch * (n_total - keep) * 4)]
    pay = sum((n + 15) // 16 * 16 for _, _, n in segs)
    ints = [5, 0, 512, 128, 512, batch, 16, n_total, 26, 3000, keep, 0, 0, 0, batch, 0, 0, 0]
    b = struct.pack('<II18iffiiq', 0x54534553, 1, *ints, 0.5, 2.0, len(segs), 0, pay)
    assert len(b) == HEAD
    for kind, index, n in segs:
        b += struct.pack('<iiq', kind, index, n)
    return b + bytes(range(256)) * (pay // 256) + bytes(pay % 256)


def _err(lib):
    return lib.se_last_error(None).decode()


def test_binding_declares_the_entry_points_and_the_abi_stays_5():
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS
    hdr = open(os.path.join(ROOT, 'include', 'se_engine.h')).read()
    for name in NEW_SYMBOLS:
        assert name + '(' in hdr
    lib = _lib.load()
    assert len(lib.se_stream_save.argtypes) == 3 and len(lib.se_stream_restore.argtypes) == 3
    assert len(lib.se_stream_state_export.argtypes) == 3 and len(lib.se_stream_state_import.argtypes) == 3
    assert lib.se_abi_version() == 5


def test_create_is_empty_and_export_of_an_empty_object_is_refused():
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.se_stream_state_create(C.byref(h)) == 0 and h.value
    assert lib.se_stream_state_bytes(h) == 0
    assert lib.se_stream_state_export(h, None, 0) == -1 and 'empty' in _err(lib)
    buf = C.create_string_buffer(64)
    assert lib.se_stream_state_export(h, C.cast(buf, C.c_void_p), 64) == -1 and 'empty' in _err(lib)
    assert lib.se_stream_state_destroy(h) == 0
    assert lib.se_stream_state_destroy(None) == 0
    assert lib.se_stream_state_create(None) != 0 and 'null' in _err(lib)


def test_import_accepts_a_well_formed_image_and_gives_it_back():
    img = _image()
    with StreamSnapshot.from_bytes(img) as snap:
        assert snap.batch == 2
        assert snap.nbytes == len(img) - HEAD - 4 * 16
        out = snap.to_bytes()
        assert out == img
        # a refused import leaves the object as it was
        lib = _lib.load()
        assert lib.se_stream_state_import(snap._h, b'nonsense' * 20, 160) != 0
        assert snap.to_bytes() == img


@pytest.mark.parametrize('what,mutate,reason', [
    ('garbage', lambda b: bytes((37 * i + 11) & 255 for i in range(len(b))), 'magic'),
    ('another version', lambda b: b[:4] + struct.pack('<I', 7) + b[8:], 'version'),
    ('cut inside the header', lambda b: b[:60], 'truncated'),
    ('cut inside the segment table', lambda b: b[:HEAD + 20], 'truncated'),
    ('cut inside the payload', lambda b: b[:-1], 'truncated'),
    ('one size field enlarged', lambda b: b[:HEAD + 8] + struct.pack('<q', 48 + 160) + b[HEAD + 16:], 'add up'),
    ('a negative size', lambda b: b[:HEAD + 8] + struct.pack('<q', -16) + b[HEAD + 16:], 'negative'),
    ('an overflowing size', lambda b: b[:HEAD + 8] + struct.pack('<q', 2 ** 62) + b[HEAD + 16:], 'overflowing'),
    ('a negative segment count', lambda b: b[:HEAD - 16] + struct.pack('<i', -3) + b[HEAD - 12:], 'segment count'),
    ('trailing bytes', lambda b: b + b'\0' * 16, 'trailing'),
    ('one trailing byte', lambda b: b + b'x', 'trailing'),
])
def test_import_refuses(what, mutate, reason):
    bad = mutate(_image())
    with pytest.raises(EngineError, match=reason):
        StreamSnapshot.from_bytes(bad)
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.se_stream_state_create(C.byref(h)) == 0
    assert lib.se_stream_state_import(h, bad, len(bad)) != 0 and reason in _err(lib), what
    assert lib.se_stream_state_bytes(h) == 0               # still empty
    assert lib.se_stream_state_import(h, None, 10) != 0 and 'null' in _err(lib)
    lib.se_stream_state_destroy(h)


def test_import_refuses_a_misplaced_window_and_bad_counters():
    img = _image()
    w = HEAD + 3 * 16                                       # the window's table row: make it a history segment, window first
    swapped = img[:HEAD] + struct.pack('<iiq', KIND_WINDOW, 0, 48) + img[HEAD + 16:w] + struct.pack('<iiq', KIND_HIST, 0, 800) + img[w + 16:]
    with pytest.raises(EngineError, match='window'):
        StreamSnapshot.from_bytes(swapped)
    with pytest.raises(EngineError, match='counters'):
        StreamSnapshot.from_bytes(img[:8 + 5 * 4] + struct.pack('<i', 0) + img[8 + 6 * 4:])          # batch 0


class _NoLib:
    def __getattr__(self, name):
        raise AssertionError(f'the library was called ({name}) by a wrapper that has to refuse first')


def _bare_engine(handle='handle', batch=2):
    e = Engine.__new__(Engine)
    e._lib, e._h, e.device, e._stream_batch = _NoLib(), handle, 0, batch
    e._stream = lambda: C.c_void_p(1)
    return e


def test_wrappers_refuse_before_the_library_is_called():
    snap = StreamSnapshot.from_bytes(_image())
    closed = StreamSnapshot()
    closed.close()
    closed.close()                                          # twice is fine
    eng = _bare_engine()
    for method in ('stream_save', 'stream_restore'):
        with pytest.raises(EngineError, match=f'^{method}: expected a StreamSnapshot, got bytes$'):
            getattr(eng, method)(b'abc')
        with pytest.raises(EngineError, match=f'^{method}: the snapshot is closed$'):
            getattr(eng, method)(closed)
        with pytest.raises(EngineError, match=f'^{method}: the engine is closed$'):
            getattr(_bare_engine(handle=C.c_void_p()), method)(snap)
    with pytest.raises(EngineError, match='^stream_restore: expected a StreamSnapshot, got NoneType$'):
        eng.stream_restore(None)
    with pytest.raises(EngineError, match='^stream_save: the engine is closed$'):
        _bare_engine(handle=C.c_void_p()).stream_save()
    with pytest.raises(EngineError, match='^stream_save without stream_begin$'):
        _bare_engine(batch=0).stream_save(snap)
    with pytest.raises(EngineError, match='closed'):
        closed.nbytes
    with pytest.raises(EngineError, match='closed'):
        closed.to_bytes()
    with pytest.raises(EngineError, match='expected bytes, got str'):
        StreamSnapshot.from_bytes('abc')
    snap.close()


def test_manifest_code_is_host_only_and_clean_under_the_host_sanitizers(tmp_path):
    """stream_manifest.h includes no HIP; its stand-alone check program, built with -fsanitize=address,undefined, builds and parses
    manifests of 0, 1 and 300 segments and feeds the parser the malformed images.  Run as a program of its own."""
    src = open(os.path.join(CSRC, 'stream_manifest.h')).read()
    assert 'hip' not in src.replace('no HIP', '').lower()
    cxx = shutil.which(os.environ.get('CXX', 'g++')) or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'stream_manifest_check')
    subprocess.run([cxx, '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                    os.path.join(CSRC, 'tests', 'stream_manifest_check.cpp'), '-o', exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), (r.returncode, r.stdout, r.stderr)
