"""CPU: the host side of parking and resuming source-rate signals (se_resampler_state_*, se_resampler_save, se_resampler_restore of
include/se_engine.h).  The object is created, queried and destroyed without a device; se_resampler_state_import parses, validates
and refuses on the host; the Python wrappers refuse a closed snapshot, a closed resampler and a wrong type before the library is
called.  Images are built here from the layout csrc/resampler_manifest.h documents - there is no GPU to export one from.  The
manifest code itself runs under the host sanitizers in a stand-alone program (csrc/tests/resampler_manifest_check.cpp)."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import pytest

import se_amd  # noqa: F401
from se_amd import _lib
from se_amd.engine import EngineError, StreamSnapshot
from se_amd.resample import ResamplerSnapshot, StreamResampler
from se_amd.source_stream import SourceRateStream, SourceStreamSnapshot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'sixty-years-of-frequency-domain-monaural-speech-enhancement_amd', 'csrc')
NEW_SYMBOLS = ['se_resampler_state_create', 'se_resampler_state_destroy', 'se_resampler_state_bytes', 'se_resampler_state_counts',
               'se_resampler_save', 'se_resampler_restore', 'se_resampler_state_export', 'se_resampler_state_import']
HEAD = 64                       # magic, version, sr_in, sr_out, batch, pad | n_total, w0, t, acc, payload bytes
REACH_48 = 193                  # 48 -> 16 kHz: floor(32769 / 170) + 1 (include/se_engine.h, LATENCY)


def _image(sr_in=48000, sr_out=16000, batch=2, n_total=5003, w0=5003 - 2 * REACH_48, t=1603, acc=4809.0):
    """a well-formed image: the header and batch rows of n_total - w0 floats"""
    pay = batch * (n_total - w0) * 4
    b = struct.pack('<II4iqqqdq', 0x53524553, 1, sr_in, sr_out, batch, 0, n_total, w0, t, acc, pay)
    assert len(b) == HEAD
    return b + bytes(range(256)) * (pay // 256) + bytes(pay % 256)


def _field(b, off, fmt, value):
    return b[:off] + struct.pack(fmt, value) + b[off + struct.calcsize(fmt):]


def _err(lib):
    return lib.se_last_error(None).decode()


def test_binding_declares_the_entry_points_and_the_abi_stays_5():
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS
    hdr = open(os.path.join(ROOT, 'include', 'se_engine.h')).read()
    for name in NEW_SYMBOLS:
        assert name + '(' in hdr
    assert 'typedef struct se_resampler_state se_resampler_state;' in hdr
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
    assert len(lib.se_resampler_save.argtypes) == 3 and len(lib.se_resampler_restore.argtypes) == 3
    assert len(lib.se_resampler_state_export.argtypes) == 3 and len(lib.se_resampler_state_import.argtypes) == 3
    assert len(lib.se_resampler_state_counts.argtypes) == 6
    assert lib.se_abi_version() == 5


def test_create_is_empty_and_export_and_counts_of_an_empty_object_are_refused():
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.se_resampler_state_create(C.byref(h)) == 0 and h.value
    assert lib.se_resampler_state_bytes(h) == 0
    assert lib.se_resampler_state_export(h, None, 0) == -1 and 'empty' in _err(lib)
    buf = C.create_string_buffer(64)
    assert lib.se_resampler_state_export(h, C.cast(buf, C.c_void_p), 64) == -1 and 'empty' in _err(lib)
    n = C.c_int64(-7)
    assert lib.se_resampler_state_counts(h, None, None, None, C.byref(n), None) != 0 and 'empty' in _err(lib) and n.value == -7
    assert lib.se_resampler_state_destroy(h) == 0
    assert lib.se_resampler_state_destroy(None) == 0
    assert lib.se_resampler_state_create(None) != 0 and 'null' in _err(lib)
    with ResamplerSnapshot() as snap:
        assert snap.nbytes == 0
        with pytest.raises(EngineError, match='empty'):
            snap.to_bytes()
        with pytest.raises(EngineError, match='empty'):
            snap.counts()


@pytest.mark.parametrize('kw,counts', [
    ({}, (48000, 16000, 2, 5003, 1603)),
    (dict(n_total=0, w0=0, t=0, acc=0.0), (48000, 16000, 2, 0, 0)),                                    # before the first push
    (dict(n_total=100, w0=0, t=0, acc=0.0, batch=3), (48000, 16000, 3, 100, 0)),                       # nothing released yet
    (dict(sr_in=44100, n_total=1681, w0=1681 - 356, t=546, acc=546 * 2.75625), (44100, 16000, 2, 1681, 546)),
    (dict(sr_in=16000, sr_out=48000, n_total=131, w0=1, t=198, acc=66.0), (16000, 48000, 2, 131, 198)),
    (dict(sr_in=16000, n_total=900, w0=900, t=900, acc=0.0), (16000, 16000, 2, 900, 900)),             # pass-through: counters only
])
def test_import_accepts_a_well_formed_image_and_gives_it_back(kw, counts):
    img = _image(**kw)
    with ResamplerSnapshot.from_bytes(img) as snap:
        assert snap.counts() == counts
        assert snap.nbytes == len(img) - HEAD
        assert snap.to_bytes() == img                      # acc included: its 8 bytes, never through a decimal
        # a refused import leaves the object as it was
        lib = _lib.load()
        assert lib.se_resampler_state_import(snap._h, b'nonsense' * 20, 160) != 0
        assert snap.to_bytes() == img and snap.counts() == counts


def test_acc_travels_as_its_eight_bytes():
    acc = 0.1 + 0.2                                         # 0.30000000000000004: not what a short decimal gives back
    img = _image(sr_in=44100, n_total=400, w0=44, t=1, acc=acc)
    with ResamplerSnapshot.from_bytes(img) as snap:
        assert snap.to_bytes()[48:56] == struct.pack('<d', acc)


@pytest.mark.parametrize('what,mutate,reason', [
    ('garbage', lambda b: bytes((37 * i + 11) & 255 for i in range(len(b))), 'magic'),
    ('the magic of a stream state image', lambda b: struct.pack('<I', 0x54534553) + b[4:], 'magic'),
    ('another version', lambda b: _field(b, 4, '<I', 7), 'version'),
    ('cut inside the magic', lambda b: b[:3], 'truncated'),
    ('cut inside the header', lambda b: b[:40], 'truncated'),
    ('cut inside the payload', lambda b: b[:-1], 'truncated'),
    ('the header alone', lambda b: b[:HEAD], 'truncated'),
    ('a payload size that is not batch * (n_total - w0) * 4', lambda b: _field(b, 56, '<q', 2 * 386 * 4 + 4), r'batch \* \(n_total - w0\) \* 4'),
    ('one row more than the payload', lambda b: _field(b, 16, '<i', 3), r'batch \* \(n_total - w0\) \* 4'),
    ('a negative payload size', lambda b: _field(b, 56, '<q', -8), 'negative or overflowing'),
    ('an overflowing payload size', lambda b: _field(b, 56, '<q', 2 ** 62), 'negative or overflowing'),
    ('negative n_total', lambda b: _field(b, 24, '<q', -1), 'negative counters'),
    ('negative w0', lambda b: _field(b, 32, '<q', -5), 'negative counters'),
    ('negative t', lambda b: _field(b, 40, '<q', -1), 'negative counters'),
    ('negative acc', lambda b: _field(b, 48, '<d', -0.5), 'negative counters'),
    ('acc not a number', lambda b: _field(b, 48, '<d', float('nan')), 'negative counters'),
    ('n_total past what se_resample accepts', lambda b: _field(b, 24, '<q', 2 ** 31), 'overflowing counters'),
    ('n_total that overflows', lambda b: _field(b, 24, '<q', 2 ** 63 - 1), 'overflowing counters'),
    ('t that overflows', lambda b: _field(b, 40, '<q', 2 ** 40), 'overflowing counters'),
    ('acc that overflows', lambda b: _field(b, 48, '<d', float('inf')), 'overflowing counters'),
    ('batch 0', lambda b: _field(b, 16, '<i', 0), 'rates or batch'),
    ('a negative rate', lambda b: _field(b, 8, '<i', -48000), 'rates or batch'),
    ('w0 > n_total', lambda b: _field(b, 32, '<q', 5004), 'behind the 5003 samples'),
    ('more history than 2 * reach', lambda b: _field(b, 32, '<q', 5003 - 387), r'more than 2 \* reach = 386 of 48000 -> 16000 Hz'),
    ('the history of 48 kHz under the rates of 32 kHz', lambda b: _field(b, 8, '<i', 32000), r'more than 2 \* reach = 258 of 32000 -> 16000 Hz'),
    ('a pass-through signal with a history', lambda b: _field(b, 8, '<i', 16000), 'pass-through'),
    ('trailing bytes', lambda b: b + b'\0' * 16, 'trailing'),
    ('one trailing byte', lambda b: b + b'x', 'trailing'),
])
def test_import_refuses(what, mutate, reason):
    bad = mutate(_image())
    with pytest.raises(EngineError, match=reason):
        ResamplerSnapshot.from_bytes(bad)
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.se_resampler_state_create(C.byref(h)) == 0
    assert lib.se_resampler_state_import(h, bad, len(bad)) != 0, what
    assert lib.se_resampler_state_bytes(h) == 0             # still empty
    assert lib.se_resampler_state_import(h, None, 10) != 0 and 'null' in _err(lib)
    lib.se_resampler_state_destroy(h)


class _NoLib:
    def __getattr__(self, name):
        raise AssertionError(f'the library was called ({name}) by a wrapper that has to refuse first')


def _bare_resampler(handle='handle', sr_in=48000, sr_out=16000, max_batch=2):
    r = StreamResampler.__new__(StreamResampler)
    r._lib, r._h, r.device, r._batch = _NoLib(), handle, 0, 2
    r.sr_in, r.sr_out, r.max_batch = sr_in, sr_out, max_batch
    r._stream = lambda: C.c_void_p(1)
    return r


def test_wrappers_refuse_before_the_library_is_called():
    snap = ResamplerSnapshot.from_bytes(_image())
    closed = ResamplerSnapshot()
    closed.close()
    closed.close()                                          # twice is fine
    assert closed.closed and not snap.closed
    rs = _bare_resampler()
    for method in ('save', 'restore'):
        with pytest.raises(EngineError, match=f'^{method}: expected a ResamplerSnapshot, got bytes$'):
            getattr(rs, method)(b'abc')
        with pytest.raises(EngineError, match=f'^{method}: expected a ResamplerSnapshot, got StreamSnapshot$'):
            with StreamSnapshot() as other:
                getattr(rs, method)(other)
        with pytest.raises(EngineError, match=f'^{method}: the snapshot is closed$'):
            getattr(rs, method)(closed)
        with pytest.raises(EngineError, match=f'^{method}: the resampler is closed$'):
            getattr(_bare_resampler(handle=C.c_void_p()), method)(snap)
    with pytest.raises(EngineError, match='^restore: expected a ResamplerSnapshot, got NoneType$'):
        rs.restore(None)
    with pytest.raises(EngineError, match='^save: the resampler is closed$'):
        _bare_resampler(handle=C.c_void_p()).save()
    for attr in ('nbytes', 'to_bytes', 'counts'):
        with pytest.raises(EngineError, match='closed'):
            v = getattr(closed, attr)
            v()
    with pytest.raises(EngineError, match='expected bytes, got str'):
        ResamplerSnapshot.from_bytes('abc')
    # what a restore can refuse, checked on the host: rates, rows (the wrapper object is never touched)
    assert rs.check_restore(snap) == (48000, 16000, 2, 5003, 1603)
    with pytest.raises(EngineError, match='44100 -> 16000 Hz'):
        _bare_resampler(sr_in=44100).check_restore(snap)
    with pytest.raises(EngineError, match='exceeds max_batch 1'):
        _bare_resampler(max_batch=1).check_restore(snap)
    with ResamplerSnapshot() as empty:
        with pytest.raises(EngineError, match='empty'):
            rs.check_restore(empty)
    snap.close()


def test_source_stream_snapshot_wrappers_refuse_on_the_host():
    pair = SourceStreamSnapshot()
    assert not pair.closed and pair.nbytes == 0
    src = SourceRateStream.__new__(SourceRateStream)
    src.engine, src.resampler, src._batch = _NoLib(), _bare_resampler(), 2
    for method in ('save', 'restore'):
        with pytest.raises(EngineError, match=f'^{method}: expected a SourceStreamSnapshot, got ResamplerSnapshot$'):
            getattr(src, method)(pair.resampler)
    with pytest.raises(EngineError, match='empty'):         # the resampler's half is checked before the engine is asked
        src.restore(pair)
    # a resampler half of another rate next to any engine half: refused before the engine is asked
    other = SourceStreamSnapshot(resampler=ResamplerSnapshot.from_bytes(_image(sr_in=44100, n_total=400, w0=44, t=1, acc=2.75625)))
    with pytest.raises(EngineError, match='44100 -> 16000 Hz'):
        src.restore(other)
    other.close()
    src._batch = 0
    with pytest.raises(EngineError, match='^save without begin$'):
        src.save()
    pair.close()
    assert pair.closed
    with pytest.raises(EngineError, match='^restore: the snapshot is closed$'):
        src.restore(pair)
    for bad, reason in [(b'\x05', 'truncated'), (struct.pack('<Q', 99) + b'abc', 'cut short'), ('abc', 'expected bytes, got str')]:
        with pytest.raises(EngineError, match=reason):
            SourceStreamSnapshot.from_bytes(bad)
    img = _image()
    with pytest.raises(EngineError, match='magic'):         # a resampler image where the engine's belongs
        SourceStreamSnapshot.from_bytes(struct.pack('<Q', len(img)) + img + struct.pack('<Q', len(img)) + img)


def test_manifest_code_is_host_only_and_clean_under_the_host_sanitizers(tmp_path):
    """resampler_manifest.h includes no HIP; its stand-alone check program, built with -fsanitize=address,undefined, builds and
    parses images of every rate pair and feeds the parser the malformed ones.  Run as a program of its own."""
    src = open(os.path.join(CSRC, 'resampler_manifest.h')).read()
    assert 'hip' not in src.lower()
    cxx = shutil.which(os.environ.get('CXX', 'g++')) or shutil.which('c++')
    if not cxx:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'resampler_manifest_check')
    subprocess.run([cxx, '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                    os.path.join(CSRC, 'tests', 'resampler_manifest_check.cpp'), '-o', exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), (r.returncode, r.stdout, r.stderr)
