"""CPU: the host side of joining parked streams that began at different times (se_stream_state_join / se_stream_state_counts of
include/se_engine.h, StreamSnapshot.join / .counts and samples_until_joinable of se_amd.engine).  The join needs an engine - a device -
to be called at all; what decides it - the left-edge threshold, the shifts, the joined window, every refusal - are pure functions
of csrc/stream_join.h and run in a stand-alone program under the host sanitizers (csrc/tests/stream_join_check.cpp).  The counters of
a parked stream are a host record and are read here off an imported image."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import pytest

import se_amd  # noqa: F401
from se_amd import _lib
from se_amd import engine as E
from se_amd.engine import EngineError, StreamSnapshot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'sixty-years-of-frequency-domain-monaural-speech-enhancement_amd', 'csrc')
NEW_SYMBOLS = ['se_stream_state_join', 'se_stream_state_counts']


def _image(batch=2, n_total=3700, t_done=26, o_done=3000, keep=3600, hop=128):
    """a well-formed stream image (csrc/stream_manifest.h) with the input window as its only segment"""
    win = batch * (n_total - keep) * 4
    return struct.pack('<II18iffiiq', 0x54534553, 1, 5, 0, 512, hop, 512, batch, 16, n_total, t_done, o_done, keep, 0, 0, 1, 0, 0, 0, 0,
                       0.5, 2.0, 1, 0, (win + 15) // 16 * 16) + struct.pack('<iiq', 8, 0, win) + bytes((win + 15) // 16 * 16)


def test_binding_declares_the_entry_points_and_the_abi_stays_5():
    hdr = open(os.path.join(ROOT, 'include', 'se_engine.h')).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS
        assert name + '(' in hdr
    lib = _lib.load()
    assert len(lib.se_stream_state_join.argtypes) == 5 and len(lib.se_stream_state_counts.argtypes) == 6
    assert lib.se_abi_version() == 5
    assert callable(StreamSnapshot.join) and callable(StreamSnapshot.counts) and callable(E.samples_until_joinable)


def test_counts_reads_an_imported_image_without_a_device():
    lib = _lib.load()
    with StreamSnapshot.from_bytes(_image()) as snap:
        assert snap.counts() == (2, 3700, 26, 3000, 128)
        # any out-pointer may be NULL
        n, hop = C.c_int64(-1), C.c_int32(-1)
        assert lib.se_stream_state_counts(snap._h, None, C.byref(n), None, None, None) == 0 and n.value == 3700
        assert lib.se_stream_state_counts(snap._h, None, None, None, None, C.byref(hop)) == 0 and hop.value == 128
        assert lib.se_stream_state_counts(snap._h, None, None, None, None, None) == 0
    with StreamSnapshot.from_bytes(_image(1, 9000, 55, 8640, 8676, 160)) as snap:
        assert snap.counts() == (1, 9000, 55, 8640, 160)


def test_counts_of_an_empty_or_closed_object_is_an_error():
    lib = _lib.load()
    empty = StreamSnapshot()
    n = C.c_int64(-7)
    assert lib.se_stream_state_counts(empty._h, None, C.byref(n), None, None, None) != 0 and n.value == -7
    assert 'se_stream_state_counts: the stream state object is empty' in lib.se_last_error(None).decode()
    assert lib.se_stream_state_counts(None, None, None, None, None, None) != 0 and 'null' in lib.se_last_error(None).decode()
    with pytest.raises(EngineError, match='the stream state object is empty'):
        empty.counts()
    empty.close()
    with pytest.raises(EngineError, match=r'^StreamSnapshot.counts: the snapshot is closed$'):
        empty.counts()


def test_join_without_an_engine_is_an_error_not_a_crash():
    lib = _lib.load()
    with StreamSnapshot.from_bytes(_image()) as snap, StreamSnapshot() as dst:
        assert lib.se_stream_state_join(None, dst._h, (C.c_void_p * 1)(snap._h.value), 1, None) != 0
        with pytest.raises(EngineError, match='^join: expected an Engine, got NoneType$'):
            StreamSnapshot.join(None, [snap])
        with pytest.raises(EngineError, match='^join: expected an Engine, got str$'):
            StreamSnapshot.join('engine', [snap], out=dst)
        assert dst.nbytes == 0


def test_samples_until_joinable():
    f = E.samples_until_joinable
    group = (3, 48000, 299, 47680, 160)
    assert f((1, 48000 - 5 * 160, 294, 0, 160), group) == 0
    assert f((1, 1000, 6, 0, 160), group) == (48000 - 1000) % 160 == 120
    assert f((1, 48000 + 7, 0, 0, 160), group) == 153                  # ahead of the group: the join rebases either way
    assert all(0 <= f((1, n, 0, 0, 160), group) < 160 and (48000 - n - f((1, n, 0, 0, 160), group)) % 160 == 0 for n in range(0, 700, 7))
    assert f((1, 1000, 6, 0, 160), (3, 48000, 374, 47616, 128)) is None           # other front ends never meet
    assert f((1, 1000, 0, 0, 6), (1, 1006, 0, 0, 6)) == 6 and f((1, 1000, 0, 0, 6), (1, 1012, 0, 0, 6)) == 0      # lcm(6, 4) = 12
    with StreamSnapshot.from_bytes(_image()) as g, StreamSnapshot.from_bytes(_image(1, 3700 - 2 * 128 - 28, 23, 2688, 3280)) as a:
        assert f(a, g) == 28 and f(g, g) == 0
    with pytest.raises(EngineError, match='expected two'):
        f((1, 2, 3), group)


def test_threshold_and_plan_are_host_only_and_clean_under_the_host_sanitizers(tmp_path):
    """stream_join.h includes no HIP; its stand-alone check program, built with -fsanitize=address,undefined and run directly, walks a
    stream sample by sample through every index expression that tests against position 0 (320 / 160, 512 / 128, 400 / 160; look-ahead
    0, 2, 6) and finds the threshold stream_left_edge_frames() gives, and checks the join plan: shifts, the joined window, per-part
    columns, and each refusal for the defect it has."""
    src = open(os.path.join(CSRC, 'stream_join.h')).read()
    assert 'hip' not in src.replace('no HIP', '').lower()
    cxx = shutil.which(os.environ.get('CXX', 'g++')) or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'stream_join_check')
    subprocess.run([cxx, '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                    os.path.join(CSRC, 'tests', 'stream_join_check.cpp'), '-o', exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), (r.returncode, r.stdout, r.stderr)
