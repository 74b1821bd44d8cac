"""CPU: the surface of the tracking unit-RMS scale (se_stream_begin_tracking / se_stream_scale of include/se_engine.h) that needs no
device: the declarations and the ABI number, the counters of an imported image whose scale mode is 2, and the host arithmetic a
tracking stream adds to the join (csrc/stream_join.h: ring rotation, live entries, the plan and its refusals) as a stand-alone program
under the host sanitizers (csrc/tests/stream_track_join_check.cpp)."""
import os
import shutil
import struct
import subprocess

import se_amd  # noqa: F401
from se_amd import _lib
from se_amd.engine import StreamSnapshot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(os.path.abspath(se_amd.__file__)), 'csrc')


def test_header_declares_the_entry_points_and_the_abi_stays_5():
    hdr = open(os.path.join(ROOT, 'include', 'se_engine.h')).read()
    for name in ('se_stream_begin_tracking', 'se_stream_scale'):
        assert name in _lib.SYMBOLS
        assert 'int ' + name + '(se_engine* e' in hdr
    lib = _lib.load()
    assert lib.se_abi_version() == 5
    assert hasattr(lib, 'se_stream_begin_tracking') and hasattr(lib, 'se_stream_scale')


def test_null_engine_is_refused():
    lib = _lib.load()
    assert lib.se_stream_begin_tracking(None, 1, 4, 8000.0, None) != 0
    assert lib.se_stream_scale(None, None, None) != 0


def test_imported_tracking_image_reports_its_counts():
    """csrc/stream_manifest.h: scale mode `running` = 2, tau_samples as float bits in reserved[0]; segments c, (E, W), the two rings, window"""
    batch, n_total, t_done, o_done, keep, hop, ring = 2, 3700, 26, 3000, 3600, 128, 64
    tau_bits = struct.unpack('<i', struct.pack('<f', 8000.0))[0]
    segs = [(1, 0, batch * 4), (2, 0, batch * 16), (3, 0, batch * ring * 4), (3, 1, batch * ring * 4), (8, 0, batch * (n_total - keep) * 4)]
    pay = sum((b + 15) // 16 * 16 for _, _, b in segs)
    img = struct.pack('<II18iffiiq', 0x54534553, 1, 5, 0, 512, hop, 512, batch, 16, n_total, t_done, o_done, keep, 2, ring, 0, 0, tau_bits, 0, 0,
                      0.5, 2.0, len(segs), 0, pay)
    img += b''.join(struct.pack('<iiq', *s) for s in segs) + bytes(pay)
    with StreamSnapshot.from_bytes(img) as snap:
        assert snap.counts() == (batch, n_total, t_done, o_done, hop)
        assert snap.to_bytes() == img


def test_join_arithmetic_of_tracking_streams_under_the_host_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get('CXX', 'g++')) or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'stream_track_join_check')
    subprocess.run([cxx, '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                    os.path.join(CSRC, 'tests', 'stream_track_join_check.cpp'), '-o', exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), (r.returncode, r.stdout, r.stderr)
