"""gemmconv's tile selection on a CPU: gc_select (csrc/gc_select.h, through the host-only probe csrc/tests/gc_select_probe.cpp ->
libse_gcselprobe.so) is given every launch recorded in tests/golden/gc_select_parent.jsonl.gz and has to return the launch records
the commit BEFORE the selector existed produced for it on the GPU (tools/gc_select_record.py wrote the fixture: the inputs from
this code's gc_launch, the records and plan facts from a probe library built from the parent commit)."""
import ctypes as C
import gzip
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_LIB = os.path.join(ROOT, 'sixty-years-of-frequency-domain-monaural-speech-enhancement_amd', 'libse_gcselprobe.so')
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'gc_select_parent.jsonl.gz')

# gcp_launch_get / gcs_select: the fields of one launch record
REC = ('family', 'BM', 'BN', 'flat_upr', 'upt', 'flat_rows', 'qt2', 'nrm', 'res', 'trim', 'stats', 'ragged', 'flat_nrm_refused', 'nblk')
# gcp_select_get / gcs_select: GCSelIn as integers, in the order of the struct's declaration (csrc/tests/gc_selin_flat.h)
GEOMS = ('main', 'n32', 'n64', 'n256', 'qt2', 'flat128', 'flat256')
SELIN = ('BM', 'BN') + tuple(f'BN_{g}' for g in GEOMS) + tuple(f'Wp_{g}' for g in GEOMS) + (
    'flat_uw', 'tail_split', 'qt2_nrows', 'qt2_qoff', 'CI_C', 'nrows', 'KCp', 'causal', 'sm_dfmin', 'sm_dfmax', 'sm_dtmin', 'sm_dtmax',
    'pl_C0', 'pl_C1', 'pl_epi', 'pl_Ws', 'epi', 'Z', 'B', 'Q', 'M', 'n_mtiles', 'Tout', 'Tin', 'Fin', 't_base', 'tb_soft', 'C0', 'C1',
    'pad_lo', 'first_step', 'pair', 'si', 's0_b', 's0_c', 's0_f', 's1_b', 's1_c', 's1_f', 'Ws', 'desc4', 'stats', 'cstats', 'nrm0',
    'nrm1', 'fz', 'dst_elu', 'tlen', 'overread0', 'overread1', 'alt_n64', 'wide_min', 'wide_fill', 'qt2_min', 'flat', 'dbg')


def lib():
    assert os.path.exists(PROBE_LIB), 'libse_gcselprobe.so is missing: run build() (make -C csrc)'
    L = C.CDLL(PROBE_LIB)
    L.gcs_last_error.restype = C.c_char_p
    L.gcs_select.argtypes = [C.POINTER(C.c_longlong)] * 3
    L.gcs_flat_rows_spanned.argtypes = [C.c_int] * 3
    assert L.gcs_selin_fields() == len(SELIN)
    return L


def fixture():
    return [json.loads(l) for l in gzip.open(FIXTURE, 'rt')]


def select(L, selin):
    """The launch records gc_select's choice for one gc_launch call leaves (the tail launch first)."""
    assert len(selin) == len(SELIN)
    out = (C.c_longlong * 28)()
    extra = (C.c_longlong * 16)()
    n = L.gcs_select((C.c_longlong * len(selin))(*selin), out, extra)
    assert n > 0, L.gcs_last_error().decode()
    return [list(out[14 * i: 14 * i + 14]) for i in range(n)]


def test_fixture_covers_the_ladder():
    """The recorded launches reach every family and tile the geometry test targets (a fixture that lost them checks nothing)."""
    recs = [dict(zip(REC, r)) for case in fixture() for r in case['recs']]
    assert len(recs) > 500
    tiles = {(r['BM'], r['BN']) for r in recs if r['family'] == 0}
    assert tiles >= {(64, 64), (64, 128), (64, 256), (128, 32), (128, 128)}
    assert {r['family'] for r in recs} >= {0, 1, 3, 4}
    assert any(r['flat_upr'] and r['nrm'] for r in recs) and any(r['flat_upr'] and r['ragged'] for r in recs)
    assert any(r['qt2'] for r in recs) and any(r['res'] for r in recs) and any(r['flat_nrm_refused'] for r in recs)
    assert any(r['stats'] for r in recs)


def test_gc_select_gives_the_parent_commits_launches():
    L = lib()
    n = 0
    for case in fixture():
        got = [r for s in case['selin'] for r in select(L, s)]
        assert got == case['recs'], (case['key'], [dict(zip(REC, r)) for r in got], [dict(zip(REC, r)) for r in case['recs']])
        n += len(got)
    assert n > 500


def rows_spanned(B, upr, upt):
    """Most batch rows one flattened tile of `upt` 32-frame units touches (B rows of `upr` units end to end): every tile scanned."""
    units = B * upr
    most = 0
    for k in range((units + upt - 1) // upt):
        u0 = k * upt
        u1 = min(u0 + upt, units) - 1
        most = max(most, u1 // upr - u0 // upr + 1)
    return most


@pytest.mark.parametrize('upt', [4, 8])
def test_flat_rows_spanned(upt):
    L = lib()
    for B in range(1, 10):
        for upr in range(1, 15):
            assert L.gcs_flat_rows_spanned(B, upr, upt) == rows_spanned(B, upr, upt), (B, upr, upt)
