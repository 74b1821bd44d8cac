"""GPU: DCCRN decodes an equal-length batch of 64 clips or more as parts side by side (csrc/engine.hip, csrc/batch_parts.h; DESIGN.md
3.9), like Uformer, DPCRN, CTSNet and TaylorSENet.  Rows are independent: every row of a split decode - DCCRN and its causal-decoder
configuration, batches 64, 65 and 67, and every part layout a switch reaches (SE_BATCH_LEAD: unequal parts, SE_BATCH_PARTS: three parts)
- against the same engine with SE_BATCH_SPLIT=0 in a fresh child process, under the bar tests/test_gpu_fallback_paths.py applies to the
split decodes of the other models.  A profiled call, a ragged call and a graph-replayed call on a split-capable engine run unsplit and
match too.  One child per (model, switches): it decodes all of its batches on one engine; the unsplit references are computed once."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, %r)
import se_amd
from se_amd import synth
from se_amd.models import DCCRN, DCCRN_SNR
name, out, extras = sys.argv[1], sys.argv[2], sys.argv[3] == '1'
batches = [int(v) for v in sys.argv[4:]]
L, MB = 8000, max(batches)
cls = {'dccrn': DCCRN, 'dccrn_snr': DCCRN_SNR}[name]
kw = dict(rnn_units=256, use_clstm=True, kernel_num=[32, 64, 128, 256, 256, 256], max_batch=MB, max_samples=L)
m = cls(**kw).load_synthetic(14)
eng = m.engine
x = torch.from_numpy(np.stack([synth.synth_clip(700 + b, 'speech', L) for b in range(MB)])).cuda()
res = {}
for B in batches:
    res['b%%d' %% B] = eng.enhance_batch(x[:B].contiguous()).cpu().numpy()
if extras:
    B = 64
    xb = x[:B].contiguous()
    eng.set_profiling(True)
    res['profiled'] = eng.enhance_batch(xb).cpu().numpy()
    prof = eng.get_profile()
    eng.set_profiling(False)
    res['profiled_work'] = np.array([prof['gemm_launches'], prof['gemm_flops']], dtype=np.float64)
    lengths = [L - 131 * (b %% 7) for b in range(B)]
    res['ragged'] = eng.enhance_ragged(xb, lengths).cpu().numpy()
    g = cls(graphs=True, **kw).load_synthetic(14)
    for _ in range(3):          # eager on the capture stream, captured, replayed
        y = g.engine.enhance_batch(xb)
    res['graph'] = y.cpu().numpy()
torch.cuda.synchronize()
np.savez(out, **res)
"""

BATCHES = (64, 65, 67)
_cache = {}


def _decode(tmp, name, env, batches, extras=False):
    """the child's arrays for (model, switches): one child per key"""
    key = (name, tuple(sorted(env.items())), tuple(batches), extras)
    if key not in _cache:
        out = os.path.join(tmp, 'y%d.npz' % len(_cache))
        r = subprocess.run([sys.executable, '-c', _CHILD % ROOT, name, out, '1' if extras else '0'] + [str(b) for b in batches],
                           env=dict(os.environ, **env), cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        _cache[key] = dict(np.load(out))
    return _cache[key]


@pytest.fixture(scope='module')
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp('dccrn_split'))


def _reference(tmp, name):
    """one unsplit decode per model for every batch and call kind the tests below compare against"""
    return _decode(tmp, name, {'SE_BATCH_SPLIT': '0'}, BATCHES + (193,), extras=True)


def _same_rows(a, b, what):
    assert a.shape == b.shape and np.isfinite(a).all(), what
    scale = float(np.sqrt(np.mean(b.astype(np.float64) ** 2)))
    err = float(np.abs(a.astype(np.float64) - b).max())
    print(what, 'max abs diff', err, 'rms', scale, 'bit-equal', bool(np.array_equal(a, b)))
    assert err <= 2e-5 * max(scale, 1e-3), (what, err, scale)


@pytest.mark.gpu
@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('name', ['dccrn', 'dccrn_snr'])
def test_split_decode_equals_one_decode_row_for_row(tmp, name, B):
    got = _decode(tmp, name, {}, BATCHES, extras=True)
    _same_rows(got['b%d' % B], _reference(tmp, name)['b%d' % B], (name, B))


# the layouts the switches reach: unequal parts (64 -> 40 + 24; 67 -> 40 + 27, a last part of 24 rows and a group of 3), three parts
# from 192 clips on (193 -> 65 + 65 + 63), three unequal parts (193 -> 80 + 72 + 41)
@pytest.mark.gpu
@pytest.mark.parametrize('env,B', [({'SE_BATCH_LEAD': '10'}, 64), ({'SE_BATCH_LEAD': '10'}, 67), ({'SE_BATCH_LEAD': '6'}, 65),
                                   ({'SE_BATCH_PARTS': '3'}, 193), ({'SE_BATCH_PARTS': '3', 'SE_BATCH_LEAD': '10'}, 193),
                                   ({'SE_BATCH_PARTS': '1'}, 64)])
def test_every_part_layout_a_switch_reaches_equals_one_decode(tmp, env, B):
    batches = (193,) if B == 193 else BATCHES
    got = _decode(tmp, 'dccrn', env, batches)
    _same_rows(got['b%d' % B], _reference(tmp, 'dccrn')['b%d' % B], (env, B))


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['profiled', 'ragged', 'graph'])
@pytest.mark.parametrize('name', ['dccrn', 'dccrn_snr'])
def test_profiled_ragged_and_replayed_calls_run_unsplit_and_match(tmp, name, kind):
    got, ref = _decode(tmp, name, {}, BATCHES, extras=True), _reference(tmp, name)
    _same_rows(got[kind], ref[kind], (name, kind))
    if kind == 'profiled':      # one decode under the profiler: the launches and the flops of all 64 rows on the first instance
        assert got['profiled_work'][0] > 0 and np.array_equal(got['profiled_work'], ref['profiled_work']), (got['profiled_work'], ref['profiled_work'])
    if kind == 'graph':         # (and the replayed decode is the eager one)
        _same_rows(got[kind], ref['b64'], (name, kind, 'eager'))
