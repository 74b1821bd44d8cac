"""Big batches of short clips through the InstanceNorm networks whose U^2-Net levels normalise their sources on the fly.

G2Net (and TaylorSENet with SE_IN_FOLD=2) run their 64 -> 64 levels with the InstanceNorm of the source applied inside the conv
(gc_kernel NRM).  At batch 256 those launches take the unit-flattened 64 x 256 tiles, and with rows of 3 or 5 units (T around 80
and 150 frames, rounded up to 96 / 160 by the row padding) a tile of 8 units spans three or four batch rows - more than the tile
holds norm parameters for.  gc_launch refuses the flattened tiles there; these decodes would come out finite and wrong otherwise.

Rows are 7 distinct clips repeated (7 is coprime with the 8 units of a tile, so every clip sits at every unit position) and each
row is compared with the float64 oracle of its clip at the bar of test_gpu_edge_cases.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import se_amd  # noqa: F401
from se_amd import synth
from conftest import rms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = {'g2net': 20, 'taylorsenet': 19}
KINDS = ('speech', 'white', 'speech', 'gap')
HOP = 160
# clip lengths (samples) and frames T = L // 160 + 1: 80 (-> 96 with the row padding: 3 units per row) and 150 (-> 160: 5 units)
L80, L150 = 79 * HOP, 149 * HOP


def _check_rows(name, y, clips, rows_of, lengths=None):
    from oracle import decode as D
    from se_amd.models import MODEL_CLASSES
    m = MODEL_CLASSES[name](max_batch=1, max_samples=16000)
    sd = synth.synth_state_dict(m.state_dict_schema(), SEEDS[name])
    worst = 0.0
    for i, c in enumerate(clips):
        ref = D.ENHANCE[name](sd, c, 0.5, 2.0, net_dtype=np.float64)
        for b in rows_of(i):
            e = rms(y[b, :len(ref)] - ref)
            assert np.isfinite(y[b]).all(), (name, b)
            assert e < 1e-4 and e < 5e-4 * max(rms(ref), 1e-3), (name, 'row', b, 'clip', i, len(c), e, rms(ref))
            worst = max(worst, e / max(rms(ref), 1e-3))
    return worst


def check_equal_length_batch(name, L, B=256):
    """B rows of 7 clips of L samples, one se_enhance_batch call, every row against the oracle."""
    import torch
    from se_amd.models import MODEL_CLASSES
    m = MODEL_CLASSES[name](max_batch=B, max_samples=L, p_in=0.5, p_out=2.0).load_synthetic(SEEDS[name])
    clips = [synth.synth_clip(900 + i, KINDS[i % 4], L) for i in range(7)]
    x = np.stack([clips[b % 7] for b in range(B)])
    y = m.enhance_batch(torch.from_numpy(x).cuda()).cpu().numpy()
    worst = _check_rows(name, y, clips, lambda i: range(i, B, 7))
    print(name, 'B', B, 'L', L, 'worst relative rms err', worst)


@pytest.mark.gpu
def test_short_clip_rows_reach_the_refused_flattened_tiles():
    """The (B, T) of the decodes below put the U^2-Net level launches (64 -> 64, 79 -> 39 rows, sources normalised) where a
    flattened tile would span more than two rows: the probe of that layer shows gc_launch refusing it."""
    from test_gpu_gemmconv_geometry import SHAPES, probe_for, run_case, rows_spanned, FAM_TILE
    sh = SHAPES['g2net_level']
    probe, w, bias, slope = probe_for('g2net_level')
    for T, upr in ((96, 3), (160, 5)):
        assert rows_spanned(256, upr, 8) > 2
        recs = run_case(probe, sh, w, bias, slope, 256, T, nrm=True, stats=True, seed=T)
        tiles = [r for r in recs if r['family'] == FAM_TILE]
        assert any(r['flat_nrm_refused'] == rows_spanned(256, upr, 8) for r in tiles), (T, recs)
        assert not any(r['flat_upr'] for r in tiles), (T, recs)


@pytest.mark.gpu
@pytest.mark.parametrize('L', [L80, L150])
def test_g2net_batch256_short_clips_match_oracle(L):
    check_equal_length_batch('g2net', L)


@pytest.mark.gpu
def test_g2net_ragged_batch_with_short_longest_row():
    """se_enhance_ragged with 256 rows of 7 lengths, the longest of about 150 frames (upr 5 after the row padding)."""
    import torch
    from se_amd.models import MODEL_CLASSES
    lengths7 = [L150, 22001, 20480, 19200, 17777, 16400, 15007]
    B = 256
    m = MODEL_CLASSES['g2net'](max_batch=B, max_samples=L150, p_in=0.5, p_out=2.0).load_synthetic(SEEDS['g2net'])
    clips = [synth.synth_clip(950 + i, KINDS[i % 4], n) for i, n in enumerate(lengths7)]
    lengths = [lengths7[b % 7] for b in range(B)]
    x = np.zeros((B, L150), np.float32)
    for b in range(B):
        c = clips[b % 7]
        x[b, :len(c)] = c
        x[b, len(c):] = 0.25 * np.sin(0.01 * np.arange(L150 - len(c)))      # junk past a row's end must be ignored
    y = m.enhance_ragged(torch.from_numpy(x).cuda(), lengths).cpu().numpy()
    _check_rows('g2net', y, clips, lambda i: range(i, B, 7))


def _child(env, L):
    code = ('import sys; sys.path[:0] = [%r, %r]; import test_gpu_short_clip_batches as t; '
            't.check_equal_length_batch("taylorsenet", %d)' % (os.path.join(ROOT, 'tests'), ROOT, L))
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, **env), cwd=ROOT, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_taylorsenet_folded_norm_batch256_short_clips():
    """TaylorSENet normalises on the fly with SE_IN_FOLD=2 (read once per process: a child process each).  Batch 256 decodes as two
    halves of 128: at 160 frames each half still clears the wide-tile threshold; at 96 frames only the whole batch does."""
    _child({'SE_IN_FOLD': '2'}, L150)
    _child({'SE_IN_FOLD': '2', 'SE_BATCH_SPLIT': '0'}, L80)
