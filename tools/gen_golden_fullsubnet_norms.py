"""Golden fixtures for FullSubNet's `offline_gaussian_norm` and `cumulative_layer_norm`, by IMPORTING the reference.

TEST INFRASTRUCTURE, build container only (needs the reference tree, as oracle/gen_golden.py does).  Run:
    python tools/gen_golden_fullsubnet_norms.py [outdir]        (default: tests/golden)
Synthetic weights come from (schema, seed 15) through se_amd.synth - the norms have no parameters, the schema is
schema_fullsubnet.json - so the fixtures hold inputs and reference outputs only.

What is imported: FullSubNet/fullsubnet_net_sa/model.py (class Model, norm_type = ... selected at base_model.py:296-308) through
oracle.gen_golden._fsn_model; the decode loop around it is oracle.gen_golden._enhance_fullsubnet (fullsubnet_sa_decode_vb.py:37-72).
Every clip runs through the reference on its own (`drop_band` fires at batch > 1, model.py:101-104), as in the existing fixtures.

  fullsubnet_gauss.npz  norm_type="offline_gaussian_norm" (base_model.py:242-255): x = |N(0,1)| default_rng(39) [2,1,257,9] and y;
                        wav = clip 11 (speech, 6000) and enh_cprs (0.5 / 2.0); wav_b = clip 64 (white, 5000) and enh_b_cprs, the ragged
                        partner (oracle/ has no Gaussian norm, so the partner's reference output comes from here)
  fullsubnet_cln.npz    norm_type="cumulative_layer_norm" (base_model.py:258-294): the same with default_rng(49) [2,1,257,11], clips 12
                        and 65, plus wav2 = clip 13 (speech, 32000) and enh2_cprs for the streamed decode; min_var_eps: the smallest
                        var + EPSILON the reference's norm formed over all of these runs (see below)

Conditioning.  cumulative_layer_norm evaluates var = (S2 - 2 mean S1) / n + mean^2 in float32, which cancels: where var + EPSILON
comes out tiny (or negative) the reference's own output is rounding noise and parity on it pins nothing.  The norm is wrapped for the
run, the smallest var + EPSILON over every call is printed and stored, and the script refuses to write the fixtures unless it is
positive and not vanishing (> 1e-4, three hundred times sqrt-argument EPSILON = 1.19e-7) and every reference output is finite.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as G  # noqa: E402
from se_amd import synth  # noqa: E402

EPSILON = float(np.finfo(np.float32).eps)      # fullsubnet_net_sa constant.py:8
MIN_VAR_EPS = 1e-4


def watch_cln(model):
    """Wrap model.norm: record the smallest var + EPSILON cumulative_layer_norm forms (its own float32 expression, restated on the
    same input), and return the list the minima go to."""
    seen = []
    inner = model.norm

    def norm(x):
        b, c, f, t = x.shape
        v = x.reshape(b * c, f, t)
        s1 = torch.cumsum(torch.sum(v, dim=1), dim=-1)
        s2 = torch.cumsum(torch.sum(torch.square(v), dim=1), dim=-1)
        n = torch.arange(f, f * t + 1, f, dtype=v.dtype).reshape(1, t).expand_as(s1)
        mean = s1 / n
        var = (s2 - 2 * mean * s1) / n + mean.pow(2)
        seen.append(float((var + EPSILON).min()))
        return inner(x)

    model.norm = norm
    return seen


def gen(tag, norm_type, rng_seed, frames, clip, clip_b, clip2=None):
    torch.manual_seed(0)
    model = G._fsn_model(norm_type=norm_type)
    G.load_synth(model, 15)
    seen = watch_cln(model) if norm_type == 'cumulative_layer_norm' else None
    rng = np.random.default_rng(rng_seed)
    x = np.abs(rng.standard_normal((1, 1, 257, frames))).astype(np.float32)
    x2 = np.abs(rng.standard_normal((1, 1, 257, frames))).astype(np.float32)
    with torch.no_grad():
        y = model(torch.from_numpy(x)).numpy()
        y2 = model(torch.from_numpy(x2)).numpy()
    wav = synth.synth_clip(clip, 'speech', 6000)
    wav_b = synth.synth_clip(clip_b, 'white', 5000)
    arrs = dict(x=np.concatenate([x, x2]), y=np.concatenate([y, y2]), wav=wav, enh_cprs=G._enhance_fullsubnet(model, wav, 0.5, 2.0),
                wav_b=wav_b, enh_b_cprs=G._enhance_fullsubnet(model, wav_b, 0.5, 2.0))
    if clip2 is not None:
        arrs['wav2'] = synth.synth_clip(clip2, 'speech', 32000)
        arrs['enh2_cprs'] = G._enhance_fullsubnet(model, arrs['wav2'], 0.5, 2.0)
    for k, v in arrs.items():
        assert np.isfinite(v).all(), f'{tag}: reference output {k} is not finite'
    if seen is not None:
        worst = min(seen)
        print(f'{tag}: smallest var + EPSILON of the reference cumulative_layer_norm over {len(seen)} calls: {worst:.6g}')
        assert worst > MIN_VAR_EPS, f'{tag}: the reference norm is ill-conditioned on these inputs ({worst}); pick other seeds'
        arrs['min_var_eps'] = np.float64(worst)
    G.save(tag, **arrs)


def main(out=None):
    if out:
        G.GOLD = out
    os.makedirs(G.GOLD, exist_ok=True)
    gen('fullsubnet_gauss', 'offline_gaussian_norm', 39, 9, 11, 64)
    gen('fullsubnet_cln', 'cumulative_layer_norm', 49, 11, 12, 65, clip2=13)


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else None)
