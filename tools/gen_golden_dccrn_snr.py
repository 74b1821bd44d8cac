"""Golden fixtures for the DCCRN of `DCCRN_SNR/` (the causal-decoder DCCRN of the WSJ0-SI84 grid), by IMPORTING the reference.

TEST INFRASTRUCTURE, build container only (needs the reference tree, as oracle/gen_golden.py does).  Run:
    python tools/gen_golden_dccrn_snr.py [outdir]        (default: tests/golden)
Synthetic weights come from (schema, seed) through se_amd.synth, so the fixtures hold inputs and reference outputs only.

What is imported: DCCRN_SNR/DCCRN.py (class DCCRN), on top of oracle/_complexnn_recall.py - the reference's third-party `complexnn.py`
is absent, so DCCRN parity is UNPINNED at that boundary exactly as for the DCCRN fixtures (oracle/gen_golden.py, gen_dccrn); these
fixtures neither worsen nor fix that.  The loop body of DCCRN_SNR/dccrn_decode_snr.py:31-67 is restated around the imported class
(`enhance` below): unit-RMS scale, zero pad to a hop multiple, torch.stft 512 / 128 / 512, network, torch.istft WITHOUT `length`,
cut to the clip's own length, / c - float64 where oracle.gen_golden._enhance_dccrn is.

Seeds, inputs and clips are those of the DCCRN fixtures, so that a pair of files differs in the model only:
  dccrn_snr.npz         the decode script's DCCRN(rnn_units=256, use_clstm=True, kernel_num=[32,64,128,256,256,256]); weights seed 14,
                        x = default_rng(8) [2,2,257,7], clip 6 (as dccrn.npz): y, enh (1.0, 1.0), enh_cprs (0.5, 2.0); and the
                        causality probe: x_future = x with frames >= T_KEEP replaced, y_future its forward - frames < T_KEEP of y
                        and y_future must agree (the `:-1` decoder reads no later frame; the `1:` decoder would)
  full_dccrn_snr.npz    its 4 s decode (clip 1, (0.5, 2.0)), as dccrn.npz:enh4_cprs
  dccrn_snr_rlstm.npz   the class default core `use_clstm=False` at rnn_units 256 and 128 (suffixes _256 / _128), default widths;
                        weights seed 24, x = default_rng(28), clip 26 (as dccrn_rlstm.npz / dccrn_rlstm128.npz)
  schema_dccrn_snr.json, schema_dccrn_snr_rlstm.json, schema_dccrn_snr_rlstm128.json
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as G  # noqa: E402
from se_amd import synth  # noqa: E402

T_KEEP = 4                    # causality probe: frames [T_KEEP, 7) of x are replaced in x_future
CL = dict(rnn_units=256, use_clstm=True, kernel_num=[32, 64, 128, 256, 256, 256])        # dccrn_decode_snr.py:12


def enhance(model, wav, p_in, p_out):
    """DCCRN_SNR/dccrn_decode_snr.py:31-67 around the imported model (`** 1.` at :45 / :53 -> p_in / p_out)."""
    feat_wav = np.asarray(wav, dtype=np.float64)
    c = np.sqrt(len(feat_wav) / np.sum(feat_wav ** 2.0))
    feat_wav = feat_wav * c
    wav_len = len(feat_wav)
    frame_num = int(np.ceil((wav_len - 512 + 512) / 128 + 1))
    fake_wav_len = (frame_num - 1) * 128 + 512 - 512
    x = torch.FloatTensor(np.concatenate((feat_wav, np.zeros([fake_wav_len - wav_len])), axis=0))
    feat_x = G.t_stft(x.unsqueeze(0), 512, 128, 512).permute(0, 3, 1, 2)
    mag, ph = torch.norm(feat_x, dim=1) ** p_in, torch.atan2(feat_x[:, 1], feat_x[:, 0])
    feat_x = torch.stack((mag * torch.cos(ph), mag * torch.sin(ph)), dim=1)
    with torch.no_grad():
        esti = model(feat_x)
    emag = torch.norm(esti, dim=1) ** p_out
    eph = torch.atan2(esti[:, 1], esti[:, 0])
    de = emag[0].double() * torch.exp(1j * eph[0].double())
    y = torch.istft(de, 512, 128, 512, window=torch.hann_window(512, dtype=torch.float64))      # :58, no `length`
    y = y[:wav_len]                                                                             # :66
    return (y / c).numpy()


def main(out=None):
    if out:
        G.GOLD = out
    os.makedirs(G.GOLD, exist_ok=True)
    mod = G.import_ref('DCCRN_SNR', 'DCCRN')
    # ---- the decode script's configuration (complex LSTM)
    torch.manual_seed(0)
    model = mod.DCCRN(**CL)
    schema, _ = G.load_synth(model, 14)
    G.save_schema('dccrn_snr', schema)
    x = np.random.default_rng(8).standard_normal((2, 2, 257, 7)).astype(np.float32)
    x_future = x.copy()
    x_future[..., T_KEEP:] = np.random.default_rng(108).standard_normal((2, 2, 257, 7 - T_KEEP)).astype(np.float32)
    with torch.no_grad():
        y = model(torch.from_numpy(x)).numpy()
        y_future = model(torch.from_numpy(x_future)).numpy()
    wav = synth.synth_clip(6, 'speech', 4000)
    G.save('dccrn_snr', x=x, y=y, x_future=x_future, y_future=y_future, t_keep=np.int64(T_KEEP), wav=wav,
           enh=enhance(model, wav, 1.0, 1.0), enh_cprs=enhance(model, wav, 0.5, 2.0))
    wav4 = synth.synth_clip(1, 'speech', G.FULL_SAMPLES)
    G.save('full_dccrn_snr', seed=np.int64(1), n=np.int64(G.FULL_SAMPLES), enh4_cprs=enhance(model, wav4, 0.5, 2.0).astype(np.float32))
    # ---- the class default core: nn.LSTM(1024, rnn_units, num_layers=2) + tranform (DCCRN.py:82-91)
    x = np.random.default_rng(28).standard_normal((2, 2, 257, 7)).astype(np.float32)
    wav = synth.synth_clip(26, 'speech', 4000)
    arrs = {'x': x, 'wav': wav}
    for units, tag in ((256, 'dccrn_snr_rlstm'), (128, 'dccrn_snr_rlstm128')):
        torch.manual_seed(0)
        model = mod.DCCRN(rnn_units=units)
        schema, _ = G.load_synth(model, 24)
        G.save_schema(tag, schema)
        with torch.no_grad():
            arrs[f'y_{units}'] = model(torch.from_numpy(x)).numpy()
        arrs[f'enh_{units}'] = enhance(model, wav, 1.0, 1.0)
        arrs[f'enh_cprs_{units}'] = enhance(model, wav, 0.5, 2.0)
    G.save('dccrn_snr_rlstm', **arrs)


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else None)
