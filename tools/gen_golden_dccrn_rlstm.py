"""Golden fixtures for DCCRN's real-LSTM forms (`use_clstm=False`: DCCRN-E / -R / -C), by IMPORTING the reference.

TEST INFRASTRUCTURE, build container only (needs the reference tree, as oracle/gen_golden.py does).  Run:
    python tools/gen_golden_dccrn_rlstm.py [outdir]        (default: tests/golden)
Synthetic weights come from (schema, seed) through se_amd.synth, so the fixtures hold inputs and reference outputs only.

Per configuration tag (rnn_units, kernel_num):
  dccrn_rlstm       256, [16, 32, 64, 128, 256, 256]   DCCRN_cprs.py:303-315 (`DCCRN(rnn_units=256, masking_mode=...)`)
  dccrn_rlstm128    128, the default widths            the class default `DCCRN()`
  dccrn_rlstm_w32   256, [32, 64, 128, 256, 256, 256]  the decode script's widths with a real LSTM
each file holds, for masking modes E / C / R, the forward on a [2, 2, 257, 7] input and decodes of a 4 000-sample clip at the
exponent pairs (1.0, 1.0) and (0.5, 2.0); full_dccrn_rlstm.npz: one 4 s decode of the main configuration (mode E, (0.5, 2.0)).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as G  # noqa: E402
from se_amd import synth  # noqa: E402

SEED = 24                     # synthetic weights: synth.synth_state_dict(schema, SEED)
CONFIGS = {
    'dccrn_rlstm': (256, [16, 32, 64, 128, 256, 256]),
    'dccrn_rlstm128': (128, [16, 32, 64, 128, 256, 256]),
    'dccrn_rlstm_w32': (256, [32, 64, 128, 256, 256, 256]),
}


def main(out=None):
    if out:
        G.GOLD = out
    os.makedirs(G.GOLD, exist_ok=True)
    mod = G.import_ref('DCCRN', 'DCCRN_cprs')
    rng = np.random.default_rng(28)
    x = rng.standard_normal((2, 2, 257, 7)).astype(np.float32)
    wav = synth.synth_clip(26, 'speech', 4000)
    for tag, (units, kn) in CONFIGS.items():
        arrs = {'x': x, 'wav': wav}
        for mode in ('E', 'C', 'R'):
            torch.manual_seed(0)
            model = mod.DCCRN(rnn_units=units, masking_mode=mode, use_clstm=False, kernel_num=list(kn))
            schema, _ = G.load_synth(model, SEED)
            if mode == 'E':
                G.save_schema(tag, schema)
            with torch.no_grad():
                arrs['y_' + mode] = model(torch.from_numpy(x)).numpy()
            arrs['enh_' + mode] = G._enhance_dccrn(model, wav, 1.0, 1.0)[0]
            arrs['enh_cprs_' + mode] = G._enhance_dccrn(model, wav, 0.5, 2.0)[0]
            if tag == 'dccrn_rlstm' and mode == 'E':
                wav4 = synth.synth_clip(21, 'speech', G.FULL_SAMPLES)
                enh4 = G._enhance_dccrn(model, wav4, 0.5, 2.0)[0].astype(np.float32)
                G.save('full_dccrn_rlstm', seed=np.int64(21), n=np.int64(G.FULL_SAMPLES), enh4_cprs=enh4)
        G.save(tag, **arrs)


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else None)
