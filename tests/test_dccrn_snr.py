"""CPU: the DCCRN of `DCCRN_SNR/` (DCCRN_SNR/DCCRN.py:9-183: the decoder keeps `out[..., :-1]`, :159) - host class, flag bits, key
schemas against the ones captured from the imported reference (tools/gen_golden_dccrn_snr.py), the decode driver's model entry,
and a check on the stored arrays that the fixture really is the causal network."""
import os
import subprocess
import sys

import numpy as np
import pytest

import se_amd  # noqa: F401
from se_amd import schemas
from conftest import GOLD, ROOT, load_golden, load_schema

CAUSAL = 1 << 16               # SE_CFG_DCCRN_CAUSAL_DEC (include/se_engine.h)
DEFAULT_KN = [16, 32, 64, 128, 256, 256]
CL = dict(rnn_units=256, use_clstm=True, kernel_num=[32, 64, 128, 256, 256, 256])       # dccrn_decode_snr.py:12


def _same(mine, ref):
    assert list(mine.keys()) == list(ref.keys())
    for k in ref:
        assert tuple(mine[k][0]) == tuple(ref[k][0]) and mine[k][1] == ref[k][1], k


def test_flag_bit_is_the_first_free_one_above_the_repeat_fields():
    """include/se_engine.h: SE_CFG_REPEATS2 ends at bit 15; the header and the host class agree on bit 16."""
    from se_amd.models import DCCRN_SNR
    with open(os.path.join(ROOT, 'include', 'se_engine.h')) as f:
        hdr = f.read()
    assert '#define SE_CFG_DCCRN_CAUSAL_DEC (1 << 16)' in hdr
    assert DCCRN_SNR.SE_CFG_DCCRN_CAUSAL_DEC == CAUSAL
    assert CAUSAL > ((15 << 12) | (15 << 8) | 255) and CAUSAL >> 1 == 1 << 15


def test_decode_script_configuration():
    from se_amd.models import DCCRN, DCCRN_SNR
    m = DCCRN_SNR(**CL)
    assert m._flags == CAUSAL and m._model == 'dccrn'
    assert isinstance(m, DCCRN_SNR) and isinstance(m, DCCRN)
    _same(m.state_dict_schema(), load_schema('dccrn_snr'))
    _same(DCCRN_SNR.state_dict_schema(), load_schema('dccrn_snr'))
    _same(schemas.SCHEMAS['dccrn_snr'](), load_schema('dccrn_snr'))
    # the look-ahead class is untouched by the new one
    assert DCCRN(masking_mode='E', **CL)._flags == 0


@pytest.mark.parametrize('units,kn,name', [(128, DEFAULT_KN, 'dccrn_snr_rlstm128'), (256, DEFAULT_KN, 'dccrn_snr_rlstm'),
                                           (256, CL['kernel_num'], None)])
def test_real_lstm_core(units, kn, name):
    """The class default `use_clstm=False` (DCCRN.py:82-91): SE_CFG_DCCRN_REAL_LSTM | SE_CFG_DCCRN_CAUSAL_DEC, DCCRN's real-LSTM keys."""
    from se_amd.models import DCCRN_SNR
    m = DCCRN_SNR(rnn_units=units, kernel_num=kn)
    assert m._flags == CAUSAL | 128 and isinstance(m, DCCRN_SNR)
    if name:
        _same(m.state_dict_schema(), load_schema(name))
        _same(schemas.SCHEMAS[name](), load_schema(name))
    else:
        _same(m.state_dict_schema(), schemas.dccrn_rlstm_schema(tuple(kn), units))


def test_class_default_is_the_reference_signature():
    import inspect
    from se_amd.models import DCCRN_SNR
    m = DCCRN_SNR()                       # rnn_units=128, use_clstm=False, the default widths
    assert m._flags == CAUSAL | 128
    _same(m.state_dict_schema(), load_schema('dccrn_snr_rlstm128'))
    names = list(inspect.signature(DCCRN_SNR.__init__).parameters)[1:10]
    assert names == ['rnn_layers', 'rnn_units', 'win_len', 'win_inc', 'fft_len', 'use_clstm', 'use_cbn', 'kernel_size', 'kernel_num']
    # positional call as the reference allows it: (rnn_layers, rnn_units)
    assert DCCRN_SNR(2, 256)._flags == CAUSAL | 128
    # the two complexnn convention bits combine
    assert DCCRN_SNR(**CL, flags=2 | 4)._flags == CAUSAL | 6


@pytest.mark.parametrize('kw', [dict(rnn_units=64), dict(rnn_units=256, kernel_num=[8, 16, 32, 64, 128, 128]),
                                dict(rnn_units=128, kernel_num=CL['kernel_num']), dict(rnn_units=256, use_cbn=True),
                                dict(rnn_units=256, kernel_size=3), dict(rnn_units=256, use_clstm=True),
                                dict(CL, rnn_layers=3), dict(CL, win_len=400), dict(CL, use_cbn=True)])
def test_unsupported_configurations_raise(kw):
    from se_amd.models import DCCRN_SNR
    with pytest.raises(NotImplementedError, match='DCCRN_SNR'):
        DCCRN_SNR(**kw)


@pytest.mark.parametrize('kw', [dict(masking_mode='E'), dict(masking_mode='C'), dict(win_type='hanning')])
def test_arguments_the_reference_class_does_not_have(kw):
    from se_amd.models import DCCRN_SNR
    with pytest.raises(TypeError):
        DCCRN_SNR(**CL, **kw)


@pytest.mark.parametrize('bits', [32, 64, 32 | 128])
def test_mask_c_and_r_do_not_combine_with_the_causal_decoder(bits):
    """The SNR class has the 'E' mask only (DCCRN.py:162-183): the host class refuses the bits before an engine exists (the engine
    refuses them at create: tests/test_gpu_dccrn_snr.py)."""
    from se_amd.models import DCCRN_SNR
    with pytest.raises(ValueError, match="'E' mask only"):
        DCCRN_SNR(**CL, flags=bits)


def test_not_in_model_classes_and_driver_entry():
    """MODEL_CLASSES is iterated by zoo-wide tools: the class lives under its own name; the decode driver knows the model by the
    script's checkpoint name and builds it from either core's keys."""
    from se_amd import decode, synth
    from se_amd.models import MODEL_CLASSES, DCCRN_SNR
    assert 'dccrn_snr' not in MODEL_CLASSES
    assert 'dccrn_snr' in decode.MODELS and 'dccrn_snr' in decode.RAGGED_MODELS and 'dccrn_snr' in decode.NO_RESAMPLE_MODELS
    assert decode.DEFAULT_CKPT['dccrn_snr'].endswith('wsj0_si84_300h_dccrn_snr_model.pth')
    built = {}

    class Probe(DCCRN_SNR):
        def load_state_dict(self, sd, strict=True):
            built['flags'], built['schema'] = self._flags, list(self.state_dict_schema())
            return self
    from se_amd import models
    orig = models.DCCRN_SNR
    models.DCCRN_SNR = Probe
    try:
        for name, flags in (('dccrn_snr', CAUSAL), ('dccrn_snr_rlstm', CAUSAL | 128), ('dccrn_snr_rlstm128', CAUSAL | 128)):
            sd = synth.synth_state_dict(schemas.SCHEMAS[name](), 3)
            decode._build('dccrn_snr', None, sd, max_batch=1, max_samples=4000)
            assert built['flags'] == flags and built['schema'] == list(sd), name
    finally:
        models.DCCRN_SNR = orig


def test_driver_cli_knows_the_model():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'decode_vb.py'), '--help'], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and 'dccrn_snr' in r.stdout and '--noise_type' in r.stdout and '--snr' in r.stdout


def test_fixture_is_the_causal_network():
    """tools/gen_golden_dccrn_snr.py stores a second forward whose input differs from x in frames >= t_keep only.  With the `:-1`
    decoder (DCCRN.py:159) no output frame < t_keep may move - float32 convolutions over the same values in the same order: not
    by one bit, asserted to 1e-6 of the signal - while the replaced frames do move.  (With `1:`, DCCRN_cprs.py:199, frame
    t_keep - 1 already reads frame t_keep through the first decoder layer, and earlier frames through the deeper ones.)"""
    G = load_golden('dccrn_snr')
    k = int(G['t_keep'])
    x, xf, y, yf = G['x'], G['x_future'], G['y'], G['y_future']
    assert 0 < k < x.shape[-1] and np.array_equal(x[..., :k], xf[..., :k]) and not np.allclose(x[..., k:], xf[..., k:])
    scale = float(np.sqrt(np.mean(y.astype(np.float64) ** 2)))
    for t in range(k):
        d = float(np.max(np.abs(y[..., t] - yf[..., t])))
        assert d <= 1e-6 * scale, (t, d, scale)
    for t in range(k, x.shape[-1]):
        assert float(np.sqrt(np.mean((y[..., t] - yf[..., t]) ** 2.0))) > 1e-2 * scale, t
    # and the network is not the look-ahead one: same weights (seed 14), same x as tests/golden/dccrn.npz, another output
    Gv = load_golden('dccrn')
    assert np.array_equal(Gv['x'], x) and np.sqrt(np.mean((Gv['y'] - y) ** 2.0)) > 1e-2 * scale


def test_fixture_decode_lengths_and_sizes():
    """dccrn_decode_snr.py:66: the decode is cut to the clip's own length (the `_vb` script returns the hop-padded one); the clip,
    seeds and inputs are the DCCRN fixtures', so the pairs differ in the model only."""
    G, Gv, R, Rv = load_golden('dccrn_snr'), load_golden('dccrn'), load_golden('dccrn_snr_rlstm'), load_golden('dccrn_rlstm')
    assert np.array_equal(G['wav'], Gv['wav']) and np.array_equal(R['wav'], Rv['wav']) and np.array_equal(R['x'], Rv['x'])
    assert len(G['wav']) == 4000 and G['enh'].shape == (4000,) and G['enh_cprs'].shape == (4000,)
    assert Gv['enh'].shape == (4096,)
    for u in (128, 256):
        assert R[f'enh_{u}'].shape == (4000,) and R[f'enh_cprs_{u}'].shape == (4000,) and R[f'y_{u}'].shape == (2, 2, 257, 7)
    F = load_golden('full_dccrn_snr')
    assert int(F['n']) == 64000 and int(F['seed']) == 1 and F['enh4_cprs'].shape == (64000,) and F['enh4_cprs'].dtype == np.float32
    for f in ('dccrn_snr', 'dccrn_snr_rlstm', 'full_dccrn_snr'):
        Z = np.load(os.path.join(GOLD, f + '.npz'))
        assert os.path.getsize(os.path.join(GOLD, f + '.npz')) < 512 * 1024
        assert all(np.isfinite(Z[k]).all() for k in Z.files), f
