"""CPU: DCCRN's real-LSTM forms (`use_clstm=False`: DCCRN-E / -R / -C, DCCRN/DCCRN_cprs.py:95-102) - key schemas against the
ones captured from the imported reference, constructor flags and limits, checkpoint recognition in se_amd.decode."""
import numpy as np
import pytest

import se_amd  # noqa: F401
from se_amd import schemas, synth
from conftest import load_schema

DEFAULT_KN = [16, 32, 64, 128, 256, 256]
CL_KN = [32, 64, 128, 256, 256, 256]


@pytest.mark.parametrize('name', ['dccrn_rlstm', 'dccrn_rlstm128', 'dccrn_rlstm_w32'])
def test_real_lstm_schema_matches_reference(name):
    ref = load_schema(name)
    mine = schemas.SCHEMAS[name]()
    assert list(mine.keys()) == list(ref.keys())
    for k in ref:
        assert tuple(mine[k][0]) == tuple(ref[k][0]) and mine[k][1] == ref[k][1], k


@pytest.mark.parametrize('units,kn,name', [(256, DEFAULT_KN, 'dccrn_rlstm'), (128, DEFAULT_KN, 'dccrn_rlstm128'),
                                           (256, CL_KN, 'dccrn_rlstm_w32')])
@pytest.mark.parametrize('mode,bits', [('E', 0), ('C', 32), ('R', 64)])
def test_constructor_flags_and_schema(units, kn, name, mode, bits):
    from se_amd.models import DCCRN
    m = DCCRN(rnn_units=units, masking_mode=mode, kernel_num=kn)
    assert m._flags == 128 | bits
    assert isinstance(m, DCCRN)
    assert list(m.state_dict_schema()) == list(load_schema(name))


def test_class_default_and_rnn_layers():
    from se_amd.models import DCCRN
    m = DCCRN()                                   # rnn_units=128, the default widths
    assert m._flags == 128
    assert list(m.state_dict_schema()) == list(load_schema('dccrn_rlstm128'))
    # num_layers is hard-coded to 2 on this path: rnn_layers is accepted and ignored
    assert list(DCCRN(rnn_layers=3, rnn_units=256).state_dict_schema()) == list(load_schema('dccrn_rlstm'))


def test_clstm_form_unchanged():
    from se_amd.models import DCCRN
    m = DCCRN(rnn_units=256, masking_mode='C', use_clstm=True, kernel_num=CL_KN)
    assert m._flags == 32
    assert list(m.state_dict_schema()) == list(load_schema('dccrn'))


@pytest.mark.parametrize('kw', [dict(rnn_units=64), dict(rnn_units=256, kernel_num=[8, 16, 32, 64, 128, 128]),
                                dict(rnn_units=128, kernel_num=CL_KN), dict(rnn_units=256, use_cbn=True),
                                dict(rnn_units=256, masking_mode='X'), dict(rnn_units=256, kernel_size=3),
                                dict(rnn_units=256, use_clstm=True)])
def test_unsupported_configurations_raise(kw):
    from se_amd.models import DCCRN
    with pytest.raises(NotImplementedError, match='use_clstm=False'):
        DCCRN(**kw)


@pytest.mark.parametrize('name,units,kn', [('dccrn_rlstm', 256, DEFAULT_KN), ('dccrn_rlstm128', 128, DEFAULT_KN),
                                           ('dccrn_rlstm_w32', 256, CL_KN)])
def test_decode_recognises_real_lstm_checkpoint(name, units, kn):
    from se_amd import decode
    sd = synth.synth_state_dict(schemas.SCHEMAS[name](), 3)
    assert decode.dccrn_real_lstm_config(sd) == dict(rnn_units=units, masking_mode='E', use_clstm=False, kernel_num=kn)
    assert decode.dccrn_real_lstm_config(synth.synth_state_dict(schemas.SCHEMAS['dccrn'](), 3)) is None


def test_fixtures_are_small():
    import os
    from conftest import GOLD
    for f in ('dccrn_rlstm', 'dccrn_rlstm128', 'dccrn_rlstm_w32', 'full_dccrn_rlstm'):
        assert os.path.getsize(os.path.join(GOLD, f + '.npz')) < 512 * 1024
        assert np.isfinite(np.load(os.path.join(GOLD, f + '.npz'))['enh4_cprs' if f.startswith('full') else 'y_E']).all()
