"""CPU: `Model(norm_type=...)` accepts the four names of the reference's norm_wrapper (FullSubNet/fullsubnet_net_sa/base_model.py:296-308)
and maps each to its SE_CFG_* bit of include/se_engine.h; the norms have no parameters, so the key schema is the reference's for every
one of them."""
import os

import pytest

import se_amd  # noqa: F401
from se_amd import models
from conftest import load_schema

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORM_BITS = {'offline_laplace_norm': 0, 'cumulative_laplace_norm': 16, 'offline_gaussian_norm': 1 << 20, 'cumulative_layer_norm': 1 << 21}
ALL = 16 | 1 << 20 | 1 << 21


@pytest.mark.parametrize('norm', list(NORM_BITS))
def test_norm_type_sets_its_bit_and_no_other(norm):
    m = models.Model(norm_type=norm)
    assert m._flags & ALL == NORM_BITS[norm]
    g = models.Model(norm_type=norm, sequence_model='GRU')
    assert g._flags & ALL == NORM_BITS[norm] and g._flags & models.Model.SE_CFG_FSN_GRU


def test_bits_are_declared_in_the_header():
    hdr = open(os.path.join(ROOT, 'include', 'se_engine.h')).read()
    assert '#define SE_CFG_FSN_GAUSSIAN (1 << 20)' in hdr and '#define SE_CFG_FSN_CUM_LAYERNORM (1 << 21)' in hdr
    assert models.Model.SE_CFG_FSN_GAUSSIAN == 1 << 20 and models.Model.SE_CFG_FSN_CUM_LAYERNORM == 1 << 21
    assert models.Model.SE_CFG_FSN_CUMULATIVE == 16


@pytest.mark.parametrize('norm', ['forgetting_norm', 'offline_gaussian', '', None])
def test_unknown_norm_raises_and_lists_the_four(norm):
    with pytest.raises(NotImplementedError) as e:
        models.Model(norm_type=norm)
    for name in NORM_BITS:
        assert name in str(e.value)


@pytest.mark.parametrize('seq,schema', [('LSTM', 'fullsubnet'), ('GRU', 'fullsubnet_gru')])
@pytest.mark.parametrize('norm', list(NORM_BITS))
def test_schema_is_the_reference_schema_for_every_norm(norm, seq, schema):
    ref = load_schema(schema)
    mine = models.Model(norm_type=norm, sequence_model=seq).state_dict_schema()
    assert list(mine.keys()) == list(ref.keys())
    for k in ref:
        assert tuple(mine[k][0]) == tuple(ref[k][0]) and mine[k][1] == ref[k][1], k
