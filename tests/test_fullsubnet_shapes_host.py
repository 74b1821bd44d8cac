"""CPU: `Model(look_ahead=, fb_num_neighbors=, sb_num_neighbors=)` - the three constructor arguments of the reference's Model
(FullSubNet/fullsubnet_net_sa/model.py:9-63) the engine builds at other values than the decode script's.

  - look_ahead 0..6 and fb_num_neighbors 0..15 are fields of the engine's flags (include/se_engine.h: SE_CFG_FSN_LOOK_AHEAD stores
    n + 1 in bits 22-24, SE_CFG_FSN_FB_NEIGHBORS stores n in bits 25-28); the script's values set nothing;
  - sb_num_neighbors 0..15 changes one shape of the key schema, sb_model.sequence_model.weight_ih_l0 [4H or 3H, (2 sbn + 1) + (2 fbn + 1)];
  - everything else is refused, and the message names the accepted ranges;
  - the numpy forward agrees with the fixtures tools/gen_golden_fullsubnet_shapes.py wrote by importing the reference (weights
    (instance schema, seed 15)).  oracle.models.fullsubnet_forward takes look_ahead and the neighbour counts and knows the two Laplace
    norms; for offline_gaussian_norm (base_model.py:242-255) and cumulative_layer_norm (:258-294) the forward is restated here on
    oracle's own unfold and sequence model.  Bar: test_oracle_golden.py's, rms err < 2e-6 max(rms y, 1)."""
import os

import numpy as np
import pytest

import se_amd  # noqa: F401
from se_amd import models, synth
from oracle import models as M
from conftest import load_golden, load_schema, rms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LA_FIELD, FB_FIELD = 7 << 22, 15 << 25
SHAPES = ['la0', 'la1_fb2_sb7', 'la3_fb0_sb3', 'la0_fb1_sb0_gru']
EPSILON = np.finfo(np.float32).eps


def fixture_model(G, **kw):
    """the engine-side Model of a fixture's configuration"""
    return models.Model(look_ahead=int(G['look_ahead']), fb_num_neighbors=int(G['fbn']), sb_num_neighbors=int(G['sbn']),
                        sequence_model='GRU' if int(G['gru']) else 'LSTM', norm_type=str(G['norm_type']), **kw)


def test_look_ahead_and_neighbour_counts_set_their_fields():
    m = models.Model(look_ahead=0)
    assert m._flags & LA_FIELD == 1 << 22 and m._flags & FB_FIELD == 0
    m = models.Model(fb_num_neighbors=2, sb_num_neighbors=7)
    assert m._flags & FB_FIELD == 2 << 25 and m._flags & LA_FIELD == 0          # look_ahead = 2: the script's, nothing stored
    for la in range(7):
        f = models.Model(look_ahead=la, norm_type='cumulative_layer_norm', sequence_model='GRU')._flags
        assert f & LA_FIELD == (0 if la == 2 else (la + 1) << 22)
        assert f & models.Model.SE_CFG_FSN_GRU and f & models.Model.SE_CFG_FSN_CUM_LAYERNORM
    assert models.Model(fb_num_neighbors=15)._flags & FB_FIELD == 15 << 25
    assert models.Model.SE_CFG_FSN_LOOK_AHEAD(6) == 7 << 22 and models.Model.SE_CFG_FSN_FB_NEIGHBORS(15) == 15 << 25


def test_integers_of_any_type_are_taken_and_nothing_else():
    """values read from an npz or a config arrive as numpy integers"""
    m = models.Model(look_ahead=np.int64(0), fb_num_neighbors=np.int32(2), sb_num_neighbors=np.int64(7))
    assert m._flags & LA_FIELD == 1 << 22 and m._flags & FB_FIELD == 2 << 25 and type(m.look_ahead) is int
    assert m.state_dict_schema()['sb_model.sequence_model.weight_ih_l0'][0] == (4 * 384, 20)
    for bad in (np.float64(1.0), True, np.bool_(True), '1', None):
        with pytest.raises(NotImplementedError):
            models.Model(look_ahead=bad)


def test_the_scripts_arguments_set_neither_field():
    kw = dict(sb_num_neighbors=15, fb_num_neighbors=0, num_freqs=257, look_ahead=2, fb_output_activate_function="ReLU",
              sb_output_activate_function=None, fb_model_hidden_size=512, sb_model_hidden_size=384, weight_init=False,
              norm_type="offline_laplace_norm", num_groups_in_drop_band=2)
    assert models.Model(sequence_model="LSTM", **kw)._flags == 0
    assert models.Model(sequence_model="GRU", **kw)._flags == models.Model.SE_CFG_FSN_GRU
    assert models.Model()._flags == 0


def test_fields_are_declared_in_the_header():
    hdr = open(os.path.join(ROOT, 'include', 'se_engine.h')).read()
    assert '#define SE_CFG_FSN_LOOK_AHEAD(n) ((((n) + 1) & 7) << 22)' in hdr
    assert '#define SE_CFG_FSN_FB_NEIGHBORS(n) (((n) & 15) << 25)' in hdr


@pytest.mark.parametrize('seq,gates', [('LSTM', 4), ('GRU', 3)])
def test_schema_of_an_instance_has_its_own_sub_band_width(seq, gates):
    ref = load_schema('fullsubnet' if seq == 'LSTM' else 'fullsubnet_gru')
    for sbn, fbn in ((7, 2), (0, 0), (15, 15), (15, 0)):
        mine = models.Model(fb_num_neighbors=fbn, sb_num_neighbors=sbn, sequence_model=seq).state_dict_schema()
        assert list(mine.keys()) == list(ref.keys())
        for k in ref:
            want = tuple(ref[k][0])
            if k == 'sb_model.sequence_model.weight_ih_l0':
                want = (gates * 384, (2 * sbn + 1) + (2 * fbn + 1))
            assert tuple(mine[k][0]) == want and mine[k][1] == ref[k][1], (k, sbn, fbn)
    # look_ahead has no parameters; the class method stays the script's schema
    assert models.Model(look_ahead=0, sequence_model=seq).state_dict_schema() == ref
    cls = type(models.Model(sequence_model=seq, sb_num_neighbors=3))
    assert cls.state_dict_schema() == ref


@pytest.mark.parametrize('kw', [dict(look_ahead=7), dict(look_ahead=-1), dict(sb_num_neighbors=16), dict(fb_num_neighbors=16),
                                dict(fb_num_neighbors=-1), dict(look_ahead=1.0), dict(num_freqs=161), dict(fb_model_hidden_size=256),
                                dict(sb_model_hidden_size=512), dict(fb_output_activate_function=None),
                                dict(sb_output_activate_function='ReLU')])
def test_everything_else_is_refused_and_the_ranges_are_named(kw):
    with pytest.raises(NotImplementedError) as e:
        models.Model(**kw)
    msg = str(e.value)
    assert 'look_ahead in 0..6' in msg and 'fb_num_neighbors and sb_num_neighbors in 0..15' in msg
    assert 'num_freqs=257' in msg and 'fb_model_hidden_size=512' in msg and 'sb_model_hidden_size=384' in msg


# ------------------------------------------------------------------------------------------------ the numpy forward against the fixtures
def _offline_gaussian_norm(a):
    """base_model.py:242-255: (x - mean) / (std + 1e-5) over everything but the batch; torch.std is the unbiased one"""
    mu = a.mean(axis=(1, 2, 3), keepdims=True)
    sd = a.std(axis=(1, 2, 3), keepdims=True, ddof=1)
    return (a - mu) / (sd + 1e-5)


def _cumulative_layer_norm(a):
    """base_model.py:258-294: running sums of x and x^2 over (features, frames <= t), the expression as written (:285-292)"""
    B, C, F, T = a.shape
    x = a.reshape(B * C, F, T)
    s1 = np.cumsum(x.sum(axis=1, dtype=x.dtype), axis=-1, dtype=x.dtype)
    s2 = np.cumsum(np.square(x).sum(axis=1, dtype=x.dtype), axis=-1, dtype=x.dtype)
    n = np.arange(F, F * T + 1, F, dtype=x.dtype)[None, :]
    mean = s1 / n
    var = (s2 - 2 * mean * s1) / n + mean ** 2
    std = np.sqrt(var + x.dtype.type(EPSILON))
    return ((x - mean[:, None, :]) / std[:, None, :]).reshape(B, C, F, T)


def shape_forward(sd, noisy_mag, look_ahead, sb_nn, fb_nn, norm_type):
    """Model.forward (model.py:68-118), one utterance at a time: oracle's for the Laplace norms, restated for the other two"""
    if norm_type in ('offline_laplace_norm', 'cumulative_laplace_norm'):
        return M.fullsubnet_forward(sd, noisy_mag, look_ahead, sb_nn, fb_nn, norm_type)
    norm = {'offline_gaussian_norm': _offline_gaussian_norm, 'cumulative_layer_norm': _cumulative_layer_norm}[norm_type]
    outs = []
    for b in range(noisy_mag.shape[0]):
        x = np.pad(noisy_mag[b:b + 1], ((0, 0), (0, 0), (0, 0), (0, look_ahead)))                     # :79
        _, _, F, T = x.shape
        fb_out = M._fsn_seq(sd, 'fb_model.', norm(x).reshape(1, F, T), 'ReLU').reshape(1, 1, F, T)    # :84-85
        fb_unf = M._fsn_unfold(fb_out, fb_nn).reshape(1, F, 2 * fb_nn + 1, T)                         # :88-89
        nz_unf = M._fsn_unfold(x, sb_nn).reshape(1, F, 2 * sb_nn + 1, T)                              # :92-93
        sb_in = norm(np.concatenate([nz_unf, fb_unf], axis=2)).reshape(F, 2 * sb_nn + 1 + 2 * fb_nn + 1, T)      # :96-110
        m = M._fsn_seq(sd, 'sb_model.', sb_in, None)                                                  # :113
        outs.append(np.transpose(m.reshape(1, F, 2, T), (0, 2, 1, 3))[:, :, :, look_ahead:])          # :114-117
    return np.concatenate(outs, axis=0)


@pytest.mark.parametrize('name', SHAPES)
def test_numpy_forward_matches_the_reference_fixture(name):
    G = load_golden('fullsubnet_shape_' + name)
    m = fixture_model(G)
    la, fbn, sbn = int(G['look_ahead']), int(G['fbn']), int(G['sbn'])
    schema = m.state_dict_schema()
    assert schema['sb_model.sequence_model.weight_ih_l0'][0] == ((3 if int(G['gru']) else 4) * 384, 2 * sbn + 2 * fbn + 2)
    sd = synth.synth_state_dict(schema, int(G['seed']))
    y = shape_forward(sd, G['x'], la, sbn, fbn, str(G['norm_type']))
    err = rms(y - G['y'])
    print(name, 'numpy forward rms err', err, 'rms ref', rms(G['y']), 'smallest reference denominator', float(G['min_denom']))
    assert y.shape == G['y'].shape and err < 2e-6 * max(rms(G['y']), 1.0), (err, rms(G['y']))
    assert float(G['min_denom']) > 1e-4
    # the script's shape is a different function of the same input
    if (la, fbn, sbn) != (2, 0, 15):
        sd0 = synth.synth_state_dict(load_schema('fullsubnet_gru' if int(G['gru']) else 'fullsubnet'), int(G['seed']))
        y0 = shape_forward(sd0, G['x'][:1], 2, 15, 0, str(G['norm_type']))
        assert rms(y0 - G['y'][:1]) > 1e-3 * rms(G['y'][:1])
