"""Host-side mirrors of the reference's model classes.

Same class names, constructor arguments, `load_state_dict` key schema, `eval()/cuda()` chaining and
`forward()` tensor shapes as the reference `nn.Module`s, but every forward runs in the HIP engine
(libse_engine.so) - these classes hold no parameters and do no arithmetic themselves.
"""
import functools
import operator

import numpy as np

from . import schemas, synth
from .engine import Engine


class _class_or_instance_method:
    """f(cls, self) reachable both as Class.f() (self = None) and instance.f()."""

    def __init__(self, f):
        self.f = f

    def __get__(self, obj, cls):
        return functools.partial(self.f, cls if obj is None else type(obj), obj)


class _EngineModule:
    """Common plumbing: lazy engine creation, strict state-dict load, torch-like call surface."""
    _model = None          # key into _lib.MODEL_IDS
    _schema = None         # key into schemas.SCHEMAS (defaults to _model)
    _repeat_prefix = None  # ModuleList whose length is a constructor argument (stage_num / order_num), decode-script value 3
    p_in = 1.0             # magnitude exponents the decode script applies around the network
    p_out = 1.0

    def __init__(self, device=0, max_batch=1, max_samples=64000, p_in=None, p_out=None, graphs=False, flags=0,
                 sliding_stream=False, row_ends=False, row_origins=False):
        # model-specific SE_CFG_* bits (include/se_engine.h); sliding_stream: SE_CFG_STREAM_SLIDING, frame-online streams of
        # this engine keep a sliding window of their input and may outlive max_samples; row_ends: SE_CFG_DCCRN_ROW_ENDS, DCCRN
        # (look-ahead decoder) alone - enhance_long_ragged then accepts it (the engine refuses the bit for every other model);
        # row_origins: SE_CFG_STREAM_ROW_ORIGINS, the cLN networks and FullSubNet with the cumulative norm alone - a frame origin per
        # stream row, with which StreamSnapshot.join accepts them
        self._flags = (flags | (Engine.SE_CFG_STREAM_SLIDING if sliding_stream else 0) | (Engine.SE_CFG_DCCRN_ROW_ENDS if row_ends else 0) |
                       (Engine.SE_CFG_STREAM_ROW_ORIGINS if row_origins else 0))
        self._graphs = graphs          # replay enhance_batch as a hipGraph per shape (small, launch-bound batches)
        self._device = device
        self._max_batch = max_batch
        self._max_samples = max_samples
        if p_in is not None:
            self.p_in = p_in
        if p_out is not None:
            self.p_out = p_out
        self.engine = None

    # -- reference-compatible surface -------------------------------------------------------------
    @_class_or_instance_method
    def state_dict_schema(cls, self):
        """Class.state_dict_schema(): the decode script's configuration; instance.state_dict_schema(): this instance's."""
        base = schemas.SCHEMAS[cls._schema or cls._model]()
        n = getattr(self, '_repeats', 3)
        return base if cls._repeat_prefix is None or n == 3 else schemas.repeat_variant(base, cls._repeat_prefix, n)

    def load_state_dict(self, sd, strict=True):
        assert strict, "the engine only supports strict loads (as every reference decode script does)"
        want = self.state_dict_schema()
        missing = [k for k in want if k not in sd]
        unexpected = [k for k in sd if k not in want]
        if missing or unexpected:
            raise RuntimeError(f"Error(s) in loading state_dict: missing {missing[:5]} unexpected {unexpected[:5]}")
        self.engine = Engine(self._model, self._device, self._max_batch, self._max_samples, self.p_in, self.p_out,
                             graphs=self._graphs, flags=self._flags)
        self.engine.load_state_dict(sd)
        return self

    def load_synthetic(self, seed=0):
        """Deterministic random-init weights (no checkpoints ship with the reference)."""
        return self.load_state_dict(synth.synth_state_dict(self.state_dict_schema(), seed))

    def eval(self):
        return self

    def cuda(self, device=None):
        return self

    def to(self, *a, **k):
        return self

    def __call__(self, x):
        return self.forward(x)

    def forward(self, x):
        if self.engine is None:
            raise RuntimeError("load_state_dict() must be called before forward()")
        return self.engine.forward(x.contiguous())

    def enhance_batch(self, wav):
        return self.engine.enhance_batch(wav)

    def enhance_long(self, wav, out=None, max_chunk_frames=0):
        """enhance_batch for clips of any length, decoded in windows (Engine.enhance_long): models that stream only."""
        return self.engine.enhance_long(wav, out, max_chunk_frames)

    def enhance_long_ragged(self, wav, lengths, max_chunk_frames=0, out=None):
        """enhance_long for rows of different lengths in one walk (Engine.enhance_long_ragged): each row as if decoded alone."""
        return self.engine.enhance_long_ragged(wav, lengths, max_chunk_frames, out)

    def enhance_ragged(self, wav, lengths):
        return self.engine.enhance_ragged(wav, lengths)


class DCCRN(_EngineModule):
    """DCCRN/DCCRN_cprs.py:8 as built by DCCRN/dccrn_decode_vb.py:11 (DCCRN-CL: `use_clstm=True`), or with the real-LSTM core of
    `use_clstm=False` (DCCRN-E / -R / -C, DCCRN_cprs.py:303-315; SE_CFG_DCCRN_REAL_LSTM).  forward: [B,2,257,T] -> [B,2,257,T]."""
    _model = 'dccrn'
    SE_CFG_DCCRN_MASK_C = 32
    SE_CFG_DCCRN_MASK_R = 64
    SE_CFG_DCCRN_REAL_LSTM = 128
    # use_clstm=False: the (rnn_units, kernel_num) pairs the engine builds
    REAL_LSTM_CONFIGS = ((256, (16, 32, 64, 128, 256, 256)), (128, (16, 32, 64, 128, 256, 256)),
                         (256, (32, 64, 128, 256, 256, 256)))

    def __init__(self, rnn_layers=2, rnn_units=128, win_len=512, win_inc=128, fft_len=512, win_type='hanning',
                 masking_mode='E', use_clstm=False, use_cbn=False, kernel_size=5,
                 kernel_num=(16, 32, 64, 128, 256, 256), **kw):
        cfg = (rnn_layers, rnn_units, win_len, win_inc, fft_len, masking_mode, use_clstm, use_cbn, kernel_size,
               tuple(kernel_num))
        clstm_ok = cfg[:5] + cfg[6:] == (2, 256, 512, 128, 512, True, False, 5, (32, 64, 128, 256, 256, 256))
        # use_clstm=False: nn.LSTM(num_layers=2) whatever rnn_layers says (DCCRN_cprs.py:95-102)
        real_ok = (not use_clstm and not use_cbn and (win_len, win_inc, fft_len, kernel_size) == (512, 128, 512, 5)
                   and (rnn_units, tuple(kernel_num)) in self.REAL_LSTM_CONFIGS)
        if not (clstm_ok or real_ok) or masking_mode not in ('E', 'C', 'R'):
            raise NotImplementedError("the engine builds DCCRN with masking_mode 'E', 'C' or 'R' as the decode script's DCCRN-CL "
                                      "(dccrn_decode_vb.py:11: rnn_units=256, use_clstm=True, kernel_num=[32,64,128,256,256,256]) "
                                      "or with use_clstm=False, use_cbn=False and (rnn_units, kernel_num) in "
                                      + repr(self.REAL_LSTM_CONFIGS) + "; got " + repr(cfg))
        # masking_mode (DCCRN_cprs.py:205-223): SE_CFG_DCCRN_MASK_C / _R (include/se_engine.h)
        kw['flags'] = kw.get('flags', 0) | {'E': 0, 'C': self.SE_CFG_DCCRN_MASK_C, 'R': self.SE_CFG_DCCRN_MASK_R}[masking_mode]
        if real_ok:
            kw['flags'] |= self.SE_CFG_DCCRN_REAL_LSTM
            self._rlstm = (rnn_units, tuple(kernel_num))
            self.__class__ = _DCCRNRealLSTM       # same engine model, the real-LSTM key schema
        super().__init__(**kw)


class _DCCRNRealLSTM(DCCRN):
    @_class_or_instance_method
    def state_dict_schema(cls, self):
        units, kn = getattr(self, '_rlstm', DCCRN.REAL_LSTM_CONFIGS[0])
        return schemas.dccrn_rlstm_schema(kn, units)


class DCCRN_SNR(DCCRN):
    """DCCRN_SNR/DCCRN.py:9 - the DCCRN of the WSJ0-SI84 grid, built at DCCRN_SNR/dccrn_decode_snr.py:12 as
    `DCCRN(rnn_units=256, use_clstm=True, kernel_num=[32, 64, 128, 256, 256, 256])`.  The reference's signature: no `masking_mode`
    (the class has the 'E' mask only) and no `win_type`.  Its decoder keeps `out[..., :-1]` after every transposed conv
    (DCCRN.py:159) where DCCRN_cprs.py:199 keeps `out[..., 1:]`: the network is causal end to end (SE_CFG_DCCRN_CAUSAL_DEC,
    include/se_engine.h), the frame-online mode finalises every frame at once, and a decode returns the clip's own length
    (dccrn_decode_snr.py:66).  The state-dict keys are DCCRN's, per core.  forward: [B,2,257,T] -> [B,2,257,T]."""
    SE_CFG_DCCRN_CAUSAL_DEC = 1 << 16

    def __init__(self, rnn_layers=2, rnn_units=128, win_len=512, win_inc=128, fft_len=512, use_clstm=False, use_cbn=False,
                 kernel_size=5, kernel_num=(16, 32, 64, 128, 256, 256), **kw):
        for k in ('masking_mode', 'win_type'):
            if k in kw:
                raise TypeError(f"DCCRN_SNR() has no argument '{k}' (DCCRN_SNR/DCCRN.py:10-21)")
        if kw.get('flags', 0) & (self.SE_CFG_DCCRN_MASK_C | self.SE_CFG_DCCRN_MASK_R):
            raise ValueError("DCCRN_SNR has the 'E' mask only (DCCRN_SNR/DCCRN.py:162-183): SE_CFG_DCCRN_MASK_C / _R do not "
                             "combine with its causal decoder")
        kw['flags'] = kw.get('flags', 0) | self.SE_CFG_DCCRN_CAUSAL_DEC
        try:
            super().__init__(rnn_layers, rnn_units, win_len, win_inc, fft_len, 'hanning', 'E', use_clstm, use_cbn, kernel_size,
                             kernel_num, **kw)
        except NotImplementedError:
            raise NotImplementedError(
                "the engine builds DCCRN_SNR as the decode script's (dccrn_decode_snr.py:12: rnn_units=256, use_clstm=True, "
                "kernel_num=[32,64,128,256,256,256]) or with use_clstm=False, use_cbn=False and (rnn_units, kernel_num) in "
                + repr(self.REAL_LSTM_CONFIGS) + "; got " + repr((rnn_layers, rnn_units, win_len, win_inc, fft_len, use_clstm,
                                                                  use_cbn, kernel_size, tuple(kernel_num)))) from None
        self.__class__ = DCCRN_SNR        # (the real-LSTM form re-classes the instance: the schema below covers both cores)

    @_class_or_instance_method
    def state_dict_schema(cls, self):
        """Class.state_dict_schema(): the decode script's configuration (complex LSTM); instance: this instance's core."""
        rl = getattr(self, '_rlstm', None)
        return schemas.dccrn_rlstm_schema(rl[1], rl[0]) if rl else schemas.SCHEMAS['dccrn']()


class lstm_net(_EngineModule):
    """LSTM/LSTM.py:14 `lstm_net()`.  forward: magnitude [B,T,161] -> enhanced magnitude [B,T,161]."""
    _model = 'lstm'


class crn_net(_EngineModule):
    """CRN/CRN.py:16 `crn_net()`.  forward: magnitude [B,T,161] -> enhanced magnitude [B,T,161]."""
    _model = 'crn'


class dpcrn(_EngineModule):
    """DPCRN/DPCRN.py:16 `dpcrn()`.  forward: RI [B,2,T,161] -> masked RI [B,2,T,161]."""
    _model = 'dpcrn'


class Model(_EngineModule):
    """FullSubNet/fullsubnet_net_sa/model.py:9 `Model(...)` as built at fullsubnet_sa_decode_vb.py:11-24.
    forward: magnitude [B,1,257,T] -> complex mask [B,2,257,T]; each utterance gets batch-1 semantics.
    sequence_model: "LSTM" (the decode script's) or "GRU" (sequence_model.py:36-43; SE_CFG_FSN_GRU); norm_type, one of the four
    of norm_wrapper (base_model.py:296-308): "offline_laplace_norm" (:197-209, the decode script's), "cumulative_laplace_norm"
    (:212-240; SE_CFG_FSN_CUMULATIVE), "offline_gaussian_norm" (:242-255; SE_CFG_FSN_GAUSSIAN) or "cumulative_layer_norm"
    (:258-294; SE_CFG_FSN_CUM_LAYERNORM).  The two cumulative norms are causal: with the LSTM the engine then also streams.
    look_ahead 0..6 (SE_CFG_FSN_LOOK_AHEAD: a stream is final look_ahead frames late), fb_num_neighbors 0..15
    (SE_CFG_FSN_FB_NEIGHBORS) and sb_num_neighbors 0..15 (read by the engine from the shape of
    sb_model.sequence_model.weight_ih_l0, [4H or 3H, (2 sbn + 1) + (2 fbn + 1)]) combine with both sequence models and all four norms.
    num_freqs, the hidden sizes and the two output activations keep the decode script's values."""
    _model = 'fullsubnet'
    SE_CFG_FSN_GRU = 8
    SE_CFG_FSN_CUMULATIVE = 16
    SE_CFG_FSN_GAUSSIAN = 1 << 20
    SE_CFG_FSN_CUM_LAYERNORM = 1 << 21
    # norm_type -> its SE_CFG_* bit (include/se_engine.h); the norms have no parameters, so the key schema is the same for all four
    NORM_FLAGS = {"offline_laplace_norm": 0, "cumulative_laplace_norm": SE_CFG_FSN_CUMULATIVE,
                  "offline_gaussian_norm": SE_CFG_FSN_GAUSSIAN, "cumulative_layer_norm": SE_CFG_FSN_CUM_LAYERNORM}
    LOOK_AHEAD_MAX = 6
    NEIGHBORS_MAX = 15

    @staticmethod
    def SE_CFG_FSN_LOOK_AHEAD(n):
        """bits 22-24, look_ahead + 1; nothing set = the decode script's 2 (include/se_engine.h)"""
        return ((n + 1) & 7) << 22

    @staticmethod
    def SE_CFG_FSN_FB_NEIGHBORS(n):
        """bits 25-28, fb_num_neighbors; the decode script's value is 0"""
        return (n & 15) << 25

    def __init__(self, num_freqs=257, look_ahead=2, sequence_model="LSTM", fb_num_neighbors=0, sb_num_neighbors=15,
                 fb_output_activate_function="ReLU", sb_output_activate_function=None, fb_model_hidden_size=512,
                 sb_model_hidden_size=384, norm_type="offline_laplace_norm", num_groups_in_drop_band=2,
                 weight_init=True, **kw):
        cfg = (num_freqs, look_ahead, fb_num_neighbors, sb_num_neighbors, fb_output_activate_function,
               sb_output_activate_function, fb_model_hidden_size, sb_model_hidden_size, norm_type)

        def whole(v, hi):      # any integer type (a numpy.int64 read from a config or an npz included), no bool, no float
            try:
                return not isinstance(v, (bool, np.bool_)) and 0 <= operator.index(v) <= hi
            except TypeError:
                return False

        fixed = (num_freqs, fb_output_activate_function, sb_output_activate_function, fb_model_hidden_size, sb_model_hidden_size)
        if (fixed != (257, "ReLU", None, 512, 384) or not whole(look_ahead, self.LOOK_AHEAD_MAX)
                or not whole(fb_num_neighbors, self.NEIGHBORS_MAX) or not whole(sb_num_neighbors, self.NEIGHBORS_MAX)
                or sequence_model not in ("LSTM", "GRU") or norm_type not in self.NORM_FLAGS):
            raise NotImplementedError("the engine builds the decode script's FullSubNet configuration (sequence model LSTM "
                                      "or GRU, norm " + ", ".join(self.NORM_FLAGS) + ") with look_ahead in 0..6 and fb_num_neighbors "
                                      "and sb_num_neighbors in 0..15 each; num_freqs=257, fb_model_hidden_size=512, "
                                      "sb_model_hidden_size=384, fb_output_activate_function='ReLU' and "
                                      "sb_output_activate_function=None are fixed; got " + repr(cfg + (sequence_model,)))
        look_ahead, fb_num_neighbors, sb_num_neighbors = (operator.index(v) for v in (look_ahead, fb_num_neighbors, sb_num_neighbors))
        # the cumulative norms are causal - the engine then also streams (se_stream_*)
        kw['flags'] = kw.get('flags', 0) | self.NORM_FLAGS[norm_type]
        # the script's values set nothing (zero in a field = the script's value): its flags stay what they were
        if look_ahead != 2:
            kw['flags'] |= self.SE_CFG_FSN_LOOK_AHEAD(look_ahead)
        kw['flags'] |= self.SE_CFG_FSN_FB_NEIGHBORS(fb_num_neighbors)
        self._neighbors = (sb_num_neighbors, fb_num_neighbors)
        self.look_ahead = look_ahead
        if sequence_model == "GRU":
            kw['flags'] = kw.get('flags', 0) | self.SE_CFG_FSN_GRU
            self.__class__ = _ModelGRU            # same engine model, the GRU's [3H, .] key schema
        super().__init__(**kw)

    @_class_or_instance_method
    def state_dict_schema(cls, self):
        """Class.state_dict_schema(): the decode script's shape; instance.state_dict_schema(): this instance's neighbour counts."""
        sbn, fbn = getattr(self, '_neighbors', (15, 0))
        return schemas.fullsubnet_schema(3 if cls._schema == 'fullsubnet_gru' else 4, sbn, fbn)

    def forward(self, x):
        B, _, F, T = x.shape
        return self.engine.forward(x.contiguous(), out_shape=(B, 2, F, T))


class _ModelGRU(Model):
    _schema = 'fullsubnet_gru'


class Net(_EngineModule):
    """GCRN/GCRN_noncprs.py:86 `Net()`.  forward: RI [B,2,T,161] -> RI estimate [B,2,T,161] (complex mapping).
    The decode script is checked in with the compressed exponents (gcrn_decode_vb.py:40,51)."""
    _model = 'gcrn'
    p_in = 0.5
    p_out = 2.0


class _CtsStage(_EngineModule):
    """One CTSNet stage; the engine model `ctsnet` holds both stages under the key prefixes step1. / step2."""
    _model = 'ctsnet'
    _prefix = ''

    def load_state_dict(self, sd, strict=True):
        want = self.state_dict_schema()
        missing = [k for k in want if k not in sd]
        unexpected = [k for k in sd if k not in want]
        if missing or unexpected:
            raise RuntimeError(f"Error(s) in loading state_dict: missing {missing[:5]} unexpected {unexpected[:5]}")
        self._sd = {self._prefix + k: v for k, v in sd.items()}
        self.engine = Engine('ctsnet', self._device, self._max_batch, self._max_samples, self.p_in, self.p_out,
                             graphs=self._graphs, flags=self._flags)
        self.engine.load_state_dict(self._sd)
        return self


class Step1_net(_CtsStage):
    """CTSNet/Step1_network.py:12 `Step1_net()`.  forward: magnitude [B,T,161] -> magnitude [B,T,161]."""
    _prefix = 'step1.'
    _schema = 'cts_step1'


class Step2_net(_CtsStage):
    """CTSNet/Step2_network.py:13 `Step2_net(X=6, R=3)`.  forward: [B,4,T,161] -> [B,2,T,161]."""
    _prefix = 'step2.'
    _schema = 'cts_step2'

    def __init__(self, X=6, R=3, **kw):
        if not (1 <= X <= 6 and 1 <= R <= 8):
            raise NotImplementedError("the engine builds Step2_net(X, R) with X in [1, 6] and R in [1, 8] (the decode "
                                      "script's: X=6, R=3)")
        # R groups of X gated blocks (Step2_network.py:13-21): SE_CFG_REPEATS(R) | SE_CFG_REPEATS2(X) (include/se_engine.h)
        self._xr = (X, R)
        if (X, R) != (6, 3):
            kw['flags'] = kw.get('flags', 0) | ((R + 1) << 8) | ((X + 1) << 12)
        super().__init__(**kw)

    @_class_or_instance_method
    def state_dict_schema(cls, self):
        X, R = getattr(self, '_xr', (6, 3))
        base = schemas.cts_step2_schema(X, R)
        return schemas.cln_variant(base) if (cls._schema or '').endswith('_new') else base

    def forward(self, x):
        B, _, T, F = x.shape
        return self.engine.forward(x.contiguous(), out_shape=(B, 2, T, F))


class CTSNet:
    """The two chained stages of CTSNet/two_stage_com_decode_vb.py:13-16,78-84 in one engine (decode path)."""

    _stages = (Step1_net, Step2_net)

    def __init__(self, X=6, R=3, **kw):
        self._kw = {k: v for k, v in kw.items() if v is not None}
        self._stage2 = self._stages[1](X=X, R=R)      # Step2_net(X, R): validates, knows its key schema and flag bits
        self.engine = None

    def load_state_dicts(self, sd1, sd2):
        kw = dict(self._kw)
        sd = {'step1.' + k: v for k, v in sd1.items()}
        sd.update({'step2.' + k: v for k, v in sd2.items()})
        self.engine = Engine('ctsnet', kw.get('device', 0), kw.get('max_batch', 1), kw.get('max_samples', 64000),
                             kw.get('p_in', 1.0), kw.get('p_out', 1.0), graphs=kw.get('graphs', False),
                             flags=kw.get('flags', 0) | self._stage2._flags, sliding_stream=kw.get('sliding_stream', False),
                             row_ends=kw.get('row_ends', False), row_origins=kw.get('row_origins', False))
        self.engine.load_state_dict(sd)
        return self

    def load_synthetic(self, seed1=17, seed2=18):
        return self.load_state_dicts(synth.synth_state_dict(self._stages[0].state_dict_schema(), seed1),
                                     synth.synth_state_dict(self._stage2.state_dict_schema(), seed2))

    def enhance_batch(self, wav):
        return self.engine.enhance_batch(wav)

    def enhance_long(self, wav, out=None, max_chunk_frames=0):
        """Both stages over clips of any length, in windows (Engine.enhance_long): the cumulative-LayerNorm (`_new`) weights only."""
        return self.engine.enhance_long(wav, out, max_chunk_frames)

    def enhance_long_ragged(self, wav, lengths, max_chunk_frames=0, out=None):
        """enhance_long for rows of different lengths in one walk (Engine.enhance_long_ragged): each row as if decoded alone."""
        return self.engine.enhance_long_ragged(wav, lengths, max_chunk_frames, out)

    def enhance_ragged(self, wav, lengths):
        return self.engine.enhance_ragged(wav, lengths)


class TaylorSENet(_EngineModule):
    """TaylorSENet/TaylorSENet.py:8 as built at taylorsenet_decode_vb.py:11-13.  forward: RI [B,2,T,161] -> RI."""
    _model = 'taylorsenet'
    _repeat_prefix = 'highorderblock_list.'

    def __init__(self, cin=2, k1=(1, 3), k2=(2, 3), c=64, kd1=3, cd1=64, d_feat=256, dilations=(1, 2, 5, 9), p=2,
                 fft_num=320, order_num=3, intra_connect='cat', inter_connect='add', is_causal=True, is_conformer=False,
                 is_u2=True, is_param_share=False, is_encoder_share=False, **kw):
        cfg = (cin, tuple(k1), tuple(k2), c, kd1, cd1, d_feat, tuple(dilations), p, fft_num, order_num, intra_connect,
               inter_connect, is_causal, is_conformer, is_u2, is_param_share, is_encoder_share)
        if (cfg[:10] + cfg[11:] != (2, (1, 3), (2, 3), 64, 5, 64, 256, (1, 2, 5, 9), 2, 320, 'cat', 'cat', True, False, True, False,
                                     False) or not 0 <= order_num <= 8):
            raise NotImplementedError("the engine builds the decode script's TaylorSENet configuration with order_num in "
                                      "[0, 8]; got " + repr(cfg))
        # order_num (TaylorSENet.py:27,66-70): SE_CFG_REPEATS(n) = (n + 1) << 8 (include/se_engine.h)
        self._repeats = order_num
        if order_num != 3:
            kw['flags'] = kw.get('flags', 0) | ((order_num + 1) << 8)
        super().__init__(**kw)



def _taylor(**kw):
    return TaylorSENet(cin=2, k1=(1, 3), k2=(2, 3), c=64, kd1=5, cd1=64, d_feat=256, dilations=[1, 2, 5, 9], p=2,
                       fft_num=320, order_num=3, intra_connect='cat', inter_connect='cat', is_causal=True,
                       is_conformer=False, is_u2=True, is_param_share=False, is_encoder_share=False, **kw)


class gaf_base(_EngineModule):
    """G2Net_VB/gaf_net_320.py:10 as built at com_decode.py:23.  forward: RI [B,2,T,161] -> list of stage outputs;
    the engine returns the list with only the LAST stage ([B,2,161,T]) materialised - the decode script uses [-1]."""
    _model = 'g2net'
    _repeat_prefix = 'gafs.'

    def __init__(self, kd1=3, cd1=64, tcm_num=2, sub_g1=4, sub_g2=4, dilas=(1, 2, 5, 9), ci=256 + 161 * 2, co1=256,
                 co2=256, k1=(2, 3), k2=(1, 3), c=64, intra_connect='cat', stage_num=3, is_causal=True, is_aux=True,
                 encoder_type='U2Net', tcm_type='full-band', **kw):
        cfg = (kd1, cd1, tcm_num, tuple(dilas), ci, co1, co2, tuple(k1), tuple(k2), c, intra_connect, stage_num,
               is_causal, is_aux, encoder_type, tcm_type)
        if (cfg[:11] + cfg[12:] != (3, 64, 2, (1, 2, 5, 9), 578, 256, 256, (2, 3), (1, 3), 64, 'cat', True, False, 'U2Net', 'full-band')
                or not 1 <= stage_num <= 8):
            raise NotImplementedError("the engine builds the decode script's gaf_base configuration with stage_num in [1, 8]; "
                                      "got " + repr(cfg))
        # stage_num (gaf_net_320.py:27,55-58): SE_CFG_REPEATS(n) = (n + 1) << 8 (include/se_engine.h)
        self._repeats = stage_num
        if stage_num != 3:
            kw['flags'] = kw.get('flags', 0) | ((stage_num + 1) << 8)
        super().__init__(**kw)


    def forward(self, x):
        B, _, T, F = x.shape
        return [self.engine.forward(x.contiguous(), out_shape=(B, 2, F, T))]


def _g2net(**kw):
    return gaf_base(3, 64, 2, 4, 4, [1, 2, 5, 9], 256 + 161 * 2, 256, 256, (2, 3), (1, 3), 64, 'cat', 3, is_aux=False,
                    encoder_type='U2Net', tcm_type='full-band', **kw)


class Uformer(_EngineModule):
    """Uformer/uformer.py:30 `Uformer()`.  forward(inputs, src): waveforms [B, L] -> the reference's 4-tuple
    (enhanced waveform [B, 160*floor(L/160)], istft(stft(src)), output_cplx [B,2,257,T], src_cplx [B,2,257,T]) - the STFT /
    iSTFT are inside the model (uformer.py:178, 276).  Without `src` the two source outputs are None (the decode script
    only reads [0], uformer_decode_vb.py:40)."""
    _model = 'uformer'
    _IGNORED = ('stft.K', 'stft.w', 'istft.K', 'istft.w')

    def __init__(self, win_len=400, win_inc=160, fft_len=512, win_type='hanning', fid=None, **kw):
        if (win_len, win_inc, fft_len) != (400, 160, 512):
            raise NotImplementedError("the engine builds Uformer() with its default front end (400/160/512)")
        super().__init__(**kw)

    def load_state_dict(self, sd, strict=True):
        return super().load_state_dict({k: v for k, v in sd.items() if k not in self._IGNORED}, strict)

    def forward(self, inputs, src=None, spectra=True):
        if self.engine is None:
            raise RuntimeError("load_state_dict() must be called before forward()")
        return self.engine.uformer_forward(inputs.contiguous(), None if src is None else src.contiguous(), spectra)

    def __call__(self, inputs, src=None, spectra=True):
        return self.forward(inputs, src, spectra)


MODEL_CLASSES = {'fullsubnet': Model, 'uformer': Uformer, 'g2net': _g2net, 'taylorsenet': _taylor, 'gcrn': Net, 'lstm': lstm_net, 'crn': crn_net, 'dpcrn': dpcrn,
                 'dccrn': lambda **kw: DCCRN(rnn_units=256, masking_mode='E', use_clstm=True,
                                             kernel_num=[32, 64, 128, 256, 256, 256], **kw)}
