"""GPU: frame-online streams that outlive max_samples (SE_CFG_STREAM_SLIDING, `sliding_stream=True`): the engine keeps a window of
max_samples + n_fft + hop input samples per stream and slides it (csrc/stream_window.h, csrc/k_misc.hip stream_slide_kernel)
instead of holding every sample since se_stream_begin.

The yardstick throughout is the OFFLINE decode of the whole signal on a second, unflagged engine with max_samples = L - the
existing tests pin that decode to the reference - and the bar is the streamed-vs-offline bar of tests/test_gpu_streaming.py:
identical shape and rms(got - ref) < 1e-6 + 2e-5 rms(ref).  The sliding engines are made for max_samples = 4000: 26 frames at
hop 160, where CTSNet_new's rings hold 128 columns and every model's frame counters run far past the frames the arena was
planned for.  Every model's se_stream_begin accepts max_samples = 4000 (the workspace is planned for at least the model's
history columns + 16 frames), so no model needs a larger engine here."""
import ctypes as C
import functools

import numpy as np
import pytest

import se_amd  # noqa: F401
from se_amd import synth
from conftest import rms

pytestmark = pytest.mark.gpu

MS = 4000                       # max_samples of the sliding engines
SEEDS = {'crn': 12, 'lstm': 11, 'gcrn': 16, 'dpcrn': 13, 'dccrn': 14, 'taylorsenet_new': 19, 'g2net_new': 20}
# (n_fft, hop, frames of look-ahead): the algorithmic latency is n_fft / 2 + 1 samples + (look-ahead + 1) hops
GEOM = {'crn': (320, 160, 0), 'g2net_new': (320, 160, 0)}
DCCRN_CL = dict(rnn_units=256, use_clstm=True, kernel_num=[32, 64, 128, 256, 256, 256])       # dccrn_decode_snr.py:12
FSN_KW = dict(sb_num_neighbors=15, fb_num_neighbors=0, num_freqs=257, look_ahead=2, sequence_model="LSTM",
              fb_output_activate_function="ReLU", sb_output_activate_function=None, fb_model_hidden_size=512,
              sb_model_hidden_size=384, weight_init=True, num_groups_in_drop_band=2)
ALL = ['crn', 'lstm', 'gcrn', 'dpcrn', 'dccrn', 'dccrn_snr', 'ctsnet_new', 'taylorsenet_new', 'g2net_new', 'fullsubnet_cum']


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _make(name, B, max_samples, **kw):
    """the models and weight seeds of the existing streaming tests (test_gpu_streaming.py, test_gpu_dccrn_snr.py, test_gpu_models.py)"""
    from se_amd import models_new
    from se_amd.models import MODEL_CLASSES, DCCRN_SNR, Model
    if name == 'ctsnet_new':
        return models_new.CTSNet(max_batch=B, max_samples=max_samples, **kw).load_synthetic(17, 18)
    if name == 'dccrn_snr':
        return DCCRN_SNR(**DCCRN_CL, max_batch=B, max_samples=max_samples, **kw).load_synthetic(14)
    if name == 'fullsubnet_cum':
        return Model(max_batch=B, max_samples=max_samples, p_in=0.5, p_out=2.0, norm_type="cumulative_laplace_norm", **FSN_KW,
                     **kw).load_synthetic(15)
    return MODEL_CLASSES[name](max_batch=B, max_samples=max_samples, **kw).load_synthetic(SEEDS[name])


def _rows(name):
    return 1 if name == 'fullsubnet_cum' else 2


@functools.lru_cache(maxsize=None)
def _offline(name, L):
    """(signal, its offline decode, its unit-RMS scale) from an unflagged engine with max_samples = L: computed once per model,
    shared by every case, never written to"""
    torch = _torch()
    B = _rows(name)
    x = np.stack([synth.synth_clip(800 + b, 'speech' if b % 2 == 0 else 'white', L) for b in range(B)])
    m = _make(name, B, L)
    xt = torch.from_numpy(x).cuda()
    ref = m.enhance_batch(xt).cpu().numpy()
    c = m.engine.rms_scale(xt).cpu().numpy()
    m.engine.close()
    for a in (x, ref, c):
        a.setflags(write=False)
    return x, ref, c


_ENGINES = {}


def _sliding(name):
    """one sliding engine per model for the whole module: its streams follow one another on it, as a server's would"""
    if name not in _ENGINES:
        _ENGINES[name] = _make(name, _rows(name), MS, sliding_stream=True).engine
    return _ENGINES[name]


@pytest.fixture(scope='module', autouse=True)
def _release_shared_engines():
    yield
    for eng in _ENGINES.values():
        eng.close()
    _ENGINES.clear()
    _offline.cache_clear()


def _stream(eng, xt, pieces, chunk, c=None, running=False):
    """push xt piecewise (the last piece size repeats), flush; returns the outputs of every call, flush last"""
    B, L = xt.shape
    if running:
        eng.stream_begin(B, max_chunk_frames=chunk, running_rms=True)
    else:
        eng.stream_begin(B, c=c, max_chunk_frames=chunk)
    outs, pos, k = [], 0, 0
    while pos < L:
        n = min(pieces[min(k, len(pieces) - 1)], L - pos)
        outs.append(eng.stream_push(xt[:, pos:pos + n].contiguous()).cpu().numpy())
        pos += n
        k += 1
    outs.append(eng.stream_flush().cpu().numpy())
    return outs


def _close(got, ref):
    e = rms(got - ref)
    return got.shape == ref.shape and e < 1e-6 + 2e-5 * rms(ref), (got.shape, ref.shape, e, rms(ref))


# ------------------------------------------------------------------------------------------------ 1. past the limit = offline
@pytest.mark.parametrize('name', ALL)
@pytest.mark.parametrize('pieces,chunk', [([160], 1), ([37, 1000, 3, 481, 2000], 4), ([4000], 16)])
def test_stream_past_max_samples_equals_offline(name, pieces, chunk):
    """L = 14001 = 3.5 x max_samples and no hop multiple: the right-edge reflection and the hop-multiple tail pad (DCCRN, CTSNet,
    TaylorSENet) are read through a window that has slid."""
    torch = _torch()
    L = 14001
    x, ref, c = _offline(name, L)
    eng = _sliding(name)
    outs = _stream(eng, torch.from_numpy(x).cuda(), pieces, chunk, c=torch.from_numpy(c).cuda())
    got = np.concatenate(outs, axis=1)
    ok, info = _close(got, ref)
    print(name, pieces, chunk, 'sliding stream vs offline (shape, shape, rms err, rms ref)', info)
    assert ok, (name, info)


# ------------------------------------------------------------------------------------------------ 2. many slides
@pytest.mark.parametrize('name', ['crn', 'g2net_new'])
def test_many_slides(name):
    """3 s in 10 ms pushes through a window of 4480 samples: the window is full after 28 pushes and after every 26 more, each
    slide frees 26 hops - 11 slides in the 300 pushes (12 x max_samples of signal; a window of max_samples + n_fft + hop slides
    every 4160 samples, not every 4000).  Output keeps arriving within the algorithmic latency after every push."""
    torch = _torch()
    L = 48000
    x, ref, c = _offline(name, L)
    eng = _sliding(name)
    outs = _stream(eng, torch.from_numpy(x).cuda(), [160], 1, c=torch.from_numpy(c).cuda())
    n_fft, hop, la = GEOM[name]
    fed = emitted = 0
    for o in outs[:-1]:
        fed += 160
        emitted += o.shape[1]
        assert emitted >= fed - (n_fft // 2 + 1) - (la + 2) * hop or fed < n_fft, (fed, emitted)
    ok, info = _close(np.concatenate(outs, axis=1), ref)
    print(name, '48000 samples through a 4000-sample engine (shape, shape, rms err, rms ref)', info)
    assert ok, (name, info)


# ------------------------------------------------------------------------------------------------ 3. sliding = bounded, push for push
@pytest.mark.parametrize('name', ['crn', 'dccrn', 'g2net_new'])
def test_running_rms_sliding_equals_bounded_push_for_push(name):
    """se_stream_begin_running: the running scale reads the newest samples of every push and keeps 1 / c per frame in a ring - both
    through the window origin.  A sliding engine (max_samples = 4000) and a bounded one (max_samples = L) fed the same pushes
    return the same number of samples every time and the same signal; scaling the input scales the output."""
    torch = _torch()
    L, B = 16000, 2
    x = np.stack([synth.synth_clip(870 + b, 'white', L) for b in range(B)])
    xt = torch.from_numpy(x).cuda()
    bounded = _make(name, B, L).engine
    want = _stream(bounded, xt, [160], 8, running=True)
    bounded.close()
    eng = _sliding(name)
    got = _stream(eng, xt, [160], 8, running=True)
    assert [o.shape for o in got] == [o.shape for o in want]
    want, got = np.concatenate(want, axis=1), np.concatenate(got, axis=1)
    ok, info = _close(got, want)
    print(name, 'running-RMS stream, sliding vs bounded (shape, shape, rms err, rms ref)', info)
    assert ok and np.isfinite(got).all(), (name, info)
    scaled = np.concatenate(_stream(eng, xt * 0.25, [160], 8, running=True), axis=1)
    assert rms(scaled - 0.25 * got) < 1e-6 + 2e-5 * rms(got), rms(scaled - 0.25 * got)


# ------------------------------------------------------------------------------------------------ 4. contract
def test_sliding_stream_refuses_a_push_longer_than_max_samples_and_goes_on():
    torch = _torch()
    from se_amd.engine import EngineError
    L = 14001
    x, ref, c = _offline('crn', L)
    xt = torch.from_numpy(x).cuda()
    eng = _sliding('crn')
    eng.stream_begin(2, c=torch.from_numpy(c).cuda(), max_chunk_frames=4)
    outs = [eng.stream_push(xt[:, :3000].contiguous()).cpu().numpy()]
    with pytest.raises(EngineError, match='max_samples'):
        eng.stream_push(xt[:, 3000:3000 + MS + 1].contiguous())               # refused by the wrapper ...
    buf, out, n_out = xt[:, 3000:3000 + MS + 1].contiguous(), torch.empty((2, MS + 2048), device='cuda'), C.c_int32(-1)
    rc = eng._lib.se_stream_push(eng._h, C.c_void_p(buf.data_ptr()), buf.stride(0), MS + 1, C.c_void_p(out.data_ptr()),
                                 out.stride(0), C.byref(n_out), eng._stream())
    assert rc != 0 and b'at most max_samples' in eng._lib.se_last_error(eng._h)      # ... and by the library itself
    for p in range(3000, L, MS):                                               # the stream is as it was: the rest, in the largest pushes
        outs.append(eng.stream_push(xt[:, p:p + MS].contiguous()).cpu().numpy())
    outs.append(eng.stream_flush().cpu().numpy())
    ok, info = _close(np.concatenate(outs, axis=1), ref)
    assert ok, info


def test_bounded_stream_still_ends_at_max_samples():
    torch = _torch()
    from se_amd.engine import EngineError
    eng = _make('crn', 2, MS).engine
    x = torch.from_numpy(np.stack([synth.synth_clip(800 + b, 'speech', MS + 160) for b in range(2)])).cuda()
    eng.stream_begin(2, max_chunk_frames=4)
    eng.stream_push(x[:, :MS - 160].contiguous())
    with pytest.raises(EngineError, match='stream longer than max_samples given at create'):
        eng.stream_push(x[:, MS - 160:MS + 160].contiguous())
    a = eng.stream_push(x[:, MS - 160:MS].contiguous())                        # up to the limit it goes on
    b = eng.stream_flush()
    assert a.shape[0] == 2 and b.shape[1] > 0
    eng.close()


def test_sliding_flag_does_not_make_a_model_streamable():
    _torch()
    from se_amd.engine import EngineError
    from se_amd.models import MODEL_CLASSES
    for name, seed in (('g2net', 20), ('fullsubnet', 15)):                     # InstanceNorm weights; the utterance-mean norm
        m = MODEL_CLASSES[name](max_batch=1, max_samples=MS, sliding_stream=True).load_synthetic(seed)
        assert m.engine.sliding_stream
        with pytest.raises(EngineError, match='no frame-online mode'):
            m.engine.stream_begin(1)
        m.engine.close()


@pytest.mark.parametrize('name', ['crn', 'dccrn'])
def test_offline_decode_of_a_sliding_engine_is_bit_identical(name):
    torch = _torch()
    x = torch.from_numpy(np.stack([synth.synth_clip(800 + b, 'speech' if b % 2 == 0 else 'white', MS) for b in range(2)])).cuda()
    plain = _make(name, 2, MS)
    want = plain.enhance_batch(x).cpu().numpy()
    plain.engine.close()
    eng = _sliding(name)
    got = eng.enhance_batch(x).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want)
    # ... also between two streams that slid (an offline call re-carves the arena the stream windows live in)
    L = 14001
    xs, ref, c = _offline(name, L)
    outs = _stream(eng, torch.from_numpy(xs).cuda(), [1000], 8, c=torch.from_numpy(c).cuda())
    assert _close(np.concatenate(outs, axis=1), ref)[0]
    assert np.array_equal(eng.enhance_batch(x).cpu().numpy(), want)


@pytest.mark.parametrize('name', ['crn', 'ctsnet_new'])
def test_second_stream_after_a_slide_starts_from_zero(name):
    """the window origin, like every other piece of stream state, is reset by se_stream_begin: case 1 twice on one engine"""
    torch = _torch()
    L = 14001
    x, ref, c = _offline(name, L)
    xt, ct = torch.from_numpy(x).cuda(), torch.from_numpy(c).cuda()
    eng = _sliding(name)
    for pieces, chunk in (([37, 1000, 3, 481, 2000], 4), ([37, 1000, 3, 481, 2000], 4), ([160], 1)):
        ok, info = _close(np.concatenate(_stream(eng, xt, pieces, chunk, c=ct), axis=1), ref)
        assert ok, (name, pieces, info)
