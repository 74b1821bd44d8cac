"""GPU: one engine through every entry point that makes it own something - graph staging rows and the capture stream, the ragged
ring, the stream window and its twin, the running-RMS ring, the window rows of a ragged long decode, the hook buffer - then
close(), and a second engine with the same weights that has to compute what the first one did: the destroy path releases
everything once and leaves the device as a fresh start finds it.  Nothing here provokes an error.  And one StreamResampler that is
created, pushed once and destroyed."""
import numpy as np
import pytest

import se_amd  # noqa: F401
from se_amd import synth

pytestmark = pytest.mark.gpu

MS = 4000


def _engine():
    from se_amd.models import MODEL_CLASSES
    return MODEL_CLASSES['crn'](max_batch=2, max_samples=MS, graphs=True, sliding_stream=True).load_synthetic(12).engine


def _clips(n, seed):
    import torch
    x = np.stack([synth.synth_clip(seed + b, 'speech' if b % 2 == 0 else 'white', n) for b in range(2)])
    return torch.from_numpy(x).cuda()


def _lifecycle(eng, short, long_):
    """the calls in turn -> {name: output}; every owner of the engine is populated at the end"""
    import torch
    out = {}
    for k in ('warm', 'capture', 'replay'):                    # three calls of one shape
        out['batch_' + k] = eng.enhance_batch(short)
    out['ragged'] = eng.enhance_ragged(short, [4000, 3000])
    eng.stream_begin(2, max_chunk_frames=4, running_rms=True)   # 9000 samples through a window made for 4000: it slides
    pieces = [eng.stream_push(long_[:, p:p + 1500].contiguous()) for p in range(0, 9000, 1500)]
    out['stream'] = torch.cat(pieces + [eng.stream_flush()], dim=1)
    out['long'] = eng.enhance_long(long_, max_chunk_frames=7)
    out['long_ragged'] = eng.enhance_long_ragged(long_, [9000, 7000])
    c, spec = eng.frontend(short)
    mag = torch.sqrt(spec[:, 0] ** 2 + spec[:, 1] ** 2).contiguous()
    out['hook'] = eng.backend('mag', mag, MS, spec=spec, c=c)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def test_close_releases_everything_and_a_second_engine_starts_fresh():
    short, long_ = _clips(MS, 810), _clips(9000, 820)
    first = _engine()
    n4, n3, n9, n7 = (first.output_samples(n) for n in (4000, 3000, 9000, 7000))
    a = _lifecycle(first, short, long_)
    first.close()
    first.close()                                               # (a closed handle stays closed)
    second = _engine()
    b = _lifecycle(second, short, long_)
    second.close()
    assert a['batch_warm'].shape == a['ragged'].shape == (2, n4) and a['hook'].shape == (2, MS)
    assert a['stream'].shape == a['long'].shape == a['long_ragged'].shape == (2, n9)
    for k, v in a.items():
        assert np.isfinite(v).all() and np.abs(v).max() > 0, k
    assert np.array_equal(a['batch_replay'], a['batch_warm'])                             # (graph replay = the eager decode)
    assert not a['ragged'][1, n3:].any() and not a['long_ragged'][1, n7:].any()           # (zeros behind a shorter row's end)
    for k in ('batch_warm', 'batch_capture', 'batch_replay', 'long'):
        assert np.array_equal(a[k], b[k]), (k, np.abs(a[k] - b[k]).max())


def test_stream_resampler_is_created_pushed_once_and_destroyed():
    from se_amd import resample as HR
    x = _clips(4800, 830)
    with HR.StreamResampler(48000, 16000, max_batch=2, max_push=4800) as rs:
        rs.begin(2)
        y = rs.push(x).cpu().numpy()
    assert y.shape == (2, HR.ready_samples(4800, 48000, 16000)) and np.isfinite(y).all() and np.abs(y).max() > 0
