"""A long clip through a bounded engine against the same clip through an engine made for it: one clip of --seconds (60) at batch 1,
synthetic weights,
  windowed  se_enhance_long on an engine of max_samples = --bound (64000), windows of --chunk frames (0 = the largest it holds)
  whole     se_enhance_batch on an engine of max_samples = the clip
Prints one JSON line per model: the median wall time of both decodes (ms, synchronised around the call, --reps runs after one
warm-up), audio seconds per second, the device memory each engine takes - the drop of the device's free memory from before the
engine is created to after its first decode: weights + activation arena + lazily grown scratch and stream state - and
rms(windowed - whole) / rms(whole).  The two engines are alive one after the other, never together.  Where the engine made for the
whole clip refuses it (the offline cLN scan of the `_new` variants holds at most 3 750 frames, 37.5 s), the line carries its error
text instead of the second set of figures.
Usage: python tools/long_decode_bench.py [--models crn,dccrn,g2net_new] [--seconds 60] [--bound 64000] [--chunk 0] [--reps 5]"""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from stream_latency import build  # noqa: E402  (the models and weight seeds of the frame-online figures)
from se_amd import synth  # noqa: E402
from se_amd.engine import EngineError  # noqa: E402


def measure(torch, name, max_samples, x, call, reps):
    """(median seconds, device bytes the engine took, its output) of `call(engine)` on a fresh engine of `max_samples`"""
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free0 = torch.cuda.mem_get_info()[0]
    m = build(name, 1, max_samples)
    y = call(m.engine, x)                       # warm-up: kernel attributes, lazily grown scratch, stream state
    torch.cuda.synchronize()
    took = free0 - torch.cuda.mem_get_info()[0]
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        y = call(m.engine, x, y)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    out = y[:, :m.engine.output_samples(x.shape[1])].cpu().numpy()
    m.engine.close()
    return float(np.median(times)), int(took), out


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument('--models', default='crn,dccrn,g2net_new')
    ap.add_argument('--seconds', type=float, default=60.0)
    ap.add_argument('--bound', type=int, default=64000, help='max_samples of the bounded engine')
    ap.add_argument('--chunk', type=int, default=0, help='frames per window of the bounded engine (0 = the largest it holds)')
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    L = int(a.seconds * 16000)
    x = torch.from_numpy(synth.synth_clip(900, 'speech', L)[None]).cuda()
    y0 = torch.empty((1, L + 1024), dtype=torch.float32, device='cuda')          # both outputs exist before anything is measured
    for name in a.models.split(','):
        t_w, b_w, y_w = measure(torch, name, a.bound, x, lambda e, w, o=y0: e.enhance_long(w, o, a.chunk), a.reps)
        windowed = {'max_samples': a.bound, 'max_chunk_frames': a.chunk, 'ms': round(t_w * 1e3, 2),
                    'x_realtime': round(a.seconds / t_w, 1), 'engine_device_bytes': b_w}
        try:
            t_b, b_b, y_b = measure(torch, name, L, x, lambda e, w, o=y0: e.enhance_batch(w, o), a.reps)
        except EngineError as ex:
            print(json.dumps({'model': name, 'seconds': a.seconds, 'batch': 1, 'windowed': windowed,
                              'whole': {'max_samples': L, 'error': str(ex)}}), flush=True)
            continue
        assert y_w.shape == y_b.shape, (y_w.shape, y_b.shape)
        err = float(np.sqrt(np.mean((y_w - y_b) ** 2)) / max(np.sqrt(np.mean(y_b ** 2)), 1e-12))
        print(json.dumps({'model': name, 'seconds': a.seconds, 'batch': 1, 'windowed': windowed,
                          'whole': {'max_samples': L, 'ms': round(t_b * 1e3, 2), 'x_realtime': round(a.seconds / t_b, 1),
                                    'engine_device_bytes': b_b},
                          'ms_ratio_windowed_over_whole': round(t_w / t_b, 3),
                          'bytes_ratio_whole_over_windowed': round(b_b / max(b_w, 1), 2),
                          'rel_rms_diff': err}), flush=True)


if __name__ == '__main__':
    main()
