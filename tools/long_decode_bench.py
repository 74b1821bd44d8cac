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
Usage: python tools/long_decode_bench.py [--models crn,dccrn,g2net_new] [--seconds 60] [--bound 64000] [--chunk 0] [--reps 5]

--ragged: --clips (8) clips of different lengths, spread evenly over --span (20,60) seconds, through ONE engine of max_samples =
--bound and max_batch = --group: once one at a time (se_enhance_long, a call per clip) and once in groups of up to --group rows
(se_enhance_long_ragged, the groups of se_amd.decode.plan_long_groups within --max-pad).  Same box, same binary, same engine.  One
JSON line per model: calls, median wall ms, clips / s and audio seconds / s of both, their ratio, and the largest
rms(grouped row - its one-at-a-time decode) / rms(the latter) over the clips.  --row-ends makes the engine with `row_ends=True`
(SE_CFG_DCCRN_ROW_ENDS: the `_vb` DCCRN, which se_enhance_long_ragged refuses without it).

--flag-cost: what the bit costs where it should cost nothing - se_enhance_long of --group (3) equal rows of --seconds on a DCCRN
engine with and without the bit, the two engines alive together and measured in turns (plain, flagged, plain, ...), --reps runs
each.  One JSON line: median, min and max wall ms of both sides."""
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


def ragged(torch, a):
    from se_amd import decode
    lo, hi = (float(v) for v in a.span.split(','))
    secs = [lo + (hi - lo) * k / max(a.clips - 1, 1) for k in range(a.clips)]
    lens = [int(s * 16000) + 37 * k for k, s in enumerate(secs)]            # (no multiples of a hop)
    clips = [torch.from_numpy(synth.synth_clip(900 + k, 'speech', L)).cuda() for k, L in enumerate(lens)]
    groups = decode.plan_long_groups(lens, a.group, a.max_pad)
    batches = []
    for g in groups:
        rows = torch.empty((len(g), max(lens[i] for i in g)), dtype=torch.float32, device='cuda')
        for r, i in enumerate(g):
            rows[r, :lens[i]].copy_(clips[i])
        batches.append((g, rows, [lens[i] for i in g]))
    audio = sum(lens) / 16000.0
    for name in a.models.split(','):
        m = build(name, a.group, a.bound, **({'row_ends': True} if a.row_ends else {}))
        eng = m.engine
        one = lambda: [eng.enhance_long(c.view(1, -1), None, a.chunk) for c in clips]
        grouped = lambda: [eng.enhance_long_ragged(rows, ls, a.chunk) for _, rows, ls in batches]

        def timed(f):
            f()
            times = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                y = f()
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
            return float(np.median(times)), y, times
        t1, y1, all1 = timed(one)
        tg, yg, allg = timed(grouped)
        err = 0.0
        for (g, _, _), y in zip(batches, yg):
            for r, i in enumerate(g):
                ref = y1[i][0].cpu().numpy()
                got = y[r, :ref.shape[0]].cpu().numpy()
                err = max(err, float(np.sqrt(np.mean((got - ref) ** 2)) / max(np.sqrt(np.mean(ref ** 2)), 1e-12)))
        eng.close()
        side = lambda t, calls, ts: {'calls': calls, 'ms': round(t * 1e3, 2), 'ms_min': round(min(ts) * 1e3, 2), 'ms_max': round(max(ts) * 1e3, 2),
                                     'clips_per_s': round(len(lens) / t, 2),
                                     'audio_s_per_s': round(audio / t, 1)}
        print(json.dumps({'model': name, 'clips': len(lens), 'seconds': [round(L / 16000.0, 2) for L in lens], 'audio_s': round(audio, 2),
                          'max_samples': a.bound, 'max_chunk_frames': a.chunk, 'group': a.group, 'max_pad': a.max_pad,
                          'row_ends': bool(a.row_ends), 'groups': [len(g) for g in groups],
                          'one_at_a_time': side(t1, len(lens), all1), 'grouped': side(tg, len(groups), allg), 'speedup_grouped': round(t1 / tg, 3), 'max_rel_rms_diff': err}), flush=True)


def flag_cost(torch, a):
    L = int(a.seconds * 16000)
    x = torch.from_numpy(np.stack([synth.synth_clip(900 + b, 'speech', L) for b in range(a.group)])).cuda()
    engines = {'plain': build('dccrn', a.group, a.bound).engine, 'row_ends': build('dccrn', a.group, a.bound, row_ends=True).engine}
    out = {k: e.enhance_long(x, None, a.chunk) for k, e in engines.items()}          # warm-up of both
    torch.cuda.synchronize()
    same = bool(torch.equal(out['plain'], out['row_ends']))
    times = {k: [] for k in engines}
    for _ in range(a.reps):
        for k, e in engines.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e.enhance_long(x, out[k], a.chunk)
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    for e in engines.values():
        e.close()
    st = lambda ts: {'ms': round(float(np.median(ts)) * 1e3, 3), 'ms_min': round(min(ts) * 1e3, 3), 'ms_max': round(max(ts) * 1e3, 3)}
    print(json.dumps({'model': 'dccrn', 'rows': a.group, 'seconds': a.seconds, 'max_samples': a.bound, 'max_chunk_frames': a.chunk,
                      'reps': a.reps, 'plain': st(times['plain']), 'row_ends': st(times['row_ends']), 'outputs_bit_equal': same,
                      'ratio_row_ends_over_plain': round(float(np.median(times['row_ends']) / np.median(times['plain'])), 4)}), flush=True)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument('--models', default='crn,dccrn,g2net_new')
    ap.add_argument('--seconds', type=float, default=60.0)
    ap.add_argument('--bound', type=int, default=64000, help='max_samples of the bounded engine')
    ap.add_argument('--chunk', type=int, default=0, help='frames per window of the bounded engine (0 = the largest it holds)')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--ragged', action='store_true', help='clips of different lengths: one at a time against grouped')
    ap.add_argument('--clips', type=int, default=8)
    ap.add_argument('--span', default='20,60', help='shortest,longest clip of --ragged in seconds')
    ap.add_argument('--group', type=int, default=8, help='rows per grouped call of --ragged (and max_batch of its engine)')
    ap.add_argument('--max-pad', dest='max_pad', type=float, default=0.15, help='padding cap of a group of --ragged')
    ap.add_argument('--row-ends', dest='row_ends', action='store_true', help='--ragged: engines with row_ends=True (DCCRN)')
    ap.add_argument('--flag-cost', dest='flag_cost', action='store_true',
                    help='enhance_long of --group equal rows on a DCCRN engine with and without row_ends, in turns')
    a = ap.parse_args()
    if a.flag_cost:
        return flag_cost(torch, a)
    if a.ragged:
        return ragged(torch, a)
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
