"""Frame-online decode cost per model: wall time of one se_stream_push that completes `chunk` STFT frames, for B parallel
streams (synthetic weights, seeded clips).  Prints one JSON line per (model, B, chunk):
  ms_per_push, frames per push, x_realtime = audio time of the push / its wall time (per stream), host_enqueue_ms = the part of it the
  call itself takes (everything enqueued, nothing waited for); launches are not counted.
--sliding N: engines made for max_samples = N with `sliding_stream=True` (SE_CFG_STREAM_SLIDING) instead of max_samples = the clip: the
  stream outlives the engine's window and slides it; the line then also carries `slides`, the number of slides among the timed pushes,
  and `mean_ms` (the median of a run in which one push in ~26 slides does not see them).
--source-rate SR: the pushes arrive at SR Hz (48000, 44100, 32000) through se_amd.source_stream.SourceRateStream - a StreamResampler
  in front of the engine's stream; a push then carries the source samples of `chunk` frames and its time includes the resampling.
--swap: time-slicing - two stream groups alternate on ONE engine through two StreamSnapshot objects, every push is
  restore -> push -> save (se_stream_restore / se_stream_save).  The line then carries, next to the plain `ms_per_push` of the same run,
  `save_ms`, `restore_ms` (one call each, timed alone) and `swapped_push_ms` (the three together), medians over the same pushes, each
  with its p95, and `snapshot_bytes`.  With --source-rate each group swaps through a SourceStreamSnapshot (the engine's stream and the
  resampler's signal); `save_ms` / `restore_ms` are then the engine's half, `resampler_save_ms` / `resampler_restore_ms` the
  resampler's (se_resampler_save / se_resampler_restore), `swapped_push_ms` a whole restore -> push -> save at the source rate, and
  `resampler_snapshot_bytes` stands beside `snapshot_bytes`.
--staggered N: N callers that arrive one hop apart, one frame per push each (models: crn,dccrn unless --models names others that
  StreamSnapshot.join accepts; ctsnet_new, taylorsenet_new, g2net_new, fullsubnet_cum and fullsubnet_cln get engines with `row_origins=True`,
  SE_CFG_STREAM_ROW_ORIGINS, without which the join refuses them).  Every caller streams alone past its left edge and is parked; then the same N snapshots are served twice,
  for the same frames: by turns at batch 1 (restore -> push -> save per caller and frame: `by_turns_ms`), and joined into one group
  (StreamSnapshot.join, `join_ms` once; then one push of N rows per frame: `joined_ms`, and `joined_swapped_ms` when the group is itself
  restored and saved around every push, as on an engine that serves other groups too).  All three are milliseconds per frame per
  caller, medians; `frame_ms` is the audio time of a frame.  A measurement tool: no threshold is attached.
  With --source-rate SR (48000, 32000) the callers are fed at SR through SourceRateStream, one hop (SR / 16000 * hop source samples)
  apart, parked as SourceStreamSnapshot pairs and joined with SourceStreamSnapshot.join (se_resampler_state_join and
  se_stream_state_join); the same result line, with `source_rate` in it.
Usage: python tools/stream_latency.py [--models crn,dccrn,ctsnet_new,fullsubnet_cln] [--batch 1,16] [--chunk 1,8] [--sliding 4000] [--source-rate 48000] [--swap] [--look-ahead 0]
       python tools/stream_latency.py --staggered 32 [--models crn,dccrn] [--source-rate 48000]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import se_amd  # noqa: E402,F401
from se_amd import synth  # noqa: E402

FSN_LOOK_AHEAD = None      # --look-ahead: Model(look_ahead=) of the FullSubNet configurations (None: the decode script's 2)
ROW_ORIGINS = ('ctsnet_new', 'taylorsenet_new', 'g2net_new', 'fullsubnet_cum', 'fullsubnet_cln')
SEEDS = {'crn': 12, 'lstm': 11, 'gcrn': 16, 'dpcrn': 13, 'dccrn': 14, 'taylorsenet_new': 19, 'g2net_new': 20}


def build(name, B, L, **kw):
    from se_amd import models_new
    from se_amd.models import MODEL_CLASSES
    if name == 'ctsnet_new':
        return models_new.CTSNet(max_batch=B, max_samples=L, **kw).load_synthetic(17, 18)
    if name.startswith('fullsubnet_') and FSN_LOOK_AHEAD is not None:
        kw['look_ahead'] = FSN_LOOK_AHEAD
    if name == 'fullsubnet_cum':        # the causal norm (base_model.py:143-166) is what makes FullSubNet streamable
        from se_amd.models import Model
        return Model(max_batch=B, max_samples=L, norm_type='cumulative_laplace_norm', **kw).load_synthetic(15)
    if name == 'fullsubnet_cln':        # the standardising causal norm (cumulative_layer_norm, base_model.py:258-294)
        from se_amd.models import Model
        return Model(max_batch=B, max_samples=L, norm_type='cumulative_layer_norm', **kw).load_synthetic(15)
    if name == 'dccrn_e':               # DCCRN(rnn_units=256, masking_mode='E'): the real-LSTM core (opt-in: --models dccrn_e)
        from se_amd.models import DCCRN
        return DCCRN(rnn_units=256, masking_mode='E', max_batch=B, max_samples=L, **kw).load_synthetic(24)
    if name == 'dccrn_snr':             # DCCRN_SNR/dccrn_decode_snr.py:12: the causal-decoder DCCRN (opt-in: --models dccrn,dccrn_snr)
        from se_amd.models import DCCRN_SNR
        return DCCRN_SNR(rnn_units=256, use_clstm=True, kernel_num=[32, 64, 128, 256, 256, 256], max_batch=B,
                         max_samples=L, **kw).load_synthetic(14)
    return MODEL_CLASSES[name](max_batch=B, max_samples=L, **kw).load_synthetic(SEEDS[name])


def count_slides(L, piece, first, max_samples, n_fft, hop):
    """slides among the pushes from index `first` on: the engine's own rule (csrc/stream_window.h) replayed on the host"""
    pitch = (max_samples + n_fft + hop + 3) // 4 * 4
    w0 = n = slides = 0
    for k, p in enumerate(range(0, L - piece + 1, piece)):
        if n - w0 + piece > pitch:
            t_done = (n - n_fft // 2 - 1) // hop + 1 if n > n_fft // 2 else 0
            w0 = max(0, min(t_done * hop - n_fft // 2, n - n_fft // 2 - 1)) // 4 * 4
            slides += k >= first
        n += piece
    return slides


def time_source_rate(a, name, B, L, hop, eng, c):
    """--source-rate: the same measurement with every push made at the source rate through SourceRateStream"""
    import torch
    from se_amd.source_stream import SourceRateStream
    sr = a.source_rate
    for chunk in map(int, a.chunk.split(',')):
        piece = round(chunk * hop * sr / 16000)                 # source samples of `chunk` frames
        Ls = L * sr // 16000 // piece * piece                   # as many whole pieces as fit the engine's max_samples at 16 kHz
        xs = torch.from_numpy(np.stack([synth.synth_clip(900 + b, 'speech', Ls, fs=sr) for b in range(B)])).cuda()
        src = SourceRateStream(eng, sr, max_push=piece)
        for rep in range(2):
            src.begin(B, c=c, max_chunk_frames=chunk)
            times, enq = [], []
            for p in range(0, Ls, piece):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                src.push(xs[:, p:p + piece])
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
                enq.append(t1 - t0)
            src.flush()
        extra = time_swap_source(src, xs, c, B, chunk, piece, Ls) if a.swap else {}
        src.close()
        t = float(np.median(times[4:]))
        print(json.dumps({'model': name, 'streams': B, 'frames_per_push': chunk, 'source_rate': sr, 'samples_per_push': piece,
                          'ms_per_push': round(t * 1e3, 3), **extra, 'p95_ms': round(float(np.percentile(times[4:], 95)) * 1e3, 3),
                          'host_enqueue_ms': round(float(np.median(enq[4:])) * 1e3, 3),
                          'x_realtime_per_stream': round(piece / sr / t, 2),
                          'x_realtime_all_streams': round(B * piece / sr / t, 1)}), flush=True)


def time_swap(eng, x, c, B, chunk, piece, L):
    """--swap: two groups by turns on one engine; returns the extra fields of the result line"""
    import torch
    from se_amd.engine import StreamSnapshot
    xs = [x, torch.flip(x, dims=[1]).contiguous()]
    snaps = [StreamSnapshot(), StreamSnapshot()]

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    for rep in range(2):                    # first pass warms up (payload and tables of the layout, lazy state slots)
        for g in range(2):
            eng.stream_begin(B, c=c, max_chunk_frames=chunk)
            eng.stream_save(snaps[g])
        sv, rs, sw = [], [], []
        for p in range(0, L - piece + 1, piece):
            for g in range(2):
                seg = xs[g][:, p:p + piece]
                if g == 0:                  # the parts alone
                    rs.append(timed(lambda: eng.stream_restore(snaps[g])))
                    eng.stream_push(seg)
                    sv.append(timed(lambda: eng.stream_save(snaps[g])))
                else:                       # one swapped push: restore -> push -> save
                    sw.append(timed(lambda: (eng.stream_restore(snaps[g]), eng.stream_push(seg), eng.stream_save(snaps[g]))))
        for g in range(2):
            eng.stream_restore(snaps[g])
            eng.stream_flush()
    med = lambda v: round(float(np.median(v[4:])) * 1e3, 3)
    p95 = lambda v: round(float(np.percentile(v[4:], 95)) * 1e3, 3)
    out = {'save_ms': med(sv), 'save_p95_ms': p95(sv), 'restore_ms': med(rs), 'restore_p95_ms': p95(rs), 'swapped_push_ms': med(sw),
           'swapped_push_p95_ms': p95(sw), 'snapshot_bytes': snaps[0].nbytes}
    for sn in snaps:
        sn.close()
    return out


def time_swap_source(src, x, c, B, chunk, piece, L):
    """--swap with --source-rate: two groups by turns on one engine and one SourceRateStream, each through a SourceStreamSnapshot"""
    import torch
    from se_amd.source_stream import SourceStreamSnapshot
    eng, res = src.engine, src.resampler
    xs = [x, torch.flip(x, dims=[1]).contiguous()]
    snaps = [SourceStreamSnapshot(), SourceStreamSnapshot()]

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    for rep in range(2):                    # first pass warms up (payloads and tables of the layout, lazy state slots)
        for g in range(2):
            src.begin(B, c=c, max_chunk_frames=chunk)
            src.save(snaps[g])
        sv, rs, rsv, rrs, sw = [], [], [], [], []
        for p in range(0, L - piece + 1, piece):
            for g in range(2):
                seg = xs[g][:, p:p + piece]
                if g == 0:                  # the parts alone: the engine's half, then the resampler's
                    rs.append(timed(lambda: eng.stream_restore(snaps[g].engine)))
                    rrs.append(timed(lambda: res.restore(snaps[g].resampler)))
                    src.push(seg)
                    sv.append(timed(lambda: eng.stream_save(snaps[g].engine)))
                    rsv.append(timed(lambda: res.save(snaps[g].resampler)))
                else:                       # one swapped push: restore -> push -> save
                    sw.append(timed(lambda: (src.restore(snaps[g]), src.push(seg), src.save(snaps[g]))))
        for g in range(2):
            src.restore(snaps[g])
            src.flush()
    med = lambda v: round(float(np.median(v[4:])) * 1e3, 3)
    p95 = lambda v: round(float(np.percentile(v[4:], 95)) * 1e3, 3)
    out = {'save_ms': med(sv), 'save_p95_ms': p95(sv), 'restore_ms': med(rs), 'restore_p95_ms': p95(rs),
           'resampler_save_ms': med(rsv), 'resampler_save_p95_ms': p95(rsv), 'resampler_restore_ms': med(rrs),
           'resampler_restore_p95_ms': p95(rrs), 'swapped_push_ms': med(sw), 'swapped_push_p95_ms': p95(sw),
           'snapshot_bytes': snaps[0].engine.nbytes, 'resampler_snapshot_bytes': snaps[0].resampler.nbytes}
    for sn in snaps:
        sn.close()
    return out


def time_staggered(name, N, ticks=100):
    """--staggered: N callers one hop apart, by turns at batch 1 and joined into one group; prints the result line"""
    import torch
    from se_amd.engine import StreamSnapshot
    hop = {'dccrn': 128, 'dccrn_snr': 128, 'fullsubnet_cum': 256, 'fullsubnet_cln': 256}.get(name, 160)
    n_fft, lag = (320 if hop == 160 else 512), {'dccrn': 6, 'fullsubnet_cum': 2, 'fullsubnet_cln': 2}.get(name, 0)
    edge = max(1, -(-(n_fft // 2) // hop), 0 if hop >= n_fft // 2 else -(-n_fft // hop) - 1 + lag)      # csrc/stream_join.h
    n0 = (edge + 1) * hop + n_fft // 2 + 1                 # the newest caller is two frames past its left edge when the group forms
    # the models whose state counts frames are joined on engines that keep a frame origin per row (SE_CFG_STREAM_ROW_ORIGINS)
    eng = build(name, N, 16000, sliding_stream=True, **({'row_origins': True} if name in ROW_ORIGINS else {})).engine
    L = n0 + (N - 1 + 2 * ticks) * hop
    x = torch.from_numpy(np.stack([synth.synth_clip(900 + b, 'speech', L) for b in range(N)])).cuda()
    c = eng.rms_scale(x[:, :16000].contiguous())
    snaps, pos = [], []
    for k in range(N):                                     # caller k arrived k hops after caller 0
        pos.append(n0 + (N - 1 - k) * hop)
        eng.stream_begin(1, c=c[k:k + 1].contiguous(), max_chunk_frames=1)
        eng.stream_push(x[k:k + 1, :pos[k]].contiguous())
        snaps.append(eng.stream_save())

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def frame(t):                                          # the callers' samples of tick t, one row each
        return torch.stack([x[k, pos[k] + t * hop:pos[k] + (t + 1) * hop] for k in range(N)])
    group = StreamSnapshot()
    StreamSnapshot.join(eng, snaps, out=group)             # (warms up: payload and tables of the layout)
    join_s = timed(lambda: StreamSnapshot.join(eng, snaps, out=group))
    eng.stream_restore(group)
    joined = [timed(lambda: eng.stream_push(frame(t))) for t in range(ticks)]
    eng.stream_save(group)
    swapped = [timed(lambda: (eng.stream_restore(group), eng.stream_push(frame(t)), eng.stream_save(group))) for t in range(ticks, 2 * ticks)]
    turns = []
    for t in range(ticks):
        seg = frame(t)
        turns.append(timed(lambda: [(eng.stream_restore(snaps[k]), eng.stream_push(seg[k:k + 1]), eng.stream_save(snaps[k])) for k in range(N)]))
    for sn in snaps + [group]:
        sn.close()
    per = lambda v: round(float(np.median(v[4:])) * 1e3 / N, 4)      # noqa: E731
    print(json.dumps({'model': name, 'callers': N, 'frame_ms': hop / 16, 'by_turns_ms': per(turns), 'joined_ms': per(joined),
                      'joined_swapped_ms': per(swapped), 'join_ms': round(join_s * 1e3, 3),
                      'by_turns_over_joined': round(float(np.median(turns[4:]) / np.median(joined[4:])), 1)}), flush=True)
    eng.close()


def time_staggered_source(name, N, sr, ticks=100):
    """--staggered with --source-rate: the same measurement with every caller fed at `sr` through SourceRateStream"""
    import torch
    from se_amd.resample import resample
    from se_amd.source_stream import SourceRateStream, SourceStreamSnapshot
    assert sr % 16000 == 0 and sr // 16000 in (2, 3), 'SourceStreamSnapshot.join takes integer decimations: 48000, 32000'
    D = sr // 16000
    hop = {'dccrn': 128, 'dccrn_snr': 128}.get(name, 160)
    n_fft, lag = (320 if hop == 160 else 512), (6 if name == 'dccrn' else 0)
    edge = max(1, -(-(n_fft // 2) // hop), 0 if hop >= n_fft // 2 else -(-n_fft // hop) - 1 + lag)      # csrc/stream_join.h
    reach = 32769 // (512 // D) + 1                        # csrc/resample_pos.h
    # the newest caller: two frames past the engine's left edge at 16 kHz (well past the resampler's own, 64 outputs) when the group forms
    n0 = D * ((edge + 1) * hop + n_fft // 2 + 1) + reach
    step = D * hop                                         # one hop at the source rate: D * lcm(hop, 4)
    eng = build(name, N, 16000, sliding_stream=True).engine
    L = n0 + (N - 1 + 2 * ticks) * step
    x = torch.from_numpy(np.stack([synth.synth_clip(900 + b, 'speech', L, fs=sr) for b in range(N)])).cuda()
    c = eng.rms_scale(resample(x[:, :16000 * D].contiguous(), sr))
    src = SourceRateStream(eng, sr, max_push=n0 + (N - 1) * step)
    snaps, pos = [], []
    for k in range(N):                                     # caller k arrived k hops after caller 0
        pos.append(n0 + (N - 1 - k) * step)
        src.begin(1, c=c[k:k + 1].contiguous(), max_chunk_frames=1)
        src.push(x[k:k + 1, :pos[k]].contiguous())
        snaps.append(src.save())

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def frame(t):                                          # the callers' samples of tick t, one row each
        return torch.stack([x[k, pos[k] + t * step:pos[k] + (t + 1) * step] for k in range(N)])
    SourceStreamSnapshot.join(eng, snaps).close()          # (warms up: payloads and tables of the layout)
    made = []
    join_s = timed(lambda: made.append(SourceStreamSnapshot.join(eng, snaps)))
    group = made[0]
    src.restore(group)
    joined = [timed(lambda: src.push(frame(t))) for t in range(ticks)]
    src.save(group)
    swapped = [timed(lambda: (src.restore(group), src.push(frame(t)), src.save(group))) for t in range(ticks, 2 * ticks)]
    turns = []
    for t in range(ticks):
        seg = frame(t)
        turns.append(timed(lambda: [(src.restore(snaps[k]), src.push(seg[k:k + 1]), src.save(snaps[k])) for k in range(N)]))
    for sn in snaps + [group]:
        sn.close()
    src.close()
    per = lambda v: round(float(np.median(v[4:])) * 1e3 / N, 4)      # noqa: E731
    print(json.dumps({'model': name, 'callers': N, 'source_rate': sr, 'frame_ms': hop / 16, 'by_turns_ms': per(turns), 'joined_ms': per(joined),
                      'joined_swapped_ms': per(swapped), 'join_ms': round(join_s * 1e3, 3),
                      'by_turns_over_joined': round(float(np.median(turns[4:]) / np.median(joined[4:])), 1)}), flush=True)
    eng.close()


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument('--models', default=None, help='default: every streaming model (--staggered: crn,dccrn)')
    ap.add_argument('--batch', default='1,16')
    ap.add_argument('--chunk', default='1,8')
    ap.add_argument('--seconds', type=float, default=2.0)
    ap.add_argument('--sliding', type=int, default=0, help='max_samples of a sliding-stream engine (0: a bounded engine as long as the clip)')
    ap.add_argument('--source-rate', type=int, default=0, help='push at this sample rate through SourceRateStream (0: push 16 kHz samples)')
    ap.add_argument('--swap', action='store_true', help='also time two groups alternating on the engine: restore -> push -> save per push')
    ap.add_argument('--staggered', type=int, default=0, help='N callers one hop apart: by turns at batch 1 against joined into one group')
    ap.add_argument('--tracking', type=float, default=None, metavar='SECONDS',
                    help='begin on the tracking unit-RMS scale with this time constant (0: never forget) instead of a fixed scale')
    ap.add_argument('--look-ahead', type=int, default=None, metavar='FRAMES',
                    help='fullsubnet_cum / fullsubnet_cln: build Model(look_ahead=FRAMES), 0..6 (default: the decode script\'s 2); a stream '
                         'is final FRAMES frames late')
    ap.add_argument('--running', action='store_true', help='begin on the running unit-RMS scale instead of a fixed scale')
    a = ap.parse_args()
    global FSN_LOOK_AHEAD
    FSN_LOOK_AHEAD = a.look_ahead
    if (a.tracking is not None or a.running) and (a.swap or a.staggered or a.source_rate):
        ap.error('--tracking / --running time the plain push loop only: not with --swap, --staggered or --source-rate')
    if a.tracking is not None and a.running:
        ap.error('--tracking and --running exclude each other')
    scale_kw = {'tracking_rms': a.tracking} if a.tracking is not None else {'running_rms': True} if a.running else None
    if a.staggered:
        for name in (a.models or 'crn,dccrn').split(','):
            if a.source_rate:
                time_staggered_source(name, a.staggered, a.source_rate)
            else:
                time_staggered(name, a.staggered)
        return
    a.models = a.models or 'crn,lstm,gcrn,dpcrn,dccrn,ctsnet_new,taylorsenet_new,g2net_new,fullsubnet_cum,fullsubnet_cln'
    L = int(a.seconds * 16000)
    for name in a.models.split(','):
        for B in map(int, a.batch.split(',')):
            m = build(name, B, a.sliding, sliding_stream=True) if a.sliding else build(name, B, L)
            eng = m.engine
            hop = {'dccrn': 128, 'dccrn_snr': 128, 'fullsubnet_cum': 256, 'fullsubnet_cln': 256}.get(name, 160)
            x = torch.from_numpy(np.stack([synth.synth_clip(900 + b, 'speech', L) for b in range(B)])).cuda()
            c = eng.rms_scale(x)
            if a.source_rate:
                time_source_rate(a, name, B, L, hop, eng, c)
                del m, eng
                continue
            for chunk in map(int, a.chunk.split(',')):
                piece = chunk * hop
                times = []
                for rep in range(2):           # first pass warms up (lazy state slots, kernel attributes)
                    eng.stream_begin(B, max_chunk_frames=chunk, **(scale_kw or {'c': c}))
                    times, enq = [], []
                    for p in range(0, L - piece + 1, piece):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        eng.stream_push(x[:, p:p + piece])
                        t1 = time.perf_counter()          # the call has returned: everything is enqueued
                        torch.cuda.synchronize()
                        times.append(time.perf_counter() - t0)
                        enq.append(t1 - t0)
                    eng.stream_flush()
                t = float(np.median(times[4:]))
                extra = {}
                if a.sliding:
                    n_fft = 320 if hop == 160 else 512
                    extra = {'sliding_max_samples': a.sliding, 'slides': count_slides(L, piece, 4, a.sliding, n_fft, hop),
                             'pushes': len(times[4:]), 'mean_ms': round(float(np.mean(times[4:])) * 1e3, 3)}
                if a.swap:
                    extra.update(time_swap(eng, x, c, B, chunk, piece, L))
                if scale_kw:
                    extra['scale'] = 'tracking %g s' % a.tracking if a.tracking is not None else 'running'
                print(json.dumps({'model': name, 'streams': B, 'frames_per_push': chunk, 'ms_per_push': round(t * 1e3, 3), **extra,
                                  'p95_ms': round(float(np.percentile(times[4:], 95)) * 1e3, 3),
                                  'p05_ms': round(float(np.percentile(times[4:], 5)) * 1e3, 3),
                                  'host_enqueue_ms': round(float(np.median(enq[4:])) * 1e3, 3),
                                  'x_realtime_per_stream': round(piece / 16000 / t, 2),
                                  'x_realtime_all_streams': round(B * piece / 16000 / t, 1)}), flush=True)
            del m, eng


if __name__ == '__main__':
    main()
