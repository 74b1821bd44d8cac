#!/usr/bin/env python
"""The offline resampler on its own: one staged batch of the file -> file driver, device-resident.

256 rows of VoiceBank+DEMAND-shaped lengths (1.2 - 9.8 s, the generator of tools/corpus_bench.py) as raw PCM_16 at `--fs`, resampled to
16 kHz two ways in one process, alternating:
  (a) per_row : se_pcm16_decode of the batch, then one se_resample call per row - what the driver's reader did per staged batch;
  (b) ragged  : one se_resample_ragged call straight from the 2-byte samples.
Each sample is the stream-synchronised wall time of one whole batch; the line reports the medians, and beside them the spread of the
repeated identical runs (min, max, and the median of |x - median|), so a difference can be read against it.  One JSON line per rate.

    python tools/resample_bench.py [--fs 48000 44100] [--rows 256] [--reps 15]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402


def _spread(xs):
    xs = np.asarray(xs)
    med = float(np.median(xs))
    return {'median_ms': round(1e3 * med, 3), 'min_ms': round(1e3 * float(xs.min()), 3), 'max_ms': round(1e3 * float(xs.max()), 3),
            'mad_ms': round(1e3 * float(np.median(np.abs(xs - med))), 3), 'n': len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--fs', type=int, nargs='+', default=[48000, 44100])
    ap.add_argument('--rows', type=int, default=256)
    ap.add_argument('--reps', type=int, default=15)
    args = ap.parse_args()
    import torch
    import se_amd  # noqa: F401
    from se_amd import _lib, resample
    from corpus_bench import corpus_lengths
    lib = _lib.load()
    dev = torch.device('cuda', torch.cuda.current_device())
    stream = torch.cuda.current_stream()
    st = C.c_void_p(stream.cuda_stream)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    for fs in args.fs:
        native = [int(round(n16 * fs / 16000.0)) for n16 in corpus_lengths(args.rows)]
        lens16 = [resample.resample_samples(n, fs, 16000) for n in native]
        nb, nmax, lmax = len(native), max(native), max(lens16)
        rng = np.random.default_rng(fs)
        x = torch.from_numpy(rng.integers(-8000, 8000, (nb, nmax), dtype=np.int16)).to(dev)
        nat = torch.empty((nb, nmax), dtype=torch.float32, device=dev)
        out_a = torch.zeros((nb, lmax), dtype=torch.float32, device=dev)
        out_b = torch.full((nb, lmax), float('nan'), dtype=torch.float32, device=dev)
        arr = (C.c_int32 * nb)(*native)

        def per_row():
            rc = lib.se_pcm16_decode(p(x), nmax, nb, nmax, p(nat), nmax, st)
            for r in range(nb):
                rc |= lib.se_resample(p(nat, 4 * r * nmax), native[r], 1, native[r], fs, 16000, p(out_a, 4 * r * lmax), lens16[r], st)
            assert rc == 0, lib.se_last_error(None).decode()

        def ragged():
            assert lib.se_resample_ragged(p(x), resample.SAMPLES_S16, nmax, nb, arr, fs, 16000, p(out_b), lmax, st) == 0, \
                lib.se_last_error(None).decode()

        def timed(fn):
            stream.synchronize()
            t0 = time.perf_counter()
            fn()
            stream.synchronize()
            return time.perf_counter() - t0

        for fn in (per_row, ragged, per_row, ragged):          # tables, code objects, clocks
            timed(fn)
        ta, tb = [], []
        for _ in range(args.reps):                              # alternating: a drift of the clocks meets both forms alike
            ta.append(timed(per_row))
            tb.append(timed(ragged))
        same = all(torch.equal(out_a[r, :lens16[r]], out_b[r, :lens16[r]]) for r in range(nb))
        a, b = _spread(ta), _spread(tb)
        print(json.dumps({'tool': 'resample_bench', 'fs_in': fs, 'rows': nb, 'audio_s': round(sum(lens16) / 16000.0, 1),
                          'samples_in': int(sum(native)), 'per_row': a, 'ragged': b,
                          'ragged_over_per_row': round(b['median_ms'] / a['median_ms'], 3), 'rows_equal': bool(same)}), flush=True)


if __name__ == '__main__':
    main()
