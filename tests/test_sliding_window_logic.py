"""CPU: the window arithmetic of sliding frame-online streams (SE_CFG_STREAM_SLIDING; csrc/stream_window.h through the host-only
probe csrc/tests/stream_probe.cpp -> libse_streamprobe.so) against a brute-force scan of the STFT kernel's index rules.

stream_keep_from(n_fft, hop, t_done, n_total) names the first sample the engine keeps when it slides the window.  The scan
below enumerates every sample any later launch can read - frames t >= t_done of every possible end of the stream (final
length L >= n_total; padded length L or the next hop multiple, the two `padded_samples` the models have), with the kernel's own
rules (csrc/k_stft2.hip `sample`: idx = t hop + n - n_fft/2, negative -> -idx, >= Lpad -> 2 (Lpad - 1) - idx, read when
0 <= idx < L) - and asserts that nothing below the bound is read, that the bound is tight to the 16 B rounding, and that what
stays live plus one push of max_samples fits the window.  The look-ahead (lag) of a model delays its OUTPUT only, so it does
not enter the bound; it is part of the scan's parameters to pin that down: the answer may not depend on it."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_LIB = os.path.join(ROOT, 'sixty-years-of-frequency-domain-monaural-speech-enhancement_amd', 'libse_streamprobe.so')
# (n_fft, hop, frames of look-ahead): CRN / LSTM / GCRN / DPCRN / the cLN variants; DCCRN; DCCRN with the causal decoder; FullSubNet
GEOMS = [(320, 160, 0), (512, 128, 6), (512, 128, 0), (512, 256, 2)]


@pytest.fixture(scope='module')
def probe():
    assert os.path.exists(PROBE_LIB), 'libse_streamprobe.so is missing: run build() (make -C csrc)'
    L = C.CDLL(PROBE_LIB)
    L.sp_keep_from.argtypes = [C.c_int] * 4
    L.sp_keep_from.restype = C.c_int
    L.sp_window_pitch.argtypes = [C.c_int] * 3
    L.sp_window_pitch.restype = C.c_long
    L.sp_sample_limit.argtypes = [C.c_int] * 3
    L.sp_sample_limit.restype = C.c_longlong
    return L


def _t_avail(n_total, n_fft, hop):
    """frames se_stream_push releases: frame t is complete once sample t hop + n_fft / 2 has arrived (csrc/engine.hip)"""
    return (n_total - n_fft // 2 - 1) // hop + 1 if n_total > n_fft // 2 else 0


def _lowest_read(n_fft, hop, t_done, n_total):
    """the lowest sample index any frame t >= t_done reads, over every way the stream can still end"""
    lo = None
    n = np.arange(n_fft)
    # (final lengths over two hops cover every phase of L against the hop and both padded lengths; the mirror image of the right
    # edge only moves up with L, and the first sample of frame t_done does not move)
    for L in range(max(n_total, n_fft), max(n_total, n_fft) + 2 * hop + 1):
        for Lpad in {L, -(-L // hop) * hop}:
            T = 1 + Lpad // hop
            if t_done >= T:
                continue
            t = np.arange(t_done, T)[:, None]
            idx = t * hop + n[None, :] - n_fft // 2
            idx = np.where(idx < 0, -idx, idx)
            idx = np.where(idx >= Lpad, 2 * (Lpad - 1) - idx, idx)
            read = idx[(idx >= 0) & (idx < L)]
            if read.size:
                lo = int(read.min()) if lo is None else min(lo, int(read.min()))
    return lo


@pytest.mark.parametrize('n_fft,hop,lag', GEOMS)
def test_keep_from_against_brute_force(probe, n_fft, hop, lag):
    rng = np.random.default_rng(n_fft + hop + lag)
    totals = sorted(set([0, 1, n_fft // 2, n_fft // 2 + 1, n_fft - 1, n_fft, n_fft + hop, 4000, 4001, 4096]
                        + [int(v) for v in rng.integers(1, 6000, 6)]))
    checked = 0
    for n_total in totals:
        ta = _t_avail(n_total, n_fft, hop)
        for t_done in sorted({ta, max(0, ta - 1), max(0, ta - lag), ta // 2, 0}):      # pushes release every complete frame; fewer is legal
            keep = probe.sp_keep_from(n_fft, hop, t_done, n_total)
            lo = _lowest_read(n_fft, hop, t_done, n_total)
            assert keep >= 0 and keep % 4 == 0 and keep <= n_total, (t_done, n_total, keep)
            assert lo is not None and keep <= lo, ('a later launch reads below the bound', t_done, n_total, keep, lo)
            assert lo - keep <= 3, ('the bound keeps more than the 16 B rounding asks for', t_done, n_total, keep, lo)
            if t_done == ta:      # what stays live after a push + the largest next push fits the window
                for max_samples in (n_fft, 4000, 4001):
                    assert n_total - keep + max_samples <= probe.sp_window_pitch(max_samples, n_fft, hop)
            checked += 1
    assert checked >= 30


@pytest.mark.parametrize('n_fft,hop,lag', GEOMS)
def test_keep_from_near_the_end_of_the_sample_range(probe, n_fft, hop, lag):
    """positions near 2^31: the bound is formed in 64 bits (t_done * hop alone would still fit, the differences must too)"""
    for max_samples in (4000, 16000 * 300):
        limit = probe.sp_sample_limit(max_samples, n_fft, hop)
        assert limit == 2 ** 31 - 1 - max(max_samples, n_fft + 32 * hop)
        assert limit + n_fft // 2 + hop + 32 * hop < 2 ** 31          # the furthest index a kernel forms past n_total
        n_total = int(limit)
        ta = _t_avail(n_total, n_fft, hop)
        keep = probe.sp_keep_from(n_fft, hop, ta, n_total)
        assert keep == (ta * hop - n_fft // 2) // 4 * 4 and 0 < n_total - keep <= n_fft + 3


def test_window_pitch_is_16_byte_aligned_and_holds_what_the_header_promises(probe):
    for max_samples in (320, 4000, 4001, 4002, 4003, 64000):
        for n_fft, hop, _ in GEOMS:
            p = probe.sp_window_pitch(max_samples, n_fft, hop)
            assert p % 4 == 0 and max_samples + n_fft + hop <= p < max_samples + n_fft + hop + 4
