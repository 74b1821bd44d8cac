"""The tracking unit-RMS scale of frame-online streams (se_stream_begin_tracking, include/se_engine.h) restated in numpy float64, for the
tests of the scale kernel and of the streams that run on it.  Not a test module."""
import numpy as np


def lam_of(tau_samples, hop):
    tau = float(np.float32(tau_samples))          # the entry point takes a float
    return float(np.exp(-hop / tau)) if tau > 0 else 1.0


def states(x, hop, lam, n_total, flush):
    """(E, W) behind every block of the first n_total samples of the rows x [B, >= n_total]: whole blocks, and at the flush the short
    block of the n_total % hop samples left; [B, nblocks] each"""
    x = np.asarray(x, np.float64)
    B = x.shape[0]
    k1, r = n_total // hop, n_total % hop
    lens = [hop] * k1 + ([r] if flush and r else [])
    E, W = np.zeros((B, len(lens))), np.zeros((B, len(lens)))
    e_prev, w_prev = np.zeros(B), np.zeros(B)
    for k, n in enumerate(lens):
        blk = x[:, k * hop:k * hop + n]
        e_prev = lam * e_prev + (blk * blk).sum(-1)
        w_prev = lam * w_prev + n
        E[:, k], W[:, k] = e_prev, w_prev
    return E, W


def frame_scales(x, n_fft, hop, lam, n_total, flush, n_frames):
    """c_t of frames [0, n_frames) in float64, [B, n_frames]: the state behind block K(t) - 1, the last state there is past it"""
    E, W = states(x, hop, lam, n_total, flush)
    B, nb = E.shape
    D = (n_fft // 2) // hop
    c = np.ones((B, n_frames))
    for t in range(n_frames):
        k = min(t + D - 1, nb - 1)
        if k >= 0:
            ok = E[:, k] > 1e-20
            c[:, t] = np.where(ok, np.sqrt(W[:, k] / np.where(ok, E[:, k], 1.0)), 1.0)
    return c


def frames_released(n_total, n_fft, hop):
    return (n_total - n_fft // 2 - 1) // hop + 1 if n_total > n_fft // 2 else 0
