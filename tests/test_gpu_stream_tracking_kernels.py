"""GPU: the scale kernel of the tracking unit-RMS scale (csrc/k_misc.hip launch_stream_track) and the forward transform with per-frame
scales (csrc/k_stft2.hip stft2_kernel<.., FSC>), one launch at a time through csrc/tests/track_probe.hip -> libse_trackprobe.so, against
the float64 restatement of tests/tracking_ref.py.  Every buffer has NaN-filled slack around it that has to stay NaN, and the input
window handed to a launch holds exactly the samples a stream's window holds (NaN elsewhere), at a non-zero origin from the first slide on.

Bounds: (E, W) are float64 sums of at most a few hundred terms - 1e-12 relative; a ring entry is one float32 rounding of a float64
value - 1e-6 relative with slack; two different splits of one signal give bit-identical ring entries."""
import ctypes as C
import os

import numpy as np
import pytest

import se_amd  # noqa: F401
import tracking_ref as TR

pytestmark = pytest.mark.gpu
PKG = os.path.dirname(os.path.abspath(se_amd.__file__))
LIB = os.path.join(PKG, 'libse_trackprobe.so')
B, RING, PAD = 3, 128, 16
_L = {}


def _lib():
    if 'l' not in _L:
        assert os.path.exists(LIB), 'libse_trackprobe.so is missing: run build() (make -C csrc)'
        L = C.CDLL(LIB)
        vp, i, d, f, lg = C.c_void_p, C.c_int, C.c_double, C.c_float, C.c_long
        L.tp_stream_track.argtypes = [i, i, vp, lg, i, i, i, i, d, vp, vp, vp, vp, i, i, i, i]
        L.tp_stft.argtypes = [i, i, vp, lg, i, i, i, vp, f, vp, vp, i, i, i, i, i, vp, i]
        L.tp_last_error.restype = C.c_char_p
        _L['l'] = L
    return _L['l']


def _keep_from(n_fft, hop, t_done, n_total):
    """csrc/stream_window.h stream_keep_from"""
    return max(0, min(t_done * hop - n_fft // 2, n_total - n_fft // 2 - 1)) & ~3


def _padded(torch, shape, dtype):
    """a NaN-filled buffer with PAD elements of slack on either side; (whole, view)"""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * PAD,), float('nan'), dtype=dtype, device='cuda')
    return whole, whole[PAD:PAD + n].view(*shape)


def _run(x, n_fft, hop, tau, pushes):
    """the pushes, then the flush; returns (E, W) and the scale c after every call, and the two rings at the end"""
    import torch
    L = _lib()
    lam = TR.lam_of(tau, hop)
    total = x.shape[1]
    assert sum(pushes) == total
    wew, ew = _padded(torch, (B, 2), torch.float64)
    wc, c = _padded(torch, (B,), torch.float32)
    wfc, fc = _padded(torch, (B, RING), torch.float32)
    wfi, fi = _padded(torch, (B, RING), torch.float32)
    ew.zero_(); c.fill_(1.0); fc.fill_(1.0); fi.fill_(1.0)
    n_total = t_done = w0 = 0
    log = []
    for n_new in list(pushes) + [None]:
        fin = n_new is None
        if not fin:
            # the engine slides before it appends: from the second half of the signal on, the window starts at its keep bound
            if n_total > total // 3:
                w0 = max(w0, _keep_from(n_fft, hop, t_done, n_total))
            n_total += n_new
        pitch = total - w0 + 8
        wwin, win = _padded(torch, (B, pitch), torch.float32)
        win[:, :n_total - w0] = torch.from_numpy(x[:, w0:n_total]).cuda()
        t1 = (1 + n_total // hop + 1) if fin else max(t_done, TR.frames_released(n_total, n_fft, hop))
        rc = L.tp_stream_track(n_fft, hop, win.data_ptr(), pitch, B, n_total, 0 if fin else n_new, int(fin), lam, ew.data_ptr(), c.data_ptr(),
                               fc.data_ptr(), fi.data_ptr(), RING, t_done, t1, w0)
        assert rc == 0, L.tp_last_error().decode()
        t_done = t1
        log.append((n_total, fin, t_done, w0, ew.cpu().numpy().copy(), c.cpu().numpy().copy()))
        for whole in (wew, wc, wfc, wfi, wwin):
            h = whole.cpu().numpy()
            assert np.isnan(h[:PAD]).all() and np.isnan(h[-PAD:]).all(), 'slack written'
        hw = win.cpu().numpy()
        assert np.isnan(hw[:, n_total - w0:]).all(), 'window written'
    assert t_done <= RING
    return log, fc.cpu().numpy(), fi.cpu().numpy(), lam


@pytest.mark.parametrize('n_fft,hop', [(320, 160), (512, 128)])
@pytest.mark.parametrize('tau_s', [0.0, 0.05, 2.0])
def test_scale_kernel_against_float64(n_fft, hop, tau_s):
    rng = np.random.default_rng(n_fft + int(tau_s * 100))
    split_a = [0, 1, hop - 1, hop, 3 * hop + 7, 0, 5 * hop + 3, 2 * hop, 77]
    total = sum(split_a)
    assert total % hop != 0
    split_b = [hop + 5, 4 * hop, 1, 1, total - 5 * hop - 7]
    x = (rng.standard_normal((B, total)) * np.array([[0.5], [0.02], [3.0]])).astype(np.float32)
    tau = tau_s * 16000.0
    log, fc_a, fi_a, lam = _run(x, n_fft, hop, tau, split_a)
    for n_total, fin, t_done, w0, ew, c in log:
        E, W = TR.states(x, hop, lam, n_total, fin)
        if E.shape[1]:
            np.testing.assert_allclose(ew[:, 0], E[:, -1], rtol=1e-12, atol=0, err_msg='E at %d' % n_total)
            np.testing.assert_allclose(ew[:, 1], W[:, -1], rtol=1e-12, atol=0, err_msg='W at %d' % n_total)
        else:
            assert (ew == 0).all()
        ref = TR.frame_scales(x, n_fft, hop, lam, n_total, fin, max(t_done, 1))
        np.testing.assert_allclose(c, ref[:, t_done - 1] if t_done else np.ones(B), rtol=1e-6, err_msg='c at %d' % n_total)
    n_total, fin, t_done = log[-1][:3]
    ref = TR.frame_scales(x, n_fft, hop, lam, n_total, True, t_done)
    np.testing.assert_allclose(fc_a[:, :t_done], ref, rtol=1e-6)
    np.testing.assert_allclose(fi_a[:, :t_done], 1.0 / ref, rtol=1e-6)
    assert (fc_a[:, t_done:] == 1.0).all() and (fi_a[:, t_done:] == 1.0).all()
    # the level is followed where the estimate forgets, and rows of different level have different scales
    assert fc_a[1, t_done - 1] > 10 * fc_a[0, t_done - 1] > 10 * fc_a[2, t_done - 1] / 2
    _, fc_b, fi_b, _ = _run(x, n_fft, hop, tau, split_b)
    assert fc_a.tobytes() == fc_b.tobytes() and fi_a.tobytes() == fi_b.tobytes(), 'ring entries depend on the split'


def test_silence_gives_unit_scale():
    x = np.zeros((B, 1000), np.float32)
    log, fc, fi, _ = _run(x, 320, 160, 800.0, [1000])
    assert (fc == 1.0).all() and (fi == 1.0).all() and (log[-1][5] == 1.0).all()


@pytest.mark.parametrize('n_fft,hop', [(320, 160), (512, 128)])
@pytest.mark.parametrize('mag,p_in', [(True, 1.0), (False, 0.5)])
def test_stft_with_per_frame_scales_equals_per_row_launches(n_fft, hop, mag, p_in):
    """The variant against the common kernel: frame t under c_t has to equal frame t of a launch whose per-row scale is c_t.  The two are
    not bit-identical: frames (t, t + 1) share one complex transform, whose rounding error in either frame is relative to the larger of
    the two - and the partner frame is scaled by c_(t+1) here, by c_t there.  The bound is the transform's own: 8 log2(n_fft) 2^-24 of the
    largest bin of the pair (a radix-2 FFT accumulates at most log2 N roundings per output, each with a few operations), taken on the
    uncompressed spectrum (a compressed one is decompressed first, |X|^0.5 amplifies the relative error of small bins without bound).
    Covers a window origin above 0, a first frame that is odd, more than one block of 32 frames, and the last frames of a clip."""
    import torch
    L = _lib()
    T_all, F = 70, n_fft // 2 + 1
    n = (T_all - 1) * hop
    rng = np.random.default_rng(5)
    x = rng.standard_normal((B, n)).astype(np.float32)
    cs = (0.5 + rng.random((B, RING))).astype(np.float32)
    for t_first, w0, T in ((0, 0, T_all), (5, 4 * ((5 * hop - n_fft // 2) // 4), T_all), (33, 0, 41)):
        pitch = n - w0 + 4
        win = torch.full((B, pitch), float('nan'), device='cuda')
        win[:, :n - w0] = torch.from_numpy(x[:, w0:]).cuda()
        Tp = T - t_first + 3
        fct = torch.from_numpy(cs).cuda()

        def launch(c_row, ring_buf):
            wspec, spec = _padded(torch, (B, 2, F, Tp), torch.float32)
            wmag, mg = _padded(torch, (B, F, Tp), torch.float32)
            rc = L.tp_stft(n_fft, hop, win.data_ptr(), pitch, B, n, n, c_row.data_ptr() if c_row is not None else None, p_in, spec.data_ptr(),
                           mg.data_ptr() if mag else None, T, Tp, t_first, 1, w0, ring_buf.data_ptr() if ring_buf is not None else None, RING)
            assert rc == 0, L.tp_last_error().decode()
            for whole in (wspec, wmag):
                h = whole.cpu().numpy()
                assert np.isnan(h[:PAD]).all() and np.isnan(h[-PAD:]).all(), 'slack written'
            return spec.cpu().numpy(), mg.cpu().numpy()

        def linear(sp):
            """[B, 2, F, Tp] compressed by p_in -> the uncompressed spectrum (same phase, magnitude^(1 / p_in))"""
            if p_in == 1.0:
                return sp.astype(np.float64)
            m = np.sqrt((sp.astype(np.float64) ** 2).sum(1, keepdims=True))
            return sp * m ** (1.0 / p_in - 1.0)

        got, gmag = launch(None, fct)
        assert np.isnan(got[..., 0]).all() and np.isnan(got[..., T - t_first + 1:]).all(), 'columns outside the launch written'
        got = linear(got[..., 1:T - t_first + 1])
        tol = 8 * np.log2(n_fft) * 2.0 ** -24
        worst = 0.0
        for t in range(t_first, T):
            ref, rmag = launch(torch.from_numpy(np.ascontiguousarray(cs[:, t & (RING - 1)])).cuda(), None)
            ref = linear(ref[..., 1:T - t_first + 1])
            col = t - t_first
            # the partner of frame t in its transform: frames are paired from the launch's first frame on
            mate = col + 1 if col % 2 == 0 else col - 1
            cols = [col] + ([mate] if mate < T - t_first else [])
            a, b = got[..., col], ref[..., col]
            scale = max(np.abs(got[..., cols]).max(), np.abs(ref[..., cols]).max())
            worst = max(worst, np.abs(a - b).max() / scale)
            assert np.isfinite(a).all() and np.abs(a - b).max() <= tol * scale, (t_first, t, np.abs(a - b).max(), scale)
            if mag:
                ga, gb = gmag[..., col + 1].astype(np.float64) ** (1 / p_in), rmag[..., col + 1].astype(np.float64) ** (1 / p_in)
                assert np.abs(ga - gb).max() <= tol * scale, (t_first, t, 'mag')
        print('stft per-frame scales', n_fft, hop, mag, p_in, 'first frame', t_first, 'worst error / pair max', worst, 'bound', tol)
