"""The front and back end every model and every stream passes through, one launch at a time against float64: the STFT / iSTFT
(csrc/k_stft2.hip: stft2_kernel<N, MAG, CP>, istft2_kernel<N, FSC>), the unit-RMS scales (k_stft.hip, stream_rms), stream_slide, the mask /
decompress kernels of k_misc.hip and the row-size helpers (k_rows.hip, fill_rows, zero_tail).  Every GPU case is one launcher call (a short
sequence for stream_rms) through csrc/tests/fe_probe.hip -> libse_feprobe.so on torch buffers with slack, pre-filled with NaN; it checks

  1. every element the launch owns against a float64 reference written here from the operation's definition (k_stft.hip: centre = True,
     reflect pad of the tail-padded clip, periodic Hann centred in n_fft, one-sided; inverse: C2R, synthesis window, division by the
     overlap-added squared window where it exceeds 1e-11, n_fft / 2 dropped at the head; masks: the definitions cited in k_misc.hip)
     under an elementwise bound, printing the worst error / bound per form;
  2. ownership: what the launch does not own is still NaN - columns outside [col0, col0 + T - t_first), the pitch slack, samples outside
     [o_lo, Lout), ring slots outside [t0, t1), the slack around every buffer;
  3. dead data: input the launch must not read holds NaN (wav samples >= len[b], wav memory below the window origin, spectrum columns
     >= tlen[b] and below t_lo); a ragged row's live outputs equal, bit for bit, the same clip launched alone as a batch of one;
  4. the form that ran (kernels.h FeLaunchRec) against a Python mirror of the launcher's selection; test_every_form_reached asserts the
     whole table (12 forward, 4 inverse instances) was seen.

Error bounds, per element (u = 2^-24; constants as the other kernel suites: ACT_ULP = 8u per hardware root / rsq / libm call, 2 ACT_ULP
for powf, C_DOT = 4; TINY = 2^-126, below which fp32 results may be flushed).

Forward.  For a frame whose float64 windowed, scaled samples are z and whose float64 spectrum is X,
    |dX_k| <= u (A_FWD log2(N) ||z||_2 + B_FWD |X_k|):
rounding accumulated through the butterfly stages, spread over the bins, and the error proportional to the bin itself (it dominates at a
spectral peak).  z is the input of the transform that produces the frame: the kernel transforms the frames (first + 2P, first + 2P + 1) of a
launch as one complex sequence z_a + i z_b, so ||z||^2 = ||z_a||^2 + ||z_b||^2 (a quiet frame next to a loud one carries the loud one's
rounding; a wholly silent frame is forced to exact zeros instead, and checked as such).  The constants are 4x the worst figures of float32 torch.stft (the transform the decode scripts call) against float64 on this
suite's inputs, measured on the CPU (measure_constants): a_obs = worst |dX_k| / (u log2 N ||z||) over the white and the decaying signals of all
four geometries, b_obs = worst |dX_k| / (u |X_k|) over the tonal signals at the bins with |X_k| >= ||z||_2.  The kernel factorises 8 x 8 x 8 /
5 x 8 x 8 with fp32 table twiddles and untangles two frames from one transform, so its rounding order is not pocketfft's: hence the factor 4;
a structural fault moves a bin by the order of |X|, orders of magnitude above that.  The products x c w (either order) are inside the measured
figures: the fp32 evaluations round them too.
Compressed planes Y = X |X|^(p-1), p <= 1, and mag = |X|^p: the map is differentiable with operator norm r^(p-1) at radius r and p-Hoelder with
constant 2^(1-p), so |dY| <= min(|dX| (|X| - |dX|)^(p-1), 2^(1-p) |dX|^p) (the second alone where |dX| >= |X|), plus, relative to |Y|, the
kernel's own calls: 2 ACT_ULP + 4u for p = 0.5 (root, rsq, two products), 4 ACT_ULP + 6u for powf and its division, ACT_ULP + 2u for a bare
magnitude.  Where the reference has |X|^2 <= 1e-37 (the kernel's threshold, 10 % margin) an exact zero is accepted too.  ||mag|| obeys the
bound of Y.  A frame of digital silence must be exactly zero in every plane.

Inverse.  For the float64 inverse frame x_t, |dx_t[n]| <= u (A_INV log2(N) ||x_t||_2 + B_INV |x_t[n]|), constants measured the same way
against float32 torch.fft.irfft; a sample sums it over the covering frames with their weights w[n] s_t / env and adds 3u of
sum_t |w x_t s_t| / env for the envelope division and the 1 / c or frame_inv product.

rms_scale sums in fp64: |c - ref| <= 2u |ref| (the cast and the root); stream_rms the same, its ring value 1 / c one more u.
Elementwise kernels: first-order propagation as in tests/test_gpu_uformer_kernels.py - every sqrtf, division and product u, tanhf ACT_ULP,
powf 2 ACT_ULP; a product of two unit phasors or of two complex numbers 2u per term of each component.

test_bound_holds_for_fp32_and_catches_faults (CPU) shows that plain fp32 evaluations (torch.stft / irfft, the two-for-one untangling, both
orders of x c w, the elementwise formulae) stay inside every bound and that each of the thirteen planted faults exceeds its bound by >= 10x on
a case of the GPU table.  test_references_match_golden pins the references here to the torch fp64 fixtures of tests/golden/stft.npz.

No GPU run of this suite is recorded in this docstring; profiles/frontend_kernel_forms.md holds the measured figures."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'sixty-years-of-frequency-domain-monaural-speech-enhancement_amd')
PROBE_LIB = os.environ.get('SE_FEPROBE_LIB') or os.path.join(PKG, 'libse_feprobe.so')

U = 2.0 ** -24
ACT_ULP = 8 * U
C_DOT = 4.0
TINY = 2.0 ** -126
f32 = np.float32
GEOMS = [(320, 160, 320), (512, 128, 512), (512, 256, 512), (512, 160, 400)]
GID = ['320_160_320', '512_128_512', '512_256_512', '512_160_400']
# 4x the worst float32 torch.stft / irfft figures (module docstring; measure_constants prints the observed values)
A_FWD, B_FWD, A_INV, B_INV = 3.6, 10.9, 0.25, 7.7
NFB = 32

REACHED = set()
WORST = {}


# ------------------------------------------------------------------------------------------------ float64 references
def window64(N, win):
    w = np.zeros(N)
    left = (N - win) // 2
    w[left:left + win] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / win)
    return w


def pad_to_hop(L, hop):
    """samples the STFT sees when the decode script tail-pads to a hop multiple (oracle.stft.pad_to_hop)"""
    return int(math.ceil(L / hop + 1) - 1) * hop


def ref_frames(x, L, Lpad, geom, ts):
    """the frames ts of the centred STFT of x[:L] zero-padded to Lpad, reflect-padded by n_fft / 2: float64 [len(ts)][N]"""
    N, hop, _ = geom
    xp = np.zeros(Lpad)
    xp[:L] = np.asarray(x[:L], np.float64)
    xr = np.pad(xp, N // 2, mode='reflect')
    ts = np.asarray(ts, np.int64)
    assert ts.size == 0 or ts.max() * hop + N <= xr.size
    return xr[ts[:, None] * hop + np.arange(N)[None, :]]


def ref_stft(x, c, L, Lpad, geom, ts):
    """X [F][len(ts)] complex128 and ||z||_2 per frame"""
    N, _, win = geom
    z = ref_frames(x, L, Lpad, geom, ts) * window64(N, win) * float(c)
    return np.fft.rfft(z, axis=-1).T, np.sqrt((z * z).sum(-1))


def bound_fwd(X, zn, N):
    """zn: ||z||_2 of consecutive frames starting at the launch's first frame.  The kernel transforms frames in pairs (first + 2P,
    first + 2P + 1) as ONE complex sequence z_a + i z_b, so the rounding of that transform scales with the norm of the pair"""
    zp = np.zeros(len(zn) + (len(zn) & 1))
    zp[:len(zn)] = zn
    pair = np.sqrt(zp[0::2] ** 2 + zp[1::2] ** 2).repeat(2)[:len(zn)]
    return U * (A_FWD * math.log2(N) * pair[None, :] + B_FWD * np.abs(X)) + TINY


def compress(X, dX, p):
    """Y = X |X|^(p-1), its bound per component, mag = |X|^p (module docstring)"""
    r = np.abs(X)
    if p == 1.0:
        return X, dX + TINY, r, dX + (ACT_ULP + 2 * U) * r + TINY
    with np.errstate(divide='ignore', invalid='ignore'):
        Y = np.where(r > 0, X * r ** (p - 1.0), 0.0)
        lo = r - dX
        mv = dX * np.where(lo > 0, lo, 1.0) ** (p - 1.0)
    hol = 2.0 ** (1.0 - p) * dX ** p
    dY = np.where(lo > 0, np.minimum(mv, hol), hol)
    rel = 2 * ACT_ULP + 4 * U if p == 0.5 else 4 * ACT_ULP + 6 * U
    bd = dY + rel * np.abs(Y) + np.where(r * r <= 1.1e-37, np.abs(Y), 0.0) + TINY
    return Y, bd, np.abs(Y), bd


def ref_inverse_frames(S, N):
    """S [F][n] complex128 -> x [n][N] (C2R: the imaginary parts of DC and Nyquist are ignored) and ||x_t||_2"""
    S = S.copy()
    S[0] = S[0].real
    S[-1] = S[-1].real
    x = np.fft.irfft(S.T, n=N, axis=-1)
    return x, np.sqrt((x * x).sum(-1))


def ref_istft(S, geom, t_lo, Tb, o_lo, Lo, scale):
    """frames t_lo .. Tb - 1 (S [F][Tb - t_lo]), frame t multiplied by scale[t - t_lo]; samples o_lo .. Lo - 1 -> (y, bound)"""
    N, hop, win = geom
    w = window64(N, win)
    x, xn = ref_inverse_frames(S, N)
    n_o = Lo - o_lo
    y, env, dy, sab = (np.zeros(n_o) for _ in range(4))
    dx = U * (A_INV * math.log2(N) * xn[:, None] + B_INV * np.abs(x))
    for i, t in enumerate(range(t_lo, Tb)):
        a = t * hop - N // 2                         # output sample of the frame's n = 0
        lo, hi = max(a, o_lo), min(a + N, Lo)
        if hi <= lo:
            continue
        sl, fr = slice(lo - o_lo, hi - o_lo), slice(lo - a, hi - a)
        y[sl] += x[i, fr] * w[fr] * scale[i]
        dy[sl] += dx[i, fr] * w[fr] * abs(scale[i])
        sab[sl] += np.abs(x[i, fr] * w[fr] * scale[i])
        env[sl] += w[fr] ** 2
    d = np.where(env > 1e-11, env, 1.0)
    return y / d, dy / d + 3 * U * sab / d + TINY


# ---- elementwise references: (value, bound) from float64 inputs that are exact fp32 numbers
def _pow_scale(mg, dmg, p):
    """sc = mg^(p-1) (0 at mg = 0; 1 at p = 1) and its bound"""
    if p == 1.0:
        return np.ones_like(mg), np.zeros_like(mg)
    if p == 2.0:
        return mg, dmg
    with np.errstate(divide='ignore', invalid='ignore'):
        sc = np.where(mg > 0, mg ** (p - 1.0), 0.0)
        dsc = np.where(mg > 0, sc * (abs(p - 1.0) * dmg / mg + 2 * ACT_ULP), 0.0)
    return sc, dsc


def _polar_out(er, ei, der, dei, p):
    mg = np.sqrt(er * er + ei * ei)
    dmg = der + dei + 3 * U * mg
    sc, dsc = _pow_scale(mg, dmg, p)
    return (np.stack([er * sc, ei * sc], 1),
            np.stack([der * sc + np.abs(er) * dsc + U * np.abs(er * sc), dei * sc + np.abs(ei) * dsc + U * np.abs(ei * sc)], 1) + TINY)


def ref_cmask(mask, spec, p):
    """est = X M, out = |est|^p est / |est| (DPCRN.py:33-42, dpcrn_decode_vb.py:48-57); [B][2][...]"""
    mr, mi, xr, xi = mask[:, 0], mask[:, 1], spec[:, 0], spec[:, 1]
    er, ei = xr * mr - xi * mi, xr * mi + xi * mr
    der, dei = 2 * U * (np.abs(xr * mr) + np.abs(xi * mi)), 2 * U * (np.abs(xr * mi) + np.abs(xi * mr))
    return _polar_out(er, ei, der, dei, p)


def ref_polar_pow(x, p):
    z = np.zeros_like(x[:, 0])
    return _polar_out(x[:, 0], x[:, 1], z, z, p)


def ref_mag_phase(mag, spec, p):
    """mag^p exp(j angle X), angle(0) = 0 (lstm_decode_vb.py:47-49)"""
    ph = np.arctan2(spec[:, 1], spec[:, 0])
    m = mag ** p
    out = np.stack([m * np.cos(ph), m * np.sin(ph)], 1)
    rel = (0.0 if p == 1.0 else (U if p == 2.0 else 2 * ACT_ULP)) + 6 * U
    return out, rel * np.abs(out) + TINY


def ref_dccrn_mask(mask, spec, p, mode, fault=None):
    """mask [B][2][F-1][T], spec [B][2][F][T] -> est [B][2][F][T], DC row zero (DCCRN_cprs.py:201-225, dccrn_decode_vb.py:45-58)"""
    padm = np.concatenate([mask[:, :, :1] if fault == 'dc_not_zeroed' else np.zeros_like(mask[:, :, :1]), mask], 2)
    mr, mi, xr, xi = padm[:, 0], padm[:, 1], spec[:, 0], spec[:, 1]
    if mode == 1:
        out, bd = ref_cmask(padm, spec, p)
    elif mode == 2:
        out, bd = _polar_out(xr * mr, xi * mi, U * np.abs(xr * mr), U * np.abs(xi * mi), p)
    else:
        mm, xm = np.sqrt(mr * mr + mi * mi), np.sqrt(xr * xr + xi * xi)
        ph = np.arctan2(xi, xr) + np.arctan2(mi / (mm + 1e-8), mr / (mm + 1e-8))
        th = np.tanh(mm)
        em = th * xm
        dem = ((1 - th * th) * mm * 3 * U + ACT_ULP * th) * xm + 4 * U * em
        if p == 2.0:
            dem = 2 * em * dem + U * em * em
        elif p != 1.0:
            with np.errstate(divide='ignore', invalid='ignore'):
                dem = np.where(em > 0, em ** p * (p * dem / em + 2 * ACT_ULP), 0.0)
        emp = em ** p
        out = np.stack([emp * np.cos(ph), emp * np.sin(ph)], 1)
        # the product of the two unit phasors, each component of each relative 4u: |p q| terms sum to at most 2
        bd = np.stack([dem, dem], 1) + emp[:, None] * 20 * U + U * np.abs(out) + TINY
    if fault != 'dc_not_zeroed':
        out[:, :, 0] = 0.0
        bd[:, :, 0] = TINY
    return out, bd


# ------------------------------------------------------------------------------------------------ inputs (shared by the CPU and the GPU cases)
def make_clip(L, kind, seed, silence=None):
    """fp32 clip: 'white', 'tonal' (three sinusoids of very different level, one of them on a bin of neither n_fft) or 'decay'"""
    g = np.random.default_rng(seed)
    n = np.arange(L)
    if kind == 'white':
        x = 0.1 * g.standard_normal(L)
    elif kind == 'tonal':
        x = 0.5 * np.sin(2 * np.pi * 0.0625 * n + 0.3) + 1e-3 * np.sin(2 * np.pi * 0.1931 * n) + 1e-5 * g.standard_normal(L)
    elif kind == 'decay':
        x = g.standard_normal(L) * np.exp(-6.0 * n / max(L, 1))
    else:
        raise ValueError(kind)
    x = x.astype(f32)
    if silence is not None:
        x[silence[0]:silence[1]] = 0.0
    return x


KINDS = ('white', 'tonal', 'decay')


def fwd_lengths(geom):
    """name -> (L, Lpad, T): the offline forward table"""
    N, hop, _ = geom
    out = {'shortest': (N // 2 + 1,) * 2}
    out['T31'] = ((30 * hop + hop // 3,) * 2)
    out['T32_exact'] = ((31 * hop,) * 2)
    out['T33'] = ((32 * hop + 1,) * 2)
    out['straddle_end'] = ((20 * hop + N // 2 + hop // 2,) * 2)          # frame 20 wholly inside the clip, its partner 21 not
    out['last_fast_pair'] = ((21 * hop + N // 2,) * 2)                   # the pair (20, 21) just meets the fast path's condition
    if geom == (512, 128, 512):
        L = 30 * hop + 57
        out['tail_padded'] = (L, pad_to_hop(L, hop))
        assert out['tail_padded'][1] > L
    return {k: (L, Lp, 1 + Lp // hop) for k, (L, Lp) in out.items()}


def fwd_clips(geom, name, B=3):
    L, Lpad, T = fwd_lengths(geom)[name]
    N, hop, _ = geom
    sil = None
    if T >= 31:
        s0 = 9 * hop + 17
        sil = (s0, s0 + N + 3 * hop)
    seed = 1000 * GEOMS.index(geom) + L
    xs = [make_clip(L, KINDS[b % 3], seed + b, sil if b == 1 else None) for b in range(B)]
    return xs, L, Lpad, T


def fast_path(geom, t, Tb, L):
    """the forward kernel's condition for the pair (t, t + 1), t even"""
    N, hop, _ = geom
    return t + 1 < Tb and t * hop >= N // 2 and (t + 1) * hop + N // 2 <= L


def make_spectrum(F, n, seed):
    """random complex128 [F][n] of fp32 values, with nonzero imaginary parts at DC and Nyquist, a 1 / f tilt so that bins differ in level"""
    g = np.random.default_rng(seed)
    tilt = 1.0 / (1.0 + 0.05 * np.arange(F))[:, None]
    re, im = (g.standard_normal((F, n)) * tilt).astype(f32), (g.standard_normal((F, n)) * tilt).astype(f32)
    return re.astype(np.float64) + 1j * im.astype(np.float64)


def inv_geometry(geom):
    N, hop, _ = geom
    halo = (N + hop - 1) // hop - 1
    halo += halo & 1
    return NFB - halo, halo


def make_ew(B, F, T, seed):
    """mask [B][2][F-1][T], spec [B][2][F][T], mag [B][F][T] >= 0 (fp32 values as float64) with planted exact zeros"""
    g = np.random.default_rng(seed)
    mask = g.standard_normal((B, 2, F - 1, T)).astype(f32).astype(np.float64)
    spec = (g.standard_normal((B, 2, F, T)) * np.exp(g.uniform(-6, 2, (B, 1, F, T)))).astype(f32).astype(np.float64)
    mag = np.abs(g.standard_normal((B, F, T))).astype(f32).astype(np.float64)
    mask[:, :, 1, 0] = 0.0
    spec[:, :, 2, T - 1] = 0.0
    spec[:, :, 3, T // 2] = 0.0
    mask[:, :, 2, T // 2] = 0.0
    mag[:, 1, 0] = 0.0
    return mask, spec, mag


# ------------------------------------------------------------------------------------------------ plain fp32 evaluations (CPU)
def eval32_frames(x, c, L, Lpad, geom, ts, order='slow', fault=None):
    """windowed, scaled frames in fp32 as the kernel gathers them: idx = t hop + n - N/2 reflected at 0 and at Lpad"""
    N, hop, win = geom
    w = window64(N, win)
    if fault == 'window_uncentred':
        w = np.roll(w, -((N - win) // 2))
    w = w.astype(f32)
    idx = np.asarray(ts, np.int64)[:, None] * hop + np.arange(N)[None, :] - N // 2
    if fault == 'shift_one':
        idx = idx + 1
    idx = np.abs(idx)
    Lr = L if fault == 'reflect_about_L' else Lpad
    idx = np.where(idx >= Lr, 2 * (Lr - 1) - idx + (1 if fault == 'reflect_off_by_one' else 0), idx)
    ok = (idx >= 0) & (idx < L)
    v = np.where(ok, np.asarray(x, f32)[np.clip(idx, 0, L - 1)], f32(0))
    c = f32(c)
    return ((v * c) * w if order == 'slow' else v * (c * w)).astype(f32)


def eval32_fwd(x, c, L, Lpad, geom, ts, order='slow', fault=None, two=False):
    """X [F][len(ts)] complex64: torch.fft.rfft in float32, or (two) the two-for-one transform of frame pairs untangled in fp32"""
    N = geom[0]
    z = eval32_frames(x, c, L, Lpad, geom, ts, order, fault)
    if not (two or fault in ('pair_swapped', 'imag_sign')):
        return torch.fft.rfft(torch.from_numpy(z), dim=-1).numpy().T
    n = z.shape[0]
    if n & 1:
        z = np.concatenate([z, np.zeros((1, N), f32)])
    Z = torch.fft.fft(torch.complex(torch.from_numpy(z[0::2]), torch.from_numpy(z[1::2])), dim=-1).numpy()
    k = np.arange(N // 2 + 1)
    zk, zc = Z[:, k], Z[:, (N - k) % N]
    h = f32(0.5)
    xa = (h * (zk.real + zc.real)) + 1j * (h * (zk.imag - zc.imag))
    xb = (h * (zk.imag + zc.imag)) + 1j * (-h * (zk.real - zc.real))
    if fault == 'pair_swapped':
        xa, xb = xb, xa
    X = np.empty((z.shape[0], N // 2 + 1), np.complex64)
    X[0::2], X[1::2] = xa, xb
    if fault == 'imag_sign':
        X = X.conj()
    X[~z.any(-1)] = 0                            # (as the kernel: a frame of digital silence is exact zeros whatever its partner holds)
    return X[:n].T


def compress32(X, p):
    re, im = X.real.astype(f32), X.imag.astype(f32)
    m = np.sqrt(re * re + im * im)
    if p == 1.0:
        return X, m
    with np.errstate(divide='ignore', invalid='ignore'):
        mp = np.power(m, f32(p))
        sc = np.where(m > 0, mp / m, f32(0)).astype(f32)
    return (re * sc) + 1j * (im * sc), mp


def eval32_inv(S, geom, t_lo, Tb, o_lo, Lo, scale, fault=None, ring=None):
    """fp32 torch.fft.irfft, synthesis window, overlap-add, envelope division.  ring (fault 'ring_no_wrap'): (flat slots, row, ring size)"""
    N, hop, win = geom
    w = window64(N, win).astype(f32)
    Sc = S.astype(np.complex64)
    x = torch.fft.irfft(torch.from_numpy(Sc.T.copy()), n=N, dim=-1).numpy()
    if fault == 'edge_imag':                     # Z = X_a + i X_b with the imaginary parts of DC / Nyquist left in
        alt = (1 - 2 * (np.arange(N) & 1)).astype(f32)
        i0, iN = Sc[0].imag, Sc[-1].imag
        for i in range(0, x.shape[0] - 1, 2):
            if (t_lo + i) % 2 == 0:
                x[i] -= (i0[i + 1] + alt * iN[i + 1]) / f32(N)
                x[i + 1] += (i0[i] + alt * iN[i]) / f32(N)
    if fault == 'no_inv_n':
        x = x * f32(N)
    sc = np.asarray(scale, f32)
    if fault == 'ring_no_wrap':
        flat, row, rs = ring
        sc = np.asarray([flat[row * rs + t] if row * rs + t < flat.size else 1.0 for t in range(t_lo, Tb)], f32)
    own, halo = inv_geometry(geom)
    n_o = Lo - o_lo
    acc, env = np.zeros(n_o, f32), np.zeros(n_o, f32)
    pos_base = (o_lo + N // 2) // hop * hop
    for i, t in enumerate(range(t_lo, Tb)):
        a = t * hop - N // 2
        lo, hi = max(a, o_lo), min(a + N, Lo)
        if hi <= lo:
            continue
        sl, fr = slice(lo - o_lo, hi - o_lo), slice(lo - a, hi - a)
        term = (x[i, fr] * (w[fr] * sc[i])).astype(f32)
        if fault == 'halo_dropped':              # every output block but the first loses the lowest frame whose window reaches its first sample
            pos = np.arange(lo, hi) + N // 2
            bx = (pos - pos_base) // (own * hop)
            pos0 = pos_base + bx * own * hop
            term = np.where((bx >= 1) & (t == (pos0 - (int(np.flatnonzero(w)[-1]) + 1)) // hop + 1), f32(0), term)
        acc[sl] += term
        env[sl] += w[fr] if fault == 'env_w' else w[fr] * w[fr]
    return np.where(env > f32(1e-11), acc / np.where(env > f32(1e-11), env, f32(1)), acc)


def _pow_scale32(m, p, fault=None):
    if p == 1.0:
        return np.ones_like(m)
    with np.errstate(divide='ignore', invalid='ignore'):
        q = f32(p) if fault == 'p_not_minus_one' else f32(p) - f32(1)
        return np.where(m > 0, m if (p == 2.0 and fault is None) else np.power(m, q), f32(0)).astype(f32)


def eval32_cmask(mask, spec, p, fault=None):
    mr, mi, xr, xi = (a.astype(f32) for a in (mask[:, 0], mask[:, 1], spec[:, 0], spec[:, 1]))
    er, ei = xr * mr - xi * mi, xr * mi + xi * mr
    sc = _pow_scale32(np.sqrt(er * er + ei * ei), p, fault)
    return np.stack([er * sc, ei * sc], 1)


def eval32_polar_pow(x, p):
    er, ei = x[:, 0].astype(f32), x[:, 1].astype(f32)
    sc = _pow_scale32(np.sqrt(er * er + ei * ei), p)
    return np.stack([er * sc, ei * sc], 1)


def eval32_mag_phase(mag, spec, p):
    m, xr, xi = mag.astype(f32), spec[:, 0].astype(f32), spec[:, 1].astype(f32)
    m = m * m if p == 2.0 else (m if p == 1.0 else np.power(m, f32(p)))
    xm = np.sqrt(xr * xr + xi * xi)
    with np.errstate(divide='ignore', invalid='ignore'):
        pr, pi = np.where(xm > 0, xr / xm, f32(1)), np.where(xm > 0, xi / xm, f32(0))
    return np.stack([m * pr, m * pi], 1).astype(f32)


def eval32_dccrn_mask(mask, spec, p, mode, fault=None):
    if mode != 0:
        padm = np.concatenate([np.zeros_like(mask[:, :, :1]), mask], 2)
        if mode == 1:
            return eval32_cmask(padm, spec, p)
        er, ei = (spec[:, 0] * padm[:, 0]).astype(f32), (spec[:, 1] * padm[:, 1]).astype(f32)
        sc = _pow_scale32(np.sqrt(er * er + ei * ei), p)
        return np.stack([er * sc, ei * sc], 1)
    padm = np.concatenate([mask[:, :, :1] if fault == 'dc_not_zeroed' else np.zeros_like(mask[:, :, :1]), mask], 2).astype(f32)
    mr, mi, xr, xi = padm[:, 0], padm[:, 1], spec[:, 0].astype(f32), spec[:, 1].astype(f32)
    mm, xm = np.sqrt(mr * mr + mi * mi), np.sqrt(xr * xr + xi * xi)
    with np.errstate(divide='ignore', invalid='ignore'):
        pr, pi = np.where(mm > 0, mr / mm, f32(1)), np.where(mm > 0, mi / mm, f32(0))
        qr, qi = np.where(xm > 0, xr / xm, f32(1)), np.where(xm > 0, xi / xm, f32(0))
    em = np.tanh(mm) * xm
    em = em * em if p == 2.0 else (em if p == 1.0 else np.power(em, f32(p)))
    return np.stack([em * (pr * qr - pi * qi), em * (pr * qi + pi * qr)], 1).astype(f32)


def ratio(got, ref, bound):
    return float((np.abs(np.asarray(got, np.complex128) - ref) / bound).max())


def cratio(got, Y, bd):
    """complex planes under a per-component bound"""
    return max(ratio(got.real, Y.real, bd), ratio(got.imag, Y.imag, bd))


def measure_constants():
    """the observed figures behind A_FWD / B_FWD / A_INV / B_INV (module docstring): float32 torch.stft / irfft against float64"""
    a_f = b_f = a_i = b_i = 0.0
    for geom in GEOMS:
        N, hop, win = geom
        L = 40 * hop + 13
        T = 1 + L // hop
        w32 = torch.from_numpy(window64(win, win).astype(f32))
        for kind in KINDS:
            x = make_clip(L, kind, 77 + N + hop)
            c = f32(1.7)
            X32 = torch.stft(torch.from_numpy(x * c), N, hop, win, w32, center=True, pad_mode='reflect', return_complex=True).numpy()
            X, zn = ref_stft((x * c).astype(np.float64), 1.0, L, L, geom, np.arange(T))
            d = np.abs(X32 - X)
            if kind == 'tonal':
                pk = np.abs(X) >= 0.25 * math.sqrt(N) * zn[None, :]
                b_f = max(b_f, float((d[pk] / (U * np.abs(X[pk]))).max()))
            else:
                a_f = max(a_f, float((d / (U * math.log2(N) * zn[None, :])).max()))
        for kind in ('white', 'peaky'):
            S = make_spectrum(N // 2 + 1, 40, 5 + N + hop)
            if kind == 'peaky':                      # a click in every frame: one sample carries the frame's energy
                k = np.arange(N // 2 + 1)[:, None]
                S = 1e-4 * S + np.exp(-2j * np.pi * k * (7 + 11 * np.arange(40))[None, :] / N)
                S = S.real.astype(f32).astype(np.float64) + 1j * S.imag.astype(f32).astype(np.float64)
            x32 = torch.fft.irfft(torch.from_numpy(np.where(np.isin(np.arange(N // 2 + 1), (0, N // 2))[:, None], S.real, S).astype(np.complex64).T.copy()),
                                  n=N, dim=-1).numpy()
            x, xn = ref_inverse_frames(S, N)
            d = np.abs(x32 - x)
            if kind == 'peaky':
                pk = np.abs(x) >= 0.25 * xn[:, None]
                b_i = max(b_i, float((d[pk] / (U * np.abs(x[pk]))).max()))
            else:
                a_i = max(a_i, float((d / (U * math.log2(N) * xn[:, None])).max()))
    return a_f, b_f, a_i, b_i


# ------------------------------------------------------------------------------------------------ CPU tests
def test_references_match_golden():
    """the STFT and iSTFT written here against the torch fp64 fixtures"""
    gold = np.load(os.path.join(ROOT, 'tests', 'golden', 'stft.npz'))
    for geom, gid in zip(GEOMS, GID):
        N, hop, win = geom
        x, spec = gold['x_' + gid], gold['spec_' + gid]
        T = spec.shape[-1]
        for b in range(x.shape[0]):
            X, _ = ref_stft(x[b].astype(np.float64), 1.0, x.shape[1], x.shape[1], geom, np.arange(T))
            assert np.abs(X - spec[b]).max() <= 1e-11 * np.abs(spec[b]).max(), gid
            for key, Lo in (('ylen_', gold['ylen_' + gid].shape[1]), ('ynolen_', gold['ynolen_' + gid].shape[1])):
                want = gold[key + gid][b]
                y, _ = ref_istft(spec[b], geom, 0, T, 0, Lo, np.ones(T))
                assert np.abs(y - want).max() <= 1e-11 * max(1.0, np.abs(want).max()), (gid, key)


def _fwd_fault_ratio(geom, name, fault, b=0, two=False, order='slow'):
    xs, L, Lpad, T = fwd_clips(geom, name)
    ts = np.arange(T)
    X, zn = ref_stft(xs[b].astype(np.float64), 1.25, L, Lpad, geom, ts)
    got = eval32_fwd(xs[b], 1.25, L, Lpad, geom, ts, order, fault, two)
    return ratio(got, X, bound_fwd(X, zn, geom[0]))


def inv_case(geom, T, seed, B=3):
    F = geom[0] // 2 + 1
    return [make_spectrum(F, T, seed + b) for b in range(B)]


def test_bound_holds_for_fp32_and_catches_faults():
    obs = measure_constants()
    print('observed a_fwd %.3f b_fwd %.3f a_inv %.3f b_inv %.3f; constants %s' % (obs + ((A_FWD, B_FWD, A_INV, B_INV),)))
    for o, k in zip(obs, (A_FWD, B_FWD, A_INV, B_INV)):
        assert 3.5 * o <= k <= 4.5 * o, 'the constants are 4x the figures observed when they were fixed (CPU FFT builds may differ a little)'
    worst = {}

    def keep(key, r):
        worst[key] = max(worst.get(key, 0.0), r)

    # ---- 1. plain fp32 stays inside every bound
    for geom, gid in zip(GEOMS, GID):
        N, hop, win = geom
        for name in fwd_lengths(geom):
            xs, L, Lpad, T = fwd_clips(geom, name)
            ts = np.arange(T)
            for b, x in enumerate(xs):
                c = f32(1.25)
                X, zn = ref_stft(x.astype(np.float64), c, L, Lpad, geom, ts)
                dX = bound_fwd(X, zn, N)
                if Lpad == L:
                    w32 = torch.from_numpy(window64(win, win).astype(f32))
                    keep('torch.stft', ratio(torch.stft(torch.from_numpy(x * c), N, hop, win, w32, center=True, pad_mode='reflect',
                                                        return_complex=True).numpy(), X, dX))
                for order in ('slow', 'fast'):
                    for two in (False, True):
                        got = eval32_fwd(x, c, L, Lpad, geom, ts, order, None, two)
                        keep('rfft' if not two else 'two-for-one', ratio(got, X, dX))
                        for p in (0.5, 0.3):
                            Y, bd, mg, bm = compress(X, dX, p)
                            g32, m32 = compress32(got, p)
                            keep('compress p%g' % p, max(cratio(g32, Y, bd), ratio(m32, mg, bm)))
        own, _ = inv_geometry(geom)
        T = 2 * own + 5
        for b, S in enumerate(inv_case(geom, T, 300 + N + hop)):
            Lo = hop * (T - 1)
            y, bd = ref_istft(S, geom, 0, T, 0, Lo, np.full(T, 1 / 1.25))
            keep('irfft + overlap-add', ratio(eval32_inv(S, geom, 0, T, 0, Lo, np.full(T, f32(1) / f32(1.25))), y, bd))
    for T in (1, 257):
        mask, spec, mag = make_ew(3, 5, T, 40 + T)
        padm = np.concatenate([np.zeros_like(mask[:, :, :1]), mask], 2)
        for p in (1.0, 2.0, 0.7):
            keep('cmask', ratio(eval32_cmask(padm, spec, p), *ref_cmask(padm, spec, p)))
            keep('polar_pow', ratio(eval32_polar_pow(spec, p), *ref_polar_pow(spec, p)))
            keep('mag_phase', ratio(eval32_mag_phase(mag, spec, p), *ref_mag_phase(mag, spec, p)))
            for mode in (0, 1, 2):
                keep('dccrn_mask mode %d' % mode, ratio(eval32_dccrn_mask(mask, spec, p, mode), *ref_dccrn_mask(mask, spec, p, mode)))
    print('fp32 inside the bounds: %s' % {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) < 1.0, worst

    # ---- 2. every planted fault leaves its bound by >= 10x on a case of the GPU table
    caught = {}
    g128, g400 = GEOMS[1], GEOMS[3]
    caught['reflect_off_by_one'] = min(_fwd_fault_ratio(g, 'T31', 'reflect_off_by_one') for g in GEOMS)
    caught['reflect_about_L'] = _fwd_fault_ratio(g128, 'tail_padded', 'reflect_about_L')
    caught['window_uncentred'] = _fwd_fault_ratio(g400, 'T33', 'window_uncentred')
    caught['pair_swapped'] = min(_fwd_fault_ratio(g, 'T32_exact', 'pair_swapped') for g in GEOMS)
    caught['imag_sign'] = min(_fwd_fault_ratio(g, 'T33', 'imag_sign') for g in GEOMS)
    caught['shift_one'] = min(_fwd_fault_ratio(g, 'T31', 'shift_one', b) for g in GEOMS for b in range(3))
    for fault in ('no_inv_n', 'edge_imag', 'env_w', 'halo_dropped'):
        rs = []
        for geom in GEOMS:
            own, _ = inv_geometry(geom)
            T = 2 * own + 5
            S = inv_case(geom, T, 300 + geom[0] + geom[1])[0]
            Lo = geom[1] * (T - 1)
            y, bd = ref_istft(S, geom, 0, T, 0, Lo, np.ones(T))
            rs.append(ratio(eval32_inv(S, geom, 0, T, 0, Lo, np.ones(T), fault), y, bd))
        caught[fault] = min(rs)
    rs = []
    for geom in GEOMS:
        S, fr, t_lo, T, o_lo, Lo = ring_case(geom, 0)
        sc = np.asarray([fr[0, t & 63] for t in range(t_lo, T)], np.float64)
        y, bd = ref_istft(S, geom, t_lo, T, o_lo, Lo, sc)
        assert ratio(eval32_inv(S, geom, t_lo, T, o_lo, Lo, sc), y, bd) < 1.0
        rs.append(ratio(eval32_inv(S, geom, t_lo, T, o_lo, Lo, sc, 'ring_no_wrap', (np.nan_to_num(fr, nan=1.0).reshape(-1), 0, 64)), y, bd))
    caught['ring_no_wrap'] = min(rs)
    mask, spec, _ = make_ew(3, 5, 257, 40 + 257)
    caught['dc_not_zeroed'] = ratio(eval32_dccrn_mask(mask, spec, 2.0, 0, 'dc_not_zeroed'), *ref_dccrn_mask(mask, spec, 2.0, 0))
    padm = np.concatenate([np.zeros_like(mask[:, :, :1]), mask], 2)
    caught['p_not_minus_one'] = ratio(eval32_cmask(padm, spec, 0.7, 'p_not_minus_one'), *ref_cmask(padm, spec, 0.7))
    low = min(caught, key=caught.get)
    print('faults: smallest error / bound %.1f (%s); all: %s' % (caught[low], low, {k: round(v, 1) for k, v in caught.items()}))
    assert len(caught) == 13 and caught[low] >= 10.0, caught


def ring_case(geom, seed):
    """frames 50 .. 80 under per-frame scales in a ring of 64: spectra of the frames [t_lo, T) of one row, the ring [3][64] (NaN outside the
    frames' slots), t_lo, T, o_lo, Lout"""
    N, hop, _ = geom
    t_lo, T = 50, 81
    g = np.random.default_rng(900 + seed)
    fr = np.full((3, 64), np.nan, f32)
    for t in range(t_lo, T):
        fr[:, t & 63] = (0.5 + g.uniform(0, 1, 3) + 0.37 * (t & 63)).astype(f32)
    return make_spectrum(N // 2 + 1, T - t_lo, 910 + seed + N + hop), fr, t_lo, T, (t_lo + 4) * hop - N // 2, T * hop - N // 2


# ------------------------------------------------------------------------------------------------ GPU side
_lib = None
SIGS = {'fp_rms_scale': 'piilppi', 'fp_stream_rms': 'pliiipppiiii', 'fp_stream_slide': 'ppliii', 'fp_dccrn_mask': 'pppiiiifi',
        'fp_cmask_apply': 'pppiiif', 'fp_mag_phase': 'pppiiif', 'fp_polar_pow': 'ppiiif', 'fp_fill_rows': 'piiiiii', 'fp_window_rows': 'ppiii'}
SIGS['fp_stft'] = 'iiipliiipfppiiiiipi'         # n_fft hop win | wav pitch B L Lpad c p_in spec mag T Tp t_first col0 w0 rows MB
SIGS['fp_istft'] = 'iiipiiippliiiipipi'         # n_fft hop win | spec B T Tp c out pitch Lout t_off t_lo o_lo frame_inv ring rows MB
SIGS['fp_zero_tail'] = 'pilipi'                 # x B nrows T rows MB
CT = {'i': C.c_int, 'p': C.c_void_p, 'l': C.c_long, 'f': C.c_float}
REC = ('N', 'MAG', 'CP', 'FSC', 'gx', 'gy', 'block', 'shmem', 'ragged')
SLACK = 64
gpu = pytest.mark.gpu


def lib():
    global _lib
    if _lib is None:
        assert os.path.exists(PROBE_LIB), 'libse_feprobe.so is missing: run build() (make -C csrc)'
        L = C.CDLL(PROBE_LIB)
        for name, sig in SIGS.items():
            getattr(L, name).argtypes = [CT[c] for c in sig]
            getattr(L, name).restype = C.c_int
        L.fp_last_error.restype = C.c_char_p
        L.fp_launch_kernel.restype = C.c_char_p
        L.fp_launch_kernel.argtypes = [C.c_int]
        L.fp_launch_get.argtypes = [C.c_int, C.POINTER(C.c_longlong), C.c_int]
        _lib = L
    return _lib


class Buf:
    """device buffer of n elements with NaN (floats) or -1 (ints) in it and in the slack around it, unless src fills it"""

    def __init__(self, n, src=None, dtype=torch.float32):
        self.n, self.dtype = n, dtype
        self.fill = -1 if dtype == torch.int32 else float('nan')
        self.t = torch.full((n + 2 * SLACK,), self.fill, dtype=dtype, device='cuda')
        self.v = self.t[SLACK:SLACK + n]
        if src is not None:
            self.v.copy_(torch.as_tensor(np.ascontiguousarray(src)).reshape(-1).to(dtype))

    @property
    def ptr(self):
        return self.t.data_ptr() + self.t.element_size() * SLACK

    def np(self, *shape):
        return self.v.cpu().numpy().reshape(shape)

    def untouched(self):
        s = torch.cat([self.t[:SLACK], self.t[SLACK + self.n:]])
        return bool(torch.isnan(s).all()) if self.dtype != torch.int32 else bool((s == -1).all())


def call(name, *args, nrec=0):
    L = lib()
    rc = getattr(L, name)(*[a.ptr if isinstance(a, Buf) else a for a in args])
    assert rc == 0, '%s: %s' % (name, L.fp_last_error().decode())
    out = []
    for i in range(L.fp_launch_count()):
        v = (C.c_longlong * 9)()
        L.fp_launch_get(i, v, 9)
        d = dict(zip(REC, list(v)))
        d['kernel'] = L.fp_launch_kernel(i).decode()
        out.append(d)
    assert len(out) == nrec, out
    return out[0] if nrec else None


def note(form, r, case):
    REACHED.add(form)
    if r > WORST.get(form, (-1.0, ''))[0]:
        WORST[form] = (r, case)


def verify(case, form, got, ref, bound):
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), '%s: non-finite value in what the launch owns' % case
    r = np.abs(got - ref) / bound
    k = int(r.argmax()) if r.size else 0
    worst = float(r.reshape(-1)[k]) if r.size else 0.0
    print('%s: worst error / bound %.3f at %s (got %.9g, want %.9g, bound %.3g) form %s' %
          (case, worst, tuple(int(i) for i in np.unravel_index(k, r.shape)) if r.size else (), got.reshape(-1)[k] if r.size else 0,
           np.asarray(ref).reshape(-1)[k] if r.size else 0, np.asarray(bound).reshape(-1)[k] if r.size else 0, form))
    note(form, worst, case)
    assert worst <= 1.0, '%s: error %.3f of the bound' % (case, worst)


def rows_buf(len_, lpad, tlen, olen):
    MB = len(len_) + 2
    a = np.full((4, MB), -12345, np.int32)
    for i, v in enumerate((len_, lpad, tlen, olen)):
        a[i, :len(v)] = v
    return Buf(4 * MB, a, torch.int32), MB


# ---- forward -----------------------------------------------------------------------------------------------------------------------------
def stft_lds(N):
    return max(4 * N * 8, (N // 2 + 1) * 33 * 4)


def istft_lds(N):
    return max(NFB * N * 4, (N // 2 + 1) * 33 * 4) + 4 * N


def run_stft(geom, xs, L, Lpad, T, p_in, planes, c=None, Tp=None, pitch=None, t_first=0, col0=0, w0=0, rows=None, shift=0):
    """one launch; xs: the clips from sample 0 (row b holds xs[b][w0:len_b] from column 0, NaN beyond).  Returns spec [B][2][F][Tp], mag
    [B][F][Tp] (None where the plane is not asked for).  shift: the launch is told that the stream is `shift` frames further on - every
    position it is given moves by shift * hop samples or shift frames, the buffers are the same"""
    N, hop, win = geom
    B, F = len(xs), N // 2 + 1
    lens = rows[0] if rows is not None else [L] * B
    Tp = Tp or T - t_first + col0
    pitch = pitch or (max(lens) - w0 + 3)
    wav = np.full((B, pitch), np.nan, f32)
    for b, x in enumerate(xs):
        wav[b, :lens[b] - w0] = x[w0:lens[b]]
    bw = Buf(B * pitch, wav)
    bs = Buf(B * 2 * F * Tp) if 'spec' in planes else None
    bm = Buf(B * F * Tp) if 'mag' in planes else None
    bc = Buf(B, c) if c is not None else None
    rb, MB = rows_buf(*rows) if rows is not None else (None, 0)
    D = shift * hop
    rec = call('fp_stft', N, hop, win, bw, pitch, B, L + D, Lpad + D, bc, p_in, bs, bm, T + shift, Tp, t_first + shift, col0, w0 + D, rb, MB, nrec=1)
    cp = 0 if p_in == 1.0 else (1 if p_in == 0.5 else 2)
    want = dict(kernel='stft2', N=N, MAG=int(bm is not None), CP=cp, FSC=0, gx=(T - t_first + NFB - 1) // NFB, gy=B, block=256,
                shmem=stft_lds(N), ragged=int(rows is not None))
    assert rec == want, (rec, want)
    for bf in (bw, bs, bm, bc, rb):
        assert bf is None or bf.untouched(), 'stft wrote outside its buffers'
    assert np.array_equal(bw.np(B, pitch), wav, equal_nan=True)
    return (bs.np(B, 2, F, Tp) if bs else None), (bm.np(B, F, Tp) if bm else None), 'stft2<%d,%d,%d>' % (N, int(bm is not None), cp)


def check_forward(case, form, geom, xs, lens, lpads, tlens, T, c, p_in, spec, mag, t_first=0, col0=0):
    """every owned element of one forward launch against float64; zero tails; NaN everywhere else"""
    N, hop, _ = geom
    Tp = (spec if spec is not None else mag).shape[-1]
    owned = np.zeros(Tp, bool)
    owned[col0:col0 + T - t_first] = True
    for arr in (spec, mag):
        if arr is not None:
            assert np.isnan(arr[..., ~owned]).all(), '%s: columns outside [col0, col0 + T - t_first) were written' % case
    for b, x in enumerate(xs):
        cb = 1.0 if c is None else float(c[b])
        Tb = min(tlens[b], T)
        ts = np.arange(t_first, Tb)
        cols = col0 + ts - t_first
        X, zn = ref_stft(x.astype(np.float64), cb, lens[b], lpads[b], geom, ts)
        Y, bd, mg, bm = compress(X, bound_fwd(X, zn, N), p_in)
        silent = zn == 0
        tail = np.arange(col0 + max(Tb, t_first) - t_first, col0 + T - t_first)
        if spec is not None:
            verify('%s row %d re' % (case, b), form, spec[b, 0][:, cols], Y.real, bd)
            verify('%s row %d im' % (case, b), form, spec[b, 1][:, cols], Y.imag, bd)
            assert (spec[b][:, :, cols[silent]] == 0).all(), '%s: a frame of digital silence is not exactly zero' % case
            assert (spec[b][:, :, tail] == 0).all(), '%s: frames >= tlen[b] are not exact zeros' % case
        if mag is not None:
            verify('%s row %d mag' % (case, b), form, mag[b][:, cols], mg, bm)
            assert (mag[b][:, cols[silent]] == 0).all() and (mag[b][:, tail] == 0).all(), '%s: silence / tail of mag' % case
    return


PLANES = (('spec', 'mag'), ('spec',), ('mag',))


@gpu
@pytest.mark.parametrize('name', ['shortest', 'T31', 'T32_exact', 'T33', 'straddle_end', 'last_fast_pair', 'tail_padded'])
@pytest.mark.parametrize('geom', GEOMS, ids=GID)
def test_stft_offline(geom, name):
    if name not in fwd_lengths(geom):
        assert name == 'tail_padded' and geom != (512, 128, 512)
        return                                           # (the tail pad is the 512 / 128 script's)
    N, hop, _ = geom
    xs, L, Lpad, T = fwd_clips(geom, name)
    if name == 'straddle_end':
        assert not fast_path(geom, 0, T, L) and fast_path(geom, 18, T, L) and not fast_path(geom, 20, T, L)
        assert 20 * hop + N // 2 <= L < 21 * hop + N // 2
    if name == 'last_fast_pair':
        assert fast_path(geom, 20, T, L) and not fast_path(geom, 22, T, L)
    if T >= 31:                                          # row 1: wholly silent frames, one of them paired with a sounding frame
        zn = ref_stft(xs[1].astype(np.float64), 1.0, L, Lpad, geom, np.arange(T))[1]
        sil = np.flatnonzero(zn == 0)
        assert len(sil) >= 2 and any(zn[t ^ 1] > 0 for t in sil if (t ^ 1) < T)
    c = np.asarray([1.25, 0.0371, 23.0], f32)
    for p_in in (1.0, 0.5, 0.3):
        for planes in PLANES:
            for cs in (None, c):
                spec, mag, form = run_stft(geom, xs, L, Lpad, T, p_in, planes, cs, Tp=T + 5, pitch=Lpad + 7)
                case = 'stft %s %s p%g %s %s' % (GID[GEOMS.index(geom)], name, p_in, '+'.join(planes), 'c' if cs is not None else 'noc')
                check_forward(case, form, geom, xs, [L] * 3, [Lpad] * 3, [T] * 3, T, cs, p_in, spec, mag)


@gpu
@pytest.mark.parametrize('geom', GEOMS, ids=GID)
def test_stft_ragged(geom):
    N, hop, _ = geom
    T, tlen = 70, [70, 33, 32, 5]
    if geom == (512, 128, 512):                          # the script pads the tail to a hop multiple: the frames count the padded clip
        lens = [(t - 1) * hop - r for t, r in zip(tlen, (hop // 2, 1, 0, hop - 1))]
        lpads = [pad_to_hop(n, hop) for n in lens]
    else:
        lens = [(t - 1) * hop + r for t, r in zip(tlen, (hop // 2, 1, 0, hop - 1))]
        lpads = list(lens)
    assert [1 + n // hop for n in lpads] == tlen
    xs = [make_clip(n, KINDS[b % 3], 50 + b + N + hop) for b, n in enumerate(lens)]
    c = np.asarray([1.25, 0.0371, 23.0, 3.0], f32)
    rows = (lens, lpads, tlen, lens)
    for p_in, planes in ((0.5, ('spec', 'mag')), (1.0, ('spec',)), (0.3, ('mag',))):
        spec, mag, form = run_stft(geom, xs, max(lens), max(lpads), T, p_in, planes, c, Tp=T + 3, rows=rows)
        case = 'stft ragged %s p%g' % (GID[GEOMS.index(geom)], p_in)
        check_forward(case, form + ':ragged', geom, xs, lens, lpads, tlen, T, c, p_in, spec, mag)
        for b in range(4):
            s1, m1, _ = run_stft(geom, xs[b:b + 1], lens[b], lpads[b], tlen[b], p_in, planes, c[b:b + 1])
            for one, many in ((s1, spec), (m1, mag)):
                if one is not None:
                    assert np.array_equal(one[0], many[b][..., :tlen[b]]), '%s: row %d differs from the clip launched alone' % (case, b)


@gpu
@pytest.mark.parametrize('T,t_first', [(60, 37), (60, 40), (41, 40)])
@pytest.mark.parametrize('geom', GEOMS, ids=GID)
def test_stft_windowed(geom, T, t_first):
    """frames [t_first, T) of a stream against the float64 STFT of the whole signal: mid-stream (every frame inside what has arrived) and at the
    end of the stream (end reflection, tail pad), at every legal kind of sample origin"""
    N, hop, _ = geom
    for end in (False, True):
        padded = end and geom == (512, 128, 512)
        L = (T - 1) * hop + (-5 if padded else 5 if end else N // 2 + 11)
        Lpad = pad_to_hop(L, hop) if padded else L
        # the lowest legal origin (stream_window.h): the first sample of frame t_first and, at the end of the stream, the mirror image of the
        # last frame's last sample, Lpad - n_fft / 2 - 1 - one sample lower when the last frame is centred on Lpad
        w_low = min(t_first * hop - N // 2, Lpad - N // 2 - 1 if end else L) // 4 * 4
        assert (1 + Lpad // hop == T) if end else (1 + L // hop >= T)
        xs = [make_clip(L, KINDS[b % 3], 70 + b + T + N + hop) for b in range(3)]
        c = np.asarray([1.25, 0.0371, 23.0], f32)
        for w0, col0, p_in, planes in ((0, 3, 0.5, ('spec', 'mag')), (w_low, 4, 1.0, ('spec',)), (w_low - 4 * 25, 0, 0.3, ('spec', 'mag')),
                                       (w_low, 2, 0.5, ('mag',))):
            Tp = col0 + T - t_first + 2
            spec, mag, form = run_stft(geom, xs, L, Lpad, T, p_in, planes, c, Tp=Tp, t_first=t_first, col0=col0, w0=w0)
            case = 'stft window %s T%d t_first%d w0=%d col0=%d %s' % (GID[GEOMS.index(geom)], T, t_first, w0, col0, 'end' if end else 'mid')
            check_forward(case, form, geom, xs, [L] * 3, [Lpad] * 3, [T] * 3, T, c, p_in, spec, mag, t_first, col0)


def late_shift(geom, top):
    """the largest number of frames a launch whose highest sample position is `top` can be moved by and stay at or below the sample limit of
    the smallest sliding engine (csrc/stream_window.h), in whole multiples of 4 samples"""
    N, hop, _ = geom
    limit = 2 ** 31 - 1 - (N + 32 * hop)
    f = (limit - top) // hop
    while (f * hop) % 4:
        f -= 1
    return f


@gpu
@pytest.mark.parametrize('T,t_first', [(60, 37), (41, 40)])
@pytest.mark.parametrize('geom', GEOMS, ids=GID)
def test_stft_windowed_near_the_stream_limit(geom, T, t_first):
    """the stream-window launches of test_stft_windowed (checked there against float64) once more with every position moved to the far end
    of the counter range - the stream ends exactly at the sample limit, the window origin and the first frame lie just below it: the
    same input, and the same spectrum BIT FOR BIT, mid-stream and with the end reflection / tail pad"""
    N, hop, _ = geom
    for end in (False, True):
        padded = end and geom == (512, 128, 512)
        L = (T - 1) * hop + (-5 if padded else 5 if end else N // 2 + 11)
        Lpad = pad_to_hop(L, hop) if padded else L
        w_low = min(t_first * hop - N // 2, Lpad - N // 2 - 1 if end else L) // 4 * 4
        xs = [make_clip(L, KINDS[b % 3], 70 + b + T + N + hop) for b in range(3)]
        c = np.asarray([1.25, 0.0371, 23.0], f32)
        f = late_shift(geom, L)
        assert 0 <= 2 ** 31 - 1 - (N + 32 * hop) - (L + f * hop) < 4 * hop and (t_first + f) * hop > 2 ** 31 - 40 * hop - 64 * hop
        for w0, col0, p_in, planes in ((w_low, 4, 0.5, ('spec', 'mag')), (w_low - 4 * 25, 0, 1.0, ('spec',))):
            Tp = col0 + T - t_first + 2
            early = run_stft(geom, xs, L, Lpad, T, p_in, planes, c, Tp=Tp, t_first=t_first, col0=col0, w0=w0)
            late = run_stft(geom, xs, L, Lpad, T, p_in, planes, c, Tp=Tp, t_first=t_first, col0=col0, w0=w0, shift=f)
            for a, b in zip(early[:2], late[:2]):
                assert (a is None and b is None) or np.array_equal(a, b, equal_nan=True), \
                    ('stft window %s T%d t_first%d w0=%d %s: the launch %d frames later differs' % (GID[GEOMS.index(geom)], T, t_first, w0,
                                                                                                  'end' if end else 'mid', f))


# ---- inverse -----------------------------------------------------------------------------------------------------------------------------
def run_istft(geom, specs, T, Lout, c=None, t_off=0, t_lo=0, o_lo=0, frame_inv=None, rows=None, Tp=None, out_pitch=None, shift=0):
    """one launch; specs[b]: complex [F][n_b] holding the frames t_lo .. t_lo + n_b - 1 of row b; every other column of the buffer is NaN.
    Returns wav [B][out_pitch].  shift: the launch is told that the stream is `shift` frames further on (as run_stft)"""
    N, hop, win = geom
    B, F = len(specs), N // 2 + 1
    Tp = Tp or T - t_off + 3
    out_pitch = out_pitch or Lout - o_lo + 5
    sp = np.full((B, 2, F, Tp), np.nan, f32)
    for b, S in enumerate(specs):
        sp[b, 0, :, t_lo - t_off:t_lo - t_off + S.shape[1]] = S.real
        sp[b, 1, :, t_lo - t_off:t_lo - t_off + S.shape[1]] = S.imag
    bs, bo = Buf(sp.size, sp), Buf(B * out_pitch)
    bc = Buf(B, c) if c is not None else None
    bf = Buf(frame_inv.size, frame_inv) if frame_inv is not None else None
    rb, MB = rows_buf(*rows) if rows is not None else (None, 0)
    D = shift * hop
    rec = call('fp_istft', N, hop, win, bs, B, T + shift, Tp, bc, bo, out_pitch, Lout + D, t_off + shift, t_lo + shift, o_lo + D, bf, 64 if bf else 0,
               rb, MB, nrec=1)
    own, halo = inv_geometry(geom)
    pos_base = (o_lo + N // 2) // hop * hop
    gx = (N // 2 + Lout - pos_base + own * hop - 1) // (own * hop)
    want = dict(kernel='istft2', N=N, MAG=0, CP=0, FSC=int(bf is not None), gx=gx, gy=B, block=512, shmem=istft_lds(N), ragged=int(rows is not None))
    assert rec == want, (rec, want)
    for x in (bs, bo, bc, bf, rb):
        assert x is None or x.untouched(), 'istft wrote outside its buffers'
    return bo.np(B, out_pitch), 'istft2<%d,%d>' % (N, int(bf is not None)), gx * B


def check_inverse(case, form, geom, specs, wav, t_lo, Tbs, o_lo, Los, Lout, scales):
    assert np.isnan(wav[:, Lout - o_lo:]).all(), '%s: samples >= Lout were written' % case
    for b, S in enumerate(specs):
        y, bd = ref_istft(S, geom, t_lo, Tbs[b], o_lo, Los[b], scales[b])
        verify('%s row %d' % (case, b), form, wav[b, :Los[b] - o_lo], y, bd)
        assert (wav[b, Los[b] - o_lo:Lout - o_lo] == 0).all(), '%s: samples in [olen[b], Lout) are not zero' % case


@gpu
@pytest.mark.parametrize('geom', GEOMS, ids=GID)
def test_istft_offline(geom):
    N, hop, _ = geom
    own, halo = inv_geometry(geom)
    assert own in (28, 30)
    c = np.asarray([1.25, 0.0371, 23.0], f32)
    grids = set()
    for T in (own, own + 1, 2 * own + 1, 2 * own + 5):
        specs = inv_case(geom, T, 300 + N + hop)
        for Lout in (hop * (T - 1), hop * (T - 1) - 37):
            for cs in (c, None):
                wav, form, nblk = run_istft(geom, specs, T, Lout, cs)
                grids.add(nblk)
                sc = [np.full(T, 1.0 if cs is None else 1.0 / float(cs[b])) for b in range(3)]
                check_inverse('istft %s T%d Lout%d %s' % (GID[GEOMS.index(geom)], T, Lout, 'c' if cs is not None else 'noc'), form, geom, specs, wav,
                              0, [T] * 3, 0, [Lout] * 3, Lout, sc)
    assert min(grids) < 8 and 9 in grids, grids          # below eight blocks: no remap; 3 x 3: eight remapped, one left in place


@gpu
@pytest.mark.parametrize('geom', GEOMS, ids=GID)
def test_istft_ragged(geom):
    N, hop, _ = geom
    own, _ = inv_geometry(geom)
    T = 2 * own + 5
    tlen = [T, own + 1, own, 5]
    olen = [hop * (t - 1) - r for t, r in zip(tlen, (0, 37, 1, hop // 2))]
    specs = [make_spectrum(N // 2 + 1, t, 400 + b + N + hop) for b, t in enumerate(tlen)]
    c = np.asarray([1.25, 0.0371, 23.0, 3.0], f32)
    Lout = max(olen)
    wav, form, _ = run_istft(geom, specs, T, Lout, c, rows=(olen, olen, tlen, olen))
    case = 'istft ragged %s' % GID[GEOMS.index(geom)]
    check_inverse(case, form + ':ragged', geom, specs, wav, 0, tlen, 0, olen, Lout, [np.full(t, 1.0 / float(c[b])) for b, t in enumerate(tlen)])
    for b in range(4):
        one, _, _ = run_istft(geom, specs[b:b + 1], tlen[b], olen[b], c[b:b + 1])
        assert np.array_equal(one[0, :olen[b]], wav[b, :olen[b]]), '%s: row %d differs from the clip launched alone' % (case, b)


@gpu
@pytest.mark.parametrize('geom', GEOMS, ids=GID)
def test_istft_windowed(geom):
    """the engine's chunk launches: frame t in column t - t_off, frames [t_lo, T) exist, samples [o_lo, Lout) land at wav_out[o - o_lo]"""
    N, hop, _ = geom
    c = np.asarray([1.25, 0.0371, 23.0], f32)
    gid = GID[GEOMS.index(geom)]
    # first chunk: four history columns that hold no frame (t_off = t0 - HC < 0)
    T = 40
    specs = inv_case(geom, T, 500 + N + hop)
    Lout = T * hop - N // 2
    wav, form, _ = run_istft(geom, specs, T, Lout, c, t_off=-4, t_lo=0, o_lo=0)
    check_inverse('istft window %s first chunk' % gid, form, geom, specs, wav, 0, [T] * 3, 0, [Lout] * 3, Lout, [np.full(T, 1.0 / float(c[b])) for b in range(3)])
    # a later chunk: t_off > 0, two columns below t_lo that hold NaN, every frame covering o_lo is >= t_lo
    T, t_off, t_lo = 70, 34, 36
    o_lo, Lout = 40 * hop - N // 2, T * hop - N // 2 - 3
    assert (o_lo + N // 2 - N) // hop + 1 >= t_lo
    specs = inv_case(geom, T - t_lo, 600 + N + hop)
    wav, form, _ = run_istft(geom, specs, T, Lout, c, t_off=t_off, t_lo=t_lo, o_lo=o_lo)
    check_inverse('istft window %s later chunk' % gid, form, geom, specs, wav, t_lo, [T] * 3, o_lo, [Lout] * 3, Lout,
                  [np.full(T - t_lo, 1.0 / float(c[b])) for b in range(3)])


@gpu
@pytest.mark.parametrize('geom', GEOMS, ids=GID)
def test_istft_windowed_near_the_stream_limit(geom):
    """the later-chunk launch of test_istft_windowed (checked there against float64) with its frames and samples moved to the far end of the
    counter range, the last sample written being the last a stream can emit: the same spectra, the same samples bit for bit.  (The first
    chunk of a stream, t_off < 0, cannot be late.)"""
    N, hop, _ = geom
    c = np.asarray([1.25, 0.0371, 23.0], f32)
    T, t_off, t_lo = 70, 34, 36
    o_lo, Lout = 40 * hop - N // 2, T * hop - N // 2 - 3
    specs = inv_case(geom, T - t_lo, 600 + N + hop)
    f = late_shift(geom, Lout)
    assert 0 <= 2 ** 31 - 1 - (N + 32 * hop) - (Lout + f * hop) < 4 * hop
    early, _, _ = run_istft(geom, specs, T, Lout, c, t_off=t_off, t_lo=t_lo, o_lo=o_lo)
    late, _, _ = run_istft(geom, specs, T, Lout, c, t_off=t_off, t_lo=t_lo, o_lo=o_lo, shift=f)
    assert np.isfinite(early[:, :Lout - o_lo]).all()
    assert np.array_equal(early, late, equal_nan=True), 'istft window %s later chunk: the launch %d frames later differs' % (GID[GEOMS.index(geom)], f)


@gpu
@pytest.mark.parametrize('geom', GEOMS, ids=GID)
def test_istft_frame_scales(geom):
    """c_scale null, a distinct scale per ring slot, frames 50 .. 80 across the wrap of a ring of 64"""
    specs, fr = [], None
    for b in range(3):
        S, fr, t_lo, T, o_lo, Lout = ring_case(geom, b)
        specs.append(S)
    assert t_lo < 64 < T and len({float(v) for v in fr[0][~np.isnan(fr[0])]}) == T - t_lo
    wav, form, _ = run_istft(geom, specs, T, Lout, None, t_off=t_lo - 2, t_lo=t_lo, o_lo=o_lo, frame_inv=fr)
    sc = [np.asarray([fr[b, t & 63] for t in range(t_lo, T)], np.float64) for b in range(3)]
    check_inverse('istft ring %s' % GID[GEOMS.index(geom)], form, geom, specs, wav, t_lo, [T] * 3, o_lo, [Lout] * 3, Lout, sc)


# ---- scales and helpers ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('L', [1, 15, 16, 17, 4097])
def test_rms_scale(L):
    B, pitch = 3, L + 9
    g = np.random.default_rng(L)
    wav = np.full((B, pitch), np.nan, f32)
    wav[:, :L] = g.standard_normal((B, L)).astype(f32)
    wav[1, :L] = 0.0                                     # digital silence: sqrt(L / 0) = +inf in float64 and in the kernel
    bw, bc = Buf(wav.size, wav), Buf(B)
    call('fp_rms_scale', bw, B, L, pitch, bc, None, 0)
    got = bc.np(B)
    with np.errstate(divide='ignore'):
        ref = np.sqrt(L / (wav[:, :L].astype(np.float64) ** 2).sum(-1))
    assert bc.untouched() and got[1] == np.inf and ref[1] == np.inf
    verify('rms_scale L%d' % L, 'rms_scale', got[[0, 2]], ref[[0, 2]], 2 * U * ref[[0, 2]])
    lens = [L, max(1, L // 2), max(1, L - 1)]            # ragged: samples >= len[b] hold NaN
    for b, n in enumerate(lens):
        wav[b, :n] = g.standard_normal(n).astype(f32)
        wav[b, n:] = np.nan
    bw, bc = Buf(wav.size, wav), Buf(B)
    rb, MB = rows_buf(lens, lens, [1] * 3, lens)
    call('fp_rms_scale', bw, B, L, pitch, bc, rb, MB)
    ref = np.asarray([math.sqrt(n / (wav[b, :n].astype(np.float64) ** 2).sum()) for b, n in enumerate(lens)])
    assert bc.untouched()
    verify('rms_scale ragged L%d' % L, 'rms_scale:ragged', bc.np(B), ref, 2 * U * ref)


@gpu
@pytest.mark.parametrize('silent_start', [False, True])
def test_stream_rms(silent_start):
    """pushes of 1, 255, 256, 257 samples and the flush on one state, the sample origin moving between pushes"""
    B, ring, hop = 3, 64, 16
    g = np.random.default_rng(11)
    total = 1 + 255 + 256 + 257
    x = (g.standard_normal((B, total)) * np.asarray([[1.0], [1e-3], [30.0]])).astype(f32)
    if silent_start:
        x[:, :256] = 0.0                                 # (the first two pushes hear silence only: c = 1)
    bsum, bc, bfr = Buf(B, np.zeros(B), torch.float64), Buf(B), Buf(B * ring)
    n_total, t_done, ring_ref = 0, 60, np.full((B, ring), np.nan)
    for i, (n_new, w0) in enumerate(((1, 0), (255, 0), (256, 128), (257, 500), (0, 512))):
        n_total += n_new
        pitch = n_total - w0 + 5
        wav = np.full((B, pitch), np.nan, f32)
        wav[:, n_total - n_new - w0:n_total - w0] = x[:, n_total - n_new:n_total]        # only the new samples may be read
        t0, t1 = t_done, t_done + (3 if n_new else 2)
        t_done = t1
        bw = Buf(wav.size, wav)
        call('fp_stream_rms', bw, pitch, B, n_total, n_new, bsum, bc, bfr, ring, t0, t1, w0)
        ss = (x[:, :n_total].astype(np.float64) ** 2).sum(-1)
        ref = np.where(ss > 1e-20, np.sqrt(n_total / np.where(ss > 0, ss, 1.0)), 1.0)
        case = 'stream_rms push %d silent_start=%s' % (i, silent_start)
        verify(case + ' sumsq', 'stream_rms', bsum.np(B), ss, 4 * 2.0 ** -53 * math.sqrt(total) * ss + 1e-300)
        verify(case + ' c', 'stream_rms', bc.np(B), ref, 2 * U * ref)
        if silent_start and n_total <= 256:
            assert (bc.np(B) == 1.0).all()
        for t in range(t0, t1):
            ring_ref[:, t & (ring - 1)] = 1.0 / ref
        got = bfr.np(B, ring)
        live = ~np.isnan(ring_ref)
        assert np.isnan(got[~live]).all() and bfr.untouched() and bc.untouched() and bsum.untouched(), case + ': wrote outside [t0, t1)'
        cur = np.zeros_like(live)
        cur[:, [t & (ring - 1) for t in range(t0, t1)]] = True
        verify(case + ' ring', 'stream_rms', got[cur], ring_ref[cur], 3 * U * ring_ref[cur])
        ring_ref[live] = got[live]                       # slots of earlier pushes must stay bit for bit
        assert np.array_equal(got[live & ~cur], ring_ref[live & ~cur])
    assert t_done > 64                                    # the ring wrapped


@gpu
@pytest.mark.parametrize('n4', [255, 256, 257, 0])
def test_stream_slide(n4):
    B, n, shift = 3, 4 * n4, 132
    pitch = shift + 4 * 257 + 8
    src = np.random.default_rng(n4).standard_normal((B, pitch)).astype(f32)
    bs, bd = Buf(src.size, src), Buf(B * pitch)
    call('fp_stream_slide', bs, bd, pitch, B, shift, n)
    got = bd.np(B, pitch)
    assert np.array_equal(got[:, :n], src[:, shift:shift + n]) and np.isnan(got[:, n:]).all() and bd.untouched() and bs.untouched()
    assert np.array_equal(bs.np(B, pitch), src)
    note('stream_slide', 0.0, 'n4 %d' % n4)


@gpu
def test_row_helpers():
    """fill_rows, window_rows against window_rows.h, zero_tail against the ragged rule and as a no-op without a ragged context"""
    MB, B = 7, 5
    d = Buf(4 * MB, dtype=torch.int32)
    call('fp_fill_rows', d, MB, B, 4000, 4096, 33, 3990)
    want = np.full((4, MB), -1, np.int32)
    want[:, :B] = np.asarray([4000, 4096, 33, 3990])[:, None]
    assert np.array_equal(d.np(4, MB), want) and d.untouched()
    src = np.full((4, MB), -7, np.int32)
    src[:, :B] = np.random.default_rng(3).integers(1, 9000, (4, B))
    src[2, :B] = [70, 33, 32, 5, 50]
    for t_hi in (1, 32, 33, 50, 200):
        bs, bd = Buf(4 * MB, src, torch.int32), Buf(4 * MB, dtype=torch.int32)
        call('fp_window_rows', bs, bd, MB, B, t_hi)
        want = np.full((4, MB), -1, np.int32)
        want[:, :B] = src[:, :B]
        want[2, :B] = np.minimum(src[2, :B], t_hi)
        assert np.array_equal(bd.np(4, MB), want) and bd.untouched() and np.array_equal(bs.np(4, MB), src)
    nrows, T, tlen = 9, 70, [70, 33, 32, 5]
    x = np.random.default_rng(4).standard_normal((4, nrows, T)).astype(f32)
    bx = Buf(x.size, x)
    call('fp_zero_tail', bx, 4, nrows, T, None, 0)
    assert np.array_equal(bx.np(4, nrows, T), x), 'zero_tail without a ragged context must touch nothing'
    rb, MB = rows_buf(tlen, tlen, tlen, tlen)
    call('fp_zero_tail', bx, 4, nrows, T, rb, MB)
    want = x.copy()
    for b, n in enumerate(tlen):
        want[b, :, n:] = 0.0
    assert np.array_equal(bx.np(4, nrows, T), want) and bx.untouched()
    note('row_helpers', 0.0, '')


# ---- masks -------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('p_out', [1.0, 2.0, 0.7])
@pytest.mark.parametrize('T', [1, 255, 256, 257])
def test_masks(T, p_out):
    B, F = 3, 5
    mask, spec, mag = make_ew(B, F, T, 40 + T)
    # dccrn_mask: Tp > T, all three modes
    Tp = T + 3
    mp, sp = np.full((B, 2, F - 1, Tp), np.nan, f32), np.full((B, 2, F, Tp), np.nan, f32)
    mp[..., :T], sp[..., :T] = mask, spec
    for mode in (0, 1, 2):
        bm, bs, be = Buf(mp.size, mp), Buf(sp.size, sp), Buf(sp.size)
        call('fp_dccrn_mask', bm, bs, be, B, F, T, Tp, p_out, mode)
        got = be.np(B, 2, F, Tp)
        assert be.untouched() and np.isnan(got[..., T:]).all()
        ref, bd = ref_dccrn_mask(mask, spec, p_out, mode)
        verify('dccrn_mask mode %d T%d p%g' % (mode, T, p_out), 'dccrn_mask:%d' % mode, got[..., :T], ref, bd)
        assert (got[:, :, 0, :T] == 0).all(), 'the DC row of est is zero'
        assert (got[:, :, 2, 0] == 0).all() and (got[:, :, 2, T - 1] == 0).all(), 'a zero mask / a zero spectrum gives an exact zero'
    full = np.concatenate([mask[:, :, :1], mask], 2)                  # a full-height mask for the complex ratio mask
    full[:, :, 0, 0] = 0.0
    bm, bs, bo = Buf(full.size, full), Buf(spec.size, spec), Buf(spec.size)
    call('fp_cmask_apply', bm, bs, bo, B, F, T, p_out)
    assert bo.untouched()
    verify('cmask_apply T%d p%g' % (T, p_out), 'cmask_apply', bo.np(B, 2, F, T), *ref_cmask(full, spec, p_out))
    assert (bo.np(B, 2, F, T)[:, :, 0, 0] == 0).all() and (bo.np(B, 2, F, T)[:, :, 2, T - 1] == 0).all()
    bg, bo = Buf(mag.size, mag), Buf(spec.size)
    call('fp_mag_phase', bg, bs, bo, B, F, T, p_out)
    got = bo.np(B, 2, F, T)
    assert bo.untouched()
    verify('mag_phase T%d p%g' % (T, p_out), 'mag_phase', got, *ref_mag_phase(mag, spec, p_out))
    m32 = mag[:, 2, T - 1].astype(f32)                                 # angle(0) = 0: the magnitude lands in the real part alone
    assert (got[:, 1, 2, T - 1] == 0).all() and np.allclose(got[:, 0, 2, T - 1], m32.astype(np.float64) ** p_out, rtol=1e-5)
    assert (got[:, :, 1, 0] == 0).all()                                # |0| ** p = 0
    bo = Buf(spec.size)
    call('fp_polar_pow', bs, bo, B, F, T, p_out)
    ref, bd = ref_polar_pow(spec, p_out)
    verify('polar_pow T%d p%g' % (T, p_out), 'polar_pow', bo.np(B, 2, F, T), ref, bd)
    out_of_place = bo.np(B, 2, F, T).copy()
    call('fp_polar_pow', bs, bs, B, F, T, p_out)                       # in place, as its callers run it
    assert bs.untouched() and np.array_equal(bs.np(B, 2, F, T), out_of_place), 'polar_pow in place differs'
    assert (out_of_place[:, :, 2, T - 1] == 0).all()


# ---- the table of forms ------------------------------------------------------------------------------------------------------------------
def target_forms():
    fwd = ['stft2<%d,%d,%d>' % (N, m, cp) for N in (320, 512) for m in (0, 1) for cp in (0, 1, 2)]
    inv = ['istft2<%d,%d>' % (N, f) for N in (320, 512) for f in (0, 1)]
    return fwd, inv


@gpu
def test_every_form_reached():
    """every template instance of the two transforms was run by the cases above on this device (runs last: pytest keeps file order)"""
    fwd, inv = target_forms()
    assert len(fwd) == 12 and len(inv) == 4
    print('forms reached: %d; worst error / bound per form:' % len(REACHED))
    for f in sorted(WORST):
        print('  %-28s %.3f  %s' % (f, WORST[f][0], WORST[f][1]))
    missing = [f for f in fwd + inv + ['stft2<512,1,1>:ragged', 'istft2<512,0>:ragged'] if f not in REACHED]
    assert not missing, 'forms not reached: %s' % missing
