"""The kernels that lived inside one model file, and the layout movers no other suite launches, one launch at a time against float64:
FullSubNet's nine kernels (csrc/k_fullsubnet.hip: fsn_mean, fsn_scale, fsn_build_sb, fsn_colsum, fsn_finish_mean, fsn_mask, fsn_cum_fb,
fsn_cum_sb, fsn_stream_apply), taylor_zero / taylor_update / gaf_combine, transpose_akt, elu and fill (k_misc.hip) through
csrc/tests/model_probe.hip -> libse_modelprobe.so, and pcm16_encode / pcm16_decode / the offline resample_kernel on short signals
(k_resample.hip) through the C ABI (se_pcm16_*, se_resample).  Every GPU case is one launcher call on torch buffers with slack on both
sides, pre-filled with NaN (PCM: an int16 sentinel); it checks

  1. every element the launch owns against a float64 reference written here from the operation's definition - the reference lines the
     kernels' comments cite: FullSubNet/fullsubnet_net_sa/base_model.py:29-42 (unfold, reflect pad), :197-209 (offline_laplace_norm),
     :212-240 (cumulative_laplace_norm), model.py:79-117, fullsubnet_sa_decode_vb.py:56-66 (complex mask, decompress);
     TaylorSENet/TaylorSENet.py:73-76, :85-93; G2Net_VB/gaf_net_320.py:104-115; GCRN/GCRN_noncprs.py:149-158 (ELU); libsndfile's
     pcm.c as restated in wavio.pcm16_bytes; oracle/resample.py - under an elementwise bound, printing the worst error / bound;
  2. ownership: what the launch does not own still holds NaN (the sentinel) - the slack around every buffer, the unwritten part of
     wider rows, the columns outside [col0, col0 + ns) and those of skipped steps, row pitch slack;
  3. dead data: input the launch must not read holds NaN (look-ahead columns of a mask row, sub-band rows at frames >= tlen[b] + LA of
     a ragged column, a first chunk's csum, spectrum columns outside the chunk's steps).

Error bounds, per element (U = 2^-24; ACT_ULP = 8U per libm / hardware call, 2 ACT_ULP for powf; TINY = 2^-126, below which fp32 results
may be flushed; A_ELU = 4U + 2e-10, the absolute figure tests/test_gpu_conv_epilogues.py derives for fm_expm1).

  exact      transpose_akt, fsn_build_sb, fill, the hook mode of fsn_mask, pcm16_decode (x / 32768 is exact in fp32), pcm16_encode
             (rint of the fp64 product, clipped): bit equality.
  fp64 sums  fsn_mean and fsn_finish_mean sum fp32 values in fp64 (at most 257 T resp. 1024 terms: 2^-53 each, nothing next to U), divide
             in fp64 and round once to fp32: 2U |ref|.
  fp32 sums  of non-negative data: a value that went through c additions carries at most c U relative, so a sum is within
             (c + 2) U of the float64 sum, c = the additions on the longest chain.
               fsn_cum_fb   one frame: v0 + v1, six shuffle steps, (p0 + p1) + (p2 + p3) = 9 levels for 257 values, then run += : frame
                            t_first + t has c = 9 + t_first + t + 1.
               fsn_cum_sb   32 sequential additions of a frame, then run += : c = 32 + t_first + t + 1.
               fsn_colsum   a thread adds one row in every 1024 per (per = 256 / B rows per block), ceil(rows / (1024 per)) of them, then
                            thread r0 = 0 adds the per partials of its column: c = ceil(rows / (1024 per)) + per (rows: of the column's own
                            tlen[b] + LA frames in a ragged batch).
             Through the division: d = run / (F frames) + EPS is a sum of positive terms, so it carries the sum's relative error plus the
             division's and the addition's U; y = v / d one more: (c + 2 + 3) U |y|.  The running sum handed back in csum: (c + 2) U.
             colsum -> finish_mean -> scale as the model chains them: mu carries (c + 2 + 2) U, y = x / (mu + 1e-5f) two more roundings.
  fsn_scale  alone, on a given mu: the addition and the division, 2U |y|.
  products   a complex product component a b - c d (fused or not): 2U (|a b| + |c d|); then tests/test_gpu_frontend_kernels.py's polar
             propagation: sqrtf U, powf 2 ACT_ULP, every product U.  g s: U.  g p + r and h + k p (fused or not): U |g p| + U |result|.
  elu        A_ELU + U |y|.
  resample   |y - oracle| < 2e-7, the tolerance tests/test_resample.py holds this comparison to; the fix_length tail is exactly 0.

Ragged rows.  fsn_mean reads a row as [257][T] and strides it by 256, fsn_colsum cuts rows by per = 256 / B: the same clip launched alone as
a batch of one with T = tlen[b] is summed in ANOTHER order (another T, another per), so it is held to the bound, not to bit equality - except
a ragged batch of one (B = 1, tlen[0] < T), where per, the grid and every thread's rows are the same and fsn_colsum's partials must agree
bit for bit.  Chunked fsn_cum_* runs continue the very additions of the one-shot run (run starts from csum, the divisor counts from
t_first): outputs and the final csum are bit-identical.

PCM.  The product x * 32767 is formed in fp64 from an fp32 x, so it is exact, and because 32767 is odd the only exact ties inside the int16
range are x = +-0.5 (16383.5, -16383.5), where ties-to-even and half-away agree.  A half-away kernel is therefore visible only in the form
that mistake takes in practice - lroundf(x * 32767.f), whose fp32 product rounds the table's near-ties (k + 0.5) / 32767 onto exact ties:
that is the planted fault.

test_bound_holds_for_fp32_and_catches_faults (CPU) shows that plain fp32 evaluations in the kernels' order stay inside every bound and that
each planted fault exceeds its bound by >= 10x (an exact operation: differs at all) on a case of the GPU table.

No GPU run of this suite is recorded in this docstring; profiles/model_kernel_forms.md holds the measured figures."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'sixty-years-of-frequency-domain-monaural-speech-enhancement_amd')
PROBE_LIB = os.environ.get('SE_MODELPROBE_LIB') or os.path.join(PKG, 'libse_modelprobe.so')

U = 2.0 ** -24
ACT_ULP = 8 * U
TINY = 2.0 ** -126
A_ELU = 4 * U + 2e-10
f32 = np.float32
NBIN, LA, SBN, SBW, SUM_BLOCKS, HC = 257, 2, 15, 32, 1024, 4
EPS32 = float(np.finfo(np.float32).eps)          # FSN_EPS
MU_EPS = float(f32(1e-5))                        # fsn_scale's 1e-5f
INF = float('inf')

KERNELS = ['transpose_akt', 'elu', 'fill', 'taylor_zero', 'taylor_update', 'gaf_combine', 'fsn_mean', 'fsn_scale', 'fsn_build_sb',
           'fsn_colsum', 'fsn_finish_mean', 'fsn_mask', 'fsn_cum_fb', 'fsn_cum_sb', 'fsn_stream_apply', 'pcm16_encode', 'pcm16_decode',
           'resample']
WORST = {}


def d64(a):
    return np.asarray(a, np.float64)


def ratio(got, ref, bound):
    got, ref = d64(got), d64(ref)
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return INF
    return float((np.abs(got - ref) / bound).max())


def exact_ratio(got, want):
    """an exact operation: 0 when every element (NaN = unwritten included) agrees, inf otherwise"""
    return 0.0 if np.array_equal(np.asarray(got), np.asarray(want), equal_nan=True) else INF


# ------------------------------------------------------------------------------------------------ transpose_akt
TR_A, TR_K, TR_T = (1, 31, 32, 33, 257), (1, 2, 5), (1, 7, 32, 65)
TR_PATTERNS = ('dense', 'k1_sk0', 'in_window', 'out_kta', 'out_window')


def tr_case(pattern, A, K, T):
    """the call-site stride patterns (csrc/model_*.hip): element (a, k, t) at in_base + a in_sa + k in_sk + t -> out_base + t out_st +
    k out_sk + a"""
    c = dict(A=A, K=K, T=T, in_base=0, in_sa=K * T, in_sk=T, out_base=0, out_st=K * A, out_sk=A, in_n=A * K * T, out_n=A * K * T)
    if pattern == 'k1_sk0':                 # model_crn.hip: (in, X, B, 1, T * NBIN, T * NBIN, 0, B, 0)
        assert K == 1
        c.update(in_sk=0, out_sk=0)
    elif pattern == 'in_window':            # (b.mag + HC, b.magT, B, NBIN, n, NBIN * Tw, Tw, NBIN * B, B): columns [HC, HC + T) of rows of Tw
        Tw = HC + T + 3
        c.update(in_base=HC, in_sa=K * Tw, in_sk=Tw, in_n=A * K * Tw)
    elif pattern == 'out_kta':              # (b.mag, b.X, B, NBIN, T, NBIN * T, T, B, T * B): out [K][T][A]
        c.update(out_st=A, out_sk=T * A)
    elif pattern == 'out_window':           # (b.Y, b.mag + HC, n, NBIN, B, NBIN * B, B, NBIN * Tw, Tw): into columns [HC, HC + A) of wider rows
        Aw = HC + A + 3
        c.update(out_base=HC, out_st=K * Aw, out_sk=Aw, out_n=T * K * Aw)
    return c


def tr_shapes(pattern):
    return [(A, K, T) for A in TR_A for K in TR_K for T in TR_T if pattern != 'k1_sk0' or K == 1]


def tr_data(c):
    """input (NaN where the launch must not read) and the expected output (NaN where it must not write); values encode (a, k, t)"""
    a, k, t = np.meshgrid(np.arange(c['A']), np.arange(c['K']), np.arange(c['T']), indexing='ij')
    v = ((a * 8 + k) * 128 + t + 1).astype(f32)
    x, want = np.full(c['in_n'], np.nan, f32), np.full(c['out_n'], np.nan, f32)
    x[c['in_base'] + a * c['in_sa'] + k * c['in_sk'] + t] = v
    want[c['out_base'] + t * c['out_st'] + k * c['out_sk'] + a] = v
    return x, want


def tr_eval(x, c, fault=None):
    """the kernel's tiles: loads guarded by (a < A, t < T) else 0, stores by the same test ('swapped_bounds': a < T, t < A)"""
    A, K, T = c['A'], c['K'], c['T']
    out = np.full(c['out_n'], np.nan, f32)
    a, k, t = np.meshgrid(np.arange(-(-A // 32) * 32), np.arange(K), np.arange(-(-T // 32) * 32), indexing='ij')
    ld = (a < A) & (t < T)
    v = np.where(ld, x[np.where(ld, c['in_base'] + a * c['in_sa'] + k * c['in_sk'] + t, 0)], f32(0))
    stg = ((a < T) & (t < A)) if fault == 'swapped_bounds' else ld
    dst = c['out_base'] + t * c['out_st'] + k * c['out_sk'] + a
    ok = stg & (dst < out.size)                       # (the emulation drops what a faulty kernel would write out of bounds)
    out[dst[ok]] = v[ok]
    return out


# ------------------------------------------------------------------------------------------------ fsn_build_sb
def sb_data(B, steps):
    t, f, b = np.meshgrid(np.arange(steps), np.arange(NBIN), np.arange(B), indexing='ij')
    magT = (((t * NBIN + f) * 4 + b) + 1).astype(f32)
    return magT, magT + f32(0.5)


def ref_build_sb(magT, fbo):
    """base_model.py:29-42: reflect-pad the frequency axis by 15, sub-band n = rows n .. n + 30 of the padded plane; model.py:88-96: the
    full-band output of bin n behind them.  -> [steps][32][257 * B], sequence s = n B + b"""
    steps, _, B = magT.shape
    pad = np.pad(magT, ((0, 0), (SBN, SBN), (0, 0)), mode='reflect')
    out = np.empty((steps, SBW, NBIN, B), magT.dtype)
    for k in range(SBW - 1):
        out[:, k] = pad[:, k:k + NBIN]
    out[:, SBW - 1] = fbo
    return out.reshape(steps, SBW, NBIN * B)


def eval_build_sb(magT, fbo, fault=None):
    """the kernel's index arithmetic"""
    steps, _, B = magT.shape
    n = np.arange(NBIN)
    out = np.empty((steps, SBW, NBIN, B), magT.dtype)
    for k in range(SBW - 1):
        f = n - SBN + k
        f = np.where(f < 0, -f - (1 if fault == 'reflect_low_off1' else 0), f)
        f = np.where(f >= NBIN, (2 * (NBIN - 1) if fault != 'reflect_high_off1' else 2 * NBIN - 1) - f, f)
        out[:, k] = magT[:, f]
    out[:, SBW - 1] = fbo
    if fault == 'pack_b_major':                        # s = b * NBIN + n
        return out.transpose(0, 1, 3, 2).reshape(steps, SBW, NBIN * B)
    return out.reshape(steps, SBW, NBIN * B)


# ------------------------------------------------------------------------------------------------ utterance means
MEAN_B, MEAN_TP = (1, 3, 7, 100, 129, 256), (3, 6)


def mean_tlen(B, T):
    """ragged: mixed frame counts with tlen[b] = 1 and = T among them"""
    return np.asarray([(1, T, max(1, T // 2), max(1, T - 1))[b % 4] for b in range(B)], np.int32)


def mag_data(B, T, tlen, seed):
    """[B][257][T] >= 0; frames >= tlen[b] are zeros, as the STFT writes them"""
    g = np.random.default_rng(seed)
    m = (np.abs(g.standard_normal((B, NBIN, T))) * np.exp(g.uniform(-3, 1, (B, 1, 1)))).astype(f32)
    if tlen is not None:
        for b in range(B):
            m[b, :, tlen[b]:] = 0
    return m


def ref_mean(mag, T, tlen, fault=None):
    la = 0 if fault == 'no_LA' else LA
    fr = (np.full(mag.shape[0], T) if tlen is None else d64(tlen)) + la
    mu = d64(mag).sum((1, 2)) / (NBIN * fr)
    return mu, 2 * U * np.abs(mu) + TINY


def eval_mean(mag, T, tlen, fault=None):
    """fp64 sum in another order, one rounding"""
    la = 0 if fault == 'no_LA' else LA
    fr = (np.full(mag.shape[0], T) if tlen is None else d64(tlen)) + la
    return (d64(mag).sum(2).sum(1) / (NBIN * fr).astype(f32).astype(np.float64)).astype(f32)


def sbx_data(B, Tp, tlen, seed, dead=np.nan):
    """sub-band tensor [rows = Tp * 32 * 257][B] >= 0; ragged: rows at frames >= tlen[b] + LA of column b hold `dead`"""
    g = np.random.default_rng(seed)
    rows = Tp * SBW * NBIN
    x = np.abs(g.standard_normal((rows, B), dtype=f32))
    x *= np.exp(g.uniform(-2, 1, (1, B))).astype(f32)
    if tlen is not None:
        r = np.arange(rows)[:, None]
        x[r >= colsum_rmax(rows, tlen)[None, :]] = dead
    return x


def colsum_rmax(rows, tlen):
    B = len(tlen) if tlen is not None else 0
    return (d64(tlen) + LA).astype(np.int64) * SBW * NBIN if tlen is not None else np.full(B, rows, np.int64)


def live_rows(rows, B, tlen):
    """[rows][B]: the rows of column b that belong to its own tlen[b] + LA frames"""
    rmax = colsum_rmax(rows, tlen) if tlen is not None else np.full(B, rows, np.int64)
    return np.arange(rows)[:, None] < rmax[None, :]


def _colsum_blocks(x, B, rmax, dtype, per, stride):
    """[J][1024][stride][B]: row r of the matrix sits at (r // (1024 stride), (r // stride) % 1024, r % stride); dead rows as zeros"""
    rows = x.shape[0]
    J = -(-rows // (SUM_BLOCKS * stride))
    z = np.zeros((J * SUM_BLOCKS * stride, B), dtype)
    z[:rows] = np.where(np.arange(rows)[:, None] < rmax[None, :], x, 0)
    return z.reshape(J, SUM_BLOCKS, stride, B)[:, :, :per]


def ref_colsum(x, B, tlen):
    """partials [1024][B] of the kernel's row partition in float64, the bound of each"""
    rows, per = x.shape[0], 256 // B
    rmax = colsum_rmax(rows, tlen) if tlen is not None else np.full(B, rows, np.int64)
    part = _colsum_blocks(d64(x), B, rmax, np.float64, per, per).sum((0, 2))
    chain = np.ceil(rmax / (SUM_BLOCKS * per)) + per
    return part, (chain[None, :] + 2) * U * np.abs(part) + TINY, chain


def eval_colsum(x, B, tlen, fault=None):
    """fp32 in the kernel's order: a thread's rows one after the other, then the per partials of a column in order"""
    rows, per = x.shape[0], 256 // B
    rmax = colsum_rmax(rows, tlen) if tlen is not None else np.full(B, rows, np.int64)
    # 'drop_r0': the block advances by ceil(256 / B) rows although only r0 < per of its threads work: the rows of r0 >= per are lost
    stride = -(-256 // B) if fault == 'drop_r0' else per
    z = _colsum_blocks(np.asarray(x, f32), B, rmax, f32, per, stride)
    s = np.zeros(z.shape[1:], f32)
    for j in range(z.shape[0]):
        s += z[j]
    t = np.zeros((SUM_BLOCKS, B), f32)
    for k in range(per):
        t += s[:, k]
    return t


def finish_den(B, rows, tlen, fault=None):
    la = 0 if fault == 'no_LA' else LA
    return np.full(B, float(rows)) if tlen is None else (d64(tlen) + la) * SBW * NBIN


def ref_finish(part, rows, tlen):
    mu = d64(part).sum(0) / finish_den(part.shape[1], rows, tlen)
    return mu, 2 * U * np.abs(mu) + TINY


def eval_finish(part, rows, tlen, fault=None):
    """fp64 sum of the fp32 partials, one rounding"""
    return (d64(np.asarray(part, f32)).sum(0) / finish_den(part.shape[1], rows, tlen, fault)).astype(f32)


def ref_scale(x, mu, e_mu=0.0):
    """y = x / (mu[i % B] + 1e-5f) for x [..][B]; e_mu: relative error mu already carries"""
    y = d64(x) / (d64(mu) + MU_EPS)
    return y, (e_mu + 2 * U) * np.abs(y) + TINY


def eval_scale(x, mu):
    return (np.asarray(x, f32) / (np.asarray(mu, f32) + f32(1e-5))).astype(f32)


# ------------------------------------------------------------------------------------------------ cumulative norms
CUM_B, CUM_N, CUM_CHUNKS = (1, 3), (1, 2, 9), (1, 3, 5)


def cum_data(n, F, S, seed, zero_first=False):
    """[n][F][S] >= 0"""
    g = np.random.default_rng(seed)
    x = (np.abs(g.standard_normal((n, F, S))) * np.exp(g.uniform(-3, 1, (n, 1, S)))).astype(f32)
    if zero_first:
        x[0] = 0
    return x


def ref_cum(x, tree, t_first=0, run0=None):
    """cumulative_laplace_norm (base_model.py:212-240) of x [n][F][S] -> y, its bound, the running sum after the last frame, its bound;
    tree: additions on the longest chain of one frame's sum (module docstring)"""
    x = d64(x)
    n, F, S = x.shape
    run = np.cumsum(x.sum(1), 0) + (0.0 if run0 is None else d64(run0)[None])
    frames = t_first + np.arange(n) + 1.0
    d = run / (F * frames[:, None]) + EPS32
    y = x / d[:, None, :]
    e_s = (tree + frames + 2) * U
    return y, (e_s[:, None, None] + 3 * U) * np.abs(y) + TINY, run[-1], e_s[-1] * np.abs(run[-1]) + TINY


def _frame_sum32(x, kind):
    """one frame's sum [S] of x [F][S] in fp32, in the kernel's order"""
    if kind == 'sb':
        s = np.zeros(x.shape[1], f32)
        for k in range(x.shape[0]):
            s = s + x[k]
        return s
    z = np.zeros((512, x.shape[1]), f32)
    z[:NBIN] = x
    w = (z[:256] + z[256:]).reshape(4, 64, -1)
    for o in (32, 16, 8, 4, 2, 1):
        w = w[:, :o] + w[:, o:2 * o]
    p = w[:, 0]
    return (p[0] + p[1]) + (p[2] + p[3])


def eval_cum(x, kind, t_first=0, run0=None, fault=None):
    """fp32 in the kernel's order -> (y, run)"""
    x = np.asarray(x, f32)
    n, F, S = x.shape
    run = np.zeros(S, f32) if (run0 is None or t_first == 0 or fault == 'csum_ignored') else np.asarray(run0, f32).copy()
    y = np.empty_like(x)
    for t in range(n):
        run = run + _frame_sum32(x[t], kind)
        frames = f32((0 if fault == 't_first_dropped' else t_first) + t + 1)
        d = run / (f32(F) * frames) + f32(EPS32)
        y[t] = x[t] / d[None]
    return y, run


def eval_cum_chunked(x, kind, chunks, fault=None):
    ys, run, t0 = [], None, 0
    for c in chunks:
        y, run = eval_cum(x[t0:t0 + c], kind, t0, run, fault)
        ys.append(y)
        t0 += c
    return np.concatenate(ys), run


# ------------------------------------------------------------------------------------------------ mask back end
def _pow_scale(mg, dmg, p):
    """sc = mg^(p-1) (0 at mg = 0; 1 at p = 1) and its bound (as tests/test_gpu_frontend_kernels.py)"""
    if p == 1.0:
        return np.ones_like(mg), np.zeros_like(mg)
    if p == 2.0:
        return mg, dmg
    with np.errstate(divide='ignore', invalid='ignore'):
        sc = np.where(mg > 0, mg ** (p - 1.0), 0.0)
        dsc = np.where(mg > 0, sc * (abs(p - 1.0) * dmg / mg + 2 * ACT_ULP), 0.0)
    return sc, dsc


def ref_cmask(mr, mi, xr, xi, p):
    """est = M X, out = |est|^p est / |est| (fullsubnet_sa_decode_vb.py:56-66) -> (re, im), (bound re, bound im)"""
    mr, mi, xr, xi = d64(mr), d64(mi), d64(xr), d64(xi)
    er, ei = mr * xr - mi * xi, mr * xi + mi * xr
    der, dei = 2 * U * (np.abs(mr * xr) + np.abs(mi * xi)), 2 * U * (np.abs(mr * xi) + np.abs(mi * xr))
    mg = np.sqrt(er * er + ei * ei)
    sc, dsc = _pow_scale(mg, der + dei + 3 * U * mg, p)
    return ((er * sc, ei * sc),
            (der * sc + np.abs(er) * dsc + U * np.abs(er * sc) + TINY, dei * sc + np.abs(ei) * dsc + U * np.abs(ei * sc) + TINY))


def eval_cmask(mr, mi, xr, xi, p):
    mr, mi, xr, xi = (np.asarray(a, f32) for a in (mr, mi, xr, xi))
    er, ei = mr * xr - mi * xi, mr * xi + mi * xr
    if p != 1.0:
        mg = np.sqrt(er * er + ei * ei)
        with np.errstate(divide='ignore', invalid='ignore'):
            sc = np.where(mg > 0, mg if p == 2.0 else np.power(mg, f32(p) - f32(1)), f32(0)).astype(f32)
        er, ei = er * sc, ei * sc
    return er, ei


def mask_data(B, T, seed):
    """mask, spec [B][2][257][T] with elements where mask x spec is exactly 0"""
    g = np.random.default_rng(seed)
    m = g.standard_normal((B, 2, NBIN, T)).astype(f32)
    s = (g.standard_normal((B, 2, NBIN, T)) * np.exp(g.uniform(-6, 2, (B, 1, NBIN, T)))).astype(f32)
    m[:, :, 3, 0] = 0
    s[:, :, 5, T - 1] = 0
    s[:, :, 256, T // 2] = 0
    return m, s


def mask_to_BT(m):
    """[B][2][257][T] -> maskBT [257 * B][2][T + LA], the look-ahead columns (never read) NaN"""
    B, _, _, T = m.shape
    out = np.full((NBIN, B, 2, T + LA), np.nan, f32)
    out[..., LA:] = m.transpose(2, 0, 1, 3)
    return out.reshape(NBIN * B, 2, T + LA)


SA_GT0, SA_N = (0, 1, 2, 5), (1, 3)


def sa_data(B, n, last, gt0, seed):
    """one chunk of the frame-online form: maskT [ns][2][S] (skipped steps NaN), spec window [B][2][257][Tw] (NaN outside the live
    columns) -> the expected est window per component and bounds (NaN where the launch must not write) for p_out"""
    ns, Tw, col0, S = n + (LA if last else 0), HC + n, HC - LA, NBIN * B
    g = np.random.default_rng(seed)
    m = g.standard_normal((ns, 2, NBIN, B)).astype(f32)
    x = (g.standard_normal((B, 2, NBIN, Tw)) * np.exp(g.uniform(-6, 2, (B, 1, NBIN, Tw)))).astype(f32)
    m[:, :, 7, 0] = 0
    x[:, :, 9] = 0
    live = [tau for tau in range(ns) if gt0 + tau >= LA]
    dead_cols = [c for c in range(Tw) if c - col0 not in live]
    x[..., dead_cols] = np.nan
    m[[tau for tau in range(ns) if tau not in live]] = np.nan
    return dict(maskT=m.reshape(ns, 2, S), m=m, spec=x, ns=ns, Tw=Tw, col0=col0, live=live)


def sa_ref(d, p, shift=0):
    """float64 est window [B][2][257][Tw] and bound; shift = 1: the mask of step tau lands on column tau + 1 (a planted fault)"""
    x, m = d['spec'], d['m']
    ref, bd = np.full(x.shape, np.nan), np.full(x.shape, np.nan)
    for tau in d['live']:
        col = d['col0'] + tau + shift
        if col >= d['Tw']:
            continue
        (er, ei), (br, bi) = ref_cmask(m[tau, 0].T, m[tau, 1].T, np.nan_to_num(x[:, 0, :, col]), np.nan_to_num(x[:, 1, :, col]), p)
        ref[:, 0, :, col], ref[:, 1, :, col], bd[:, 0, :, col], bd[:, 1, :, col] = er, ei, br, bi
    return ref, bd


def sa_eval(d, p, fault=None):
    x, m = d['spec'], d['m']
    out = np.full(x.shape, np.nan, f32)
    for tau in d['live']:
        col = d['col0'] + tau + (1 if fault == 'mask_col_shift' else 0)
        if col >= d['Tw']:
            continue
        er, ei = eval_cmask(m[tau, 0].T, m[tau, 1].T, np.nan_to_num(x[:, 0, :, col]), np.nan_to_num(x[:, 1, :, col]), p)
        out[:, 0, :, col], out[:, 1, :, col] = er, ei
    return out


def nan_ratio(got, ref, bound):
    """worst error / bound over the elements the reference owns; inf when the NaN patterns differ (an element written that is not owned,
    or an owned one left unwritten)"""
    own = ~np.isnan(ref)
    if not np.array_equal(np.isnan(np.asarray(got)), ~own):
        return INF
    return ratio(np.asarray(got)[own], ref[own], bound[own])


# ------------------------------------------------------------------------------------------------ Taylor / GAF / ELU
def ew_data(B, T, seed):
    g = np.random.default_rng(seed)
    plane = 161 * T
    r = lambda *s: g.standard_normal(s).astype(f32)
    return dict(plane=plane, gain=(1 / (1 + np.exp(-r(B, plane)))).astype(f32), spec=r(B, 2, plane), hob1=r(B, 2, plane), hob2=r(B, 2, plane),
                resi=r(B, 2, plane))


def ref_taylor_zero(gain, spec):
    z = d64(gain)[:, None] * d64(spec)
    return z, U * np.abs(z) + TINY


def ref_taylor_update(hob, pre, out, k, inv, dpre=0.0, dout=0.0):
    """update = hob + k pre; pre <- update; out += update inv (TaylorSENet.py:85-93); dpre / dout: bounds the inputs already carry"""
    hob, pre, out = d64(hob), d64(pre), d64(out)
    u = hob + k * pre
    du = k * dpre + U * np.abs(k * pre) + U * np.abs(u) + TINY
    o = out + u * inv
    return u, du, o, dout + du * inv + U * np.abs(u * inv) + U * np.abs(o) + TINY


def eval_taylor_update(hob, pre, out, k, inv):
    u = np.asarray(hob, f32) + f32(k) * np.asarray(pre, f32)
    return u, np.asarray(out, f32) + u * f32(inv)


def ref_gaf(gain, pre, resi):
    gp = d64(gain)[:, None] * d64(pre)
    o = gp + d64(resi)
    return o, U * np.abs(gp) + U * np.abs(o) + TINY


ELU_PLANT = [-100.0, 0.0, 2.0 ** -126, -2.0 ** -126, -1e-3, float(np.nextafter(f32(-1e-3), f32(0))), float(np.nextafter(f32(-1e-3), f32(-1))),
             1e-3, -1e-20, 1e-20, 20.0, -20.0]


def elu_data(n):
    x = (2 * np.random.default_rng(n).standard_normal(n)).astype(f32)
    k = min(n, len(ELU_PLANT))
    x[:k] = ELU_PLANT[:k]
    return x


def ref_elu(x):
    x = d64(x)
    y = np.where(x > 0, x, np.expm1(np.minimum(x, 0)))
    return y, A_ELU + U * np.abs(y)


def eval_elu(x):
    """fastmath.h fm_expm1: x + x^2 / 2 above -1e-3, exp(x) - 1 below"""
    x = np.asarray(x, f32)
    ser = (d64(x) + 0.5 * d64(x) * d64(x)).astype(f32)
    return np.where(x > 0, x, np.where(x > f32(-1e-3), ser, np.exp(np.minimum(x, f32(0))) - f32(1))).astype(f32)


# ------------------------------------------------------------------------------------------------ PCM_16
def pcm_table():
    ks = [0, 1, 2, 3, 100, 101, 16382, 16383, 32765, 32766]
    near = [(k + 0.5) / 32767 for k in ks] + [-(k + 0.5) / 32767 for k in ks]
    t = [0.0, 1.0, -1.0, 1 + 2.0 ** -23, -(1 + 2.0 ** -23), 2.0, -2.0, INF, -INF, 0.5, -0.5, 1.5, -1.5, 32766.5 / 32767, -32766.5 / 32767,
         2.0 ** -149, -2.0 ** -149, 1 / 32767, -1 / 32767, 32768 / 32767, -32768 / 32767, -32767.5 / 32767] + near
    g = np.random.default_rng(7)
    return np.concatenate([np.asarray(t, f32), g.uniform(-1.2, 1.2, 300).astype(f32)])


def ref_pcm_encode(x, fault=None):
    """float64 rint (ties to even) of x * 0x7FFF, clipped to int16"""
    if fault == 'half_away_f32':                       # lroundf(x * 32767.f)
        v = d64(np.asarray(x, f32) * f32(32767))
        v = np.sign(v) * np.floor(np.abs(v) + 0.5)
    else:
        v = np.rint(d64(x) * (32768.0 if fault == 'scale_8000' else 32767.0))
    return np.clip(v, -32768, 32767).astype(np.int16)


# ------------------------------------------------------------------------------------------------ short offline resample
RS_RATES = (48000, 44100, 8000)
RS_LENGTHS = (1, 2, 3, 4, 100, 193)      # 4 at 48 kHz: int(4 / 3) = 1 < ceil = 2, the fix_length tail; 100 the same at 48 and 44.1 kHz


# ================================================================================================ CPU
def test_bound_holds_for_fp32_and_catches_faults():
    # transpose_akt: the mirror of the kernel's tiles is exact on every case of the table; swapped bound tests are not
    for pat in TR_PATTERNS:
        for A, K, T in tr_shapes(pat):
            c = tr_case(pat, A, K, T)
            x, want = tr_data(c)
            assert exact_ratio(tr_eval(x, c), want) == 0.0, (pat, A, K, T)
    c = tr_case('dense', 33, 2, 7)
    x, want = tr_data(c)
    assert exact_ratio(tr_eval(x, c, 'swapped_bounds'), want) == INF

    # fsn_build_sb
    for B, steps in ((1, 1), (3, 3)):
        magT, fbo = sb_data(B, steps)
        want = ref_build_sb(magT, fbo)
        assert exact_ratio(eval_build_sb(magT, fbo), want) == 0.0
        for fault in ('reflect_low_off1', 'reflect_high_off1', 'pack_b_major'):
            if fault == 'pack_b_major' and B == 1:
                continue
            assert exact_ratio(eval_build_sb(magT, fbo, fault), want) == INF, fault

    # utterance means
    for B, Tp in ((3, 3), (100, 6), (129, 3), (7, 6)):
        T = Tp - LA
        for tlen in (None, mean_tlen(B, T)):
            mag = mag_data(B, T, tlen, 10 * B + Tp)
            mu, bd = ref_mean(mag, T, tlen)
            assert ratio(eval_mean(mag, T, tlen), mu, bd) <= 1.0
            assert ratio(eval_mean(mag, T, tlen, 'no_LA'), mu, bd) >= 10
            x = sbx_data(B, Tp, tlen, 20 * B + Tp, dead=7.0)
            part, pbd, chain = ref_colsum(x, B, tlen)
            got = eval_colsum(x, B, tlen)
            assert ratio(got, part, pbd) <= 1.0, (B, Tp)
            if 256 % B:
                assert ratio(eval_colsum(x, B, tlen, 'drop_r0'), part, pbd) >= 10, (B, Tp)
            mu2, bd2 = ref_finish(part, x.shape[0], tlen)
            assert ratio(eval_finish(got, x.shape[0], tlen), mu2, bd2 + (chain + 2) * U * mu2) <= 1.0
            if tlen is not None:
                assert ratio(eval_finish(got, x.shape[0], tlen, 'no_LA'), mu2, bd2 + (chain + 2) * U * mu2) >= 10
            y, ybd = ref_scale(x, mu2)
            live = live_rows(x.shape[0], B, tlen)
            assert ratio(eval_scale(x, mu2.astype(f32))[live], y[live], (ybd + U * np.abs(y))[live]) <= 1.0      # (+ U: mu rounded to fp32 here)

    # cumulative norms: one shot, chunked, the two csum faults
    for kind, F, tree in (('fb', NBIN, 9), ('sb', SBW, 32)):
        for B in CUM_B:
            S = B if kind == 'fb' else NBIN * B
            for n in CUM_N:
                x = cum_data(n, F, S, 100 * n + B, zero_first=(n == 2))
                y, ybd, run, rbd = ref_cum(x, tree)
                g, r = eval_cum(x, kind)
                assert ratio(g, y, ybd) <= 1.0 and ratio(r, run, rbd) <= 1.0, (kind, B, n)
                if n == 2:
                    assert (g[0] == 0).all()
            x = cum_data(9, F, S, 900 + B)
            y, ybd, run, rbd = ref_cum(x, tree)
            g, r = eval_cum_chunked(x, kind, CUM_CHUNKS)
            g1, r1 = eval_cum(x, kind)
            assert np.array_equal(g, g1) and np.array_equal(r, r1)
            for fault in ('csum_ignored', 't_first_dropped'):
                g, r = eval_cum_chunked(x, kind, CUM_CHUNKS, fault)
                assert ratio(g, y, ybd) >= 10, (kind, fault)

    # mask back end
    for T, B, p in ((1, 3, 2.0), (255, 1, 0.6), (257, 1, 1.0)):
        m, s = mask_data(B, T, T + B)
        (er, ei), (br, bi) = ref_cmask(m[:, 0], m[:, 1], s[:, 0], s[:, 1], p)
        gr, gi = eval_cmask(m[:, 0], m[:, 1], s[:, 0], s[:, 1], p)
        assert ratio(gr, er, br) <= 1.0 and ratio(gi, ei, bi) <= 1.0, (T, B, p)
        assert (gr[:, 3, 0] == 0).all() and (gi[:, 5, T - 1] == 0).all()
    for gt0 in SA_GT0:
        for n in SA_N:
            for last in (False, True):
                for p in (1.0, 2.0, 0.6):
                    d = sa_data(3, n, last, gt0, 10 * gt0 + n)
                    ref, bd = sa_ref(d, p)
                    assert nan_ratio(sa_eval(d, p), ref, bd) <= 1.0, (gt0, n, last, p)
                    if d['live']:
                        assert nan_ratio(sa_eval(d, p, 'mask_col_shift'), ref, bd) >= 10, (gt0, n, last, p)

    # Taylor recurrence, GAF stage, ELU
    for B, T in ((1, 1), (3, 5)):
        e = ew_data(B, T, B + T)
        z, zbd = ref_taylor_zero(e['gain'], e['spec'])
        z32 = e['gain'][:, None] * e['spec']
        assert ratio(z32, z, zbd) <= 1.0
        pre, out, dpre, dout = z, z, zbd, zbd
        p32, o32 = z32, z32
        for k, hob in ((1, e['hob1']), (2, e['hob2'])):
            inv = float(f32(1) / f32(math.factorial(k + 1)))
            pre, dpre, out, dout = ref_taylor_update(hob, pre, out, k, inv, dpre, dout)
            p32, o32 = eval_taylor_update(hob, p32, o32, k, inv)
            assert ratio(p32, pre, dpre) <= 1.0 and ratio(o32, out, dout) <= 1.0
        o, obd = ref_gaf(e['gain'], e['spec'], e['resi'])
        assert ratio(e['gain'][:, None] * e['spec'] + e['resi'], o, obd) <= 1.0
    for n in (1, 255, 1025):
        x = elu_data(n)
        assert ratio(eval_elu(x), *ref_elu(x)) <= 1.0

    # PCM_16: the reference is wavio.pcm16_bytes; the two planted faults move a sample of the table
    import se_amd  # noqa: F401
    from se_amd import wavio
    t = pcm_table()
    want = ref_pcm_encode(t)
    assert np.array_equal(want, wavio.pcm16_bytes(t).astype(np.int16))
    assert want[9] == 16384 and want[10] == -16384 and want[7] == 32767 and want[8] == -32768 and want[15] == 0
    for fault in ('scale_8000', 'half_away_f32'):
        assert not np.array_equal(ref_pcm_encode(t, fault), want), fault


# ================================================================================================ GPU
_lib = None
SIGS = {
    'mp_transpose_akt': 'ppiiillll', 'mp_elu': 'ppl', 'mp_fill': 'plf', 'mp_taylor_zero': 'ppppll', 'mp_taylor_update': 'ppplff',
    'mp_gaf_combine': 'ppppll', 'mp_fsn_mean': 'piifppi', 'mp_fsn_scale': 'pplip', 'mp_fsn_build_sb': 'pppii', 'mp_fsn_colsum': 'plippi',
    'mp_fsn_finish_mean': 'ppfipi', 'mp_fsn_mask': 'pppiif', 'mp_fsn_cum_fb': 'ppiipi', 'mp_fsn_cum_sb': 'piipi',
    'mp_fsn_stream_apply': 'pppiiiiif',
}
CT = {'i': C.c_int, 'p': C.c_void_p, 'l': C.c_long, 'f': C.c_float}
SLACK = 64
SENTINEL = 0x5A5A
gpu = pytest.mark.gpu


def lib():
    global _lib
    if _lib is None:
        assert os.path.exists(PROBE_LIB), 'libse_modelprobe.so is missing: run build() (make -C csrc)'
        L = C.CDLL(PROBE_LIB)
        for name, sig in SIGS.items():
            getattr(L, name).argtypes = [CT[c] for c in sig]
            getattr(L, name).restype = C.c_int
        L.mp_last_error.restype = C.c_char_p
        _lib = L
    return _lib


class Buf:
    """device buffer of n elements with NaN (floats), -1 (int32) or SENTINEL (int16) in it and in the slack around it, unless src fills it"""

    def __init__(self, n, src=None, dtype=torch.float32):
        self.n, self.dtype = n, dtype
        self.fill = {torch.int32: -1, torch.int16: SENTINEL}.get(dtype, float('nan'))
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
        return bool(torch.isnan(s).all()) if self.dtype == torch.float32 else bool((s == self.fill).all())


def call(name, *args):
    L = lib()
    rc = getattr(L, name)(*[a.ptr if isinstance(a, Buf) else a for a in args])
    assert rc == 0, '%s: %s' % (name, L.mp_last_error().decode())


def note(kernel, r, case):
    if r > WORST.get(kernel, (-1.0, ''))[0]:
        WORST[kernel] = (r, case)


def verify(case, kernel, got, ref, bound):
    got = d64(got)
    assert np.isfinite(got).all(), '%s: non-finite value in what the launch owns' % case
    r = np.abs(got - ref) / bound
    k = int(r.argmax()) if r.size else 0
    worst = float(r.reshape(-1)[k]) if r.size else 0.0
    print('%s: worst error / bound %.3f at %s (got %.9g, want %.9g, bound %.3g)' %
          (case, worst, tuple(int(i) for i in np.unravel_index(k, r.shape)) if r.size else (), got.reshape(-1)[k] if r.size else 0,
           d64(ref).reshape(-1)[k] if r.size else 0, np.broadcast_to(bound, r.shape).reshape(-1)[k] if r.size else 0))
    note(kernel, worst, case)
    assert worst <= 1.0, '%s: error %.3f of the bound' % (case, worst)


def verify_exact(case, kernel, got, want):
    assert np.array_equal(got, want, equal_nan=True), '%s: %d elements differ' % (
        case, int((~((got == want) | (np.isnan(got) & np.isnan(want)))).sum()))
    note(kernel, 0.0, case)


def rows_buf(tlen):
    """a Ragged as the engine uploads it, [4][MB] (len | lpad | tlen | olen); only tlen is meaningful here"""
    MB = len(tlen) + 2
    a = np.full((4, MB), -12345, np.int32)
    a[2, :len(tlen)] = tlen
    return Buf(4 * MB, a, torch.int32), MB


# ---- layout movers ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('pattern', TR_PATTERNS)
def test_transpose_akt(pattern):
    for A, K, T in tr_shapes(pattern):
        c = tr_case(pattern, A, K, T)
        x, want = tr_data(c)
        bi, bo = Buf(x.size, x), Buf(want.size)
        call('mp_transpose_akt', bi.ptr + 4 * c['in_base'], bo.ptr + 4 * c['out_base'], A, K, T, c['in_sa'], c['in_sk'], c['out_st'],
             c['out_sk'])
        verify_exact('transpose_akt %s A%d K%d T%d' % (pattern, A, K, T), 'transpose_akt', bo.np(want.size), want)
        assert bo.untouched() and bi.untouched()


@gpu
@pytest.mark.parametrize('n', [1, 255, 1025])
def test_elu_and_fill(n):
    x = elu_data(n)
    bx, by = Buf(n, x), Buf(n)
    call('mp_elu', bx, by, n)
    assert by.untouched()
    verify('elu n%d' % n, 'elu', by.np(n), *ref_elu(x))
    for v in (0.0, -3.25):
        bp = Buf(n + 5)
        call('mp_fill', bp, n, v)
        want = np.full(n + 5, np.nan, f32)
        want[:n] = v
        verify_exact('fill n%d v%g' % (n, v), 'fill', bp.np(n + 5), want)
        assert bp.untouched()


# ---- TaylorSENet / G2Net -----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('T', [1, 5])
@pytest.mark.parametrize('B', [1, 3])
def test_taylor_and_gaf(B, T):
    e = ew_data(B, T, B + T)
    plane, tot = e['plane'], e['plane'] * B
    assert tot % 256
    bg, bs, bz, bo = Buf(tot, e['gain']), Buf(2 * tot, e['spec']), Buf(2 * tot), Buf(2 * tot)
    call('mp_taylor_zero', bg, bs, bz, bo, plane, tot)
    assert bz.untouched() and bo.untouched()
    z, zbd = ref_taylor_zero(e['gain'], e['spec'])
    case = 'B%d T%d' % (B, T)
    verify('taylor_zero zero ' + case, 'taylor_zero', bz.np(B, 2, plane), z, zbd)
    verify('taylor_zero out ' + case, 'taylor_zero', bo.np(B, 2, plane), z, zbd)
    assert np.array_equal(bz.np(2 * tot), bo.np(2 * tot))
    pre, out, dpre, dout = z, z, zbd, zbd                     # the chain from the float64 start, bounds carried along
    for k, hob in ((1, e['hob1']), (2, e['hob2'])):
        inv = float(f32(1) / f32(math.factorial(k + 1)))
        p_in, o_in = bz.np(B, 2, plane).copy(), bo.np(B, 2, plane).copy()
        bh = Buf(2 * tot, hob)
        call('mp_taylor_update', bh, bz, bo, 2 * tot, float(k), inv)
        assert bz.untouched() and bo.untouched() and np.array_equal(bh.np(B, 2, plane), hob)
        u, du, o, do = ref_taylor_update(hob, p_in, o_in, k, inv)             # this launch alone, from what it was given
        verify('taylor_update pre k%d %s' % (k, case), 'taylor_update', bz.np(B, 2, plane), u, du)
        verify('taylor_update out k%d %s' % (k, case), 'taylor_update', bo.np(B, 2, plane), o, do)
        pre, dpre, out, dout = ref_taylor_update(hob, pre, out, k, inv, dpre, dout)
        verify('taylor_update chain pre k%d %s' % (k, case), 'taylor_update', bz.np(B, 2, plane), pre, dpre)
        verify('taylor_update chain out k%d %s' % (k, case), 'taylor_update', bo.np(B, 2, plane), out, dout)
    br, bn = Buf(2 * tot, e['resi']), Buf(2 * tot)
    call('mp_gaf_combine', bg, bs, br, bn, plane, tot)
    assert bn.untouched()
    verify('gaf_combine ' + case, 'gaf_combine', bn.np(B, 2, plane), *ref_gaf(e['gain'], e['spec'], e['resi']))


# ---- FullSubNet: unfold --------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('steps', [1, 3])
@pytest.mark.parametrize('B', [1, 3])
def test_fsn_build_sb(B, steps):
    magT, fbo = sb_data(B, steps)
    want = ref_build_sb(magT, fbo)
    bm, bf, bs = Buf(magT.size, magT), Buf(fbo.size, fbo), Buf(want.size)
    call('mp_fsn_build_sb', bm, bf, bs, B, steps)
    got = bs.np(steps, SBW, NBIN * B)
    verify_exact('fsn_build_sb B%d steps%d' % (B, steps), 'fsn_build_sb', got, want)
    assert bs.untouched()
    # both reflected edges and the full-band slot, spelt out for sub-band 0 and 256 of utterance B - 1
    b = B - 1
    assert got[0, 0, 0 * B + b] == magT[0, 15, b] and got[0, 14, b] == magT[0, 1, b] and got[0, 15, b] == magT[0, 0, b]
    assert got[0, 30, 256 * B + b] == magT[0, 241, b] and got[0, 16, 256 * B + b] == magT[0, 255, b] and got[0, 31, 256 * B + b] == fbo[0, 256, b]


# ---- FullSubNet: utterance means -------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('ragged', [False, True])
@pytest.mark.parametrize('Tp', MEAN_TP)
@pytest.mark.parametrize('B', MEAN_B)
def test_fsn_mean(B, Tp, ragged):
    T = Tp - LA
    tlen = mean_tlen(B, T) if ragged else None
    mag = mag_data(B, T, tlen, 10 * B + Tp)
    bm, bu = Buf(mag.size, mag), Buf(B)
    rb, MB = rows_buf(tlen) if ragged else (None, 0)
    call('mp_fsn_mean', bm, B, NBIN * T, float(NBIN * Tp), bu, rb, MB)
    assert bu.untouched()
    mu, bd = ref_mean(mag, T, tlen)
    verify('fsn_mean B%d Tp%d %s' % (B, Tp, 'ragged' if ragged else 'equal'), 'fsn_mean', bu.np(B), mu, bd)
    if ragged:          # the clip alone, T = tlen[b]: another summation order (module docstring), so under the sum of the two bounds
        b = B - 1 if tlen[B - 1] < T else 0
        one = np.ascontiguousarray(mag[b:b + 1, :, :tlen[b]])
        b1, u1 = Buf(one.size, one), Buf(1)
        call('mp_fsn_mean', b1, 1, NBIN * int(tlen[b]), float(NBIN * (int(tlen[b]) + LA)), u1, None, 0)
        assert abs(float(u1.np(1)[0]) - float(bu.np(B)[b])) <= 2 * bd[b]


@gpu
@pytest.mark.parametrize('ragged', [False, True])
@pytest.mark.parametrize('Tp', MEAN_TP)
@pytest.mark.parametrize('B', MEAN_B)
def test_fsn_colsum_finish_scale(B, Tp, ragged):
    """fsn_colsum, fsn_finish_mean and fsn_scale, each launch checked on its own, chained as model_fullsubnet.hip chains them"""
    T = Tp - LA
    tlen = mean_tlen(B, T) if ragged else None
    if ragged and B == 1 and T > 1:
        tlen = np.asarray([T // 2], np.int32)
    case = 'B%d Tp%d %s' % (B, Tp, 'ragged' if ragged else 'equal')
    x = sbx_data(B, Tp, tlen, 20 * B + Tp)
    rows = x.shape[0]
    rb, MB = rows_buf(tlen) if ragged else (None, 0)
    bx, bp = Buf(x.size, x), Buf(SUM_BLOCKS * B)
    call('mp_fsn_colsum', bx, rows, B, bp, rb, MB)
    assert bp.untouched() and bx.untouched()
    part, pbd, chain = ref_colsum(x, B, tlen)
    got_part = bp.np(SUM_BLOCKS, B)
    verify('fsn_colsum ' + case, 'fsn_colsum', got_part, part, pbd)
    if ragged and B == 1 and T > 1:      # a ragged batch of one: the same per, grid and rows as the clip alone -> bit for bit
        n1 = (int(tlen[0]) + LA) * SBW * NBIN
        b1, p1 = Buf(n1, x[:n1]), Buf(SUM_BLOCKS)
        call('mp_fsn_colsum', b1, n1, 1, p1, None, 0)
        assert np.array_equal(p1.np(SUM_BLOCKS, 1), got_part), 'a ragged batch of one differs from the clip alone'
    bu = Buf(B)
    call('mp_fsn_finish_mean', bp, bu, float(rows), B, rb, MB)
    assert bu.untouched()
    mu_l, bd_l = ref_finish(got_part, rows, tlen)                 # this launch alone, from the partials it was given
    verify('fsn_finish_mean ' + case, 'fsn_finish_mean', bu.np(B), mu_l, bd_l)
    mu, bd = ref_finish(part, rows, tlen)                         # the chain from float64 partials
    verify('fsn_finish_mean chain ' + case, 'fsn_finish_mean', bu.np(B), mu, bd + (chain + 2) * U * np.abs(mu))
    mu_gpu = bu.np(B).copy()
    live = live_rows(rows, B, tlen)
    call('mp_fsn_scale', bx, bx, rows * B, B, bu)                 # in place, as the model runs it
    assert bx.untouched()
    got = bx.np(rows, B)
    y_l, ybd_l = ref_scale(np.nan_to_num(x), mu_gpu)
    verify('fsn_scale ' + case, 'fsn_scale', got[live], y_l[live], ybd_l[live])
    y, ybd = ref_scale(np.nan_to_num(x), mu, (chain + 4) * U)
    verify('fsn_scale chain ' + case, 'fsn_scale', got[live], y[live], np.broadcast_to(ybd, y.shape)[live])
    if ragged and B > 1:      # the clip alone (another per: another order) agrees under the two bounds
        b = 0
        n1 = (int(tlen[b]) + LA) * SBW * NBIN
        b1, p1, u1 = Buf(n1, x[:n1, b]), Buf(SUM_BLOCKS), Buf(1)
        call('mp_fsn_colsum', b1, n1, 1, p1, None, 0)
        call('mp_fsn_finish_mean', p1, u1, float(n1), 1, None, 0)
        c1 = math.ceil(n1 / (SUM_BLOCKS * 256)) + 256
        assert abs(float(u1.np(1)[0]) - float(mu_gpu[b])) <= ((chain[b] + 4) + (c1 + 4)) * U * mu[b]


# ---- FullSubNet: cumulative norms ------------------------------------------------------------------------------------------------------------
def run_cum(kind, x, B, csum=None, t_first=0):
    """one launch on x [n][F][S] -> y (fb: out of place; sb: in place); csum: a Buf or None"""
    n, F, S = x.shape
    bx = Buf(x.size, x)
    if kind == 'fb':
        by = Buf(x.size)
        call('mp_fsn_cum_fb', bx, by, n, B, csum, t_first)
        assert np.array_equal(bx.np(*x.shape), x)
    else:
        by = bx
        call('mp_fsn_cum_sb', bx, n, S, csum, t_first)
    assert by.untouched() and (csum is None or csum.untouched())
    return by.np(n, F, S)


@gpu
@pytest.mark.parametrize('B', CUM_B)
@pytest.mark.parametrize('kind', ['fb', 'sb'])
def test_fsn_cum(kind, B):
    F, tree = (NBIN, 9) if kind == 'fb' else (SBW, 32)
    S = B if kind == 'fb' else NBIN * B
    name = 'fsn_cum_' + kind
    for n in CUM_N:                                   # one call from t_first = 0, csum = null; n = 2: an all-zero first frame
        x = cum_data(n, F, S, 100 * n + B, zero_first=(n == 2))
        got = run_cum(kind, x, B)
        y, ybd, _, _ = ref_cum(x, tree)
        verify('%s B%d n%d' % (name, B, n), name, got, y, ybd)
        if n == 2:
            assert (got[0] == 0).all(), '0 / EPS must be an exact, finite zero'
    x = cum_data(9, F, S, 900 + B)
    y, ybd, run, rbd = ref_cum(x, tree)
    cs1 = Buf(S)                                      # NaN in it: a first chunk (t_first = 0) must not read it
    one = run_cum(kind, x, B, cs1, 0)
    verify('%s B%d one shot with csum' % (name, B), name, one, y, ybd)
    verify('%s B%d csum' % (name, B), name, cs1.np(S), run, rbd)
    assert np.array_equal(one, run_cum(kind, x, B))
    cs, t0, outs = Buf(S), 0, []
    for c in CUM_CHUNKS:
        outs.append(run_cum(kind, np.ascontiguousarray(x[t0:t0 + c]), B, cs, t0))
        t0 += c
    assert np.array_equal(np.concatenate(outs), one), 'chunked outputs differ from the one-shot run'
    assert np.array_equal(cs.np(S), cs1.np(S)), 'the carried sum differs from the one-shot run'


# ---- FullSubNet: mask back end -------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('p_out', [1.0, 2.0, 0.6])
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('T', [1, 255, 257])
def test_fsn_mask(T, B, p_out):
    m, s = mask_data(B, T, T + B)
    mbt = mask_to_BT(m)
    bm, bs, bo = Buf(mbt.size, mbt), Buf(s.size, s), Buf(s.size)
    case = 'T%d B%d p%g' % (T, B, p_out)
    call('mp_fsn_mask', bm, bs, bo, B, T, p_out)
    assert bo.untouched()
    got = bo.np(B, 2, NBIN, T)
    (er, ei), (br, bi) = ref_cmask(m[:, 0], m[:, 1], s[:, 0], s[:, 1], p_out)
    verify('fsn_mask re ' + case, 'fsn_mask', got[:, 0], er, br)
    verify('fsn_mask im ' + case, 'fsn_mask', got[:, 1], ei, bi)
    assert (got[:, :, 3, 0] == 0).all() and (got[:, :, 5, T - 1] == 0).all() and (got[:, :, 256, T // 2] == 0).all(), 'mask x spec = 0 gives 0'
    if p_out == 1.0:                                  # the forward hook: spec = null, the mask itself
        bh = Buf(s.size)
        call('mp_fsn_mask', bm, None, bh, B, T, 1.0)
        verify_exact('fsn_mask hook ' + case, 'fsn_mask', bh.np(B, 2, NBIN, T), m)
        assert bh.untouched()


@gpu
@pytest.mark.parametrize('p_out', [1.0, 2.0, 0.6])
@pytest.mark.parametrize('B', [1, 3])
def test_fsn_stream_apply(B, p_out):
    for gt0 in SA_GT0:
        for n in SA_N:
            for last in (False, True):
                d = sa_data(B, n, last, gt0, 10 * gt0 + n)
                bm, bs, be = Buf(d['maskT'].size, d['maskT']), Buf(d['spec'].size, d['spec']), Buf(d['spec'].size)
                call('mp_fsn_stream_apply', bm, bs, be, B, d['Tw'], d['ns'], d['col0'], gt0, p_out)
                assert be.untouched()
                got = be.np(*d['spec'].shape)
                ref, bd = sa_ref(d, p_out)
                own = ~np.isnan(ref)
                case = 'fsn_stream_apply B%d p%g gt0 %d n%d%s' % (B, p_out, gt0, n, ' last' if last else '')
                assert np.isnan(got[~own]).all(), case + ': a column outside the chunk\'s live steps was written'
                verify(case, 'fsn_stream_apply', got[own], ref[own], bd[own])
                if d['live']:
                    assert (got[:, :, 9, d['col0'] + d['live'][0]] == 0).all(), 'mask x spec = 0 gives 0'


# ---- PCM_16 --------------------------------------------------------------------------------------------------------------------------------
def engine_lib():
    import se_amd  # noqa: F401
    from se_amd import _lib as EL
    return EL.load()


@gpu
def test_pcm16():
    from se_amd import wavio
    L = engine_lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    t = pcm_table()
    n, pin, pout = t.size, t.size + 5, t.size + 3
    x = np.full((2, pin), np.nan, f32)
    x[0, :n], x[1, :n] = t, -t[::-1]
    bx, bq = Buf(x.size, x), Buf(2 * pout, dtype=torch.int16)
    rc = L.se_pcm16_encode(C.c_void_p(bx.ptr), pin, 2, n, C.c_void_p(bq.ptr), pout, st)
    assert rc == 0, L.se_last_error(None).decode()
    torch.cuda.synchronize()
    q = bq.np(2, pout)
    assert bq.untouched() and (q[:, n:] == SENTINEL).all(), 'pcm16_encode wrote outside its rows'
    for b in range(2):
        want = ref_pcm_encode(x[b, :n])
        assert np.array_equal(q[b, :n], want), np.nonzero(q[b, :n] != want)
        assert np.array_equal(q[b, :n].astype('<i2'), wavio.pcm16_bytes(x[b, :n])), 'the device and wavio.pcm16_bytes disagree'
    note('pcm16_encode', 0.0, 'table of %d' % n)
    g = np.random.default_rng(8)
    s = np.concatenate([np.asarray([-32768, 32767, 0, 1, -1, 16384, -16384], np.int16), g.integers(-32768, 32768, 300).astype(np.int16)])
    n, pin, pout = s.size, s.size + 3, s.size + 6
    src = np.full((2, pin), SENTINEL, np.int16)
    src[0, :n], src[1, :n] = s, s[::-1]
    bs, bf = Buf(src.size, src, torch.int16), Buf(2 * pout)
    rc = L.se_pcm16_decode(C.c_void_p(bs.ptr), pin, 2, n, C.c_void_p(bf.ptr), pout, st)
    assert rc == 0, L.se_last_error(None).decode()
    torch.cuda.synchronize()
    want = np.full((2, pout), np.nan, f32)
    want[:, :n] = (src[:, :n].astype(np.float64) / 32768.0).astype(f32)
    assert np.array_equal(want[:, :n].astype(np.float64) * 32768.0, src[:, :n].astype(np.float64))      # x / 32768 is exact in fp32
    verify_exact('pcm16_decode', 'pcm16_decode', bf.np(2, pout), want)
    assert bf.untouched()


# ---- offline resample on signals shorter than the filter's reach -----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('sr_in', RS_RATES)
def test_resample_short(sr_in):
    from oracle import resample as R
    L = engine_lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    seen_tail = False
    for n in RS_LENGTHS:
        ratio_ = 16000.0 / sr_in
        n_out, n_calc = int(math.ceil(n * ratio_)), int(n * ratio_)
        assert n_out == int(L.se_resample_samples(n, sr_in, 16000))
        seen_tail |= n_out > n_calc
        pin, pout = n + 7, n_out + 5
        x = np.full((2, pin), np.nan, f32)
        x[:, :n] = (0.1 * np.random.default_rng(sr_in + n).standard_normal((2, n))).astype(f32)
        bx, by = Buf(x.size, x), Buf(2 * pout)
        rc = L.se_resample(C.c_void_p(bx.ptr), pin, 2, n, sr_in, 16000, C.c_void_p(by.ptr), pout, st)
        assert rc == 0, L.se_last_error(None).decode()
        torch.cuda.synchronize()
        got = by.np(2, pout)
        assert by.untouched() and np.isnan(got[:, n_out:]).all(), 'resample wrote outside its rows'
        for b in range(2):
            ref = R.librosa_resample(x[b, :n].astype(np.float64), sr_in, 16000)
            assert ref.shape == (n_out,)
            verify('resample %d -> 16000 n%d row %d' % (sr_in, n, b), 'resample', got[b, :n_out], ref, 2e-7)
            assert (got[b, n_calc:n_out] == 0).all(), 'the fix_length tail is exactly 0'
    assert seen_tail or sr_in == 8000


@gpu
def test_every_kernel_launched():
    """every kernel of the table was launched by the cases above on this device (runs last: pytest keeps file order)"""
    print('worst error / bound per kernel:')
    for k in sorted(WORST):
        print('  %-18s %.3f  %s' % (k, WORST[k][0], WORST[k][1]))
    missing = [k for k in KERNELS if k not in WORST]
    assert not missing, 'kernels not launched: %s' % missing
