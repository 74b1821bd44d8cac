"""One normalisation pass or one TCM block at a time against float64.  The norm passes of csrc/k_misc.hip and csrc/k_cln.hip (InstanceNorm in four
forms, cumulative LayerNorm offline and frame-online, layernorm_cf, the TCM branch head) and the one-workgroup-per-utterance TCM
block of csrc/k_tcm.hip each choose a code path from something the whole-model fixtures do not vary: the mutual 16 B alignment of
input, output and residual, P = F * T against the unroll widths, T against 1024 and against 4, the chunk width of a stream, the
batch and T of a TCM call.  Every case here is one operation, called as the models call it (csrc/tests/norm_probe.hip ->
libse_normprobe.so), on torch buffers with slack; it checks

  1. every stored element against a float64 reference written here from the operation's definition (InstanceNorm1d / 2d: torch;
     cumulative LayerNorm: CTSNet_new/Step1_network.py:213-286; the TCM block `Glu`: CTSNet/Step1_network.py:158-188,
     Step2_network.py:126-158, G2Net_VB/gaf_net_320.py:245-274, TaylorSENet/TaylorSENet.py:641-685; LayerNorm([F, C]):
     DPCRN/DPCRN.py:56-88, Uformer/dsconv2d_cplx.py:56) under an elementwise bound, printing the worst error / bound;
  2. ownership: outputs are pre-filled with NaN, the slack and the 0-3 float offsets included; what the operation does not own must
     still be NaN (in-place and residual-aliases-output cases are checked for values);
  3. dead data: in ragged cases the frames t >= tlen[b] of the input hold NaN, then 1e30; outputs at t < tlen[b] must equal, bit
     for bit, those of the same case with finite tails;
  4. the form that ran (kernels.h NormLaunchRec) against a Python mirror of the launcher's conditions; test_every_form_reached
     asserts the whole table of forms was seen.

Error bound, per element (u = 2^-24; constants as tests/test_gpu_lstm_forms.py: C_DOT = 4, Q_PROP = 3, ACT_ULP = 8u).  For
y = PReLU(z) + r, z = (x - mu) rs g + b evaluated in fp32 with statistics off by d_mu and (relatively) e_rs:
    |dz| <= |rs g| (d_mu + u |x - mu|) + |(x - mu) rs g| (e_rs + 2u) + u |z|,   |dy| <= max(1, |slope|) |dz| + u |PReLU(z)| + u |y|
  * statistics accumulated in fp64 from fp32 values: d_mu = u |mu|, e_rs = u, plus the fp64 sums' own rounding
    C_DOT 2^-53 sqrt(n) E[x^2] / (var + eps) (1e-9 in the worst regime here);
  * statistics from fp32 partial sums (the conv epilogue's, or the fp32 accumulation of tcm_fused_kernel's InstanceNorm heads): a
    partial of n terms carries C_DOT u sqrt(n) of its magnitude sum, so dS = sum_p C_DOT u sqrt(n_p) sum_p |x|, dQ likewise on x^2,
    d_mu = dS / N + u |mu|, d_var = dQ / N + 2 |mu| dS / N, e_rs = d_var / (2 (var + eps)) + u: the mu^2 / var amplification of
    a plane whose mean dominates its spread (regime b) is in this term;
  * FIR of K taps: sum |w_k| |dz_k| + C_DOT u sqrt(K) sum |w_k z_k|;
  * the TCM block chains these with its three GEMMs as the LSTM reference chains its gates: a dot product of K terms adds
    C_DOT u sqrt(K) of its magnitude sum, carried error goes through a matrix in quadrature with Q_PROP, the hardware sigmoid adds
    ACT_ULP, an error field E entering a norm moves mu by Q_PROP sqrt(sum E^2) / n and var by 2 Q_PROP sqrt(sum (a - mu)^2 E^2) / n.
test_bound_holds_for_fp32_and_catches_faults (CPU) shows that plain fp32 evaluations stay inside the bound in every regime and that
each plausible fault exceeds it by >= 10x.

Forms that only an environment switch selects (SE_CLN_PLANE=0, SE_CLN_STREAM_RES=0) run in one child process each."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'sixty-years-of-frequency-domain-monaural-speech-enhancement_amd')
PROBE_LIB = os.environ.get('SE_NORMPROBE_LIB') or os.path.join(PKG, 'libse_normprobe.so')
GCPROBE_LIB = os.environ.get('SE_GCPROBE_LIB') or os.path.join(PKG, 'libse_gcprobe.so')
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

U = 2.0 ** -24
ACT_ULP = 8 * U
C_DOT = 4.0
Q_PROP = 3.0
EPS = 1e-5
F64 = torch.float64
REGIMES = ('normal', 'offset', 'const', 'tiny', 'outlier')
NU = 8                      # kernels.h: loads in flight per thread

REACHED = set()             # forms seen by the GPU cases of this process (test_every_form_reached)
WORST = {}                  # form -> worst error / bound


# ------------------------------------------------------------------------------------------------ inputs
def make(shape, regime, seed):
    """fp32 values widened to float64 (both sides start from the same numbers); the last axis is time, the plane is the last two."""
    g = np.random.default_rng(seed)
    if regime == 'normal':
        x = g.standard_normal(shape)
    elif regime == 'offset':                 # mean 100x the spread: the conditioning of E[x^2] - mu^2
        x = 100.0 + g.standard_normal(shape)
    elif regime == 'const':                  # variance 0: eps decides
        x = np.full(shape, 3.7)
    elif regime == 'tiny':                   # variance below eps
        x = 1e-4 * g.standard_normal(shape)
    elif regime == 'outlier':                # one 1e4 in a plane of unit values
        x = np.ones(shape)
        x.reshape(-1, int(np.prod(shape[-2:])))[:, 3] = 1e4
    else:
        raise ValueError(regime)
    return torch.from_numpy(x.astype(np.float32)).to(F64)


def params(C_, seed, lo=0.5, hi=1.5):
    g = np.random.default_rng(seed + 991)
    f = lambda a, b: torch.from_numpy(g.uniform(a, b, C_).astype(np.float32)).to(F64)
    return f(lo, hi) * torch.from_numpy(g.choice([-1.0, 1.0], C_)), f(-0.5, 0.5), f(0.05, 0.45)     # gain, bias, PReLU slope


def prelu(v, s):
    return torch.where(v >= 0, v, s * v)


# ------------------------------------------------------------------------------------------------ float64 references + bounds
def affine_bound(x, mu, rs, g, b, sl, res, d_mu, e_rs):
    """y = PReLU((x - mu) rs g + b, sl) (+ res) and its fp32 bound (module docstring).  All broadcastable float64 tensors."""
    t3 = (x - mu) * rs * g
    z = t3 + b
    dz = (rs * g).abs() * (d_mu + U * (x - mu).abs()) + t3.abs() * (e_rs + 2 * U) + U * z.abs()
    p = prelu(z, sl) if sl is not None else z
    y = p + res if res is not None else p
    lip = torch.clamp(sl.abs(), min=1.0) if sl is not None else 1.0
    return y, lip * dz + U * p.abs() + U * y.abs()


def f64_sum_term(n, msq, var):
    return C_DOT * 2.0 ** -53 * math.sqrt(n) * msq / (var + EPS)


def ref_instnorm(x, g, b, sl, res=None, tlen=None, parts=None):
    """nn.InstanceNorm1d / 2d (affine, biased variance, eps 1e-5) + PReLU + residual on x [B][C][L][T]; ragged: the statistics of
    row b cover frames < tlen[b] of every line.  parts = frames per fp32 partial sum along a line (the epilogue forms: one (sum,
    sum of squares) pair per line and 32 frames) or None (fp64 statistics).  Returns y, bound, (mu, rs, d_mu, e_rs)."""
    B, C_, L, T = x.shape
    live = torch.ones((B, 1, 1, T), dtype=F64, device=x.device)
    if tlen is not None:
        live = (torch.arange(T, device=x.device)[None, :] < torch.as_tensor(tlen, device=x.device)[:, None]).to(F64)[:, None, None, :]
    xl = torch.where(live > 0, x, torch.zeros_like(x))
    n = live.sum((2, 3), keepdim=True) * L
    mu = xl.sum((2, 3), keepdim=True) / n
    msq = (xl * xl).sum((2, 3), keepdim=True) / n
    var = torch.clamp(msq - mu * mu, min=0.0)
    rs = 1.0 / torch.sqrt(var + EPS)
    if parts is None:
        d_mu = U * mu.abs()
        e_rs = U + f64_sum_term(float(n.max()), msq, var)
    else:
        pad = (-T) % parts
        xa = torch.nn.functional.pad(xl.abs(), (0, pad)).reshape(B, C_, L, -1, parts)
        cnt = torch.nn.functional.pad(live.expand(B, 1, L, T), (0, pad)).reshape(B, 1, L, -1, parts).sum(-1)
        dS = (C_DOT * U * torch.sqrt(cnt) * xa.sum(-1)).sum((2, 3), keepdim=False)[..., None, None]
        dQ = (C_DOT * U * torch.sqrt(cnt) * (xa * xa).sum(-1)).sum((2, 3), keepdim=False)[..., None, None]
        d_mu = dS / n + U * mu.abs()
        e_rs = (dQ / n + 2 * mu.abs() * dS / n) / (2 * (var + EPS)) + U
    sh = (1, C_, 1, 1)
    y, bd = affine_bound(x, mu, rs, g.view(sh), b.view(sh), sl.view(sh) if sl is not None else None, res, d_mu, e_rs)
    return y, bd, (mu, rs, d_mu, e_rs)


def cln_stats(v, first_live=0):
    """cumulative statistics over all C * F values of frames <= t (CTSNet_new/Step1_network.py:213-286), v [B][C][F][T]."""
    B, C_, F_, T = v.shape
    s = v.sum((1, 2)).cumsum(-1)
    q = (v * v).sum((1, 2)).cumsum(-1)
    cnt = (C_ * F_) * torch.arange(1, T + 1, dtype=F64, device=v.device)
    mu = s / cnt
    msq = q / cnt
    var = (q - 2 * mu * s) / cnt + mu * mu
    return mu[:, None, None, :], var[:, None, None, :], msq[:, None, None, :], cnt


def fir_apply(z, dz, fir):
    """y[t] = sum_k fir[k] z[t - (K - 1) + k] (causal, zero left pad) and its bound."""
    K = fir.numel()
    T = z.shape[-1]
    zp = torch.nn.functional.pad(z, (K - 1, 0))
    dp = torch.nn.functional.pad(dz, (K - 1, 0))
    y = torch.zeros_like(z)
    mag = torch.zeros_like(z)
    e = torch.zeros_like(z)
    for k in range(K):
        y += fir[k] * zp[..., k:k + T]
        mag += (fir[k] * zp[..., k:k + T]).abs()
        e += fir[k].abs() * dp[..., k:k + T]
    return y, e + C_DOT * U * math.sqrt(K) * mag


def ref_cln(x, gain, bias, pre=None, post=None, fir=None, res=None, parts_f32=False, Ein=None):
    """y = FIR( cLN( PReLU_pre(x) ) ) or PReLU_post( cLN(x) ) (+ res) on x [B][C][F][T]; statistics in fp64 (parts_f32: the per-
    (row, frame) sums over the channels are fp32, C terms each).  Ein: error field of x (the TCM block)."""
    B, C_, F_, T = x.shape
    sh = (1, C_, 1, 1)
    v = prelu(x, pre.view(sh)) if pre is not None else x
    dv = U * v.abs() if pre is not None else torch.zeros_like(v)
    if Ein is not None:
        dv = dv + (torch.clamp(pre.abs(), min=1.0).view(sh) if pre is not None else 1.0) * Ein
    mu, var, msq, cnt = cln_stats(v)
    var = torch.clamp(var, min=0.0)
    rs = 1.0 / torch.sqrt(var + EPS)
    d_mu = U * mu.abs()
    e_rs = U + C_DOT * 2.0 ** -53 * torch.sqrt(cnt) * msq / (var + EPS)
    if parts_f32:
        dS = (C_DOT * U * math.sqrt(C_) * v.abs().sum(1)).sum(1).cumsum(-1)[:, None, None, :]
        dQ = (C_DOT * U * math.sqrt(C_) * (v * v).sum(1)).sum(1).cumsum(-1)[:, None, None, :]
        d_mu = d_mu + dS / cnt
        e_rs = e_rs + (dQ / cnt + 2 * mu.abs() * dS / cnt) / (2 * (var + EPS))
    if Ein is not None:
        d_mu = d_mu + Q_PROP * torch.sqrt((dv * dv).sum((1, 2)).cumsum(-1))[:, None, None, :] / cnt
        e_rs = e_rs + Q_PROP * torch.sqrt((((v - mu) * dv) ** 2).sum((1, 2)).cumsum(-1))[:, None, None, :] / cnt / (var + EPS)
    z, dz = affine_bound(v, mu, rs, gain.view(sh), bias.view(sh), post.view(sh) if post is not None else None, None, d_mu, e_rs)
    dz = dz + (rs * gain.view(sh)).abs() * dv
    if fir is not None:
        z, dz = fir_apply(z, dz, fir)
    if res is not None:
        z = z + res
        dz = dz + U * z.abs()
    return z, dz


def ref_tcm_head(x, sl, g, b, fir=None, tlen=None, f32acc=False, Ein=None):
    """TCM branch head (CTSNet/Step1_network.py:161-176): FIR( InstanceNorm1d( PReLU(x) ) ) on x [B][C][T].  f32acc: the fused
    kernel's fp32 two-pass statistics.  Ein: error field of x."""
    B, C_, T = x.shape
    sh = (1, C_, 1)
    a = prelu(x, sl.view(sh))
    da = U * a.abs()
    if Ein is not None:
        da = da + torch.clamp(sl.abs(), min=1.0).view(sh) * Ein
    live = torch.ones((B, 1, T), dtype=F64, device=x.device)
    if tlen is not None:
        live = (torch.arange(T, device=x.device)[None, :] < torch.as_tensor(tlen, device=x.device)[:, None]).to(F64)[:, None, :]
    al = torch.where(live > 0, a, torch.zeros_like(a))
    n = live.sum(-1, keepdim=True)
    mu = al.sum(-1, keepdim=True) / n
    dev = torch.where(live > 0, a - mu, torch.zeros_like(a))
    var = (dev * dev).sum(-1, keepdim=True) / n
    rs = 1.0 / torch.sqrt(var + EPS)
    dl = torch.where(live > 0, da, torch.zeros_like(da))
    d_mu = U * mu.abs() + Q_PROP * torch.sqrt((dl * dl).sum(-1, keepdim=True)) / n
    d_var = 2 * Q_PROP * torch.sqrt(((dev * dl) ** 2).sum(-1, keepdim=True)) / n
    if f32acc:
        d_mu = d_mu + C_DOT * U * torch.sqrt(n) * al.abs().sum(-1, keepdim=True) / n
        # two passes: sum (a - mu')^2 / n = var + (mu' - mu)^2 exactly (the cross term sums to zero), plus the fp32 sum's rounding
        d_var = d_var + C_DOT * U * torch.sqrt(n) * var + 2 * U * var + d_mu * d_mu
    e_rs = U + d_var / (2 * (var + EPS))
    z, dz = affine_bound(a, mu, rs, g.view(sh), b.view(sh), None, None, d_mu, e_rs)
    dz = dz + (rs * g.view(sh)).abs() * da
    if fir is not None:
        z, dz = fir_apply(z, dz, fir)
    return z, dz


def ref_layernorm_cf(x, w, b, eps, res=None, post=0, slope=None):
    """nn.LayerNorm([F, C]) over the (C, F) plane of every (b, t) of x [B][C][F][T], weight / bias [F][C] (DPCRN/DPCRN.py:56-57);
    then swish (post = 1, Uformer/dsconv2d_cplx.py:56), scalar PReLU, + res."""
    B, C_, F_, T = x.shape
    n = C_ * F_
    mu = x.mean((1, 2), keepdim=True)
    msq = (x * x).mean((1, 2), keepdim=True)
    var = torch.clamp(msq - mu * mu, min=0.0)
    rs = 1.0 / torch.sqrt(var + eps)
    wt, bt = w.t()[None, :, :, None], b.t()[None, :, :, None]
    e_rs = U + C_DOT * 2.0 ** -53 * math.sqrt(n) * msq / (var + eps)
    z, dz = affine_bound(x, mu, rs, wt, bt, None, None, U * mu.abs(), e_rs)
    if post == 1:
        sg = torch.sigmoid(z)
        dz = 1.1 * dz + z.abs() * ACT_ULP + U * (z * sg).abs()        # |d/dz z sigmoid(z)| <= 1.0998
        z = z * sg
    if slope is not None:
        dz = max(1.0, abs(float(slope))) * dz + U * z.abs()
        z = torch.where(z >= 0, z, slope * z)
    if res is not None:
        z = z + res
        dz = dz + U * z.abs()
    return z, dz


def tcm_params(seed, ks, gated, cum, K, saturate=False):
    """The block's tensors in torch layout, default initialisation (Conv1d: U(+-1/sqrt(fan_in)); norms 1 / 0; PReLU 0.25; the shared
    FIR U(+-1/sqrt(K))), gains and slopes perturbed so that channels differ.  saturate: head gains x8 - the gate saturates."""
    g = np.random.default_rng(seed)
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).to(F64)
    cw = lambda co, ci, k: f32(g.uniform(-1, 1, (co, ci, k)) / math.sqrt(ci * k))
    p = {'w_in': cw(64, 256, 1), 'w_l': cw(64, 64, ks), 'w_out': cw(256, 64, 1)}
    heads = ('L', 'R', 'O') if gated else ('L', 'O')
    if gated:
        p['w_r'] = cw(64, 64, ks)
    for h in heads:
        p['g' + h] = f32((1.0 + 0.2 * g.standard_normal(64)) * (8.0 if saturate and h != 'O' else 1.0))
        p['b' + h] = f32(0.1 * g.standard_normal(64))
        p['s' + h] = f32(0.25 + 0.1 * g.uniform(-1, 1, 64))
        if K > 0 and h != 'O':
            p['fir' + h] = f32(g.uniform(-1, 1, K) / math.sqrt(K))
    return p


def dconv(v, dv, w, dil):
    """causal dilated Conv1d (left pad (ks - 1) dil): out[t] = sum_k w[:, :, k] v[t - (ks - 1 - k) dil], and its bound."""
    ks = w.shape[2]
    T = v.shape[-1]
    pad = (ks - 1) * dil
    vp, dp = torch.nn.functional.pad(v, (pad, 0)), torch.nn.functional.pad(dv, (pad, 0))
    y = torch.zeros((v.shape[0], w.shape[0], T), dtype=F64, device=v.device)
    mag, q = torch.zeros_like(y), torch.zeros_like(y)
    for k in range(ks):
        sl = slice(k * dil, k * dil + T)
        y += torch.einsum('oc,bct->bot', w[:, :, k], vp[..., sl])
        mag += torch.einsum('oc,bct->bot', w[:, :, k].abs(), vp[..., sl].abs())
        q += torch.einsum('oc,bct->bot', w[:, :, k] ** 2, dp[..., sl] ** 2)
    return y, C_DOT * U * math.sqrt(w.shape[1] * ks) * mag + Q_PROP * torch.sqrt(q)


def ref_tcm(x, p, dil, K, gated, cum, tlen=None, f32acc=True, fault=None):
    """The TCM / GLU block on x [B][256][T] (module docstring: `Glu`) and the bound of its fp32 form."""
    dev = x.device
    p = {k: v.to(dev) for k, v in p.items()}
    w1 = p['w_in'][:, :, 0]
    h = torch.einsum('oc,bct->bot', w1, x)
    Eh = C_DOT * U * math.sqrt(256) * torch.einsum('oc,bct->bot', w1.abs(), x.abs())

    def head(v, Ev, hd, fir):
        if cum:
            z, dz = ref_cln(v[:, :, None, :], p['g' + hd], p['b' + hd], pre=p['s' + hd], fir=fir, Ein=Ev[:, :, None, :])
            return z[:, :, 0, :], dz[:, :, 0, :]
        return ref_tcm_head(v, p['s' + hd], p['g' + hd], p['b' + hd], fir, tlen, f32acc, Ev)

    dl = dil + 1 if fault == 'dilation' else dil
    a, Ea = head(h, Eh, 'L', p.get('firL'))
    m, Em = dconv(a, Ea, p['w_l'], dl)
    if gated:
        r, Er = head(h, Eh, 'L' if fault == 'right_uses_left' else 'R', p.get('firL' if fault == 'right_uses_left' else 'firR'))
        gte, Eg = dconv(r, Er, p['w_r'], dl)
        sg = torch.sigmoid(gte)
        Esg = sg * (1 - sg) * Eg + ACT_ULP
        Em = sg * Em + m.abs() * Esg + U * (m * sg).abs()
        m = m * sg
    o, Eo = head(m, Em, 'O', None)
    w3 = p['w_out'][:, :, 0]
    y = torch.einsum('oc,bct->bot', w3, o)
    Ey = C_DOT * U * math.sqrt(64) * torch.einsum('oc,bct->bot', w3.abs(), o.abs()) + \
        Q_PROP * torch.sqrt(torch.einsum('oc,bct->bot', w3 ** 2, Eo ** 2))
    y = y + x
    return y, Ey + U * y.abs()


# ------------------------------------------------------------------------------------------------ fp32 evaluations (CPU side)
def f32(t):
    return t.detach().cpu().numpy().astype(np.float32)


def stats64(v32, axis, order):
    """sum and sum of squares in float64 of fp32 values, in one of two summation orders"""
    v = v32.astype(np.float64)
    if order == 1:
        v = np.flip(v, axis=axis[-1] if isinstance(axis, tuple) else axis)
    return v.sum(axis=axis, keepdims=True), (v * v).sum(axis=axis, keepdims=True)


def apply32(x, mu, rs, g, b, sl=None, res=None):
    o = (x - np.float32(1) * mu.astype(np.float32)) * rs.astype(np.float32) * g + b
    if sl is not None:
        o = np.where(o >= 0, o, sl * o)
    return o + res if res is not None else o


def eval32_instnorm(x, g, b, sl, res=None, tlen=None, parts=None, order=0, fault=None):
    """plain fp32 InstanceNorm + PReLU: fp64 statistics (or fp32 partial sums of `parts` frames, combined in fp64), fp32 apply"""
    x = f32(x)
    B, C_, L, T = x.shape
    sh = (1, C_, 1, 1)
    tl = np.full(B, T) if tlen is None or fault == 'stats_over_T' else np.asarray(tlen)
    live = (np.arange(T)[None, :] < tl[:, None])[:, None, None, :]
    xl = np.where(live, x, np.float32(0))
    n = (live.sum(-1, keepdims=True) * L).astype(np.float64)
    if parts is None and fault != 'f32_stats':
        s, q = stats64(xl, (2, 3), order)
    elif parts is None:
        s = np.cumsum(xl.reshape(B, C_, -1), axis=-1, dtype=np.float32)[..., -1].astype(np.float64)[..., None, None]
        q = np.cumsum((xl * xl).reshape(B, C_, -1), axis=-1, dtype=np.float32)[..., -1].astype(np.float64)[..., None, None]
    else:
        pad = (-T) % parts
        xp = np.pad(xl, ((0, 0),) * 3 + ((0, pad),)).reshape(B, C_, L, -1, parts)
        if order == 1:
            xp = xp[..., ::-1]
        ps = np.cumsum(xp, axis=-1, dtype=np.float32)[..., -1]
        pq = np.cumsum(xp * xp, axis=-1, dtype=np.float32)[..., -1]
        s, q = ps.astype(np.float64).sum((2, 3))[..., None, None], pq.astype(np.float64).sum((2, 3))[..., None, None]
    mu = s / n
    var = np.maximum(q / n - mu * mu, 0.0)
    rs = 1.0 / np.sqrt(var + EPS)
    if fault == 'neighbour_plane':
        mu, rs = np.roll(mu, 1, axis=1), np.roll(rs, 1, axis=1)
    y = apply32(x, mu, rs, f32(g).reshape(sh), f32(b).reshape(sh), f32(sl).reshape(sh) if sl is not None else None,
                None if res is None or fault == 'no_residual' else f32(res))
    if fault == 'head_skipped':
        y.reshape(B, C_, -1)[:, :, :3] = x.reshape(B, C_, -1)[:, :, :3]
    if fault == 'tail_skipped':
        y.reshape(B, C_, -1)[:, :, -3:] = x.reshape(B, C_, -1)[:, :, -3:]
    return y


def eval32_cln(x, gain, bias, pre=None, post=None, fir=None, res=None, order=0, fault=None, chunk=None, hist=0, parts_f32=False):
    """plain fp32 cumulative LayerNorm: fp64 sums over the rows of a frame, fp64 running totals, fp32 apply and FIR.
    chunk: frames per frame-online push (the carry faults act at its boundaries)."""
    x = f32(x)
    B, C_, F_, T = x.shape
    sh = (1, C_, 1, 1)
    v = np.where(x >= 0, x, f32(pre).reshape(sh) * x) if pre is not None else x
    if parts_f32:       # the `cstats` epilogue: per (row, frame) fp32 sums over the channels (either order), rows added in fp64
        vc = v[:, ::-1] if order == 1 else v
        s = np.cumsum(vc, axis=1, dtype=np.float32)[:, -1].astype(np.float64).sum(1)
        q = np.cumsum(vc * vc, axis=1, dtype=np.float32)[:, -1].astype(np.float64).sum(1)
    else:
        s, q = stats64(v, (1, 2), order)
        s, q = s[:, 0, 0, :], q[:, 0, 0, :]
    cs, cq = np.cumsum(s, -1), np.cumsum(q, -1)
    if fault == 'carry_reset' and chunk:
        for b0 in range(chunk, T, chunk):       # the totals restart at the second chunk boundary
            if b0 == 2 * chunk:
                cs[:, b0:] -= cs[:, b0 - 1:b0]
                cq[:, b0:] -= cq[:, b0 - 1:b0]
    if fault == 'history_live':                 # a (zero) history column before the stream start counted as a frame
        cnt = (C_ * F_) * (np.arange(1, T + 1, dtype=np.float64) + 1)
    elif fault == 'count_off_by_one':
        cnt = (C_ * F_) * np.arange(0, T, dtype=np.float64).clip(min=1)
    else:
        cnt = (C_ * F_) * np.arange(1, T + 1, dtype=np.float64)
    mu = cs / cnt
    var = (cq - 2 * mu * cs) / cnt + mu * mu
    rs = 1.0 / np.sqrt(var + EPS)
    mu, rs = mu[:, None, None, :], rs[:, None, None, :]
    if fault == 'wrapped_group':                # the first frame of every row normalised with frame T - 1's statistics
        mu, rs = np.broadcast_to(mu, x.shape).copy(), np.broadcast_to(rs, x.shape).copy()
        mu[..., 1:, 0], rs[..., 1:, 0] = mu[..., 1:, -1], rs[..., 1:, -1]
    z = apply32(v, mu, rs, f32(gain).reshape(sh), f32(bias).reshape(sh), f32(post).reshape(sh) if post is not None else None)
    if fir is not None:
        w = f32(fir)
        K = len(w)
        sft = 1 if fault == 'fir_shift' else 0
        zp = np.pad(z, ((0, 0),) * 3 + ((K - 1 + sft, 0),))
        y = np.zeros_like(z)
        ks = range(K) if order == 0 else range(K - 1, -1, -1)
        for k in ks:
            y = y + w[k] * zp[..., k:k + T]
        z = y
    if res is not None and fault != 'no_residual':
        z = z + f32(res)
    return z


def eval32_layernorm_cf(x, w, b, eps, res=None, post=0, slope=None, order=0):
    """plain fp32 LayerNorm over (C, F) per (b, t): fp64 statistics of the fp32 values (two orders), fp32 apply, libm swish"""
    x = f32(x)
    n = x.shape[1] * x.shape[2]
    s, q = stats64(x, (1, 2), order)
    mu = s / n
    rs = 1.0 / np.sqrt(np.maximum(q / n - mu * mu, 0.0) + eps)
    y = apply32(x, mu, rs, f32(w).T[None, :, :, None], f32(b).T[None, :, :, None])
    if post == 1:
        y = y * (np.float32(1) / (np.float32(1) + np.exp(-y)))
    if slope is not None:
        y = np.where(y >= 0, y, np.float32(float(slope)) * y)
    return y + f32(res) if res is not None else y


def eval32_finalize(x, g, b, sl, tlen=None, order=0):
    """the finalize quadruple from fp32 partial sums of 32 frames (either order), combined and folded in float64, stored in fp32"""
    x = f32(x)
    B, C_, L, T = x.shape
    tl = np.full(B, T) if tlen is None else np.asarray(tlen)
    live = (np.arange(T)[None, :] < tl[:, None])[:, None, None, :]
    xl = np.where(live, x, np.float32(0))
    xp = np.pad(xl, ((0, 0),) * 3 + ((0, (-T) % 32),)).reshape(B, C_, L, -1, 32)
    if order == 1:
        xp = xp[..., ::-1]
    s = np.cumsum(xp, axis=-1, dtype=np.float32)[..., -1].astype(np.float64).sum((2, 3))
    q = np.cumsum(xp * xp, axis=-1, dtype=np.float32)[..., -1].astype(np.float64).sum((2, 3))
    n = (tl * L).astype(np.float64)[:, None]
    mu = s / n
    sc = 1.0 / np.sqrt(np.maximum(q / n - mu * mu, 0.0) + EPS) * f32(g).astype(np.float64)[None, :]
    sh = f32(b).astype(np.float64)[None, :] - mu * sc
    sm = np.broadcast_to((f32(sl) - np.float32(1))[None, :], sc.shape)
    return np.stack((sc.astype(np.float32), sh.astype(np.float32), sm, (-sh / sc).astype(np.float32)), -1)


def eval32_f_nrm(x, p):
    """the two fused multiply-adds of instnorm_apply2_kernel: each an exact product and one rounding"""
    x, p = f32(x).astype(np.float64), p.astype(np.float64)
    t = (x * p[..., 0] + p[..., 1]).astype(np.float32).astype(np.float64)        # p [...][4] broadcasts against x
    return (np.minimum(t, 0.0) * p[..., 2] + t).astype(np.float32)


def eval32_tcm(x, p, dil, K, gated, cum, order=0):
    """plain fp32 TCM block: fp32 matmuls (two association orders), fp32 two-pass statistics, libm sigmoid"""
    q = {k: f32(v) for k, v in p.items()}
    x = f32(x)
    T = x.shape[-1]

    def mm(w, v):
        if order == 0:
            return np.einsum('oc,bct->bot', w, v, optimize=False).astype(np.float32)
        hlf = w.shape[1] // 2
        return (np.einsum('oc,bct->bot', w[:, hlf:], v[:, hlf:]) + np.einsum('oc,bct->bot', w[:, :hlf], v[:, :hlf])).astype(np.float32)

    def head(v, hd, fir):
        a = np.where(v >= 0, v, q['s' + hd][None, :, None] * v)
        if cum:
            y = eval32_cln(torch.from_numpy(a[:, :, None, :]), p['g' + hd], p['b' + hd], fir=p.get('fir' + hd) if fir else None, order=order)
            return y[:, :, 0, :]
        mu = a.mean(-1, keepdims=True, dtype=np.float32)
        var = ((a - mu) ** 2).mean(-1, keepdims=True, dtype=np.float32)
        z = (a - mu) * (np.float32(1) / np.sqrt(var + np.float32(EPS))) * q['g' + hd][None, :, None] + q['b' + hd][None, :, None]
        if fir and K > 0:
            zp = np.pad(z, ((0, 0), (0, 0), (K - 1, 0)))
            z = sum(q['fir' + hd][k] * zp[..., k:k + T] for k in range(K)).astype(np.float32)
        return z

    def conv(v, w):
        ks = w.shape[2]
        vp = np.pad(v, ((0, 0), (0, 0), ((ks - 1) * dil, 0)))
        return sum(mm(w[:, :, k], vp[..., k * dil:k * dil + T]) for k in range(ks)).astype(np.float32)

    h = mm(q['w_in'][:, :, 0], x)
    m = conv(head(h, 'L', True), q['w_l'])
    if gated:
        gt = conv(head(h, 'R', True), q['w_r'])
        m = m * (np.float32(1) / (np.float32(1) + np.exp(-gt)))
    return mm(q['w_out'][:, :, 0], head(m, 'O', False)) + x


# ------------------------------------------------------------------------------------------------ CPU tests
def rel(a, b):
    a, b = a.detach(), b.detach()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


def test_reference_matches_torch():
    """the float64 references against torch.nn and oracle/nnops, in float64, to 1e-12 relative"""
    from oracle import nnops
    tol = 1e-12
    for regime in ('normal', 'tiny'):
        x = make((2, 3, 5, 7), regime, 1)
        g, b, sl = params(3, 2)
        res = make((2, 3, 5, 7), 'normal', 3)
        y, _, _ = ref_instnorm(x, g, b, sl, res)
        n2 = torch.nn.InstanceNorm2d(3, affine=True).double()
        n2.weight.data, n2.bias.data = g.clone(), b.clone()
        want = torch.nn.functional.prelu(n2(x), sl) + res
        assert rel(y, want) < tol
        y1, _ = ref_tcm_head(x[:, :, 0, :], sl, g, b)
        n1 = torch.nn.InstanceNorm1d(3, affine=True).double()
        n1.weight.data, n1.bias.data = g.clone(), b.clone()
        assert rel(y1, n1(torch.nn.functional.prelu(x[:, :, 0, :], sl))) < tol
        # cumulative LayerNorm: oracle layout is [B, C, T, F]
        yc, _ = ref_cln(x, g, b, post=sl)
        oc = nnops.cumulative_layernorm(x.permute(0, 1, 3, 2).numpy(), g.numpy().reshape(1, 3, 1, 1), b.numpy().reshape(1, 3, 1, 1))
        oc = torch.from_numpy(nnops.prelu(oc, sl.numpy())).permute(0, 1, 3, 2)
        assert rel(yc, oc) < tol
        w, bb = make((5, 3), 'normal', 4), make((5, 3), 'normal', 5)
        yl, _ = ref_layernorm_cf(x, w, bb, 1e-5)
        want = torch.nn.functional.layer_norm(x.permute(0, 3, 2, 1), (5, 3), w, bb, 1e-5).permute(0, 3, 2, 1)
        assert rel(yl, want) < tol
    # the TCM block from oracle/nnops pieces
    for ks, gated, cum, K in ((5, True, False, 3), (3, False, True, 0), (5, True, True, 7)):
        p = tcm_params(7, ks, gated, cum, K)
        x = make((2, 256, 40), 'normal', 8)
        y, _ = ref_tcm(x, p, 2, K, gated, cum)
        xn = x.numpy()

        def head(v, hd, use_fir):
            a = nnops.prelu(v, p['s' + hd].numpy())
            if cum:
                z = nnops.cumulative_layernorm(a, p['g' + hd].numpy().reshape(1, -1, 1), p['b' + hd].numpy().reshape(1, -1, 1))
            else:
                z = nnops.instancenorm(a, p['g' + hd].numpy(), p['b' + hd].numpy())
            if use_fir and K > 0:
                z = nnops.conv1d(z.reshape(-1, 1, z.shape[-1]), p['fir' + hd].numpy().reshape(1, 1, K), padding=K - 1)[..., :z.shape[-1]].reshape(z.shape)
            return z

        def dc(v, w):
            pad = (w.shape[2] - 1) * 2
            return nnops.conv1d(np.pad(v, ((0, 0), (0, 0), (pad, 0))), w.numpy(), dilation=2)

        h = nnops.conv1d(xn, p['w_in'].numpy())
        m = dc(head(h, 'L', True), p['w_l'])
        if gated:
            m = m * nnops.sigmoid(dc(head(h, 'R', True), p['w_r']))
        want = nnops.conv1d(head(m, 'O', False), p['w_out'].numpy()) + xn
        assert rel(y, torch.from_numpy(want)) < tol


def worst(got, ref, bound):
    r = (torch.as_tensor(np.asarray(got, dtype=np.float64)) - ref.cpu()).abs() / bound.cpu()
    assert torch.isfinite(r).all(), 'non-finite output or zero bound'
    return float(r.max())


def test_bound_holds_for_fp32_and_catches_faults():
    """(i) plain fp32 evaluations in two summation orders stay inside the bound in every regime; (ii) each fault exceeds it >= 10x"""
    inside = {}
    for regime in REGIMES:
        for order in (0, 1):
            x = make((2, 3, 6, 45), regime, 11)
            g, b, sl = params(3, 12)
            res = make(x.shape, 'normal', 13)
            tlen = [45, 17]
            for parts in (None, 32):
                y, bd, _ = ref_instnorm(x, g, b, sl, res, tlen, parts)
                inside['instnorm', regime, order, parts] = worst(eval32_instnorm(x, g, b, sl, res, tlen, parts, order), y, bd)
            fir = make((5,), 'normal', 14) * 0.4
            for kw in (dict(post=sl, res=res), dict(pre=sl, fir=fir)):
                y, bd = ref_cln(x, g, b, **kw)
                inside['cln', regime, order, 'fir' in kw] = worst(eval32_cln(x, g, b, order=order, **kw), y, bd)
            # cLN from the fp32 channel partials of the `cstats` epilogue
            y, bd = ref_cln(x, g, b, post=sl, res=res, parts_f32=True)
            inside['cln_parts', regime, order] = worst(eval32_cln(x, g, b, post=sl, res=res, order=order, parts_f32=True), y, bd)
            # layernorm_cf: plain, swish, swish + PReLU + residual (the plane is (C, F): the regimes vary those axes)
            xl = make((2, 45, 3, 6), regime, 15).permute(0, 2, 3, 1).contiguous()
            wl, bl = make((6, 3), 'normal', 16), make((6, 3), 'normal', 17)
            for post, slope, rr in ((0, None, None), (1, None, None), (1, torch.tensor(0.2, dtype=F64), res.permute(0, 1, 2, 3)), (0, torch.tensor(1.7, dtype=F64), res)):
                y, bd = ref_layernorm_cf(xl, wl, bl, 1e-5, rr, post, slope)
                inside['layernorm_cf', regime, order, post, slope is not None] = worst(eval32_layernorm_cf(xl, wl, bl, 1e-5, rr, post, slope, order), y, bd)
            # the finalize quadruple, the folded elementwise pass on it, and f_nrm on given parameters
            _, _, stat = ref_instnorm(x, g, b, sl, None, tlen, 32)
            want, bnd = ref_finalize(g, b, sl, stat)
            nrm = eval32_finalize(x, g, b, sl, tlen, order)
            inside['finalize', regime, order] = worst(nrm, want, bnd)
            y, bd = folded_bound(x, g, b, sl, stat)
            inside['folded', regime, order] = worst(eval32_f_nrm(x, nrm[:, :, None, None, :]), y, bd)
            pn = torch.from_numpy(nrm.astype(np.float64))
            y, bd = f_nrm(x.reshape(2, 3, -1), pn)
            inside['f_nrm', regime, order] = worst(eval32_f_nrm(x.reshape(2, 3, -1), nrm[:, :, None, :]), y, bd)
            y, bd = ref_tcm_head(x[:, :, 0, :], sl, g, b, fir, tlen)
            a = prelu(x[:, :, 0, :], sl.view(1, 3, 1))
            e = eval32_instnorm(torch.from_numpy(f32(a)).to(F64)[:, :, None, :], g, b, None, None, tlen, None, order)
            zp = np.pad(e[:, :, 0, :], ((0, 0), (0, 0), (4, 0)))
            e = sum(f32(fir)[k] * zp[..., k:k + 45] for k in range(5))
            inside['tcm_head', regime, order] = worst(e, y, bd)
    for order in (0, 1):
        for ks, gated, cum, K, sat in ((5, True, False, 3, False), (3, False, True, 0, False), (5, True, True, 3, True)):
            p = tcm_params(21, ks, gated, cum, K, sat)
            x = make((2, 256, 48), 'normal', 22)
            y, bd = ref_tcm(x, p, 4, K, gated, cum)
            inside['tcm', ks, gated, cum, sat, order] = worst(eval32_tcm(x, p, 4, K, gated, cum, order), y, bd)
    top = max(inside.values())
    print('fp32 evaluations: worst error / bound %.3f at %s' % (top, max(inside, key=inside.get)))
    assert top <= 1.0, {k: v for k, v in inside.items() if v > 1.0}

    # (ii) faults, on the normal regime (the bound is tightest relative to the values there) unless the fault needs another
    x = make((2, 3, 6, 45), 'normal', 31)
    g, b, sl = params(3, 32)
    res = make(x.shape, 'normal', 33)
    tlen = [45, 17]
    fir = make((5,), 'normal', 34) * 0.4
    caught = {}
    y, bd, _ = ref_instnorm(x, g, b, sl, res, tlen)
    for f in ('stats_over_T', 'no_residual', 'neighbour_plane', 'head_skipped', 'tail_skipped'):
        caught[f] = worst(eval32_instnorm(x, g, b, sl, res, tlen, fault=f), y, bd)
    xo = make((2, 3, 64, 401), 'offset', 35)       # fp32 sums where the kernel documents fp64: visible where the mean dominates
    yo, bo, _ = ref_instnorm(xo, g, b, sl)
    caught['f32_stats'] = worst(eval32_instnorm(xo, g, b, sl, fault='f32_stats'), yo, bo)
    y, bd = ref_cln(x, g, b, post=sl, res=res)
    for f in ('count_off_by_one', 'wrapped_group', 'carry_reset', 'history_live'):
        caught[f] = worst(eval32_cln(x, g, b, post=sl, res=res, fault=f, chunk=8), y, bd)
    y, bd = ref_cln(x, g, b, pre=sl, fir=fir)
    caught['fir_shift'] = worst(eval32_cln(x, g, b, pre=sl, fir=fir, fault='fir_shift'), y, bd)
    p = tcm_params(41, 5, True, False, 3)
    xt = make((2, 256, 48), 'normal', 42)
    y, bd = ref_tcm(xt, p, 4, 3, True, False)
    for f in ('right_uses_left', 'dilation'):
        yf, _ = ref_tcm(xt, p, 4, 3, True, False, fault=f)
        caught[f] = worst(yf.numpy(), y, bd)
    low = min(caught, key=caught.get)
    print('faults: smallest error / bound %.1f (%s); all: %s' % (caught[low], low, {k: round(v, 1) for k, v in caught.items()}))
    assert caught[low] >= 10.0, caught


# ------------------------------------------------------------------------------------------------ GPU side
_lib = None
SIGS = {
    'np_norm2d_prelu': 'ipppppiiiippPiil', 'np_instnorm_prelu': 'pppppiiipip', 'np_instnorm_prelu_stats': 'ppppppiiiipip',
    'np_instnorm_finalize': 'pippppiiiip', 'np_instnorm_apply2': 'pppppiii', 'np_tcm_head': 'ippppppiiiipPiil',
    'np_cln': 'pppppppiiiiip', 'np_cln_parts': 'ppppppiiiip', 'np_layernorm_cf': 'pppppiiiifip', 'np_tcm_run': 'Pppiiip',
}
CT = {'i': C.c_int, 'p': C.c_void_p, 'P': C.c_void_p, 'l': C.c_long, 'f': C.c_float}


def lib():
    global _lib
    if _lib is None:
        assert os.path.exists(PROBE_LIB), 'libse_normprobe.so is missing: run build() (make -C csrc)'
        L = C.CDLL(PROBE_LIB)
        for name, sig in SIGS.items():
            getattr(L, name).argtypes = [CT[c] for c in sig]
            getattr(L, name).restype = C.c_int
        L.np_last_error.restype = C.c_char_p
        L.np_launch_kernel.restype = C.c_char_p
        L.np_launch_kernel.argtypes = [C.c_int]
        L.np_launch_get.argtypes = [C.c_int, C.POINTER(C.c_longlong), C.c_int]
        L.np_stream_create.restype = C.c_void_p
        L.np_stream_create.argtypes = [C.c_int]
        L.np_stream_destroy.argtypes = [C.c_void_p]
        L.np_sd_create.restype = C.c_void_p
        L.np_sd_destroy.argtypes = [C.c_void_p]
        L.np_sd_put.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_longlong), C.c_int]
        L.np_tcm_create.restype = C.c_void_p
        L.np_tcm_create.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int]
        L.np_tcm_destroy.argtypes = [C.c_void_p]
        _lib = L
    return _lib


def call(name, *args):
    L = lib()
    rc = getattr(L, name)(*[a.ptr if isinstance(a, Buf) else (a.data_ptr() if torch.is_tensor(a) else a) for a in args])
    assert rc == 0, '%s: %s' % (name, L.np_last_error().decode())
    out = []
    for i in range(L.np_launch_count()):
        v = (C.c_longlong * 13)()
        L.np_launch_get(i, v, 13)
        d = dict(zip(('W', 'VPT', 'KS', 'GATED', 'CUM', 'strip', 'ragged', 'c0', 'WP', 'grid', 'block', 'shmem', 'res'), list(v)))
        d['kernel'] = L.np_launch_kernel(i).decode()
        out.append(d)
    return out


def refused(name, *args):
    """a launcher's SE_CHECK refusal: host side, nothing launched"""
    L = lib()
    rc = getattr(L, name)(*[a.ptr if isinstance(a, Buf) else (a.data_ptr() if torch.is_tensor(a) else a) for a in args])
    return rc != 0 and L.np_launch_count() == 0


TAILS = (None, math.nan, 1e30)      # what the frames behind a ragged row's end hold (math.nan is one object: a dict key)
SLACK = 64      # floats before and after every buffer (a multiple of 4: the offset alone decides the 16 B alignment)


class Buf:
    """device buffer of n floats at `off` (0-3) floats past a 16 B boundary, NaN in the slack around it"""

    def __init__(self, n, off=0, src=None, like=None):
        self.n, self.off = n, off
        self.t = torch.full((n + 2 * SLACK + 4,), float('nan'), dtype=torch.float32, device='cuda') if like is None else like.t
        self.v = self.t[SLACK + off:SLACK + off + n]
        if src is not None:
            self.v.copy_(src.reshape(-1).to(torch.float32))

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * (SLACK + self.off)

    def untouched(self):
        return bool(torch.isnan(self.t[:SLACK + self.off]).all() and torch.isnan(self.t[SLACK + self.off + self.n:]).all())


def dev32(t):
    return t.to(torch.float32).cuda().contiguous()


def note(form, ratio, case):
    REACHED.add(form)
    if ratio > WORST.get(form, (0.0, ''))[0]:
        WORST[form] = (ratio, case)


def verify(case, forms, got, ref, bound, bufs=()):
    """elementwise check of one stored tensor + ownership of the buffers around it; prints the worst error / bound"""
    got = got.to(F64).reshape(ref.shape)
    assert torch.isfinite(got).all(), '%s: non-finite output' % case
    r = (got - ref).abs() / bound
    k = int(r.argmax())
    ratio = float(r.reshape(-1)[k])
    print('%s: worst error / bound %.3f at %s (got %.9g, want %.9g, bound %.3g) forms %s' %
          (case, ratio, tuple(int(i) for i in np.unravel_index(k, ref.shape)), float(got.reshape(-1)[k]), float(ref.reshape(-1)[k]),
           float(bound.reshape(-1)[k]), forms))
    for f in forms:
        note(f, ratio, case)
    for bf in bufs:
        assert bf.untouched(), '%s: wrote outside its output' % case
    assert ratio <= 1.0, '%s: error %.3f of the bound' % (case, ratio)
    return ratio


def kernels(recs):
    return [r['kernel'] for r in recs]


gpu = pytest.mark.gpu


# ---- InstanceNorm: stand-alone pass ------------------------------------------------------------------------------------------------
def apply_path(P, ox, oy, orr):
    """norm_apply_pass / instnorm_apply2_kernel / cln_apply_plane_kernel: 'vec' (16 B groups, head = (4 - start) & 3, tail) when
    every plane of input, output and residual starts at the same offset mod 4 floats, else 'scalar'"""
    same = all(o is None or o == ox for o in (oy, orr))
    return 'vec' if same else 'scalar'


INSTNORM_CASES = []
for _i, (_C, _L, _T) in enumerate([(1, 1, 7), (3, 5, 51), (2, 7, 101), (5, 4, 256), (3, 3, 401), (2, 161, 13), (7, 8, 641), (2, 16, 128),
                                   (3, 1, 2049)]):
    INSTNORM_CASES.append((_C, _L, _T, _i % 4, _i % 4, 'sep', REGIMES[_i % 5], None))
INSTNORM_CASES += [
    (3, 5, 51, 1, 1, 'alias', 'normal', None), (3, 5, 51, 2, 2, 'none', 'offset', None), (3, 5, 51, 3, 3, 'inplace', 'const', None),
    (3, 5, 51, 0, 1, 'sep', 'tiny', None), (3, 5, 51, 1, 1, 'sep_mis', 'outlier', None), (3, 5, 51, 2, 0, 'none', 'normal', None),
    (2, 9, 455, 0, 0, 'noslope', 'normal', None), (2, 9, 455, 1, 3, 'alias', 'offset', None),
    (3, 5, 51, 0, 0, 'sep', 'normal', 'one'), (3, 5, 51, 1, 1, 'alias', 'offset', 'Tm1'), (3, 5, 51, 2, 2, 'none', 'const', 'T'),
    (3, 6, 200, 3, 3, 'sep', 'tiny', 'mixed'), (3, 6, 200, 0, 2, 'sep', 'outlier', 'mixed'), (1, 7, 401, 0, 0, 'inplace', 'normal', 'mixed'),
]
for _r in REGIMES:
    INSTNORM_CASES.append((2, 4, 300, 0, 0, 'sep', _r, 'mixed'))


def tlens(kind, B, T):
    if kind is None:
        return None
    return {'one': [1] * B, 'Tm1': [max(T - 1, 1)] * B, 'T': [T] * B, 'mixed': [(1, max(T // 3, 1), max(T - 1, 1), T)[b % 4] for b in range(B)]}[kind]


@gpu
@pytest.mark.parametrize('Cc,L,T,ox,oy,resk,regime,rag', INSTNORM_CASES)
def test_instnorm_prelu(Cc, L, T, ox, oy, resk, regime, rag):
    """launch_instnorm_prelu through blocks.h norm2d_prelu (no slope: the launcher).  P = L * T odd / even, below 256 / 1024 and off
    the 1024 / 2048 multiples; every start alignment; 'sep_mis': the residual alone misaligned (scalar path)."""
    B = 4 if rag == 'mixed' else 3
    P = L * T
    x = make((B, Cc, L, T), regime, 100 + P)
    g, b, sl = params(Cc, P)
    if resk == 'noslope':
        sl = None
    tl = tlens(rag, B, T)
    res = make(x.shape, 'normal', 200 + P) if resk in ('sep', 'alias', 'sep_mis') else None
    y, bd, _ = ref_instnorm(x.cuda(), g.cuda(), b.cuda(), sl.cuda() if sl is not None else None, res.cuda() if res is not None else None, tl)
    orr = {'sep': oy, 'alias': oy, 'sep_mis': (oy + 1) % 4}.get(resk)
    path = apply_path(P, ox, oy if resk != 'inplace' else ox, orr)
    form = 'instnorm_prelu_ragged' if tl else 'instnorm_prelu'
    outs = {}
    gd, bd_, sld = dev32(g), dev32(b), (dev32(sl) if sl is not None else None)
    for tail in TAILS[:3 if tl else 1]:
        xin = x.clone()
        if tail is not None:
            for bi, n in enumerate(tl):
                xin[bi, :, :, n:] = tail
        xb = Buf(x.numel(), ox, xin)
        yb = xb if resk == 'inplace' else Buf(x.numel(), oy)
        rb = None
        if resk == 'alias':
            yb.v.copy_(res.reshape(-1).to(torch.float32))
            rb = yb
        elif res is not None:
            rb = Buf(x.numel(), orr, res)
        tld = torch.tensor(tl, dtype=torch.int32, device='cuda') if tl else None
        if sl is None:
            recs = call('np_instnorm_prelu', xb, yb, gd, bd_, None, B, Cc, P, rb, T, tld)
        else:
            recs = call('np_norm2d_prelu', 0, xb, yb, gd, bd_, sld, B, Cc, L, T, rb, tld, None, 0, 0, 0)
        assert kernels(recs) == [form] and recs[0]['grid'] == B * Cc and recs[0]['ragged'] == (1 if tl else 0)
        assert recs[0]['res'] == (1 if rb is not None else 0)
        out = yb.v.clone().reshape(x.shape)
        assert yb.untouched() and xb.untouched() and (rb is None or rb.untouched())
        if resk not in ('inplace', 'alias'):
            assert torch.equal(xb.v.reshape(x.shape).cpu().isnan(), xin.isnan()) and \
                torch.equal(xb.v.reshape(x.shape).cpu().nan_to_num(), xin.to(torch.float32).nan_to_num()), 'input changed'
        outs[tail] = out
    if tl:      # dead data: live frames bit-identical whatever the tails hold
        for bi, n in enumerate(tl):
            for tail in TAILS[1:]:
                assert torch.equal(outs[None][bi, :, :, :n], outs[tail][bi, :, :, :n]), 'a dead frame reached a live one'
    verify('instnorm %s C%d L%d T%d x%d y%d %s %s %s' % (form, Cc, L, T, ox, oy, resk, regime, rag), [form, form + ':' + path],
           outs[None], y, bd)


# ---- InstanceNorm from epilogue partial sums --------------------------------------------------------------------------------------
def epilogue_stats(x, tl=None):
    """(sum, sum of squares) per (b, c), output row and 32-frame block, in fp32, as the conv epilogue lays them out
    ([B][C][Fout][ceil(T / 32)][2]); ragged: cut at the row's own frame count"""
    B, C_, L, T = x.shape
    xf = x.to(torch.float32)
    if tl is not None:
        live = torch.arange(T, device=x.device)[None, :] < torch.as_tensor(tl, device=x.device)[:, None]
        xf = torch.where(live[:, None, None, :], xf, torch.zeros_like(xf))
    xp = torch.nn.functional.pad(xf, (0, (-T) % 32)).reshape(B, C_, L, -1, 32)
    s, q = torch.zeros_like(xp[..., 0]), torch.zeros_like(xp[..., 0])
    for k in range(32):                      # fp32, in frame order
        s = s + xp[..., k]
        q = q + xp[..., k] * xp[..., k]
    return torch.stack((s, q), -1).contiguous()


STATS_CASES = [(1, 1, 1, 20, 'normal', None, 0), (2, 3, 13, 32, 'offset', None, 1), (2, 2, 16, 100, 'const', None, 2),
               (1, 3, 43, 200, 'tiny', None, 3), (2, 2, 64, 401, 'outlier', None, 0), (4, 2, 13, 75, 'normal', 'mixed', 1),
               (4, 2, 5, 401, 'offset', 'mixed', 0), (2, 2, 161, 101, 'offset', None, 3), (2, 2, 8, 416, 'normal', None, 0)]


@gpu
@pytest.mark.parametrize('B,Cc,L,T,regime,rag,off', STATS_CASES)
def test_instnorm_from_partials(B, Cc, L, T, regime, rag, off):
    """launch_instnorm_prelu_stats, launch_instnorm_finalize + launch_instnorm_apply2 on fp32 partials made here in the epilogue's
    layout (nslot = L * ceil(T / 32): 1, 13, 64, 301, 322, ...).  The bound is the fp32-partials one; the printed `fp64-bound ratio`
    is the same error against the bound that assumes fp64 statistics (expected above 1 in the offset regime)."""
    x = make((B, Cc, L, T), regime, 300 + L * T).cuda()
    g, b, sl = (v.cuda() for v in params(Cc, L * T))
    res = make(x.shape, 'normal', 301).cuda()
    tl = tlens(rag, B, T)
    tld = torch.tensor(tl, dtype=torch.int32, device='cuda') if tl else None
    st = epilogue_stats(x, tl)
    nslot = L * ((T + 31) // 32)
    y, bd, (mu, rs, d_mu, e_rs) = ref_instnorm(x, g, b, sl, res, tl, parts=32)
    _, bd64, _ = ref_instnorm(x, g, b, sl, res, tl, parts=None)
    P = L * T
    xb, yb, rb = Buf(x.numel(), off, x), Buf(x.numel(), off), Buf(x.numel(), off, res)
    recs = call('np_instnorm_prelu_stats', xb, yb, dev32(g), dev32(b), dev32(sl), st, nslot, B, Cc, P, rb, T, tld)
    assert kernels(recs) == ['instnorm_prelu_stats'] and recs[0]['ragged'] == (1 if tl else 0) and recs[0]['res'] == 1
    got = yb.v.reshape(x.shape)
    if tl:      # dead data: the same partials (cut at the rows' own ends), NaN / 1e30 behind them in the plane
        for tail in TAILS[1:]:
            xd = x.clone()
            for bi, n in enumerate(tl):
                xd[bi, :, :, n:] = tail
            xb2, yb2 = Buf(x.numel(), off, xd), Buf(x.numel(), off)
            call('np_instnorm_prelu_stats', xb2, yb2, dev32(g), dev32(b), dev32(sl), st, nslot, B, Cc, P, rb, T, tld)
            for bi, n in enumerate(tl):
                assert torch.equal(yb2.v.reshape(x.shape)[bi, :, :, :n], got[bi, :, :, :n]), 'a dead frame reached a live one'
    print('  fp64-bound ratio %.2f' % float(((got.to(F64) - y).abs() / bd64).max()))
    verify('instnorm_prelu_stats B%d C%d L%d T%d %s %s nslot %d' % (B, Cc, L, T, regime, rag, nslot), ['instnorm_prelu_stats'], got, y, bd, [yb])
    # finalize: {scale, shift, slope - 1, x0}
    nrm = torch.full((B * Cc * 4 + 8,), float('nan'), dtype=torch.float32, device='cuda')
    recs = call('np_instnorm_finalize', st, nslot, dev32(g), dev32(b), dev32(sl), nrm, B, Cc, P, T, tld)
    assert kernels(recs) == ['instnorm_finalize'] and recs[0]['grid'] == (B * Cc + 3) // 4
    assert torch.isnan(nrm[B * Cc * 4:]).all()
    nr = nrm[:B * Cc * 4].reshape(B, Cc, 4).to(F64)
    want, bnd = ref_finalize(g, b, sl, (mu, rs, d_mu, e_rs))
    verify('instnorm_finalize B%d C%d %s %s' % (B, Cc, regime, rag), ['instnorm_finalize'], nr, want, bnd)


def ref_finalize(g, b, sl, stat):
    """launch_instnorm_finalize's {scale = rs g, shift = b - mu scale, slope - 1, x0 = -shift / scale} per (b, c) and their bounds;
    stat = (mu, rs, d_mu, e_rs) of ref_instnorm"""
    mu, rs, d_mu, e_rs = stat
    B, Cc = mu.shape[:2]
    mu2, rs2, dm, er = (v.reshape(B, Cc) for v in (mu, rs, d_mu.expand_as(mu), e_rs.expand_as(mu)))
    sc = rs2 * g.view(1, Cc)
    shf = b.view(1, Cc) - mu2 * sc
    d_sc = sc.abs() * (er + 2 * U)
    d_sh = U * shf.abs() + dm * sc.abs() + mu2.abs() * d_sc + U * (mu2 * sc).abs()
    x0 = -shf / sc
    sm = (sl - 1).view(1, Cc).expand(B, Cc)
    want = torch.stack((sc, shf, sm, x0), -1)
    bnd = torch.stack((d_sc, d_sh, U * sm.abs() + 1e-300, d_sh / sc.abs() + x0.abs() * (d_sc / sc.abs() + 2 * U)), -1)
    return want, bnd


def folded_bound(x, g, b, sl, stat):
    """PReLU(InstanceNorm(x)) evaluated in the folded form t = fma(x, scale, shift), y = fma(min(t, 0), slope - 1, t) with the
    finalize quadruple: the scale error multiplies |x| + |mu| instead of |x - mu| (the fold cancels mu scale against shift)"""
    want, bnd = ref_finalize(g, b, sl, stat)
    sc, shf, sm = (want[..., k][:, :, None, None] for k in range(3))
    d_sc, d_sh = bnd[..., 0][:, :, None, None], bnd[..., 1][:, :, None, None]
    t = x * sc + shf
    dt = x.abs() * d_sc + d_sh + U * t.abs()
    y = torch.clamp(t, max=0.0) * sm + t
    return y, (1 + sm.abs()) * dt + U * sm.abs() * t.abs() + 2 * U * y.abs()


def f_nrm(x, p):
    """gc_kernel NRM / instnorm_apply2_kernel: t = fma(x, scale, shift); fma(min(t, 0), slope - 1, t), and its bound"""
    sc, sh, sm = p[..., 0:1], p[..., 1:2], p[..., 2:3]        # x [B][C][P], p [B][C][4]
    t = x * sc + sh
    y = torch.clamp(t, max=0.0) * sm + t
    return y, 2 * U * ((x * sc).abs() + sh.abs()) * (1 + sm.abs()) + U * y.abs()


APPLY2_CASES = [(2, 3, 51, 0, 0, 0, 'y', 1.0), (2, 3, 51, 1, 1, 1, 'xa', 1.0), (2, 3, 51, 2, 2, 2, 'xb', 1e-6), (2, 3, 51, 3, 3, 3, 'one', 1.0),
                (2, 3, 51, 0, 1, 0, 'y', 1.0), (2, 3, 51, 0, 0, 2, 'y', 2e-6), (1, 2, 4099, 1, 1, 1, 'y', 1.0), (2, 2, 2, 3, 3, 3, 'y', 1.0),
                (2, 3, 1023, 0, 0, 0, 'one', 1.0), (1, 1, 5000, 2, 0, 2, 'one_mis', 1.0)]


@gpu
@pytest.mark.parametrize('B,Cc,P,oa,ob,oy,mode,gain', APPLY2_CASES)
def test_instnorm_apply2(B, Cc, P, oa, ob, oy, mode, gain):
    """y = f_a(xa) (+ f_b(xb)); y a buffer of its own or aliasing xa / xb; gains at the 1e-6 fold limit of blocks.h"""
    g = np.random.default_rng(P + oa)
    xa, xb_ = make((B, Cc, P), 'normal', 400 + P), make((B, Cc, P), 'offset', 401 + P)
    pa = torch.from_numpy(np.stack((g.uniform(0.5, 2, (B, Cc)) * gain, g.uniform(-1, 1, (B, Cc)), g.uniform(-0.9, -0.5, (B, Cc)),
                                    np.zeros((B, Cc))), -1).astype(np.float32)).to(F64)
    pb = torch.from_numpy(np.stack((g.uniform(0.01, 0.02, (B, Cc)), g.uniform(-1, 1, (B, Cc)), g.uniform(-0.9, -0.5, (B, Cc)),
                                    np.zeros((B, Cc))), -1).astype(np.float32)).to(F64)
    two = not mode.startswith('one')
    ya, ba = f_nrm(xa, pa)
    want, bd = ya, ba
    if two:
        yb2, bb2 = f_nrm(xb_, pb)
        want, bd = ya + yb2, ba + bb2 + U * (ya + yb2).abs()
    A, Bb = Buf(xa.numel(), oa, xa), (Buf(xa.numel(), ob, xb_) if two else None)
    Y = {'xa': A, 'xb': Bb}.get(mode) or Buf(xa.numel(), oy)
    recs = call('np_instnorm_apply2', A, dev32(pa), Bb, dev32(pb) if two else None, Y, B, Cc, P)
    assert kernels(recs) == ['instnorm_apply2']
    oyy = {'xa': oa, 'xb': ob}.get(mode, oy)
    path = 'vec' if (oyy == oa and (not two or ob == oa)) else 'scalar'
    verify('instnorm_apply2 P%d a%d b%d y%d %s' % (P, oa, ob, oyy, mode), ['instnorm_apply2', 'instnorm_apply2:' + path], Y.v.reshape(want.shape),
           want.cuda(), bd.cuda(), [Y, A] + ([Bb] if two else []))


@gpu
@pytest.mark.parametrize('rag', [None, 'mixed'])
def test_instnorm_partials_from_the_engines_conv(rag):
    """the hand-made partial-sum layout pinned: the same statistics buffer written by the engine's own conv epilogue (the gemmconv
    probe; ragged: cut at the rows' own frame counts), handed to launch_instnorm_prelu_stats and to launch_instnorm_finalize +
    launch_instnorm_apply2; reference = float64 InstanceNorm of the conv's stored output"""
    assert os.path.exists(GCPROBE_LIB)
    G = C.CDLL(GCPROBE_LIB)
    G.gcp_conv_create.restype = C.c_void_p
    G.gcp_conv_create.argtypes = [C.c_void_p] * 3 + [C.c_int] * 12
    G.gcp_run.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    G.gcp_destroy.argtypes = [C.c_void_p]
    G.gcp_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int]
    G.gcp_last_error.restype = C.c_char_p
    B, Cin, M, Fq, T = 4, 16, 64, 9, 101
    tl = tlens(rag, B, T)
    tld = torch.tensor(tl, dtype=torch.int32, device='cuda') if tl else None
    g = np.random.default_rng(5)
    w = (g.standard_normal((M, Cin, 3, 2)) / math.sqrt(Cin * 6)).astype(np.float32)
    bias = (5.0 + g.standard_normal(M)).astype(np.float32)          # planes whose mean dominates their spread
    h = G.gcp_conv_create(w.ctypes.data, bias.ctypes.data, None, M, Cin, 3, 2, 1, 1, 1, 1, 1, 0, 0, -1)
    assert h, G.gcp_last_error().decode()
    info = (C.c_int * 19)()
    G.gcp_info(h, 0, info, 19)
    assert info[4] == 1, 'this layer must support epilogue statistics'
    x = dev32(make((B, Cin, Fq, T), 'normal', 6))
    dst = torch.full((B, M, Fq, T), float('nan'), dtype=torch.float32, device='cuda')
    nslot = Fq * ((T + 31) // 32)
    st = torch.full((B, M, nslot, 2), float('nan'), dtype=torch.float32, device='cuda')
    rc = G.gcp_run(h, x.data_ptr(), None, None, None, Fq, dst.data_ptr(), M, Fq, B, T, T, st.data_ptr(), tld.data_ptr() if tl else None)
    assert rc == 0, G.gcp_last_error().decode()
    G.gcp_destroy(h)
    assert torch.isfinite(dst).all()
    want_st = epilogue_stats(dst.to(F64), tl).reshape(B, M, nslot, 2).to(F64)
    tot, wtot = st.to(F64).sum(2), want_st.sum(2)
    assert torch.isfinite(st).all()
    # each partial: at most 32 fp32 terms on either side (+ the squares' own rounding)
    assert ((tot - wtot).abs() <= 2 * (C_DOT * math.sqrt(32) + 1) * U * epilogue_stats(dst.to(F64).abs(), tl).reshape(B, M, nslot, 2).to(F64).sum(2)).all()
    gg, bb_, sl = (v.cuda() for v in params(M, 7))
    y, bd, stat = ref_instnorm(dst.to(F64), gg, bb_, sl, None, tl, parts=32)
    yb = Buf(dst.numel(), 0)
    recs = call('np_instnorm_prelu_stats', dst, yb, dev32(gg), dev32(bb_), dev32(sl), st, nslot, B, M, Fq * T, None, T, tld)
    assert kernels(recs) == ['instnorm_prelu_stats'] and recs[0]['ragged'] == (1 if tl else 0) and recs[0]['res'] == 0
    verify('instnorm_prelu_stats behind the conv epilogue %s' % rag, ['instnorm_prelu_stats:conv'], yb.v.reshape(dst.shape), y, bd, [yb])
    # the folded route: statistics -> {scale, shift, slope - 1, x0} -> the elementwise pass
    nrm = torch.full((B * M * 4,), float('nan'), dtype=torch.float32, device='cuda')
    recs = call('np_instnorm_finalize', st, nslot, dev32(gg), dev32(bb_), dev32(sl), nrm, B, M, Fq * T, T, tld)
    assert kernels(recs) == ['instnorm_finalize'] and recs[0]['ragged'] == (1 if tl else 0)
    want, bnd = ref_finalize(gg, bb_, sl, stat)
    verify('instnorm_finalize behind the conv epilogue %s' % rag, ['instnorm_finalize:conv'], nrm.reshape(B, M, 4), want, bnd)
    y2, bd2 = folded_bound(dst.to(F64), gg, bb_, sl, stat)
    assert float((y2 - y).abs().max()) <= 1e-9 * float(y.abs().max())          # the fold is the same function
    yb2 = Buf(dst.numel(), 0)
    recs = call('np_instnorm_apply2', dst, nrm, None, None, yb2, B, M, Fq * T)
    assert kernels(recs) == ['instnorm_apply2']
    verify('instnorm_apply2 behind the conv epilogue %s' % rag, ['instnorm_apply2:conv'], yb2.v.reshape(dst.shape), y2, bd2, [yb2])


# ---- TCM branch head -------------------------------------------------------------------------------------------------------------------
HEAD_CASES = [(T, K, rag, REGIMES[i % 5]) for i, (T, K, rag) in enumerate(
    [(1, 0, None), (31, 3, None), (255, 7, None), (256, 0, None), (257, 15, None), (511, 31, 'mixed'), (513, 63, None), (1501, 3, 'mixed'),
     (401, 63, 'mixed'), (64, 1, 'one'), (100, 7, 'Tm1'), (3, 7, None)])]


@gpu
@pytest.mark.parametrize('T,K,rag,regime', HEAD_CASES)
def test_tcm_head(T, K, rag, regime):
    """launch_tcm_head through blocks.h tcm_head (InstanceNorm flavour); FIR lengths 2 d - 1 of the models' dilations"""
    B, Cc = 4, 5
    x = make((B, Cc, 1, T), regime, 500 + T)[:, :, 0, :].cuda()
    g, b, sl = (v.cuda() for v in params(Cc, T))
    fir = (make((max(K, 1),), 'normal', 501 + T) / math.sqrt(max(K, 1))).cuda() if K else None
    tl = tlens(rag, B, T)
    tld = torch.tensor(tl, dtype=torch.int32, device='cuda') if tl else None
    y, bd = ref_tcm_head(x, sl, g, b, fir, tl)
    outs = {}
    for tail in TAILS[:3 if tl else 1]:
        xin = x.clone()
        if tail is not None:
            for bi, n in enumerate(tl):
                xin[bi, :, n:] = tail
        xb, yb = Buf(x.numel(), 1, xin), Buf(x.numel(), 3)
        recs = call('np_tcm_head', 0, xb, yb, dev32(sl), dev32(g), dev32(b), dev32(fir) if K else None, K, B, Cc, T, tld, None, 0, 0, 0)
        assert kernels(recs) == ['tcm_head'] and recs[0]['shmem'] == 4 * T and recs[0]['ragged'] == (1 if tl else 0)
        assert yb.untouched()
        outs[tail] = yb.v.clone().reshape(x.shape)
    if tl:
        for bi, n in enumerate(tl):
            for tail in TAILS[1:]:
                assert torch.equal(outs[None][bi, :, :n], outs[tail][bi, :, :n]), 'a dead frame reached a live one'
    verify('tcm_head T%d K%d %s %s' % (T, K, rag, regime), ['tcm_head'], outs[None], y, bd)


@gpu
def test_refusals_launch_nothing():
    """SE_CHECK limits are host side: T * 4 > 60000 (TCM head), T * 16 > 60000 (cLN scan), residual with a FIR"""
    t = torch.zeros(16, dtype=torch.float32, device='cuda')
    assert refused('np_tcm_head', 0, t, t, t, t, t, None, 0, 1, 1, 15001, None, None, 0, 0, 0)
    assert refused('np_cln', t, t, t, t, None, None, None, 0, 1, 1, 1, 3751, None)
    assert refused('np_cln', t, t, t, t, None, None, t, 3, 1, 1, 1, 8, t)


# ---- offline cumulative LayerNorm ------------------------------------------------------------------------------------------------------
def cln_forms(K, pre, res, plane_on=True):
    apply_ = 'cln_apply_plane' if (K <= 0 and not pre and (plane_on or res)) else 'cln_apply'
    return ['cln_stats', 'cln_scan', apply_]


CLN_T = [1, 2, 3, 5, 63, 64, 65, 401, 1023, 1025, 1876, 3750]
CLN_CASES = []
for _i, _T in enumerate(CLN_T):
    _big = _T > 1100
    CLN_CASES.append((2, 3 if _big else 5, 1 if _i % 3 == 0 else (2 if _big else 7), _T, 'post', _i % 4, REGIMES[_i % 5]))
    CLN_CASES.append((1, 4, 1, _T, 'prefir', 0, REGIMES[(_i + 1) % 5]))
    CLN_CASES.append((2, 2, 3, _T, 'res', (_i + 1) % 4, REGIMES[(_i + 2) % 5]))
CLN_CASES += [(1, 16, 40, 101, 'post', 0, 'normal'), (1, 64, 9, 33, 'res_alias', 1, 'offset'), (2, 3, 5, 401, 'res_mis', 2, 'normal'),
              (2, 5, 7, 3, 'res_alias', 3, 'outlier'), (1, 3, 171, 401, 'pre2d', 0, 'normal'),
              (1, 1, 1100, 3, 'post', 1, 'normal'), (1, 1, 1600, 2, 'res', 0, 'offset'), (1, 2, 1600, 1, 'post', 2, 'normal'),
              (1, 2, 1100, 3, 'res_mis', 0, 'tiny')]


def run_cln_case(B, Cc, Fq, T, kind, off, regime, plane_on=True):
    x = make((B, Cc, Fq, T), regime, 600 + T + Fq).cuda()
    g, b, sl = (v.cuda() for v in params(Cc, T))
    K = 0
    pre = post = fir = res = None
    if kind in ('prefir', 'pre2d'):
        pre = sl
        K = 0 if kind == 'pre2d' else (5 if T > 2 else 2)
        fir = (make((K,), 'normal', 601) / 2).cuda() if K else None
    else:
        post = sl
    if kind.startswith('res'):
        res = make(x.shape, 'normal', 602).cuda()
    y, bd = ref_cln(x, g, b, pre, post, fir, res)
    xb = Buf(x.numel(), off, x)
    yb = Buf(x.numel(), off)
    rb = None
    if kind == 'res_alias':
        yb.v.copy_(res.reshape(-1).to(torch.float32))
        rb = yb
    elif res is not None:
        rb = Buf(x.numel(), (off + 1) % 4 if kind == 'res_mis' else off, res)
    recs = call('np_cln', xb, yb, dev32(g), dev32(b), dev32(pre) if pre is not None else None, dev32(post) if post is not None else None,
                dev32(fir) if fir is not None else None, K, B, Cc, Fq, T, rb)
    want = cln_forms(K, pre is not None, res is not None, plane_on)
    assert kernels(recs) == want, (kernels(recs), want)
    assert recs[0]['grid'] == ((T + 63) // 64) * B and recs[1]['shmem'] == 16 * T and recs[2]['res'] == (1 if res is not None else 0)
    forms = list(want)
    if want[2] == 'cln_apply_plane':
        forms.append('cln_apply_plane:' + ('scalar' if kind == 'res_mis' else 'vec') + (':T>1024' if T > 1024 else ':T<4' if T < 4 else ''))
        if T < 4 and Fq * T > 3072:      # the unrolled body and the incremental frame tracking (step1 = 1024 % T) run too
            forms.append(forms[-1] + ':swept')
    forms.append('cln_stats:' + ('unrolled' if Cc * Fq > 4 * (NU - 1) else 'remainder'))      # 4 row groups x NU rows in flight
    verify('cln B%d C%d F%d T%d %s off%d %s' % (B, Cc, Fq, T, kind, off, regime), forms, yb.v.reshape(x.shape), y, bd, [yb, xb])
    if T >= 3 and kind != 'res_alias':      # dead data: the norm is causal, so frames behind a row's end must not reach the ones before it
        n = T - T // 3
        first = yb.v.clone().reshape(x.shape)[..., :n]
        for tail in TAILS[1:]:
            xd = x.clone()
            xd[..., n:] = tail
            xb2, yb2 = Buf(x.numel(), off, xd), Buf(x.numel(), off)
            call('np_cln', xb2, yb2, dev32(g), dev32(b), dev32(pre) if pre is not None else None, dev32(post) if post is not None else None,
                 dev32(fir) if fir is not None else None, K, B, Cc, Fq, T, rb)
            assert torch.equal(yb2.v.reshape(x.shape)[..., :n], first), 'a dead frame reached a live one'


@gpu
@pytest.mark.parametrize('B,Cc,Fq,T,kind,off,regime', CLN_CASES)
def test_cln_offline(B, Cc, Fq, T, kind, off, regime):
    """launch_cln offline: 1-D (F = 1) and 2-D, post-slope (plane apply), pre-slope + FIR (row apply), residual separate / aliasing y
    / misaligned, T from 1 to the LDS limit 3750, rows C * F either side of the statistics pass's unrolled body (4 row groups x NU = 8 rows in flight)"""
    run_cln_case(B, Cc, Fq, T, kind, off, regime)


PARTS_CASES = [(F_, T, REGIMES[(i + j) % 5]) for i, F_ in enumerate((1, 7, 8, 9, 161)) for j, T in enumerate(CLN_T)]


@gpu
@pytest.mark.parametrize('Fq,T,regime', PARTS_CASES)
def test_cln_parts(Fq, T, regime):
    """launch_cln_parts: per-(row, frame) fp32 sums over the channels as the `cstats` epilogue lays them out (parts [B][F][T][2])"""
    B, Cc = 2, (3 if Fq * T > 100000 else 6)
    x = make((B, Cc, Fq, T), regime, 700 + T + Fq).cuda()
    g, b, sl = (v.cuda() for v in params(Cc, T + Fq))
    res = make(x.shape, 'normal', 701).cuda()
    xf = x.to(torch.float32)
    s, q = torch.zeros_like(xf[:, 0]), torch.zeros_like(xf[:, 0])
    for c in range(Cc):
        s = s + xf[:, c]
        q = q + xf[:, c] * xf[:, c]
    parts = torch.stack((s, q), -1).contiguous()
    y, bd = ref_cln(x, g, b, None, sl, None, res, parts_f32=True)
    _, bd64 = ref_cln(x, g, b, None, sl, None, res)
    xb, yb, rb = Buf(x.numel(), 2, x), Buf(x.numel(), 2), Buf(x.numel(), 2, res)
    recs = call('np_cln_parts', xb, yb, dev32(g), dev32(b), dev32(sl), parts, B, Cc, Fq, T, rb)
    assert kernels(recs) == ['cln_scan_parts', 'cln_apply_plane'] and recs[1]['res'] == 1
    got = yb.v.reshape(x.shape)
    print('  fp64-bound ratio %.2f' % float(((got.to(F64) - y).abs() / bd64).max()))
    verify('cln_parts F%d T%d %s' % (Fq, T, regime), ['cln_scan_parts'], got, y, bd, [yb])


# ---- frame-online cumulative LayerNorm -------------------------------------------------------------------------------------------------
def stream_form(n, R, Cc, K, pre, W, T, res_on=True):
    """mirror of launch_cln's frame-online branch; W = T - c0"""
    if K <= 0 and not pre and n <= 2 and R <= 256 * 41 and Cc <= 256:
        return ['cln_window_reg']
    if R * W <= 32768 and (K <= 0 or R * W * 4 + T * 24 <= 60000):
        return ['cln_window']
    return ['cln_stats', 'cln_scan', 'cln_apply']


STREAM_CASES = [((1,), 4, 7, 'post', 0), ((2,), 4, 7, 'post', 0), ((1,), 64, 161, 'res', 0), ((2,), 64, 161, 'res', 0), ((1,), 66, 161, 'post', 0),
                ((3,), 4, 7, 'post', 0), ((16,), 8, 20, 'res', 0), ((64,), 8, 20, 'post', 0), ((64,), 64, 33, 'post', 0),
                ((1, 2, 3, 16, 1, 64, 5), 6, 5, 'res', 0), ((1,), 5, 1, 'prefir', 5), ((2,), 5, 1, 'prefir', 3), ((3,), 64, 1, 'prefir', 15),
                ((16,), 64, 1, 'prefir', 63), ((64,), 64, 1, 'prefir', 31), ((1, 2, 3, 16, 64), 64, 1, 'prefir', 7), ((64,), 600, 1, 'prefir', 7),
                ((1,), 4, 7, 'res', 0), ((2,), 8, 9, 'post', 0), ((5,), 4, 7, 'res', 0), ((7,), 6, 3, 'post', 0), ((64,), 64, 33, 'res', 0),
                ((64,), 64, 33, 'post', 0), ((64,), 64, 33, 'post', 0)]


def run_stream_case(widths, Cc, Fq, kind, K, res_on=True, regime='normal'):
    B, Ttot, Hmin = 2, 100, 8
    H = max(Hmin, K - 1 if K else 0)
    x = make((B, Cc, Fq, Ttot), regime, 800 + Cc + Fq + K).cuda()
    g, b, sl = (v.cuda() for v in params(Cc, Fq))
    fir = (make((K,), 'normal', 801) / math.sqrt(K)).cuda() if K else None
    res = make(x.shape, 'normal', 802).cuda() if kind == 'res' else None
    if kind == 'prefir':
        y, bd = ref_cln(x, g, b, sl, None, fir)
    else:
        y, bd = ref_cln(x, g, b, None, sl, None, res)
    L = lib()
    st = L.np_stream_create(B)
    assert st
    got = torch.full(x.shape, float('nan'), dtype=torch.float32, device='cuda')
    t0, i, forms, added = 0, 0, set(), False
    gd, bdv, sld, fird = dev32(g), dev32(b), dev32(sl), dev32(fir) if K else None
    try:
        while t0 < Ttot:
            n = min(widths[i % len(widths)], Ttot - t0)
            i += 1
            T = H + n
            win = torch.full((B, Cc, Fq, T), float('nan'), dtype=torch.float32, device='cuda')      # history columns: whatever was there
            win[..., H:] = x[..., t0:t0 + n].to(torch.float32)
            xb, yb = Buf(win.numel(), 0, win), Buf(win.numel(), 0)
            rb = None
            if res is not None:
                rw = torch.full_like(win, float('nan'))
                rw[..., H:] = res[..., t0:t0 + n].to(torch.float32)
                rb = Buf(win.numel(), 0, rw)
            if kind == 'prefir':          # (the models' FIR heads are 1-D: blocks.h tcm_head)
                assert Fq == 1
                recs = call('np_tcm_head', 1, xb, yb, sld, gd, bdv, fird, K, B, Cc, T, None, st, H, n, t0)
            else:
                recs = call('np_norm2d_prelu', 1, xb, yb, gd, bdv, sld, B, Cc, Fq, T, rb, None, st, H, n, t0)
            c0 = H - (K - 1 if K else 0)
            want = stream_form(n, Cc * Fq, Cc, K, kind == 'prefir', T - c0, T, res_on)
            in_kernel = res is not None and res_on and want == ['cln_window_reg']      # blocks.h norm2d_prelu / cln_stream_takes_res
            full = want + (['add'] if res is not None and not in_kernel else [])
            assert kernels(recs) == full, (kernels(recs), full, n)
            assert recs[0]['c0'] == c0 and [r['res'] for r in recs] == [1 if in_kernel else 0] + [0] * (len(full) - 1)
            if want == ['cln_window_reg']:
                assert recs[0]['W'] == n and recs[0]['VPT'] == 41 * n
            forms.add(want[0] + ('<%d>' % n if want[0] == 'cln_window_reg' else ''))
            added = added or 'add' in kernels(recs)          # from the launch record
            yw = yb.v.reshape(win.shape)
            assert yb.untouched() and torch.isnan(yw[..., :H]).all(), 'the chunk wrote outside its new frames'
            got[..., t0:t0 + n] = yw[..., H:]
            t0 += n
    finally:
        L.np_stream_destroy(st)
    tags = ['stream:' + f for f in forms] + (['stream:launch_add'] if added else [])
    verify('stream cln widths %s C%d F%d %s K%d' % (widths, Cc, Fq, kind, K), tags, got, y, bd)


@gpu
@pytest.mark.parametrize('widths,Cc,Fq,kind,K,regime', [c + (REGIMES[(i + 1) % 5],) for i, c in enumerate(STREAM_CASES)])
def test_cln_frame_online(widths, Cc, Fq, kind, K, regime):
    """a 100-frame utterance pushed in chunks through StreamSlots / StreamScope (8 history columns, more under a long FIR: the first
    chunks' history lies before the stream start, tg0 < 0, later ones' inside it), every chunk's new frames against the float64
    whole-utterance cLN; R = C * F either side of 256 * 41; residual in the register form or by launch_add (blocks.h)"""
    run_stream_case(widths, Cc, Fq, kind, K, regime=regime)


# ---- frame-online cumulative LayerNorm, late in a stream ---------------------------------------------------------------------------------
# the chunk's last frame: 2^24 + 3, and the last frame a 320 / 160 stream (the cLN networks) reaches at its sample limit, csrc/stream_window.h
LATE_FRAMES = (2 ** 24 + 3, (2 ** 31 - 1 - (320 + 32 * 160)) // 160)
# (n, C, F, kind, regime): the register form for n = 1 and n = 2 (the second with the residual in the kernel, R just below 256 * 41), the
# window form with and without launch_add, the three-launch form (R * W > 32768); 'offset': mean 100 x the spread, the cancelling regime
LATE_CASES = [(1, 4, 7, 'post', 'normal'), (2, 64, 161, 'res', 'offset'), (5, 4, 7, 'res', 'offset'), (16, 8, 20, 'post', 'normal'),
              (64, 64, 33, 'post', 'offset')]


def ref_cln_late(x, g, b, sl, res, t0, carry):
    """cLN of a chunk x [B][C][F][n] whose first frame is the row's frame t0, carried sums carry [B][2] (float64, an input: exact on both
    sides) -> y, its bound (ref_cln's: the statistics are float64 in the kernels, divisor R (t + 1) included, so no rounding is added
    for the late index; its float64 term counts the R n additions of this chunk and the four operations of the variance, not every term
    since frame 0, which the exact carry stands for), and the sums after the chunk with their bound: every one of the R n + 1 additions rounds once in float64"""
    B, C_, F_, n = x.shape
    sh = (1, C_, 1, 1)
    R = C_ * F_
    s = carry[:, 0:1] + x.sum((1, 2)).cumsum(-1)
    q = carry[:, 1:2] + (x * x).sum((1, 2)).cumsum(-1)
    cnt = R * (t0 + torch.arange(1, n + 1, dtype=F64, device=x.device))
    mu, msq = s / cnt, q / cnt
    var = torch.clamp((q - 2 * mu * s) / cnt + mu * mu, min=0.0)
    mu, var, msq = mu[:, None, None, :], var[:, None, None, :], msq[:, None, None, :]
    rs = 1.0 / torch.sqrt(var + EPS)
    z, dz = affine_bound(x, mu, rs, g.view(sh), b.view(sh), sl.view(sh), None, U * mu.abs(), U + C_DOT * 2.0 ** -53 * math.sqrt(R * n + 4) * msq / (var + EPS))
    if res is not None:
        z = z + res
        dz = dz + U * z.abs()
    sums = torch.stack([s[:, -1], q[:, -1]], 1)
    sbd = (R * n + 2) * 2.0 ** -53 * torch.stack([carry[:, 0].abs() + x.abs().sum((1, 2, 3)), carry[:, 1] + (x * x).sum((1, 2, 3))], 1)
    return z, dz, sums, sbd


@gpu
@pytest.mark.parametrize('n,Cc,Fq,kind,regime', LATE_CASES)
@pytest.mark.parametrize('t_last', LATE_FRAMES)
def test_cln_frame_online_late(t_last, n, Cc, Fq, kind, regime):
    """launch_cln's frame-online forms at a late frame index of their own (the engine-level late streams keep a row's own index small through
    its origin): one chunk of n frames ending at frame 2^24 + 3 / at the last reachable frame.  The carried sums are those of a stationary
    signal - t0 frames with the chunk's own mean and mean square, formed in float64 - and are put into the stream's state slot in place of
    the sums a first chunk left there.  Outputs against float64 under the bound of the frame-online cases above; the sums the chunk leaves
    against float64 too."""
    B, H = 2, 8
    t0 = t_last - (n - 1)
    R = Cc * Fq
    x = make((B, Cc, Fq, n), regime, 900 + Cc + Fq + n).cuda()
    g, b, sl = (v.cuda() for v in params(Cc, Fq + 1))
    res = make(x.shape, 'normal', 902).cuda() if kind == 'res' else None
    carry = torch.stack([t0 * R * x.mean((1, 2, 3)), t0 * R * (x * x).mean((1, 2, 3))], 1)          # [B][2] float64
    y, bd, sums, sbd = ref_cln_late(x, g, b, sl, res, t0, carry)
    L = lib()
    L.np_slot_read.argtypes = L.np_slot_write.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong]
    st = L.np_stream_create(B)
    assert st
    gd, bdv, sld = dev32(g), dev32(b), dev32(sl)
    T = H + n
    want = stream_form(n, R, Cc, 0, False, n, T)
    in_kernel = res is not None and want == ['cln_window_reg']
    full = want + (['add'] if res is not None and not in_kernel else [])
    try:
        for first, at in ((True, 0), (False, t0)):      # a first chunk makes the slot; then the late chunk on the seeded sums
            win = torch.full((B, Cc, Fq, T), float('nan'), dtype=torch.float32, device='cuda')
            win[..., H:] = x.to(torch.float32)
            xb, yb = Buf(win.numel(), 0, win), Buf(win.numel(), 0)
            rb = None
            if res is not None:
                rw = torch.full_like(win, float('nan'))
                rw[..., H:] = res.to(torch.float32)
                rb = Buf(win.numel(), 0, rw)
            recs = call('np_norm2d_prelu', 1, xb, yb, gd, bdv, sld, B, Cc, Fq, T, rb, None, st, H, n, at)
            assert kernels(recs) == full, (kernels(recs), full)
            if first:
                host = np.ascontiguousarray(carry.cpu().numpy(), np.float64)
                assert L.np_slot_write(st, 0, host.ctypes.data, host.nbytes) == 0, L.np_last_error().decode()
        left = np.zeros((B, 2), np.float64)
        assert L.np_slot_read(st, 0, left.ctypes.data, left.nbytes) == 0, L.np_last_error().decode()
    finally:
        L.np_stream_destroy(st)
    yw = yb.v.reshape(win.shape)
    assert yb.untouched() and torch.isnan(yw[..., :H]).all(), 'the chunk wrote outside its new frames'
    case = 'late cln t0 %d n%d C%d F%d %s %s' % (t0, n, Cc, Fq, kind, regime)
    tags = ['stream:' + want[0] + ('<%d>' % n if want[0] == 'cln_window_reg' else '')] + (['stream:launch_add'] if 'add' in full else [])
    verify(case, tags, yw[..., H:], y, bd)
    verify(case + ' carried sums', [], torch.from_numpy(left).cuda(), sums, sbd)


# ---- layernorm_cf ----------------------------------------------------------------------------------------------------------------------
LN_CASES = [(T, C_, F_, post, pr, rs_, REGIMES[i % 5]) for i, (T, C_, F_, post, pr, rs_) in enumerate(
    [(1, 3, 1, 0, False, False), (63, 2, 2, 0, False, True), (64, 31, 1, 1, False, False), (65, 4, 8, 0, True, True), (401, 3, 11, 1, True, True),
     (64, 257, 1, 0, False, True), (65, 16, 50, 1, False, True), (63, 8, 129, 0, True, False), (401, 1, 32, 0, False, True), (5, 128, 50, 0, False, True)])]


@gpu
@pytest.mark.parametrize('T,Cc,Fq,post,pr,rs_,regime', LN_CASES)
def test_layernorm_cf(T, Cc, Fq, post, pr, rs_, regime):
    """launch_layernorm_cf: C * F in {3, 4, 31, 32, 33, 257, 800, 1032 (Uformer), 6400 (DPCRN)} across the 8-deep body and its
    remainder, T either side of the 64-frame block, swish / PReLU / residual, eps 1e-5 as the models pass it"""
    B = 2
    # the regimes' plane is (C, F) here: put the varied axes there
    x = make((B, T, Cc, Fq), regime, 900 + T).permute(0, 2, 3, 1).contiguous().cuda()
    w, bb_ = make((Fq, Cc), 'normal', 901).cuda(), make((Fq, Cc), 'normal', 902).cuda()
    res = make(x.shape, 'normal', 903).cuda() if rs_ else None
    slope = make((1,), 'normal', 904).abs().cuda() * 0.3 if pr else None
    y, bd = ref_layernorm_cf(x, w, bb_, 1e-5, res, post, slope)
    xb, yb = Buf(x.numel(), 1, x), Buf(x.numel(), 2)
    rb = Buf(x.numel(), 3, res) if rs_ else None
    recs = call('np_layernorm_cf', xb, rb, dev32(w), dev32(bb_), yb, B, Cc, Fq, T, 1e-5, post, dev32(slope) if pr else None)
    assert kernels(recs) == ['layernorm_cf'] and recs[0]['grid'] == ((T + 63) // 64) * B
    verify('layernorm_cf T%d C%d F%d post%d prelu%d res%d %s' % (T, Cc, Fq, post, pr, rs_, regime), ['layernorm_cf'], yb.v.reshape(x.shape), y, bd, [yb])


# ---- TCM block -------------------------------------------------------------------------------------------------------------------------
def tcm_block(p, dil, K, ks, gated, cum):
    """the block's state dict in torch layout -> TcmBlock::load with the key names the models use"""
    L = lib()
    sd = L.np_sd_create()
    keep = []

    def put(key, t, shape):
        a = np.ascontiguousarray(t.numpy().astype(np.float32))
        keep.append(a)
        L.np_sd_put(sd, ('blk.' + key).encode(), a.ctypes.data, (C.c_longlong * len(shape))(*shape), len(shape))

    nk = 'gain' if cum else 'weight'
    put('in_conv.weight', p['w_in'], (64, 256, 1))
    put('out_conv.2.weight', p['w_out'], (256, 64, 1))
    for hd, name in (('L', 'left_conv'), ('R', 'right_conv')) if gated else (('L', 'left_conv'),):
        put(name + '.0.weight', p['s' + hd], (64,))
        put(name + '.1.' + nk, p['g' + hd], (64,))
        put(name + '.1.bias', p['b' + hd], (64,))
        if K > 0:
            put(name + '.2.weight', p['fir' + hd], (1, 1, K))
        put(name + ('.4' if K > 0 else '.3') + '.weight', p['w_l' if hd == 'L' else 'w_r'], (64, 64, ks))
    put('out_conv.0.weight', p['sO'], (64,))
    put('out_conv.1.' + nk, p['gO'], (64,))
    put('out_conv.1.bias', p['bO'], (64,))
    h = L.np_tcm_create(sd, b'blk.', dil, b'left_conv', b'right_conv' if gated else b'left_conv', 4 if K > 0 else 3, K, ks, int(gated))
    L.np_sd_destroy(sd)
    assert h, L.np_last_error().decode()
    return h


def tcm_forms(B, T, min_batch, gated, cum):
    if B >= min_batch and 32 <= T <= 512:
        return ['tcm_fused']
    head = ['cln_stats', 'cln_scan', 'cln_apply'] if cum else ['tcm_head']
    return head * (3 if gated else 2)


TCM_T = [31, 32, 33, 100, 101, 400, 401, 416, 417, 480, 511, 512, 513]
TCM_CASES = []
for _i, _T in enumerate(TCM_T):
    _ks, _g, _c = (5, 3)[_i % 2], (_i // 2) % 2 == 0, (_i // 4) % 2 == 1
    TCM_CASES.append((_ks, _g, _c, 1 << (_i % 8), (_i % 3 != 0), _T, 3, 'mixed' if _i % 2 else None, False))
TCM_CASES += [(5, True, False, 128, True, 401, 1, None, False), (3, False, False, 16, False, 417, 96, 'mixed', False),
              (5, False, True, 4, True, 512, 3, 'mixed', True), (3, True, True, 32, False, 480, 4, None, True),
              (5, True, False, 64, True, 100, 257, 'mixed', True), (3, True, False, 2, True, 416, 96, None, False),
              (5, False, False, 8, True, 33, 5, 'mixed', False), (3, False, True, 1, True, 64, 2, None, False)]


@gpu
@pytest.mark.parametrize('ks,gated,cum,dil,fir,T,B,rag,sat', TCM_CASES)
def test_tcm_block(ks, gated, cum, dil, fir, T, B, rag, sat):
    """run_tcm on one block's weights: the fused kernel (tcm_fused_min_override = 1; T outside [32, 512] falls back) and the
    multi-launch path (override above B) against the same float64 block; all eight template instances, strip (T <= 416) and
    plain epilogues, dilations 1-128, FIR lengths 2 d - 1 (capped at 63), ragged rows of 1, T / 3, T - 1 and T frames"""
    K = min(2 * dil - 1, 63) if fir else 0
    p = tcm_params(1000 + T + ks, ks, gated, cum, K, sat)
    x = make((B, 256, 1, T), 'normal', 1001 + T)[:, :, 0, :].cuda()
    tl = tlens(rag, B, T)
    tld = torch.tensor(tl, dtype=torch.int32, device='cuda') if tl else None
    h = tcm_block(p, dil, K, ks, gated, cum)
    L = lib()
    try:
        for min_batch in (1, B + 1):
            f32acc = min_batch == 1 and not cum
            y, bd = ref_tcm(x, p, dil, K, gated, cum, tl, f32acc)
            outs = {}
            for tail in TAILS[:3 if tl else 1]:
                xin = x.clone()
                if tail is not None:
                    for bi, n in enumerate(tl):
                        xin[bi, :, n:] = tail
                xb, yb = Buf(x.numel(), 0, xin), Buf(x.numel(), 0)
                recs = call('np_tcm_run', h, xb, yb, B, T, min_batch, tld)
                want = tcm_forms(B, T, min_batch, gated, cum)
                assert kernels(recs) == want, (kernels(recs), want)
                if want == ['tcm_fused']:
                    r = recs[0]
                    Tp = (T + 31) // 32 * 32
                    lds = (64 * Tp + 8 * 64 + 5 * 64 + 2 * 16 * 128) * 4
                    strip = 1 if lds + 8 * 32 * 36 * 4 <= 160 * 1024 else 0
                    assert strip == (1 if T <= 416 else 0)
                    assert (r['KS'], r['GATED'], r['CUM'], r['strip'], r['grid'], r['block'], r['ragged']) == \
                        (ks, int(gated), int(cum), strip, B, 512, 1 if tl else 0)
                    assert r['shmem'] == lds + strip * 8 * 32 * 36 * 4
                    form = 'tcm_fused<%d,%d,%d>' % (ks, gated, cum)
                    forms = [form, 'tcm_fused:' + ('strip' if strip else 'plain')]
                else:
                    forms = ['run_tcm:multi-launch' + (':cln' if cum else ':instnorm')]
                assert yb.untouched()
                outs[tail] = yb.v.clone().reshape(x.shape)
            live = torch.ones_like(x, dtype=torch.bool)
            if tl:
                for bi, n in enumerate(tl):
                    live[bi, :, n:] = False
                    for tail in TAILS[1:]:
                        assert torch.equal(outs[None][bi, :, :n], outs[tail][bi, :, :n]), 'a dead frame reached a live one'
            # frames behind a row's own end are not defined by the block (the multi-launch path's convs store zeros there, the fused
            # kernel carries them on): the comparison covers every live frame
            outs[None] = torch.where(live, outs[None].to(F64), y)
            verify('tcm ks%d gated%d cum%d dil%d K%d T%d B%d %s sat%d min_batch %d' % (ks, gated, cum, dil, K, T, B, rag, sat, min_batch),
                   forms, outs[None], y, bd)
    finally:
        L.np_tcm_destroy(h)


# ---- forms that only an environment switch selects ------------------------------------------------------------------------------------
def child_cases(which):
    if which == 'SE_CLN_PLANE':
        for (B, Cc, Fq, T, kind, off, regime) in [(2, 5, 7, 401, 'post', 0, 'normal'), (2, 5, 1, 65, 'post', 1, 'offset'), (1, 3, 2, 1025, 'post', 2, 'const'),
                                                  (2, 2, 3, 63, 'res', 0, 'normal')]:
            run_cln_case(B, Cc, Fq, T, kind, off, regime, plane_on=False)
    else:
        for (widths, Cc, Fq, kind, K) in [((1,), 64, 161, 'res', 0), ((2,), 4, 7, 'res', 0)]:
            run_stream_case(widths, Cc, Fq, kind, K, res_on=False)
    print('CHILD_FORMS ' + json.dumps(sorted(REACHED)))


@gpu
@pytest.mark.parametrize('switch', ['SE_CLN_PLANE', 'SE_CLN_STREAM_RES'])
def test_switch_only_forms(switch):
    """SE_CLN_PLANE=0: the row apply pass behind the plain 2-D norm (a residual still takes the plane pass); SE_CLN_STREAM_RES=0:
    blocks.h adds the residual of a one- / two-frame push with launch_add.  The switches are read once per process: a fresh child."""
    env = dict(os.environ, **{switch: '0'})
    code = 'import sys; sys.path.insert(0, %r); import test_gpu_norm_forms as t; t.child_cases(%r)' % (os.path.dirname(os.path.abspath(__file__)), switch)
    r = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    forms = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('CHILD_FORMS ')][-1][12:])
    for f in forms:
        REACHED.add(switch + '=0:' + f)
    if switch == 'SE_CLN_PLANE':
        assert 'cln_apply' in forms and 'cln_apply_plane' in forms
    else:
        assert 'stream:launch_add' in forms and 'stream:cln_window_reg<1>' in forms and 'stream:cln_window_reg<2>' in forms


TARGET_FORMS = [
    'instnorm_prelu', 'instnorm_prelu:vec', 'instnorm_prelu:scalar', 'instnorm_prelu_ragged', 'instnorm_prelu_ragged:vec',
    'instnorm_prelu_ragged:scalar', 'instnorm_prelu_stats', 'instnorm_prelu_stats:conv', 'instnorm_finalize', 'instnorm_finalize:conv', 'instnorm_apply2:conv', 'instnorm_apply2:vec',
    'instnorm_apply2:scalar', 'tcm_head', 'cln_stats', 'cln_scan', 'cln_apply', 'cln_apply_plane:vec', 'cln_apply_plane:scalar',
    'cln_apply_plane:vec:T>1024', 'cln_apply_plane:vec:T<4', 'cln_apply_plane:vec:T<4:swept', 'cln_apply_plane:scalar:T<4:swept', 'cln_stats:unrolled', 'cln_stats:remainder', 'cln_scan_parts',
    'stream:cln_window_reg<1>', 'stream:cln_window_reg<2>', 'stream:cln_window', 'stream:cln_stats', 'stream:launch_add', 'layernorm_cf',
    'tcm_fused:strip', 'tcm_fused:plain', 'run_tcm:multi-launch:instnorm', 'run_tcm:multi-launch:cln',
    'SE_CLN_PLANE=0:cln_apply', 'SE_CLN_STREAM_RES=0:stream:launch_add',
] + ['tcm_fused<%d,%d,%d>' % (k, g_, c) for k in (3, 5) for g_ in (0, 1) for c in (0, 1)]


@gpu
def test_every_form_reached():
    """every form in the launchers' tables was run by the cases above on this device (runs last: pytest keeps file order)"""
    missing = [f for f in TARGET_FORMS if f not in REACHED]
    print('forms reached: %d; worst error / bound per form:' % len(REACHED))
    for f in sorted(WORST):
        print('  %-40s %.3f  %s' % (f, WORST[f][0], WORST[f][1]))
    assert not missing, 'forms not reached: %s' % missing
