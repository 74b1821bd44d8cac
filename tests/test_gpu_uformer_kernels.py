"""Uformer's private kernels (csrc/k_uformer.hip) one launch at a time against float64: the attention along time
(uf_att_t_mfma_kernel: online softmax over 16-key tiles on the matrix cores, K / V streamed through LDS in blocks of
KB = min(ceil16(T), 512) keys, row pitch Tk = KB or KB + 16, 128 queries per workgroup, keys masked at tlen[b] in ragged batches), the
attention along frequency (uf_att_f_mfma_kernel, and uf_att_f_kernel behind SE_UF_ATT_F_MFMA=0) and the four elementwise kernels
(uf_prep / uf_fusion / uf_post / uf_src_cplx).  Every GPU case is one launcher call through csrc/tests/att_probe.hip ->
libse_attprobe.so on torch buffers with slack; it checks

  1. every stored element against a float64 reference written here from the operation's definition (one head:
     O = softmax(Q K^T / 4) V over the keys < tlen[b], Uformer/t_att_cplx.py:24-38, heads combined as :58-67 / f_att_cplx.py:51-60;
     elementwise: Uformer/uformer.py:182-210, :236-262, fusion.py:13-19 with EPS = finfo(float32).eps) under an elementwise bound,
     printing the worst error / bound;
  2. ownership: outputs are pre-filled with NaN, the slack included; what the launch does not own must still be NaN;
  3. dead data: in ragged cases the frames t >= tlen[b] of q, k and v hold 1e30, then NaN; outputs at t < tlen[b] must equal, bit for
     bit, those of the same case with finite tails, and those of the same clip launched alone at T = tlen[b];
  4. the form that ran (k_uformer.h UfLaunchRec) against a Python mirror of the launcher's conditions; test_every_form_reached asserts
     the whole table of forms was seen.

Error bound, per element (u = 2^-24; constants as tests/test_gpu_norm_forms.py: C_DOT = 4, ACT_ULP = 8u; TINY = 2^-126, below which
fp32 results may be flushed).  One head, one query, keys i with scores s_i, m = max s_i, p_i = exp(s_i - m), l = sum p_i:
  * a score is a 16-term dot product of q / 4 (exact scaling) and k_i: ds_i = C_DOT u sqrt(16) sum_d |q_d k_id| / 4;
  * p_i carries, relatively, e_i = ds_i + (|s_i - m| + 1) 2u (the subtraction and the argument rounding of the hardware exp)
    + ACT_ULP (the exp itself) + e_t, where e_t is what the tile-wise rescaling adds to every earlier term: 2u per key tile (the
    products l * corr, o * corr), and for every tile that raises the running maximum - or comes within twice the score error of it,
    where fp32 may see a rise - one more hardware exp, ACT_ULP + 2u, plus 2u times the total climb of the running maximum from
    the first tile's to m (corr = exp(0) = 1 exactly where the maximum stays);
  * l carries e_l = sum p_i e_i / l + C_DOT u sqrt(T) (its own summation), so
    |dO_d| <= sum_i p_i |v_id| e_i / l + (sum_i p_i |v_id| / l) (e_l + C_DOT u sqrt(T) + 4u) + T TINY max|v| + TINY
    (the summation of P V, the division by l, the sign and the product with it; keys whose p_i underflows);
  * the head combination adds the eight bounds and u per accumulation of the magnitude sums.
Elementwise kernels: every libm or hardware call (atan2f, cosf, sinf, expf, tanhf, hardware exp) is given ACT_ULP of its result, powf
2 ACT_ULP, sqrt and IEEE + - * / u each, propagated through the formulae to first order: for the phase atan2(y, x) with y = im + EPS
(one rounding, dy = u |y|; the sign of y is the same in fp32 and float64, so no element is excluded)
    |dph| <= (|x| dy + |y| dx) / (x^2 + y^2) + ACT_ULP |ph|,
for m = sqrt(max(re^2 + im^2, EPS)) relatively 3u (max is 1-Lipschitz: the clamp needs no exclusion either), for a hardware sigmoid
s(z) an error s (1 - s) ((|z| + 1) 2u + ACT_ULP) + 3u s, and for m cos(ph) the error dm |cos| + m |sin| dph + (ACT_ULP + u) |m cos|.
test_bound_holds_for_fp32_and_catches_faults (CPU) shows that plain fp32 evaluations, the tile-wise online softmax included, stay
inside the bound in every regime and that each planted fault exceeds it by >= 10x.

The VALU frequency attention, which only SE_UF_ATT_F_MFMA=0 selects, runs in one child process."""
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
PROBE_LIB = os.environ.get('SE_ATTPROBE_LIB') or os.path.join(PKG, 'libse_attprobe.so')

U = 2.0 ** -24
ACT_ULP = 8 * U
C_DOT = 4.0
Q_PROP = 3.0                # (as the other kernel suites; nothing here carries an error through a matrix)
TINY = 2.0 ** -126
EPS = float(np.finfo(np.float32).eps)
F64 = torch.float64
HD, NBIN, KBMAX, TILE = 16, 257, 512, 16
REGIMES = ('normal', 'flat', 'peaked', 'late_max', 'early_max')
SR = (1.0, -1.0, -1.0, -1.0, 1.0, 1.0, 1.0, -1.0)       # A - B - C - D | E + F + G - H

REACHED = set()
WORST = {}


# ------------------------------------------------------------------------------------------------ inputs
def make_pq(B, nh, F, T, regime, seed, along='t'):
    """pq [B][nh * 48][F][T] (q, k, v x 16 rows per head): fp32 values widened to float64"""
    g = np.random.default_rng(seed)
    x = g.standard_normal((B, nh, 3, HD, F, T))
    ax = 5 if along == 't' else 4                      # the key axis
    n = x.shape[ax]
    idx = np.arange(n).reshape([-1 if i == ax else 1 for i in range(6)])
    if regime == 'flat':                               # every output is the exact mean of v over the live keys
        x[:, :, 0] = 0.0
        d = np.arange(HD).reshape(1, 1, HD, 1, 1)
        x[:, :, 2] = ((1.0 + idx / n) * (1.0 + d / HD))[:, :, 0] + 0 * x[:, :, 2]
    elif regime == 'peaked':                           # raw maximum of q k / 4 above 100: overflows without the running max
        s = np.einsum('bhdft,bhdfs->bhfts' if along == 't' else 'bhdft,bhdgt->bhtfg', x[:, :, 0], x[:, :, 1]) / 4
        x[:, :, 0] *= 120.0 / np.abs(s).max()
        if s.max() < -s.min():
            x[:, :, 0] *= -1.0
    elif regime in ('late_max', 'early_max'):          # one key dominates every query by ~ e^20
        j = n - 1 if regime == 'late_max' else 0
        x[:, :, 0, 0] = 2.0
        sel = [slice(None)] * 6
        sel[2], sel[3], sel[ax] = 1, 0, j
        x[tuple(sel)] = 40.0
    elif regime != 'normal':
        raise ValueError(regime)
    return torch.from_numpy(x.astype(np.float32).reshape(B, nh * 48, F, T)).to(F64)


# ------------------------------------------------------------------------------------------------ float64 references + bounds
def att_core(q, k, v, nlive=None, tile=TILE):
    """O = softmax(q k^T / 4) v over the keys < nlive[n] of q [N][Tq][16], k, v [N][Tk][16] and its fp32 bound (module docstring);
    tile = 0: a softmax in one piece (the frequency attention).  Returns O, bound, sum p |v| / l."""
    N, Tk, _ = k.shape
    S = q @ k.transpose(1, 2) / 4
    ds = C_DOT * U * math.sqrt(HD) * (q.abs() @ k.abs().transpose(1, 2)) / 4
    dead = None
    if nlive is not None:
        dead = (torch.arange(Tk, device=q.device)[None, None, :] >= nlive[:, None, None]).expand_as(S)
        S = S.masked_fill(dead, -math.inf)
    m = S.max(-1, keepdim=True).values
    P = torch.exp(S - m)
    P = P / P.sum(-1, keepdim=True)
    O = P @ v
    gap = m - S
    if dead is not None:
        gap = gap.masked_fill(dead, 0.0)
    e = ds + (gap + 1) * 2 * U + ACT_ULP
    del gap
    if tile:
        nt = (Tk + tile - 1) // tile
        Sp = torch.nn.functional.pad(S, (0, nt * tile - Tk), value=-math.inf)
        tm = Sp.reshape(N, -1, nt, tile).max(-1).values
        del Sp
        run = torch.cummax(tm, -1).values
        margin = 2 * ds.max(-1).values
        nchg = ((tm[..., 1:] >= run[..., :-1] - margin[..., None]) & torch.isfinite(tm[..., 1:])).sum(-1)
        e_t = 2 * U * nt + nchg * (ACT_ULP + 2 * U) + 2 * U * (m[..., 0] - tm[..., 0])
        e = e + e_t[..., None]
    del S, ds
    Pe = P * e
    del e
    e_l = Pe.sum(-1, keepdim=True) + C_DOT * U * math.sqrt(Tk)
    va = v.abs()
    pv = P @ va
    bound = Pe @ va + pv * (e_l + C_DOT * U * math.sqrt(Tk) + 4 * U) + Tk * TINY * float(va.max()) + TINY
    return O, bound, pv


def ref_att(pq, nh, along, tlen=None):
    """attention along T ('t': keys < tlen[b]) or along F ('f') of pq [B][nh * 48][F][T] -> out [B][16 or 32][F][T], bound"""
    B, _, F, T = pq.shape
    x = pq.reshape(B, nh, 3, HD, F, T)
    perm = (0, 1, 3, 4, 2) if along == 't' else (0, 1, 4, 3, 2)          # [B][nh][F][T][16] / [B][nh][T][F][16]
    q, k, v = (x[:, :, i].permute(*perm).reshape(-1, T if along == 't' else F, HD) for i in range(3))
    nlive = None
    if tlen is not None:
        nlive = torch.as_tensor(tlen, device=pq.device).repeat_interleave(nh * F)
    O, bd, pv = att_core(q, k, v, nlive, TILE if along == 't' else 0)
    sh = (B, nh, F, T, HD) if along == 't' else (B, nh, T, F, HD)
    back = (0, 1, 4, 2, 3) if along == 't' else (0, 1, 4, 3, 2)          # -> [B][nh][16][F][T]
    O, bd, pv = (a.reshape(sh).permute(*back) for a in (O, bd, pv))
    if nh == 1:
        return O[:, 0], bd[:, 0] + U * pv[:, 0]
    sg = torch.tensor(SR, dtype=F64, device=pq.device).view(1, 8, 1, 1, 1)
    Os, tot = O * sg, bd + nh * U * pv
    out = torch.cat([Os[:, :4].sum(1), Os[:, 4:].sum(1)], 1)
    return out, torch.cat([tot[:, :4].sum(1), tot[:, 4:].sum(1)], 1)


def sig_hw(z):
    """sigmoid through the hardware exp and its bound"""
    s = torch.sigmoid(z)
    return s, s * (1 - s) * ((z.abs() + 1) * 2 * U + ACT_ULP) + 3 * U * s + TINY


def polar_front(re, im, p):
    """m = sqrt(clamp(re^2 + im^2, EPS)) [** p], ph = atan2(im + EPS, re) (uformer.py:187, :197) with bounds"""
    m = torch.sqrt(torch.clamp(re * re + im * im, min=EPS))
    em = 3 * U
    if p != 1.0:
        m = m ** p
        em = p * em + 2 * ACT_ULP
    y = im + EPS
    ph = torch.atan2(y, re)
    r2 = re * re + y * y
    dph = torch.where(r2 > 0, re.abs() * U * y.abs() / r2.clamp(min=1e-300), torch.zeros_like(r2)) + ACT_ULP * ph.abs() + TINY
    return m, em * m + TINY, ph, dph


def polar_to_ri(m, dm, ph, dph):
    c, s = torch.cos(ph), torch.sin(ph)
    re, im = m * c, m * s
    return (re, dm * c.abs() + m * s.abs() * dph + (ACT_ULP + U) * re.abs() + TINY,
            im, dm * s.abs() + m * c.abs() * dph + (ACT_ULP + U) * im.abs() + TINY)


def ref_prep(spec, p_in):
    """spec [B][2][257][T] -> (mag0, ph0 [B][257][T], xc [B][2][256][T], xm [B][256][T]) as (value, bound) pairs"""
    m, dm, ph, dph = polar_front(spec[:, 0], spec[:, 1], p_in)
    re, dre, im, dim_ = polar_to_ri(m, dm, ph, dph)
    return ((m, dm), (ph, dph), (torch.stack([re[:, 1:], im[:, 1:]], 1), torch.stack([dre[:, 1:], dim_[:, 1:]], 1)),
            (m[:, 1:], dm[:, 1:]))


def ref_src_cplx(spec, p_in):
    m, dm, ph, dph = polar_front(spec[:, 0], spec[:, 1], p_in)
    re, dre, im, dim_ = polar_to_ri(m, dm, ph, dph)
    return torch.stack([re, im], 1), torch.stack([dre, dim_], 1)


def ref_fusion(cplx, mag):
    """fusion.py:13-19 on cplx [B][2][CP], mag [B][CP]"""
    re, im = cplx[:, 0], cplx[:, 1]
    cm = torch.sqrt(torch.clamp(re * re + im * im, min=EPS))
    s, ds = sig_hw(mag)
    sc, dsc = sig_hw(cm)
    dsc = dsc + sc * (1 - sc) * 3 * U * cm
    oc = torch.stack([re + s, im + s], 1)
    om = mag + sc
    return oc, torch.stack([ds, ds], 1) + U * oc.abs(), om, dsc + U * om.abs()


def ref_post(dc, dm, mag0, ph0, p_out, fault=None):
    """uformer.py:236-262: dc [B][2][256][T], dm [B][256][T], mag0 (>= 0), ph0 [B][257][T] -> est [B][2][257][T], bound"""
    mr, mi = dc[:, 0], dc[:, 1]
    mm = torch.sqrt(torch.clamp(mr * mr + mi * mi, min=EPS))
    e_mm = 3 * U
    den = mm + EPS
    rp, ip = mr / den, mi / den
    y = ip + EPS
    dy = ip.abs() * (e_mm + 2 * U) + U * y.abs()
    dx = rp.abs() * (e_mm + 2 * U)
    cph = torch.atan2(y, rp)
    r2 = rp * rp + y * y
    dcph = (rp.abs() * dy + y.abs() * dx) / r2 + ACT_ULP * cph.abs()
    cm = torch.tanh(den)
    dcm = (1 - cm * cm) * den * (e_mm + U) + ACT_ULP * cm
    mk = torch.sigmoid(dm)
    dmk = mk * (1 - mk) * ACT_ULP + 3 * U * mk                          # libm exp of an exact argument
    pad = lambda a: torch.nn.functional.pad(a, (0, 0, 1, 0))            # the DC bin: zero masks, zero phase
    if fault == 'dc_not_zeroed':
        pad = lambda a: torch.cat([a[:, :1], a], 1)
    cm, dcm, mk, dmk, cph, dcph = (pad(a) for a in (cm, dcm, mk, dmk, cph, dcph))
    em = (cm * mag0 + mk * mag0) * 0.5
    dem = 0.5 * (mag0 * (dcm + dmk) + 2 * U * (cm * mag0 + mk * mag0)) + TINY * (1 + mag0)
    if p_out != 1.0:
        dem = p_out * em ** (p_out - 1) * dem + 2 * ACT_ULP * em ** p_out + TINY
        em = em ** p_out
    ep = ph0 + cph
    dep = dcph + U * ep.abs()
    re, dre, im, dim_ = polar_to_ri(em, dem, ep, dep)
    return torch.stack([re, im], 1), torch.stack([dre, dim_], 1)


# ------------------------------------------------------------------------------------------------ plain fp32 evaluations (CPU)
f32 = np.float32


def eval32_att_t(pq, nh, tlen=None, KB=KBMAX, online=True, fault=None, fkey=None):
    """the time attention in numpy fp32: a softmax in one piece (online = False) or over 16-key tiles with the state carried across
    blocks of KB keys, as the kernel orders it.  fault: a planted defect; fkey: the key it hits."""
    x = pq.numpy().astype(f32)
    B, _, F, T = x.shape
    x = x.reshape(B, nh, 3, HD, F, T)
    nout = 1 if nh == 1 else 2
    out = np.zeros((B, nout * HD, F, T), f32)
    lastq = 16 * ((T - 1) // 16)
    for b in range(B):
        Tl = T if tlen is None else int(tlen[b])
        for f in range(F):
            for h in range(nh):
                q = x[b, h, 0, :, f, :].T.copy()
                if fault == 'query_neighbour':           # the last query tile reads frame t + 1 (clamped)
                    src = np.arange(T)
                    src[lastq:] = np.minimum(src[lastq:] + 1, T - 1)
                    q = q[src]
                if fault != 'no_scale':
                    q = q * f32(0.25)
                k, v = x[b, h, 1, :, f, :Tl].T, x[b, h, 2, :, f, :Tl].T
                live = np.ones(Tl, bool)
                if fault == 'drop_key':
                    live[fkey] = False
                if not online:
                    s = (q @ k.T).astype(f32)
                    s[:, ~live] = f32(-3.0e38)
                    p = np.exp(s - s.max(-1, keepdims=True)).astype(f32)
                    if fault == 'double_key':
                        p = np.concatenate([p, p[:, fkey:fkey + 1]], 1)
                        v = np.concatenate([v, v[fkey:fkey + 1]], 0)
                    o = (p @ v).astype(f32) / p.sum(-1, keepdims=True, dtype=f32)
                else:
                    mx = np.full((T, 1), -3.0e38, f32)
                    l = np.zeros((T, 1), f32)
                    o = np.zeros((T, HD), f32)
                    for k0 in range(0, Tl, TILE):
                        if fault == 'max_reset' and k0 > 0 and k0 % KB == 0:
                            mx[:] = f32(-3.0e38)        # the running max re-initialised with every block
                        kk, vv, lv = k[k0:k0 + TILE], v[k0:k0 + TILE], live[k0:k0 + TILE]
                        s = (q @ kk.T).astype(f32)
                        s[:, ~lv] = f32(-3.0e38)
                        mn = np.maximum(mx, s.max(-1, keepdims=True))
                        corr = np.exp(mx - mn).astype(f32)
                        pe = np.exp(s - mn).astype(f32)
                        if fault == 'double_key' and k0 <= fkey < k0 + TILE:
                            pe = np.concatenate([pe, pe[:, fkey - k0:fkey - k0 + 1]], 1)
                            vv = np.concatenate([vv, vv[fkey - k0:fkey - k0 + 1]], 0)
                        l = l * corr + pe.sum(-1, keepdims=True, dtype=f32)
                        o = o * corr + (pe @ vv).astype(f32)
                        mx = mn
                    o = o / l
                sg = f32(1.0 if nh == 1 else SR[h])
                if fault == 'head_sign' and h == 2:
                    sg = -sg
                half = 0 if (nh == 1 or h < 4) else 1
                out[b, half * HD:(half + 1) * HD, f, :] += sg * o.T
    if fault == 'swap_ri':
        out = np.concatenate([out[:, HD:], out[:, :HD]], 1)
    return out


def eval32_att_f(pq, nh):
    x = pq.numpy().astype(f32)
    B, _, F, T = x.shape
    x = x.reshape(B, nh, 3, HD, F, T)
    q, k, v = (np.transpose(x[:, :, i], (0, 1, 4, 3, 2)) for i in range(3))      # [B][nh][T][F][16]
    s = np.matmul(q * f32(0.25), np.swapaxes(k, -1, -2)).astype(f32)
    p = np.exp(s - s.max(-1, keepdims=True)).astype(f32)
    o = np.matmul(p, v).astype(f32) / p.sum(-1, keepdims=True, dtype=f32)
    o = np.transpose(o, (0, 1, 4, 3, 2))                                          # [B][nh][16][F][T]
    if nh == 1:
        return o[:, 0]
    o = o * np.asarray(SR, f32).reshape(1, 8, 1, 1, 1)
    return np.concatenate([o[:, :4].sum(1, dtype=f32), o[:, 4:].sum(1, dtype=f32)], 1)


def polar32(re, im, p, clamp=True):
    s = re * re + im * im
    m = np.sqrt(np.maximum(s, f32(EPS)) if clamp else s)
    if p != 1.0:
        m = np.power(m, f32(p))
    ph = np.arctan2(im + f32(EPS), re)
    return m.astype(f32), ph.astype(f32)


def eval32_prep(spec, p_in, fault=None):
    x = spec.numpy().astype(f32)
    m, ph = polar32(x[:, 0], x[:, 1], p_in, fault != 'no_clamp')
    re, im = m * np.cos(ph), m * np.sin(ph)
    return m, ph, np.stack([re[:, 1:], im[:, 1:]], 1), m[:, 1:], np.stack([re, im], 1)


def sig32(z):
    with np.errstate(over='ignore'):
        return (f32(1) / (f32(1) + np.exp(-z))).astype(f32)


def eval32_fusion(cplx, mag, fault=None):
    c, m = cplx.numpy().astype(f32), mag.numpy().astype(f32)
    s2 = c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]
    cm = np.sqrt(s2 if fault == 'no_clamp' else np.maximum(s2, f32(EPS)))
    s = sig32(m)
    return np.stack([c[:, 0] + s, c[:, 1] + s], 1), m + sig32(cm)


def eval32_post(dc, dm, mag0, ph0, p_out, fault=None):
    dc, dm, mag0, ph0 = (a.numpy().astype(f32) for a in (dc, dm, mag0, ph0))
    mr, mi = dc[:, 0], dc[:, 1]
    s2 = mr * mr + mi * mi
    mm = np.sqrt(s2 if fault == 'no_clamp' else np.maximum(s2, f32(EPS)))
    with np.errstate(invalid='ignore', divide='ignore'):
        rp, ip = mr / (mm + f32(EPS)), mi / (mm + f32(EPS))
    cm = np.tanh(mm + f32(EPS))
    cph = np.arctan2(ip + f32(EPS), rp)
    mk = sig32(dm)
    if fault == 'dc_not_zeroed':
        pad = lambda a: np.concatenate([a[:, :1], a], 1)
    else:
        pad = lambda a: np.pad(a, ((0, 0), (1, 0), (0, 0)))
    cm, cph, mk = pad(cm), pad(cph), pad(mk)
    em = (cm * mag0 + mk * mag0) * f32(0.5)
    if p_out != 1.0:
        em = np.power(em, f32(p_out))
    ep = ph0 + cph
    return np.stack([em * np.cos(ep), em * np.sin(ep)], 1).astype(f32)


# ------------------------------------------------------------------------------------------------ elementwise inputs
PLANTS = [(0.0, 0.0), (-1.0, 0.0), (-2.5, 0.0), (1.0, -EPS), (-1.0, -EPS), (0.0, -EPS), (1e-20, 1e-20), (-1e-20, 1e-20), (1e4, 1e4),
          (-1e4, -1e4), (1e4, 1e-20), (1e-20, -1e4)]


def plant(re, im, T):
    """the planted points in the DC bin and in ordinary bins of row 0 (first frame) and row 1 (last frame)"""
    for i, (a, c) in enumerate(PLANTS):
        for b, k, t in ((0, i % 2 * (i + 1), 0), (1 % re.shape[0], 100 + i, T - 1), (0, re.shape[1] - 1 - i, T // 2)):
            re[b, k, t], im[b, k, t] = a, c


def make_spec(B, T, seed):
    g = np.random.default_rng(seed)
    x = g.standard_normal((B, 2, NBIN, T)) * g.choice([1e-3, 1.0, 30.0], (B, 1, NBIN, T))
    plant(x[:, 0], x[:, 1], T)
    return torch.from_numpy(x.astype(np.float32)).to(F64)


def make_post(B, T, seed):
    g = np.random.default_rng(seed)
    dc = g.standard_normal((B, 2, NBIN - 1, T)) * g.choice([1e-3, 1.0, 5.0], (B, 1, NBIN - 1, T))
    plant(dc[:, 0], dc[:, 1], T)
    dm = g.standard_normal((B, NBIN - 1, T)) * 3
    dm[0, 5, 0], dm[0, 6, 0], dm[B - 1, 200, T - 1], dm[B - 1, 201, T - 1] = 100.0, -100.0, 100.0, -100.0
    mag0 = np.abs(g.standard_normal((B, NBIN, T))) + 0.1
    ph0 = g.uniform(-math.pi, math.pi, (B, NBIN, T))
    return tuple(torch.from_numpy(a.astype(np.float32)).to(F64) for a in (dc, dm, mag0, ph0))


def make_fusion(B, CP, seed):
    g = np.random.default_rng(seed)
    c = g.standard_normal((B, 2, CP)) * 2
    m = g.standard_normal((B, CP)) * 3
    for i, (a, b_) in enumerate(PLANTS):
        c[0, 0, i], c[0, 1, i] = a, b_
    m[0, 20], m[0, 21], m[B - 1, CP - 1], m[B - 1, CP - 2] = 100.0, -100.0, 100.0, -100.0
    c[0, 0, 22], c[0, 1, 23], c[B - 1, 0, CP - 3] = 100.0, -100.0, -100.0
    return torch.from_numpy(c.astype(np.float32)).to(F64), torch.from_numpy(m.astype(np.float32)).to(F64)


# ------------------------------------------------------------------------------------------------ CPU tests
def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


def test_reference_matches_torch():
    """the float64 references against torch.softmax / einsum and the elementwise formulae of the definition, in float64"""
    tol = 1e-12
    for nh in (1, 8):
        for regime in REGIMES:
            pq = make_pq(2, nh, 3, 37, regime, 1)
            x = pq.reshape(2, nh, 3, HD, 3, 37)
            for along, tlen in (('t', None), ('t', [37, 17]), ('f', None)):
                heads = []
                for h in range(nh):
                    q, k, v = (x[:, h, i].permute(0, 2, 3, 1) for i in range(3))          # [B][F][T][16]
                    if along == 'f':
                        q, k, v = (a.transpose(1, 2) for a in (q, k, v))
                    en = torch.einsum('...tf,...fy->...ty', q, k.transpose(-1, -2)) / HD ** 0.5
                    if tlen is not None:
                        for b in range(2):
                            en[b, :, :, tlen[b]:] = -math.inf
                    o = torch.einsum('...tf,...fy->...ty', torch.softmax(en, -1), v)
                    heads.append(o.transpose(1, 2) if along == 'f' else o)               # [B][F][T][16]
                if nh == 1:
                    want = heads[0]
                else:
                    A, B_, C_, D, E, F_, G, H = heads
                    want = torch.cat([A - B_ - C_ - D, E + F_ + G - H], -1)
                want = want.permute(0, 3, 1, 2)
                got, _ = ref_att(pq, nh, along, tlen)
                if tlen is not None:
                    got, want = got[1, ..., :17], want[1, ..., :17]
                assert rel(got, want) < tol, (nh, regime, along)
    spec = make_spec(2, 5, 2)
    re, im = spec[:, 0], spec[:, 1]
    for p in (1.0, 0.5):
        mag = torch.sqrt(torch.clamp(re ** 2 + im ** 2, EPS)) ** p
        ph = torch.atan2(im + EPS, re)
        (m_, _), (p_, _), (xc, _), (xm, _) = ref_prep(spec, p)
        full = torch.stack([mag * torch.cos(ph), mag * torch.sin(ph)], 1)
        assert rel(m_, mag) < tol and rel(p_, ph) < tol and rel(xc, full[:, :, 1:]) < tol and rel(xm, mag[:, 1:]) < tol
        assert rel(ref_src_cplx(spec, p)[0], full) < tol
    c, m = make_fusion(2, 40, 3)
    oc, _, om, _ = ref_fusion(c, m)
    cmag = torch.sqrt(torch.clamp(c[:, 0] ** 2 + c[:, 1] ** 2, EPS))
    assert rel(om, m + torch.sigmoid(cmag)) < tol and rel(oc, c + torch.sigmoid(m)[:, None]) < tol
    dc, dm, mag0, ph0 = make_post(2, 5, 4)
    pad = lambda a: torch.nn.functional.pad(a, [0, 0, 1, 0])
    mmag = torch.sqrt(torch.clamp(dc[:, 0] ** 2 + dc[:, 1] ** 2, EPS))
    rph, iph = dc[:, 0] / (mmag + EPS), dc[:, 1] / (mmag + EPS)
    est_m = (pad(torch.tanh(mmag + EPS)) * mag0 + pad(torch.sigmoid(dm)) * mag0) * 0.5
    est_p = ph0 + pad(torch.atan2(iph + EPS, rph))
    for p in (1.0, 2.0):
        want = torch.stack([est_m ** p * torch.cos(est_p), est_m ** p * torch.sin(est_p)], 1)
        assert rel(ref_post(dc, dm, mag0, ph0, p)[0], want) < tol


def worst(got, ref, bound):
    r = (torch.as_tensor(np.asarray(got, dtype=np.float64)) - ref.cpu()).abs() / bound.cpu()
    assert torch.isfinite(r).all(), 'non-finite output or zero bound'
    return float(r.max())


def test_bound_holds_for_fp32_and_catches_faults():
    """(i) plain fp32 evaluations, tile-wise online softmax included, stay inside the bound in every regime; (ii) each planted fault
    exceeds it >= 10x"""
    inside = {}
    T, KB = 45, 32                                       # two key blocks, a last tile of 13 keys
    for regime in REGIMES:
        for nh in (1, 8):
            pq = make_pq(2, nh, 2, T, regime, 11)
            for tl in (None, [T, 17]):
                y, bd = ref_att(pq, nh, 't', tl)
                for online in (False, True):
                    got = eval32_att_t(pq, nh, tl, KB, online)
                    if tl is not None:
                        inside['att_t', regime, nh, 'ragged', online] = worst(got[1, ..., :17], y[1, ..., :17], bd[1, ..., :17])
                    else:
                        inside['att_t', regime, nh, online] = worst(got, y, bd)
            if regime in ('normal', 'flat', 'peaked'):
                pf = make_pq(2, nh, 4, 9, regime, 12, along='f')
                y, bd = ref_att(pf, nh, 'f')
                inside['att_f', regime, nh] = worst(eval32_att_f(pf, nh), y, bd)
    for p in (1.0, 0.5):
        spec = make_spec(2, 7, 13)
        got = eval32_prep(spec, p)
        for name, g_, (y, bd) in zip(('mag0', 'ph0', 'xc', 'xm'), got, ref_prep(spec, p)):
            inside['prep', name, p] = worst(g_, y, bd)
        y, bd = ref_src_cplx(spec, p)
        inside['src_cplx', p] = worst(got[4], y, bd)
    c, m = make_fusion(2, 300, 14)
    oc, bc, om, bm = ref_fusion(c, m)
    gc_, gm = eval32_fusion(c, m)
    inside['fusion', 'cplx'], inside['fusion', 'mag'] = worst(gc_, oc, bc), worst(gm, om, bm)
    post_in = make_post(2, 7, 15)
    for p in (1.0, 2.0):
        y, bd = ref_post(*post_in, p)
        inside['post', p] = worst(eval32_post(*post_in, p), y, bd)
    top = max(inside.values())
    print('fp32 evaluations: worst error / bound %.3f at %s' % (top, max(inside, key=inside.get)))
    assert top <= 1.0, {k: v for k, v in inside.items() if v > 1.0}

    # (ii) faults, each in the regime made to show it
    caught = {}
    flat, normal = make_pq(2, 8, 2, T, 'flat', 21), make_pq(2, 8, 2, T, 'normal', 22)
    yf, bf = ref_att(flat, 8, 't')
    yn, bn = ref_att(normal, 8, 't')
    for f, key in (('drop_key', 31), ('drop_key', T - 1), ('double_key', 32), ('double_key', 15)):
        for online in (False, True):
            caught[f, key, online] = worst(eval32_att_t(flat, 8, None, KB, online, f, key), yf, bf)
    for f in ('no_scale', 'head_sign', 'swap_ri', 'max_reset'):
        caught[f] = worst(eval32_att_t(normal, 8, None, KB, True, f), yn, bn)
    lastq = 16 * ((T - 1) // 16)
    got = eval32_att_t(normal, 8, None, KB, True, 'query_neighbour')
    caught['query_neighbour'] = worst(got[..., lastq:T - 1], yn[..., lastq:T - 1], bn[..., lastq:T - 1])
    one = make_pq(2, 1, 2, T, 'flat', 23)
    y1, b1 = ref_att(one, 1, 't', [T, 17])
    caught['drop_key', 'ragged', 16] = worst(eval32_att_t(one, 1, [T, 17], KB, True, 'drop_key', 16)[1, ..., :17], y1[1, ..., :17], b1[1, ..., :17])
    spec = make_spec(2, 7, 24)
    (ym, bm_), _, _, _ = ref_prep(spec, 1.0)
    caught['prep_no_clamp'] = worst(eval32_prep(spec, 1.0, 'no_clamp')[0], ym, bm_)
    c, m = make_fusion(2, 300, 25)
    _, _, om, bm_ = ref_fusion(c, m)
    caught['fusion_no_clamp'] = worst(eval32_fusion(c, m, 'no_clamp')[1], om, bm_)
    post_in = make_post(2, 7, 26)
    y, bd = ref_post(*post_in, 1.0)
    caught['post_dc_not_zeroed'] = worst(eval32_post(*post_in, 1.0, 'dc_not_zeroed'), y, bd)
    low = min(caught, key=caught.get)
    print('faults: smallest error / bound %.1f (%s); all: %s' % (caught[low], low, {str(k): round(v, 1) for k, v in caught.items()}))
    assert caught[low] >= 10.0, caught


# ------------------------------------------------------------------------------------------------ GPU side
_lib = None
SIGS = {'ap_att_t': 'ppiiiip', 'ap_att_f': 'ppiiii', 'ap_prep': 'pppppiif', 'ap_fusion': 'ppil', 'ap_post': 'pppppiif',
        'ap_src_cplx': 'ppiif'}
CT = {'i': C.c_int, 'p': C.c_void_p, 'l': C.c_long, 'f': C.c_float}
REC = ('nh', 'KB', 'Tk', 'nblocks', 'ragged', 'grid', 'block', 'shmem')
SLACK = 64


def lib():
    global _lib
    if _lib is None:
        assert os.path.exists(PROBE_LIB), 'libse_attprobe.so is missing: run build() (make -C csrc)'
        L = C.CDLL(PROBE_LIB)
        for name, sig in SIGS.items():
            getattr(L, name).argtypes = [CT[c] for c in sig]
            getattr(L, name).restype = C.c_int
        L.ap_last_error.restype = C.c_char_p
        L.ap_launch_kernel.restype = C.c_char_p
        L.ap_launch_kernel.argtypes = [C.c_int]
        L.ap_launch_get.argtypes = [C.c_int, C.POINTER(C.c_longlong), C.c_int]
        _lib = L
    return _lib


class Buf:
    """device buffer of n floats with NaN in the slack around it (and in it, unless src fills it)"""

    def __init__(self, n, src=None):
        self.n = n
        self.t = torch.full((n + 2 * SLACK,), float('nan'), dtype=torch.float32, device='cuda')
        self.v = self.t[SLACK:SLACK + n]
        if src is not None:
            self.v.copy_(src.reshape(-1).to(torch.float32))

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * SLACK

    def untouched(self):
        return bool(torch.isnan(self.t[:SLACK]).all() and torch.isnan(self.t[SLACK + self.n:]).all())


def call(name, *args):
    L = lib()
    rc = getattr(L, name)(*[a.ptr if isinstance(a, Buf) else (a.data_ptr() if torch.is_tensor(a) else a) for a in args])
    assert rc == 0, '%s: %s' % (name, L.ap_last_error().decode())
    out = []
    for i in range(L.ap_launch_count()):
        v = (C.c_longlong * 8)()
        L.ap_launch_get(i, v, 8)
        d = dict(zip(REC, list(v)))
        d['kernel'] = L.ap_launch_kernel(i).decode()
        out.append(d)
    assert len(out) == 1, out
    return out[0]


def note(form, ratio, case):
    REACHED.add(form)
    if ratio > WORST.get(form, (0.0, ''))[0]:
        WORST[form] = (ratio, case)


def verify(case, form, got, ref, bound, bufs=(), live=None):
    """elementwise check of one stored tensor + ownership of the buffers around it; prints the worst error / bound"""
    got = got.to(F64).reshape(ref.shape)
    if live is not None:
        got, ref, bound = got[live], ref[live], bound[live]
    assert torch.isfinite(got).all(), '%s: non-finite output' % case
    r = (got - ref).abs() / bound
    k = int(r.argmax())
    ratio = float(r.reshape(-1)[k])
    print('%s: worst error / bound %.3f at %s (got %.9g, want %.9g, bound %.3g) form %s' %
          (case, ratio, tuple(int(i) for i in np.unravel_index(k, r.shape)), float(got.reshape(-1)[k]), float(ref.reshape(-1)[k]),
           float(bound.reshape(-1)[k]), form))
    note(form, ratio, case)
    for bf in bufs:
        assert bf.untouched(), '%s: wrote outside its output' % case
    assert ratio <= 1.0, '%s: error %.3f of the bound' % (case, ratio)
    return ratio


gpu = pytest.mark.gpu


# ---- attention along time ----------------------------------------------------------------------------------------------------------------
def att_t_geometry(T):
    """launch_uf_att_t: keys per LDS block, row pitch of the K block, key blocks, dynamic LDS bytes, workgroups per (b, f)"""
    KB = min((T + 15) // 16 * 16, KBMAX)
    Tk = KB if KB % 32 == 16 else KB + 16
    return KB, Tk, (T + KB - 1) // KB, (HD * Tk + KB * 17) * 4, (T + 127) // 128


def att_t_form(nh, T, ragged):
    KB, Tk, nb, _, _ = att_t_geometry(T)
    return 'att_t:nh%d:%s:%s:%s' % (nh, 'several' if nb > 1 else 'one', 'padded' if Tk > KB else 'unpadded', 'ragged' if ragged else 'full')


def run_att_t(pq, nh, tlen=None):
    """one launch on pq [B][nh * 48][F][T] (any float dtype, on the GPU); returns the output [B][nout * 16][F][T], its buffer and form"""
    B, _, F, T = pq.shape
    nout = 1 if nh == 1 else 2
    src, out = Buf(pq.numel(), pq), Buf(B * nout * HD * F * T)
    tl = torch.tensor(tlen, dtype=torch.int32, device='cuda') if tlen is not None else None
    rec = call('ap_att_t', src, out, B, F, T, nh, tl.data_ptr() if tl is not None else None)
    KB, Tk, nb, lds, qb = att_t_geometry(T)
    assert rec['kernel'] == 'uf_att_t_mfma' and (rec['nh'], rec['KB'], rec['Tk'], rec['nblocks'], rec['ragged'], rec['grid'], rec['block'],
                                                 rec['shmem']) == (nh, KB, Tk, nb, int(tlen is not None), B * F * qb, 256, lds), rec
    return out.v.reshape(B, nout * HD, F, T).clone(), out, att_t_form(nh, T, tlen is not None)


ATT_T = [1, 15, 16, 17, 26, 127, 128, 129, 401, 496, 511, 512, 513, 1025]


@gpu
@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('T', ATT_T)
@pytest.mark.parametrize('nh', [1, 8])
@pytest.mark.parametrize('F', [1, 4])
def test_att_t(F, nh, T, regime):
    pq = make_pq(2, nh, F, T, regime, 1000 * F + 10 * T + nh).cuda()
    if regime == 'peaked':
        x = pq.reshape(2, nh, 3, HD, F, T)
        assert float(torch.einsum('bhdft,bhdfs->bhfts', x[:, :, 0], x[:, :, 1]).max()) / 4 > 100
    got, out, form = run_att_t(pq, nh)
    ref, bd = ref_att(pq, nh, 't')
    verify('att_t F%d nh%d T%d %s' % (F, nh, T, regime), form, got, ref, bd, [out])
    assert not torch.isnan(out.v).any()


RAGGED = [(530, [530, 513, 512, 17, 1]), (60, [60, 33, 32, 17, 1]), (48, [48, 47, 16, 15, 1])]


@gpu
@pytest.mark.parametrize('T,tlen', RAGGED)
@pytest.mark.parametrize('nh', [1, 8])
@pytest.mark.parametrize('regime', ['normal', 'flat', 'late_max'])
def test_att_t_ragged(regime, nh, T, tlen):
    """keys masked at tlen[b]: live outputs against float64, against the clip launched alone, and with 1e30 / NaN in the dead frames"""
    B, F = len(tlen), 2
    pq = make_pq(B, nh, F, T, regime, 7 * T + nh).cuda()
    if regime == 'late_max':                     # the dominant key is the row's own last live key
        x = pq.reshape(B, nh, 3, HD, F, T)
        for b, n in enumerate(tlen):
            x[b, :, 1, 0, :, T - 1] = x[b, :, 1, 0, :, 0]
            x[b, :, 1, 0, :, n - 1] = 40.0
    got, out, form = run_att_t(pq, nh, tlen)
    ref, bd = ref_att(pq, nh, 't', tlen)
    live = (torch.arange(T, device='cuda')[None, :] < torch.tensor(tlen, device='cuda')[:, None])[:, None, None, :].expand_as(ref)
    case = 'att_t ragged nh%d T%d %s' % (nh, T, regime)
    verify(case, form, got, ref, bd, [out], live)
    for b, n in enumerate(tlen):
        alone, _, _ = run_att_t(pq[b:b + 1, :, :, :n].contiguous(), nh)
        assert torch.equal(alone[0], got[b, :, :, :n]), '%s: row %d differs from the clip launched alone' % (case, b)
    dead = ~(torch.arange(T, device='cuda')[None, :] < torch.tensor(tlen, device='cuda')[:, None])[:, None, None, :].expand_as(pq)
    for tail in (1e30, math.nan):
        g2, o2, _ = run_att_t(torch.where(dead, torch.full_like(pq, tail), pq), nh, tlen)
        assert o2.untouched()
        assert torch.equal(g2[live], got[live]), '%s: dead frames holding %s reach live outputs' % (case, tail)


# ---- attention along frequency -----------------------------------------------------------------------------------------------------------
def run_att_f(pq, nh, kernel):
    B, _, F, T = pq.shape
    nout = 1 if nh == 1 else 2
    src, out = Buf(pq.numel(), pq), Buf(B * nout * HD * F * T)
    rec = call('ap_att_f', src, out, B, F, T, nh)
    grid = (((T + 15) // 16 + 3) // 4) * B if kernel == 'uf_att_f_mfma' else (T + 255) // 256 * F * B
    assert (rec['kernel'], rec['nh'], rec['grid'], rec['block'], rec['shmem']) == (kernel, nh, grid, 256, 0), rec
    assert not torch.isnan(out.v).any()
    return out.v.reshape(B, nout * HD, F, T).clone(), out


def att_f_case(F, nh, T, regime, kernel):
    pq = make_pq(2, nh, F, T, regime, 31 * T + nh + F, along='f').cuda()
    got, out = run_att_f(pq, nh, kernel)
    ref, bd = ref_att(pq, nh, 'f')
    verify('%s F%d nh%d T%d %s' % (kernel, F, nh, T, regime), '%s:nh%d' % (kernel[3:], nh), got, ref, bd, [out])


@gpu
@pytest.mark.parametrize('regime', ['normal', 'flat', 'peaked'])
@pytest.mark.parametrize('T', [1, 15, 16, 17, 63, 64, 65, 401])
@pytest.mark.parametrize('nh', [1, 8])
def test_att_f_mfma(nh, T, regime):
    att_f_case(4, nh, T, regime, 'uf_att_f_mfma')


def child_cases():
    for F in (1, 4, 5, 8):
        for nh in (1, 8):
            for T, regime in ((17, 'normal'), (257, 'peaked'), (256, 'flat')):
                att_f_case(F, nh, T, regime, 'uf_att_f')
    print('CHILD_FORMS ' + json.dumps({f: WORST[f] for f in sorted(REACHED)}))


@gpu
def test_att_f_valu():
    """SE_UF_ATT_F_MFMA=0: the one-thread-per-query kernel, F in {1, 4, 5, 8}.  The switch is read once per process: a fresh child."""
    env = dict(os.environ, SE_UF_ATT_F_MFMA='0')
    code = 'import sys; sys.path.insert(0, %r); import test_gpu_uformer_kernels as t; t.child_cases()' % os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    forms = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('CHILD_FORMS ')][-1][12:])
    for f, (ratio, case) in forms.items():
        note(f, ratio, case)
    assert set(forms) == {'att_f:nh1', 'att_f:nh8'}


# ---- elementwise kernels -----------------------------------------------------------------------------------------------------------------
def check_rec(rec, kernel, grid):
    assert (rec['kernel'], rec['grid'], rec['block'], rec['shmem']) == (kernel, grid, 256, 0), rec


@gpu
@pytest.mark.parametrize('p_in', [1.0, 0.5])
@pytest.mark.parametrize('T', [1, 255, 256, 257])
def test_prep_and_src_cplx(T, p_in):
    B = 2
    spec = make_spec(B, T, 50 + T).cuda()
    src = Buf(spec.numel(), spec)
    outs = [Buf(B * NBIN * T), Buf(B * NBIN * T), Buf(B * 2 * (NBIN - 1) * T), Buf(B * (NBIN - 1) * T)]
    check_rec(call('ap_prep', src, *outs, B, T, p_in), 'uf_prep', (T + 255) // 256 * NBIN * B)
    for name, o, (y, bd) in zip(('mag0', 'ph0', 'xc', 'xm'), outs, ref_prep(spec, p_in)):
        verify('prep %s T%d p%g' % (name, T, p_in), 'uf_prep', o.v, y, bd, outs)       # (xc / xm have no DC row: a write for k = 0 lands in the slack)
    sc = Buf(spec.numel())
    check_rec(call('ap_src_cplx', src, sc, B, T, p_in), 'uf_src_cplx', (T + 255) // 256 * NBIN * B)
    y, bd = ref_src_cplx(spec, p_in)
    verify('src_cplx T%d p%g' % (T, p_in), 'uf_src_cplx', sc.v, y, bd, [sc])


@gpu
@pytest.mark.parametrize('CP', [255, 256, 257])
def test_fusion_in_place(CP):
    B = 2
    c, m = make_fusion(B, CP, 60 + CP)
    c, m = c.cuda(), m.cuda()
    bc, bm = Buf(c.numel(), c), Buf(m.numel(), m)
    check_rec(call('ap_fusion', bc, bm, B, CP), 'uf_fusion', (CP + 255) // 256 * B)
    oc, dc, om, dm = ref_fusion(c, m)
    verify('fusion cplx CP%d' % CP, 'uf_fusion', bc.v, oc, dc, [bc, bm])
    verify('fusion mag CP%d' % CP, 'uf_fusion', bm.v, om, dm, [bc, bm])


@gpu
@pytest.mark.parametrize('p_out', [1.0, 2.0])
@pytest.mark.parametrize('T', [1, 255, 256, 257])
def test_post(T, p_out):
    B = 2
    ins = [a.cuda() for a in make_post(B, T, 70 + T)]
    bufs = [Buf(a.numel(), a) for a in ins]
    est = Buf(B * 2 * NBIN * T)
    check_rec(call('ap_post', *bufs, est, B, T, p_out), 'uf_post', (T + 255) // 256 * NBIN * B)
    y, bd = ref_post(*ins, p_out)
    verify('post T%d p%g' % (T, p_out), 'uf_post', est.v, y, bd, [est])
    assert bool((est.v.reshape(B, 2, NBIN, T)[:, :, 0] == 0).all()), 'the DC bin of est is the zero-magnitude path'


# ---- the table of forms ------------------------------------------------------------------------------------------------------------------
def target_forms():
    """every form the launchers can reach: the time attention's from the mirror of its conditions over all T up to four key blocks"""
    forms = {att_t_form(nh, T, rag) for nh in (1, 8) for T in range(1, 4 * KBMAX + 1) for rag in (False, True)}
    return sorted(forms) + ['att_f_mfma:nh1', 'att_f_mfma:nh8', 'att_f:nh1', 'att_f:nh8', 'uf_prep', 'uf_fusion', 'uf_post', 'uf_src_cplx']


@gpu
def test_every_form_reached():
    """every form in the launchers' table was run by the cases above on this device (runs last: pytest keeps file order)"""
    want = target_forms()
    assert len(want) == 2 * 3 * 2 + 8, want         # one / padded, one / unpadded, several / padded (KB = 512 is always padded)
    missing = [f for f in want if f not in REACHED]
    print('forms reached: %d; worst error / bound per form:' % len(REACHED))
    for f in sorted(WORST):
        print('  %-40s %.3f  %s' % (f, WORST[f][0], WORST[f][1]))
    assert not missing, 'forms not reached: %s' % missing
