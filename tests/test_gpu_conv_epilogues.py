"""gemmconv's epilogues and the three-product complex layers against float64, one layer launch at a time.

The geometry suite (test_gpu_gemmconv_geometry.py) launches every layer with EPI_ACT and identity / PReLU; the frame-online suite
reaches EPI_ADD / MUL / GLU only on the few-frame forms.  Here one small layer per tile height is built and launched through the
functions the models call (csrc/tests/epi_probe.hip -> libse_epiprobe.so: make_conv_plan / make_deconv_plan / set_post_bn,
run_conv / run_deconv, gauss::make_*_plans / fold_tail / run_layer) with every optional operand of the epilogue - aux, dst_elu, the
two statistics riders, the folded branch interaction (fz), ragged rows - and every stored value is compared with a float64
reference of the same OPERATION (not of the kernel's arithmetic).  Every buffer a launch writes starts as NaN: what the launch
does not own must still be NaN afterwards, what it owns must be within the bound.

The error bound, per stored element (u = 2^-24, K = accumulated products per output):

  pre-activation     e0 = 4 u K (sum |w| |x| + |bias|)                      (as the geometry suite takes it)
  activation f       e  = L e0 + a_f + u |f|,  L = sup |f'|, a_f the absolute error of the hardware form:
      identity / ReLU / PReLU   L = max(1, |slope|), a = 0
      sigmoid                   L = 1/4, a = 8 u      (v_exp + v_rcp, as test_gpu_lstm_forms.py takes it)
      tanh                      L = 1,   a = 8 u      (1 - 2 rcp(1 + exp 2x): the same two instructions, doubled)
      softplus                  L = 1,   a = 1e-7     (fastmath.h's documented figure)
      ELU (fm_expm1)            L = 1,   a = 4 u + 2e-10:  x > -1e-3 takes x + x^2 / 2, whose remainder is |x|^3 / 6 <= 1.7e-10 and
                                whose two roundings are part of u |f|; x <= -1e-3 takes __expf(x) - 1: the exponential is 2^(x log2 e),
                                its argument's rounding costs |x| log2(e) u relative, i.e. <= 1.45 u |x| e^x <= 0.53 u absolute, the
                                instruction itself 1 ulp of a value < 1 (<= u), and the subtraction is exact to u |f| - together < 4 u
  EPI_ADD            e + u |y|;   EPI_MUL   e |aux| + u |y|
  EPI_GLU            v = a sig(g):  e_a sig(g) + |a| (e_g / 4 + 8 u) + u |v|;  post-BatchNorm v s + h:  e |s| + 2 u (|v s| + |h|)
                     (s, h are formed in float64 on the host and rounded once: the reference uses the rounded values)
  dst_elu            ELU of the stored value: e + a_ELU + u |elu|
  fz                 sg = sig(v): e / 4 + 8 u;  re' = re + sg: + u |re'|;  S = re' + im': both + u |S|;
                     dst = v + sig(|z|): e + (4 u |z|) / 4 + 8 u + u |dst|  (|z| = sqrt(re^2 + im^2): three roundings and v_sqrt)
  riders             a sum of n fp32 additions: sum of the addends' own bounds + n u sum |x| (stats: n = 32; cstats: n = M outputs);
                     sums of squares likewise with 2 |x| e + e^2 per addend
  three products     the operands are rounded sums (Wi - Wr, Wr + Wi on the host, S = R + I on the device) and the outputs
                     differences of products, so the magnitude is that of the products: real  |Wr| * |S| + |Wr + Wi| * |x_i|,
                     imaginary  |Wr| * |S| + |Wi - Wr| * |x_r|  (* = the layer's conv), e0 = (4 K + 1) u magnitude - the + 1 is the
                     u of each rounded operand - then scale / shift / PReLU as above, and S = R + I: e_R + e_I + u |S|.

Nothing is excluded from a comparison: frames >= tlen[b] of dst, dst_elu and the three-plane outputs are documented zeros (layers.h
conv_zeroes_tail, gauss.h) and the riders do not count them.  The one exception to the zeros is a launch with `fz`: the interaction is
applied AFTER the mask in both store paths, as the stand-alone pass (launch_uf_fusion, which knows no tlen) would apply it to a zeroed
tensor, so those frames hold dst = 0 + sig(|z|) and fz = z + sig(0) = z + 0.5 - not zeros, although layers.h conv_zeroes_tail speaks of zeros
without that exception.  The reference
does the same and those frames are compared like every other.  The direct (<= 4 channel) path does not zero tails (layers.h): no ragged case uses it.
"""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_gemmconv_geometry import conv_f64, deconv_f64      # noqa: E402  (the references of the geometry suite, unchanged)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'sixty-years-of-frequency-domain-monaural-speech-enhancement_amd')
PROBE_LIB = os.environ.get('SE_EPIPROBE_LIB') or os.path.join(PKG, 'libse_epiprobe.so')

ACT_NONE, ACT_PRELU, ACT_ELU, ACT_SOFTPLUS, ACT_SIGMOID, ACT_TANH, ACT_RELU = range(7)
ACTS = dict(none=ACT_NONE, prelu=ACT_PRELU, elu=ACT_ELU, softplus=ACT_SOFTPLUS, sigmoid=ACT_SIGMOID, tanh=ACT_TANH, relu=ACT_RELU)
EPI_ACT, EPI_GLU, EPI_ADD, EPI_MUL, EPI_CMB = 0, 2, 3, 4, 5
EPIS = dict(act=EPI_ACT, add=EPI_ADD, mul=EPI_MUL, glu=EPI_GLU)
FAM_TILE, FAM_THIN, FAM_THIN_PAIR, FAM_DIRECT, FAM_DIRECT_LDS = 0, 1, 2, 3, 4
FORM_PLAIN, FORM_RES, FORM_TRIM, FORM_FZ = 0, 1, 2, 3
U24 = 2.0 ** -24
A_HW = 8 * U24            # hardware sigmoid / tanh
A_SOFTPLUS = 1e-7
A_ELU = 4 * U24 + 2e-10
NAN = float('nan')
GUARD = 256               # floats of sentinel behind every buffer


# ------------------------------------------------------------------------------------------------ float64 reference
def act_f64(v, e, act, slope):
    """f(v) and its bound from the bound e of v.  slope: [C] along dim 1 or None."""
    if act in (ACT_NONE,):
        return v, e
    if act in (ACT_PRELU, ACT_RELU):
        s = slope[None, :, None, None] if act == ACT_PRELU else torch.zeros((), dtype=v.dtype, device=v.device)
        y = torch.where(v >= 0, v, s * v)
        return y, e * torch.clamp(s.abs() + 0 * v, min=1.0) + U24 * y.abs()
    if act == ACT_ELU:
        y = torch.where(v > 0, v, torch.expm1(torch.clamp(v, max=0.0)))
        return y, e + A_ELU + U24 * y.abs()
    if act == ACT_SOFTPLUS:
        y = torch.where(v > 20, v, torch.log1p(torch.exp(torch.clamp(v, max=20.0))))
        return y, e + A_SOFTPLUS + U24 * y.abs()
    if act == ACT_SIGMOID:
        y = torch.sigmoid(v)
        return y, e / 4 + A_HW + U24 * y.abs()
    y = torch.tanh(v)
    return y, e + A_HW + U24 * y.abs()


def layer_conv(sh, x, w, Fout):
    if sh['kind'] == 'conv':
        return conv_f64(x, w, sh['sf'], sh['pf'], sh['pt'], sh.get('dil_f', 1), sh.get('dil_t', 1), Fout=Fout)
    pad = max(0, -sh['pf'])          # a left frequency pad: rows fo < pad see no input
    y = deconv_f64(x, w, sh['sf'], max(sh['pf'], 0), sh['toff'], Fout - pad)
    return torch.nn.functional.pad(y, (0, 0, pad, 0))


def epi_reference(sh, x, w, bias, T, Fout, *, act=ACT_NONE, epi=EPI_ACT, slope=None, post=None, bias_pad=None, aux=None, tlen=None,
                  fz=None, fz_planes=2, elu=False, stats=False, cstats=False, fault=None):
    """Everything one launch stores, in float64, each with its bound: dict name -> (value, bound).  x [B][Cin][Fin][T] (both sources
    concatenated), w [M][Cin][nkf][nkt], post = (scale, shift) [M / 2] as the plan holds them, fz [B][planes * C][Fout][T].
    fault: one deliberate defect of the reference (test_bound_catches_plausible_faults)."""
    B = x.shape[0]
    M = w.shape[0]
    K = w.shape[1] * w.shape[2] * w.shape[3]
    pre = layer_conv(sh, x, w, Fout)
    mag = layer_conv(sh, x.abs(), w.abs(), Fout)
    bb = bias[None, :, None, None].expand(B, M, Fout, T).clone()
    pad = max(0, -sh.get('pf', 0)) if sh['kind'] == 'deconv' else 0
    if pad and fault != 'bias_pad':
        bb[:, :, :pad] = bias_pad[None, :, None, None]
    pre = pre + bb
    e = 4 * U24 * K * (mag + bb.abs())
    if epi == EPI_GLU:
        a, g = (pre[:, 1::2], pre[:, 0::2]) if fault == 'glu_swap' else (pre[:, 0::2], pre[:, 1::2])
        ea, eg = e[:, 0::2], e[:, 1::2]
        sg = torch.sigmoid(g)
        v = a * sg
        e = ea * sg + a.abs() * (eg / 4 + A_HW) + U24 * v.abs()
        if post is not None:
            s, h = (p[None, :, None, None] for p in post)
            e = e * s.abs() + 2 * U24 * ((v * s).abs() + h.abs())
            v = v * s + h
        sl = slope
        if sl is not None:
            sl = sl[1::2][:M // 2] if fault == 'slope_row' else sl[:M // 2]       # (row 2 j + 1 instead of output j)
        y, e = act_f64(v, e, act, sl)
    else:
        y, e = act_f64(pre, e, act, slope)
    if epi == EPI_ADD:
        y = y + aux
        e = e + U24 * y.abs()
    elif epi == EPI_MUL:
        y = y * aux
        e = e * aux.abs() + U24 * y.abs()
    live = torch.ones((B, 1, 1, T), dtype=torch.float64, device=x.device)
    if tlen is not None:
        live = (torch.arange(T, device=x.device)[None, :] < tlen[:, None]).to(torch.float64)[:, None, None, :]
    y_raw = y
    y, e = y * live, e * live
    out = {}
    if elu:
        src = y_raw if fault == 'elu_premask' else y
        out['dst_elu'] = (torch.where(src > 0, src, torch.expm1(torch.clamp(src, max=0.0))), e + A_ELU + U24 * src.abs())
    if stats or cstats:
        yc = y_raw if fault == 'cstats_ragged' else y
        if stats:
            ns = -(-T // 32)
            padt = ns * 32 - T
            shift = 1 if fault == 'stats_shift' else 0
            ysh = torch.roll(y, shift, dims=-1) if shift else y
            yr = torch.nn.functional.pad(ysh, (0, padt)).view(*y.shape[:3], ns, 32)
            er = torch.nn.functional.pad(e, (0, padt)).view(*y.shape[:3], ns, 32)
            out['stats'] = (torch.stack([yr.sum(-1), (yr * yr).sum(-1)], -1),
                            torch.stack([(er + 32 * U24 * yr.abs()).sum(-1), (2 * yr.abs() * er + er * er + 32 * U24 * yr * yr).sum(-1)], -1))
        if cstats:
            n = y.shape[1]
            out['cstats'] = (torch.stack([yc.sum(1), (yc * yc).sum(1)], -1),
                             torch.stack([(e + n * U24 * yc.abs()).sum(1), (2 * yc.abs() * e + e * e + n * U24 * yc * yc).sum(1)], -1))
    if fz is not None:
        Cz = y.shape[1]
        re, im = fz[:, (fz_planes - 2) * Cz:(fz_planes - 1) * Cz], fz[:, (fz_planes - 1) * Cz:]
        cm = torch.sqrt(torch.clamp(re * re + im * im, min=2.0 ** -23))
        sg = torch.sigmoid(y)
        esg = e / 4 + A_HW
        k = 2 if fault == 'fz_twice' else 1
        re2, im2 = re + k * sg, im + k * sg
        ere, eim = esg + U24 * re2.abs(), esg + U24 * im2.abs()
        planes = [(re2, ere), (im2, eim)]
        if fz_planes == 3:
            S = re + im if fault == 'fz_s_stale' else re2 + im2
            planes.insert(0, (S, ere + eim + U24 * S.abs()))
        out['fz'] = (torch.cat([p[0] for p in planes], 1), torch.cat([p[1] for p in planes], 1))
        y = y + torch.sigmoid(cm)
        e = e + U24 * cm + A_HW + U24 * y.abs()
    out['dst'] = (y, e)
    return out


def gauss_reference(x3s, wr, wi, bias, bn, slope, T, Fout, *, deconv=False, toff=0, dst3=True, sum_plane=True, tlen=None, fault=None):
    """The COMPLEX layer y = PReLU(BN(W * x + bias)), out_r = Wr * x_r - Wi * x_i, out_i = Wi * x_r + Wr * x_i, of three-plane
    sources [B][3 C][Fin][T] (only their R and I planes are read; S enters the bound).  bias / slope [2 co], bn 4 x [2 co]."""
    co = wr.shape[0]
    S = torch.cat([x[:, :x.shape[1] // 3] for x in x3s], 1)
    R = torch.cat([x[:, x.shape[1] // 3:2 * x.shape[1] // 3] for x in x3s], 1)
    I = torch.cat([x[:, 2 * x.shape[1] // 3:] for x in x3s], 1)
    if fault == 'planes_swapped':
        R, I = I, R
    if deconv:
        f = lambda a, ww: deconv_f64(a, ww, 2, 2, toff, Fout)
        K = wr.shape[1] * 6
    else:
        f = lambda a, ww: conv_f64(a, ww, 2, 2, 1, Fout=Fout)
        K = wr.shape[1] * 10
    sgn = -1.0 if fault == 'cmb_neg' else 1.0
    yr = f(R, wr) - sgn * f(I, wi)
    yi = f(R, wi) + f(I, wr)
    wd, ws = (wi.float() - wr.float()).double(), (wr.float() + wi.float()).double()      # the rounded operands
    k1m = f(S.abs(), wr.abs())
    er = (4 * K + 1) * U24 * (k1m + f(I.abs(), ws.abs()))
    ei = (4 * K + 1) * U24 * (k1m + f(R.abs(), wd.abs()))
    ga, be, mu, va = bn
    kk = (ga / torch.sqrt(va + 1e-5)).float().double()
    hh = (be - mu * (ga / torch.sqrt(va + 1e-5)) + bias * (ga / torch.sqrt(va + 1e-5))).float().double()
    sl = slope
    if fault == 'ps_z':      # scale / shift / slope of the other half
        kk, hh, sl = torch.roll(kk, co), torch.roll(hh, co), torch.roll(slope, co)
    pre = torch.cat([yr, yi], 1)
    e = torch.cat([er, ei], 1)
    k4, h4 = kk[None, :, None, None], hh[None, :, None, None]
    e = e * k4.abs() + 3 * U24 * ((pre * k4).abs() + h4.abs())
    y, e = act_f64(pre * k4 + h4, e, ACT_PRELU, sl)
    if tlen is not None:
        live = (torch.arange(T, device=y.device)[None, :] < tlen[:, None]).to(torch.float64)[:, None, None, :]
        y, e = y * live, e * live
    if dst3 and sum_plane:
        Sy = y[:, :co] + y[:, co:]
        y = torch.cat([Sy, y], 1)
        e = torch.cat([e[:, :co] + e[:, co:] + U24 * Sy.abs(), e], 1)
    return y, e


# ------------------------------------------------------------------------------------------------ layers and inputs
TAPS = {
    'c32': dict(kind='conv', nkf=3, nkt=2, sf=1, pf=1, pt=1),                       # (3, 2) causal
    'd13': dict(kind='conv', nkf=1, nkt=3, sf=1, pf=0, pt=4, dil_t=2),              # (1, 3), time dilation 2, causal
    'pw': dict(kind='conv', nkf=1, nkt=1, sf=1, pf=0, pt=0),                        # pointwise
    's2': dict(kind='conv', nkf=3, nkt=2, sf=2, pf=1, pt=1),                        # frequency stride 2
    'dc': dict(kind='deconv', nkf=3, nkt=2, sf=2, pf=0, toff=0),                    # transposed, two parity classes
    'dcp': dict(kind='deconv', nkf=3, nkt=2, sf=2, pf=-1, toff=0),                  # ... behind a left frequency pad (bias_pad)
}


def layer_shape(taps, M, Cin, c0=-1, Fin=None):
    sh = dict(TAPS[taps], M=M, Cin=Cin, c0=c0, taps=taps)
    if sh['kind'] == 'conv':
        sh['Fin'] = Fin or (9 if taps == 's2' else 5)
        sh['Fout'] = (sh['Fin'] + 2 * sh['pf'] - (sh['nkf'] - 1) - 1) // sh['sf'] + 1
    else:
        sh['Fin'] = Fin or 4
        sh['Fout'] = 9
    return sh


def make_weights(sh, seed, epi, act):
    g = np.random.default_rng(seed)
    M, Cin = sh['M'], sh['Cin']
    K = Cin * sh['nkf'] * sh['nkt']
    p = dict(w=(g.standard_normal((M, Cin, sh['nkf'], sh['nkt'])) * (1.5 / math.sqrt(K))).astype(np.float32),
             bias=(0.3 * g.standard_normal(M)).astype(np.float32), slope=None, post=None, bias_pad=None)
    if act == ACT_PRELU:
        p['slope'] = g.uniform(0.05, 0.9, M).astype(np.float32)      # (EPI_GLU reads the first M / 2: one per OUTPUT)
    if epi == EPI_GLU:
        h = M // 2
        p['post'] = np.stack([g.uniform(0.5, 1.5, h), 0.3 * g.standard_normal(h), 0.2 * g.standard_normal(h), g.uniform(0.5, 2.0, h)]).astype(np.float32)
    if sh['kind'] == 'deconv' and sh['pf'] < 0:
        p['bias_pad'] = (0.5 + g.uniform(0.2, 1.0, M)).astype(np.float32)
    return p


def post_scale_shift(post, dev):
    """set_post_bn's fold: float64, rounded once"""
    ga, be, mu, va = (torch.from_numpy(post[i]).double().to(dev) for i in range(4))
    s = ga / torch.sqrt(va + 1e-5)
    return s.float().double(), (be - mu * s).float().double()


class Buf:
    """A device tensor [.., Tp] inside a flat NaN-filled allocation with a guard behind it."""
    def __init__(self, shape, dev, fill=NAN):
        n = int(np.prod(shape))
        self.flat = torch.full((n + GUARD,), fill, device=dev, dtype=torch.float32)
        self.t = self.flat[:n].view(*shape)
        self.n = n

    def ptr(self):
        return self.flat.data_ptr()

    def assert_unowned(self, T, what):
        assert bool(torch.isnan(self.flat[self.n:]).all()), f'{what}: the launch wrote behind the tensor'
        if self.t.shape[-1] > T:
            assert bool(torch.isnan(self.t[..., T:]).all()), f'{what}: the launch wrote row-pitch columns >= T'


def randn_into(buf, T, gen, scale=1.0):
    """random fp32 values in [.., :T]; the row-pitch columns behind get a value no stored result may show"""
    v = buf.t
    v[..., :T] = torch.randn(v[..., :T].shape, generator=gen, device=v.device) * scale
    if v.shape[-1] > T:
        v[..., T:] = 1.0e3


# ------------------------------------------------------------------------------------------------ the probe
class Lib:
    REC = ('family', 'BM', 'BN', 'form', 'Z', 'epi', 'qt2', 'res', 'trim', 'stats', 'ragged', 'flat_upr', 'nblk')
    INFO = ('BM', 'BN', 'nplans', 'direct', 'stats_ok', 'folds', 'zero_tail', 'pair')
    _lib = None

    @classmethod
    def get(cls):
        if cls._lib is None:
            assert os.path.exists(PROBE_LIB), f'{PROBE_LIB} is not built (make -C {PKG}/csrc)'
            lib = C.CDLL(PROBE_LIB)
            vp, i32, fp = C.c_void_p, C.c_int, C.POINTER(C.c_float)
            lib.epp_last_error.restype = C.c_char_p
            lib.epp_conv_create.restype = vp
            lib.epp_conv_create.argtypes = [fp, fp, fp, i32, fp] + [i32] * 12
            lib.epp_deconv_create.restype = vp
            lib.epp_deconv_create.argtypes = [fp, fp, fp, i32, fp, fp] + [i32] * 10
            lib.epp_destroy.argtypes = [vp]
            lib.epp_info.argtypes = [vp, C.POINTER(i32), i32]
            lib.epp_run.argtypes = [vp, vp, vp, i32, vp, i32, i32, i32, i32, i32, vp, i32, vp, vp, i32, vp, i32, vp]
            lib.epp_launch_get.argtypes = [i32, C.POINTER(C.c_longlong), i32]
            lib.epp_register_overread.argtypes = [vp, C.c_size_t]
            lib.epp_unregister_overread.argtypes = [vp]
            lib.epp_gauss_create.restype = vp
            lib.epp_gauss_create.argtypes = [fp] * 5 + [i32] * 5
            lib.epp_gauss_destroy.argtypes = [vp]
            lib.epp_gauss_run.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp, i32, i32, vp, vp]
            lib.epp_gauss_sum.argtypes = [vp, i32, i32, i32, i32]
            lib.epp_gauss_planes23.argtypes = [vp, vp, i32, C.c_long]
            cls._lib = lib
        return cls._lib

    @classmethod
    def records(cls):
        lib = cls.get()
        recs = []
        for i in range(lib.epp_launch_count()):
            out = (C.c_longlong * len(cls.REC))()
            lib.epp_launch_get(i, out, len(cls.REC))
            recs.append(dict(zip(cls.REC, out)))
        return recs

    @classmethod
    def error(cls):
        return cls.get().epp_last_error().decode()


def fptr(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32).ctypes.data_as(C.POINTER(C.c_float))


class Layer:
    def __init__(self, sh, p, act, epi):
        lib = Lib.get()
        self.sh, self.p, self.act, self.epi = sh, p, act, epi
        keep = {k: (None if v is None else np.ascontiguousarray(v, dtype=np.float32)) for k, v in p.items()}
        self._keep = keep
        ns = 0 if keep['slope'] is None else keep['slope'].size
        if sh['kind'] == 'conv':
            self.h = lib.epp_conv_create(fptr(keep['w']), fptr(keep['bias']), fptr(keep['slope']), ns, fptr(keep['post']), sh['M'], sh['Cin'],
                                         sh['nkf'], sh['nkt'], sh['sf'], sh['pf'], sh['pt'], sh.get('dil_f', 1), sh.get('dil_t', 1), act, epi,
                                         sh['c0'])
        else:
            self.h = lib.epp_deconv_create(fptr(keep['w']), fptr(keep['bias']), fptr(keep['slope']), ns, fptr(keep['post']),
                                           fptr(keep['bias_pad']), sh['M'], sh['Cin'], sh['nkf'], sh['nkt'], sh['sf'], sh['pf'], sh['toff'],
                                           act, epi, sh['c0'])
        assert self.h, Lib.error()
        out = (C.c_int * len(Lib.INFO))()
        lib.epp_info(self.h, out, len(Lib.INFO))
        self.info = dict(zip(Lib.INFO, out))

    def close(self):
        if self.h:
            Lib.get().epp_destroy(self.h)
            self.h = None


RATIO = {}          # group -> worst error / bound seen (printed per case; profiles/conv_epilogues.md)
REACHED = {}        # (BM or 'direct', epilogue, 'fz' | 'plain') -> the case that reached it


def compare(name, got, ref, bound, what, group):
    err = (got.double() - ref).abs()
    bad = ~(err <= bound)                # (NaN: a value that was never stored)
    ratio = float((err / bound.clamp(min=1e-300)).nan_to_num(nan=float('inf')).max()) if err.numel() else 0.0
    RATIO[group] = max(RATIO.get(group, 0.0), ratio)
    if bad.any():
        idx = bad.nonzero()[:5].tolist()
        i0 = tuple(idx[0])
        raise AssertionError(f'{name}: {int(bad.sum())} of {bad.numel()} values out of bound, first at {idx} (got {got[i0].item():.9g}, '
                             f'want {ref[i0].item():.9g}, bound {bound[i0].item():.3e}, worst err / bound {ratio:.3g}); {what}')
    return ratio


def run_layer_case(L, B, T, *, Tp=None, aux_xf0=False, elu=False, stats=False, cstats=False, fz_planes=0, tlen=None, seed=0,
                   group='misc', expect_refusal=None, overread=False, x_plant=None, extra_c=0):
    """One launch of layer L on random (or planted) sources, every operand asked for, everything stored compared with float64.
    extra_c: the tensors dst is laid out like have this many channels more than the layer writes (they must stay NaN)."""
    dev = 'cuda'
    sh, p, act, epi = L.sh, L.p, L.act, L.epi
    gen = torch.Generator(device=dev)
    gen.manual_seed(77 + seed)
    Tp = Tp or T
    M, Cin, Fin, Fout = sh['M'], sh['Cin'], sh['Fin'], sh['Fout']
    Mo = M // 2 if epi == EPI_GLU else M
    assert not (extra_c and fz_planes)
    dstC = Mo + extra_c
    C0 = Cin if sh['c0'] < 0 else sh['c0']
    srcs = [Buf((B, c, Fin, Tp), dev, 0.0) for c in ([C0] + ([Cin - C0] if C0 < Cin else []))]
    for s in srcs:
        randn_into(s, T, gen)
    if x_plant is not None:
        srcs[0].t[..., :T] = x_plant
    dst = Buf((B, dstC, Fout, Tp), dev)
    aux = None
    if epi in (EPI_ADD, EPI_MUL):
        aux = Buf((B, dstC, Fout, Tp), dev, 0.0)
        randn_into(aux, T, gen)
    de = Buf((B, dstC, Fout, Tp), dev) if elu else None
    ns = -(-T // 32)
    st = Buf((B, Fout, T, 2), dev) if cstats else (Buf((B, dstC, Fout, ns, 2), dev) if stats else None)
    fz = None
    if fz_planes:
        fz = Buf((B, fz_planes * dstC, Fout, Tp), dev, 0.0)
        randn_into(fz, T, gen)
        if fz_planes == 3:
            fz.t[:, :dstC] = NAN            # the S plane: rewritten by the launch
        fz0 = fz.t[..., :T].double().clone()
    tl = None if tlen is None else torch.as_tensor(tlen, dtype=torch.int32, device=dev)
    lib = Lib.get()
    if overread:
        for s in srcs:
            lib.epp_register_overread(s.ptr(), s.flat.numel() * 4)
    pt = lambda b: None if b is None else b.ptr()
    torch.cuda.synchronize()
    try:
        rc = lib.epp_run(L.h, srcs[0].ptr(), srcs[1].ptr() if len(srcs) > 1 else None, Fin, dst.ptr(), dstC, Fout, B, T, Tp, pt(aux),
                         int(aux_xf0), pt(de), pt(st), int(cstats), pt(fz), fz_planes or 2, None if tl is None else tl.data_ptr())
    finally:
        if overread:
            for s in srcs:
                lib.epp_unregister_overread(s.ptr())
    what = f'{sh} act={act} epi={epi} B={B} T={T} Tp={Tp} elu={elu} stats={stats} cstats={cstats} fz={fz_planes} tlen={tlen}'
    if expect_refusal is not None:
        assert rc != 0 and expect_refusal in Lib.error(), f'expected the launcher to refuse ("{expect_refusal}"), got rc={rc} "{Lib.error()}"; {what}'
        assert bool(torch.isnan(dst.flat).all()), f'a refused launch stored something; {what}'
        return []
    assert rc == 0, f'{Lib.error()}; {what}'
    recs = Lib.records()
    what += f' dispatches={recs}'
    d64 = lambda k: None if p[k] is None else torch.from_numpy(p[k]).double().to(dev)
    x64 = torch.cat([s.t[..., :T].double() for s in srcs], 1)
    ref = epi_reference(sh, x64, d64('w'), d64('bias'), T, Fout, act=act, epi=epi, slope=d64('slope'),
                        post=None if p['post'] is None else post_scale_shift(p['post'], dev), bias_pad=d64('bias_pad'),
                        aux=None if aux is None else aux.t[:, :Mo, :, :T].double(), tlen=None if tl is None else tl.long(),
                        fz=fz0 if fz_planes else None, fz_planes=fz_planes or 2, elu=elu, stats=stats and not cstats, cstats=cstats)
    worst = compare('dst', dst.t[:, :Mo, :, :T], *ref['dst'], what, group)
    dst.assert_unowned(T, 'dst; ' + what)
    assert bool(torch.isnan(dst.t[:, Mo:]).all()), f'dst: channels outside the layer were written; {what}'
    if elu:
        worst = max(worst, compare('dst_elu', de.t[:, :Mo, :, :T], *ref['dst_elu'], what, group))
        de.assert_unowned(T, 'dst_elu; ' + what)
        assert bool(torch.isnan(de.t[:, Mo:]).all()), f'dst_elu: channels outside the layer were written; {what}'
    if cstats:
        worst = max(worst, compare('cstats', st.t, *ref['cstats'], what, group + ' riders'))
        st.assert_unowned(2, 'cstats; ' + what)
    elif stats:
        worst = max(worst, compare('stats', st.t[:, :Mo], *ref['stats'], what, group + ' riders'))
        st.assert_unowned(2, 'stats; ' + what)
        # (run_conv fixes the layout at ceil(T / 32) slots per row: a store past a row's last group would land in the next row's
        # first slot - the rows of the channels outside the layer, right behind each batch item's last channel, show it)
        assert bool(torch.isnan(st.t[:, Mo:]).all()), f'stats: slots outside the layer were written; {what}'
    if fz_planes:
        worst = max(worst, compare('fz', fz.t[..., :T], *ref['fz'], what, group))
        assert bool((fz.flat[fz.n:] == 0).all()), f'fz: the launch wrote behind the tensor; {what}'
        if Tp > T:
            assert bool((fz.t[:, (fz_planes - 2) * dstC:, :, T:] == 1.0e3).all()) and \
                (fz_planes == 2 or bool(torch.isnan(fz.t[:, :dstC, :, T:]).all())), f'fz: row-pitch columns were written; {what}'
    for s in srcs + ([aux] if aux else []):
        assert bool((s.flat[s.n:] == 0).all()), f'an operand was written; {what}'
    print(f'[{group}] {sh["taps"]} M={M} epi={epi} act={act} B={B} T={T}: worst err / bound {worst:.3f} '
          f'forms {[(r["family"], r["BM"], r["BN"], r["form"]) for r in recs]}')
    for r in recs:
        assert r['epi'] == epi and r['Z'] == 1, what
        if L.info['direct']:
            assert r['family'] in (FAM_DIRECT, FAM_DIRECT_LDS, FAM_THIN), what
            REACHED.setdefault(('direct', epi, 'plain'), what)
        elif r['family'] == FAM_TILE:
            assert r['BM'] == L.info['BM'], what
            assert (r['form'] == FORM_FZ) == bool(fz_planes), what
            assert r['stats'] == int(stats or cstats) and r['ragged'] == int(tlen is not None), what
            assert r['form'] in (FORM_PLAIN, FORM_RES, FORM_FZ), what
            REACHED.setdefault((r['BM'], epi, {FORM_PLAIN: 'plain', FORM_RES: 'res', FORM_FZ: 'fz'}[r['form']]), what)
            REACHED.setdefault(('vector store' if T >= 4 else 'tail store', epi), what)
            if T % 4:
                REACHED.setdefault(('tail store', epi), what)
        else:
            assert r['family'] in (FAM_THIN, FAM_THIN_PAIR) and T <= 8 and not (stats or cstats or fz_planes), what
    return recs


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')


# ------------------------------------------------------------------------------------------------ epilogue cases (GPU)
T_SWEEP = (1, 3, 4, 5, 31, 32, 33, 36, 63, 64, 65, 100, 129)
# (M, taps, Cin): every tile height gc_plan_shape gives (M < 48: 32 rows, < 96: 64, else 128; <= 4: the direct path), the last m-tile
# partly filled except at M = 64 / 128
TILE_LAYERS = ((24, 'c32', 7), (40, 'd13', 5), (64, 's2', 16), (72, 's2', 9), (104, 'c32', 6), (128, 'c32', 6), (3, 'c32', 8))


def tile_rows(M, taps, Cin):
    """gc_select.h gc_plan_shape's tile height (pointwise layers of 96 .. 384 rows and <= 128 input channels take 64-row tiles)"""
    if taps == 'pw' and 96 <= M <= 384 and Cin <= 128:
        return 64
    return 128 if M >= 96 else (64 if M >= 48 else 32)
ACT_CYCLE = ('prelu', 'elu', 'softplus', 'sigmoid', 'tanh', 'relu', 'none')


def t_points(i):
    """four frame counts of the sweep per layer, rotating so that every count is used by some layer of each epilogue"""
    return [T_SWEEP[(3 * i + k * 4) % len(T_SWEEP)] for k in range(4)] + [T_SWEEP[(i * 2 + 1) % len(T_SWEEP)]]


@pytest.mark.gpu
@pytest.mark.parametrize('epi', ['act', 'add', 'mul'])
def test_epilogue_every_tile_height(epi):
    need_gpu()
    for i, (M, taps, Cin) in enumerate(TILE_LAYERS):
        act = ACTS[ACT_CYCLE[(i + len(epi)) % 7]]
        two = M == 40                                  # the two-source case of this epilogue
        sh = layer_shape(taps, M, Cin + (4 if two else 0), c0=Cin if two else -1)
        L = Layer(sh, make_weights(sh, 10 * i + len(epi), EPIS[epi], act), act, EPIS[epi])
        try:
            assert L.info['direct'] == int(M <= 4) and (M <= 4 or L.info['BM'] == tile_rows(M, taps, sh['Cin']))
            for k, T in enumerate(t_points(i)):
                run_layer_case(L, 1 if (i + k) % 2 else 3, T, Tp=T + 3 if k == 1 else None, seed=100 * i + T, group=f'EPI_{epi.upper()}',
                               overread=(k == 2), extra_c=3 if k == 3 else 0)
        finally:
            L.close()


@pytest.mark.gpu
@pytest.mark.parametrize('epi', ['act', 'add', 'mul'])
def test_epilogue_pointwise_and_xf0(epi):
    """pointwise layers on one-row tensors, the aux strides in the x_f = 0 form of blocks.h / model_uformer.hip"""
    need_gpu()
    for i, (M, Cin) in enumerate(((24, 5), (64, 16), (128, 12))):
        sh = layer_shape('pw', M, Cin, Fin=1)
        act = ACTS[ACT_CYCLE[(i + 2) % 7]]
        L = Layer(sh, make_weights(sh, 40 + i, EPIS[epi], act), act, EPIS[epi])
        try:
            for T in (5, 36, 65, 100):
                run_layer_case(L, 3 if T < 64 else 1, T, aux_xf0=epi != 'act', seed=T + i, group=f'EPI_{epi.upper()}', overread=T % 4 != 0)
        finally:
            L.close()


PLANT = np.array([-15.0, -5.0, -1.5e-3, -1.001e-3, -1.0e-3, -0.999e-3, -5e-4, -1e-7, 0.0, 1e-7, 0.5, 5.0, 15.0, 19.9, 20.0, 20.1, 25.0],
                 dtype=np.float32)


def planted_layer(M, Cin, epi):
    """a pointwise layer whose pre-activations ARE its inputs: row m copies channel m % Cin (EPI_GLU: value row 2 j copies, gate row
    2 j + 1 has bias 30, sig = 1 to 1e-13)"""
    w = np.zeros((M, Cin, 1, 1), np.float32)
    bias = np.zeros(M, np.float32)
    for m in range(M):
        if epi == EPI_GLU and m % 2:
            bias[m] = 30.0
        else:
            w[m, (m // 2 if epi == EPI_GLU else m) % Cin, 0, 0] = 1.0
    return w, bias


@pytest.mark.gpu
@pytest.mark.parametrize('epi', ['act', 'add', 'mul', 'glu'])
@pytest.mark.parametrize('act', list(ACTS))
def test_every_activation_at_its_edges(epi, act):
    """both sides of 0, both sides of fm_expm1's switch at -1e-3, softplus beyond 20, |x| to 15 and beyond: in both store paths"""
    need_gpu()
    M, Cin = (2 * 18, 7) if epi == 'glu' else (40, 7)
    sh = layer_shape('pw', M, Cin, Fin=5)
    p = make_weights(sh, 5, EPIS[epi], ACTS[act])
    p['w'], p['bias'] = planted_layer(M, Cin, EPIS[epi])
    if p['post'] is not None:
        p['post'] = np.stack([np.ones(M // 2), np.zeros(M // 2), np.zeros(M // 2), np.ones(M // 2) - 1e-5]).astype(np.float32)
    L = Layer(sh, p, ACTS[act], EPIS[epi])
    try:
        for B, T in ((3, 33), (1, 36)):
            c, f, t = np.meshgrid(np.arange(Cin), np.arange(5), np.arange(T), indexing='ij')
            xp = torch.from_numpy(PLANT[(t + 3 * c + f) % len(PLANT)]).cuda()[None].expand(B, -1, -1, -1)
            run_layer_case(L, B, T, x_plant=xp, seed=T, group='activations')
    finally:
        L.close()


@pytest.mark.gpu
@pytest.mark.parametrize('M', [2 * 12, 2 * 18, 2 * 30, 2 * 64])
def test_glu_pairs_post_bn_slope_and_elu_store(M):
    need_gpu()
    for i, taps in enumerate(('c32', 's2', 'd13')):
        two = i == 1
        sh = layer_shape(taps, M, 6 + i + (4 if two else 0), c0=6 + i if two else -1)
        act = (ACT_PRELU, ACT_NONE, ACT_ELU)[i]
        L = Layer(sh, make_weights(sh, M + i, EPI_GLU, act), act, EPI_GLU)
        try:
            assert L.info['stats_ok']
            for k, T in enumerate(t_points(i + M)):
                run_layer_case(L, 3 if k % 2 else 1, T, Tp=T + 5 if k == 0 else None, elu=True, stats=(k % 2 == 0 and T > 8), seed=M + T,
                               group='EPI_GLU', extra_c=k % 3)
            run_layer_case(L, 3, 65, elu=True, stats=True, tlen=[65, 31, 4], seed=9, group='EPI_GLU ragged')
        finally:
            L.close()


@pytest.mark.gpu
@pytest.mark.parametrize('epi', ['act', 'glu'])
def test_deconv_pad_lo_rows_take_bias_pad(epi):
    need_gpu()
    M = 40 if epi == 'act' else 36
    sh = layer_shape('dcp', M, 6)
    L = Layer(sh, make_weights(sh, 3, EPIS[epi], ACT_PRELU), ACT_PRELU, EPIS[epi])
    try:
        for B, T in ((1, 33), (3, 36), (1, 100)):
            run_layer_case(L, B, T, seed=T, group='bias_pad')
    finally:
        L.close()


@pytest.mark.gpu
def test_stats_rider_on_64_row_act_tiles():
    need_gpu()
    for taps, M, Cin in (('c32', 64, 8), ('dc', 56, 6)):
        sh = layer_shape(taps, M, Cin)
        L = Layer(sh, make_weights(sh, 21, EPI_ACT, ACT_NONE), ACT_NONE, EPI_ACT)
        try:
            assert L.info['stats_ok']
            for B, T in ((1, 31), (3, 33), (1, 64), (3, 100), (1, 129)):
                run_layer_case(L, B, T, stats=True, seed=T, group='stats', extra_c=2 if B == 3 else 0)
            run_layer_case(L, 3, 100, stats=True, tlen=[100, 33, 64], seed=1, group='stats ragged', extra_c=1)
        finally:
            L.close()
    # tiles without the rider refuse it
    sh = layer_shape('c32', 24, 7)
    L = Layer(sh, make_weights(sh, 22, EPI_ACT, ACT_NONE), ACT_NONE, EPI_ACT)
    try:
        assert not L.info['stats_ok']
        run_layer_case(L, 1, 36, stats=True, expect_refusal='no statistics epilogue')
    finally:
        L.close()


@pytest.mark.gpu
def test_cstats_rider():
    """per (b, row, frame) sums over ALL output channels; gemmconv.h: 'same tile configurations, one m-tile' - a layer of two m-tiles
    is refused"""
    need_gpu()
    for taps, M, Cin, epi in (('c32', 64, 8, EPI_ACT), ('dc', 56, 6, EPI_ACT), ('s2', 2 * 16, 7, EPI_GLU), ('dc', 2 * 24, 6, EPI_GLU)):
        sh = layer_shape(taps, M, Cin)
        L = Layer(sh, make_weights(sh, 31, epi, ACT_PRELU), ACT_PRELU, epi)
        try:
            for B, T in ((3, 5), (1, 33), (3, 36), (1, 100), (3, 129)):
                run_layer_case(L, B, T, cstats=True, seed=T, group='cstats')      # (T = 5: the riders keep a few-frame launch on the tiles)
            run_layer_case(L, 3, 65, cstats=True, tlen=[65, 32, 9], seed=2, group='cstats ragged')
        finally:
            L.close()
    sh = layer_shape('c32', 2 * 80, 6)          # 160 rows: two 128-row m-tiles of the gated kernel
    L = Layer(sh, make_weights(sh, 32, EPI_GLU, ACT_NONE), ACT_NONE, EPI_GLU)
    try:
        run_layer_case(L, 1, 36, cstats=True, expect_refusal='column statistics need')
    finally:
        L.close()


@pytest.mark.gpu
@pytest.mark.parametrize('epi', ['act', 'add'])
@pytest.mark.parametrize('planes', [2, 3])
def test_fz_interaction_applied_exactly_once(epi, planes):
    need_gpu()
    cases = (('c32', 24, 7), ('dc', 40, 6), ('pw', 64, 16), ('s2', 72, 9), ('dc', 128, 5))
    for i, (taps, M, Cin) in enumerate(cases):
        sh = layer_shape(taps, M, Cin)
        act = ACT_PRELU if i % 2 else ACT_NONE
        L = Layer(sh, make_weights(sh, 50 + i, EPIS[epi], act), act, EPIS[epi])
        try:
            assert L.info['folds']
            for k, T in enumerate((33, 36, 100) if i % 2 else (31, 64, 129)):
                run_layer_case(L, 3 if k == 0 else 1, T, Tp=T + 4 if k == 1 else None, fz_planes=planes, seed=T + i, group='FZ')
            run_layer_case(L, 3, 36, fz_planes=planes, tlen=[36, 5, 20], seed=4, group='FZ ragged')
        finally:
            L.close()


@pytest.mark.gpu
def test_fz_refusals():
    need_gpu()
    sh = layer_shape('c32', 3, 8)
    L = Layer(sh, make_weights(sh, 60, EPI_ACT, ACT_NONE), ACT_NONE, EPI_ACT)
    try:
        run_layer_case(L, 1, 36, fz_planes=2, expect_refusal='direct')
    finally:
        L.close()
    sh = layer_shape('c32', 40, 8)
    L = Layer(sh, make_weights(sh, 61, EPI_MUL, ACT_NONE), ACT_NONE, EPI_MUL)
    try:
        run_layer_case(L, 1, 36, fz_planes=2, expect_refusal='cannot fold the branch interaction')
    finally:
        L.close()
    sh = layer_shape('c32', 64, 8)
    L = Layer(sh, make_weights(sh, 62, EPI_ACT, ACT_NONE), ACT_NONE, EPI_ACT)
    try:
        run_layer_case(L, 1, 36, fz_planes=2, stats=True, expect_refusal='statistics variant')
    finally:
        L.close()


@pytest.mark.gpu
@pytest.mark.parametrize('epi', ['act', 'add', 'mul', 'glu'])
def test_ragged_rows_on_each_epilogue(epi):
    need_gpu()
    for taps, M, Cin in (('c32', 24, 7), ('s2', 64, 8), ('dc', 104, 6)):
        sh = layer_shape(taps, M, Cin)
        L = Layer(sh, make_weights(sh, 70, EPIS[epi], ACT_TANH), ACT_TANH, EPIS[epi])
        try:
            assert L.info['zero_tail']
            run_layer_case(L, 3, 33, tlen=[33, 7, 32], seed=1, group='ragged')
            run_layer_case(L, 3, 100, Tp=104, tlen=[61, 100, 1], seed=2, group='ragged')
        finally:
            L.close()


# ------------------------------------------------------------------------------------------------ three-product cases (GPU)
def gauss_params(co, ci, seed):
    g = np.random.default_rng(seed)
    f = lambda *s: g.standard_normal(s).astype(np.float32)
    wr, wi = f(co, ci, 5, 2) / math.sqrt(10 * ci), f(co, ci, 5, 2) / math.sqrt(10 * ci)
    br, bi = 0.2 * f(co), 0.2 * f(co)
    bias = np.concatenate([br - bi, br + bi]).astype(np.float32)             # layers.h complex_expand
    bn = np.stack([g.uniform(0.5, 1.5, 2 * co), 0.3 * g.standard_normal(2 * co), 0.2 * g.standard_normal(2 * co),
                   g.uniform(0.5, 2.0, 2 * co)]).astype(np.float32)
    slope = g.uniform(0.05, 0.9, 2 * co).astype(np.float32)
    return dict(wr=wr.astype(np.float32), wi=wi.astype(np.float32), br=br, bi=bi, bias=bias, bn=bn, slope=slope)


def three_planes(B, C, F, T, gen, dev):
    """[B][3 C][F][T] = S | R | I with S = R + I rounded to fp32, as launch_sum leaves it"""
    b = Buf((B, 3 * C, F, T), dev, 0.0)
    b.t[:, C:] = torch.randn((B, 2 * C, F, T), generator=gen, device=dev)
    b.t[:, :C] = b.t[:, C:2 * C] + b.t[:, 2 * C:]
    return b


def gauss_layer(co, ci, deconv, toff, c0, seed):
    gp = gauss_params(co, ci, seed)
    h = Lib.get().epp_gauss_create(fptr(gp['wr']), fptr(gp['wi']), fptr(gp['bias']), fptr(gp['bn']), fptr(gp['slope']), co, ci, int(deconv), toff,
                                   c0)
    assert h, Lib.error()
    return h, gp


def run_gauss_case(co, ci, Fin, Fout, B, T, *, deconv=False, toff=0, c0=-1, dst3=True, sum_plane=True, tlen=None, seed=0, group='gauss',
                   expect_cmb=None, layer=None, cover=None):
    """layer: (handle, parameters) of gauss_layer() to run on (else one is built for the case); cover: a set that receives
    (combine epilogue?, T, dst3, sum_plane, B) of the case"""
    dev = 'cuda'
    lib = Lib.get()
    h, gp = layer or gauss_layer(co, ci, deconv, toff, c0, seed)
    try:
        gen = torch.Generator(device=dev)
        gen.manual_seed(500 + seed)
        C0 = ci if c0 < 0 else c0
        srcs = [three_planes(B, c, Fin, T, gen, dev) for c in ([C0] + ([ci - C0] if C0 < ci else []))]
        CP = co * Fout * T
        dst = Buf((B, (3 if dst3 else 2) * co, Fout, T), dev)
        K = Buf((3, B, co, Fout, T), dev)
        tl = None if tlen is None else torch.as_tensor(tlen, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        rc = lib.epp_gauss_run(h, srcs[0].ptr(), srcs[1].ptr() if len(srcs) > 1 else None, Fin, Fout, B, T, dst.ptr(), int(dst3),
                               int(sum_plane), K.ptr(), None if tl is None else tl.data_ptr())
        recs = Lib.records()
        what = f'co={co} ci={ci} c0={c0} Fin={Fin} Fout={Fout} B={B} T={T} deconv={deconv} toff={toff} dst3={dst3} sum={sum_plane} ' \
               f'tlen={tlen} dispatches={recs}'
        assert rc == 0, f'{Lib.error()}; {what}'
        d = lambda k: torch.from_numpy(gp[k]).double().to(dev)
        ref, bound = gauss_reference([s.t.double() for s in srcs], d('wr'), d('wi'), d('bias'), d('bn'), d('slope'), T, Fout, deconv=deconv,
                                     toff=toff, dst3=dst3, sum_plane=sum_plane, tlen=None if tl is None else tl.long())
        got = dst.t
        if dst3 and not sum_plane:
            assert bool(torch.isnan(got[:, :co]).all()), f'the S plane was written without sum_plane; {what}'
            got = got[:, co:]
        worst = compare('planes ' + ('S|R|I' if dst3 and sum_plane else 'R|I'), got, ref, bound, what, group)
        dst.assert_unowned(T, 'dst; ' + what)
        assert bool(torch.isnan(K.flat[K.n:]).all()), f'the launch wrote behind K; {what}'
        for s in srcs:
            assert bool((s.flat[s.n:] == 0).all()), what
        cmb = any(r['epi'] == EPI_CMB for r in recs)
        if expect_cmb is not None:
            assert cmb == expect_cmb, what
        ncls = 2 if deconv else 1
        BM = 128 if co >= 96 else (64 if co >= 48 else 32)
        # (the k1 launch of a few frames takes the thin form; everything else is a tile of the layer's height)
        assert all((r['family'] == FAM_TILE and r['BM'] == BM) or (r['family'] == FAM_THIN and T <= 8 and r['epi'] == EPI_ACT and r['Z'] == 1)
                   for r in recs), what
        if cmb:
            zs = [r['Z'] for r in recs]
            assert zs == ([1, 1, 1] if sum_plane else [1, 2]) * ncls, what
            assert [r['epi'] for r in recs] == ([EPI_ACT, EPI_CMB, EPI_CMB] if sum_plane else [EPI_ACT, EPI_CMB]) * ncls, what
            assert bool(torch.isnan(K.t[1:]).all()), f'the combine epilogue needs k1 only, K beyond it was written; {what}'
            REACHED.setdefault((BM, EPI_CMB, 'sum' if sum_plane else 'pair'), what)
        else:
            assert [r['Z'] for r in recs] == [3] * ncls and all(r['epi'] == EPI_ACT for r in recs), what
            REACHED.setdefault(('combine kernel', 'vector' if T % 4 == 0 else 'scalar'), what)
        print(f'[{group}] co={co} ci={ci} {"dec" if deconv else "enc"} Fout={Fout} B={B} T={T} dst3={dst3} sum={sum_plane} cmb={cmb}: '
              f'worst err / bound {worst:.3f}')
        if cover is not None:
            cover.add((cmb, T, dst3, sum_plane, B))
    finally:
        if layer is None:
            lib.epp_gauss_destroy(h)


def assert_grid_covered(cover, co, Ts, what):
    """every frame count with every plane form and both batch sizes, on the path it belongs to"""
    want = {(co >= 64 and T % 4 == 0, T, d3, sp, B) for T in Ts for d3, sp in PLANES for B in (1, 3)}
    assert want <= cover, f'{what}: not run: {sorted(want - cover)}'


PLANES = ((False, False), (True, False), (True, True))


def gauss_frames(co):
    """the issue's frame counts: (4, 8, 36, 100, 132) - at co >= 64 the combine epilogue - and at co = 32 (1, 3, 5, 33, 101) as
    well; co >= 64 also gets 33, which no 16 B group divides: Z = 3 and the combine kernel's scalar branch"""
    return (4, 8, 36, 100, 132) + ((1, 3, 5, 33, 101) if co == 32 else (33,))


@pytest.mark.gpu
@pytest.mark.parametrize('co', [32, 64, 128])
def test_three_product_encoder(co):
    """the whole grid: (ci, Fin) x T x plane form x B"""
    need_gpu()
    cover = set()
    for blk, (ci, Fin) in enumerate(((6, 8), (6, 9), (16, 8), (16, 9))):
        Fout = (Fin + 4 - 4 - 1) // 2 + 1
        layer = gauss_layer(co, ci, False, 0, -1, blk)
        try:
            for T in gauss_frames(co):
                for dst3, sp in PLANES:
                    for B in (1, 3):
                        run_gauss_case(co, ci, Fin, Fout, B, T, dst3=dst3, sum_plane=sp, seed=blk + T, group=f'gauss enc co={co}',
                                       expect_cmb=(co >= 64 and T % 4 == 0), layer=layer, cover=cover)
        finally:
            Lib.get().epp_gauss_destroy(layer[0])
    assert_grid_covered(cover, co, gauss_frames(co), f'encoder co={co}')
    for dst3, sp in PLANES:
        run_gauss_case(co, 6, 9, 5, 3, 36, dst3=dst3, sum_plane=sp, tlen=[36, 9, 20], seed=7, group='gauss ragged', expect_cmb=co >= 64)
    run_gauss_case(co, 6, 9, 5, 3, 33, tlen=[33, 9, 32], seed=8, group='gauss ragged', expect_cmb=False)


@pytest.mark.gpu
@pytest.mark.parametrize('co', [32, 64, 128])
def test_three_product_decoder(co):
    """(Fout, toff, sources) x T, the (plane form, B) pair stepping with the frame count AND the block, so that over the eight
    blocks every frame count meets all six pairs (asserted)"""
    need_gpu()
    cover = set()
    pairs = [(pl, B) for pl in PLANES for B in (1, 3)]
    blocks = [(Fout, toff, c0) for Fout in (8, 9) for toff in (0, 1) for c0 in (-1, 6)]
    for blk, (Fout, toff, c0) in enumerate(blocks):
        layer = gauss_layer(co, 10, True, toff, c0, 20 + blk)
        try:
            for ti, T in enumerate(gauss_frames(co)):
                (dst3, sp), B = pairs[(ti + blk) % 6]
                run_gauss_case(co, 10, 4, Fout, B, T, deconv=True, toff=toff, c0=c0, dst3=dst3, sum_plane=sp, seed=blk + T,
                               group=f'gauss dec co={co}', expect_cmb=(co >= 64 and T % 4 == 0), layer=layer, cover=cover)
        finally:
            Lib.get().epp_gauss_destroy(layer[0])
    assert_grid_covered(cover, co, gauss_frames(co), f'decoder co={co}')
    run_gauss_case(co, 10, 4, 9, 3, 36, deconv=True, toff=1, c0=6, tlen=[36, 9, 20], seed=7, group='gauss ragged', expect_cmb=co >= 64)
    run_gauss_case(co, 10, 4, 8, 3, 5, deconv=True, tlen=[5, 1, 4], dst3=False, sum_plane=False, seed=8, group='gauss ragged', expect_cmb=False)


_CMB0_CHILD = """
import sys
sys.path.insert(0, {tests!r})
import test_gpu_conv_epilogues as t
for T, planes in ((36, (True, True)), (100, (False, False)), (8, (True, False))):
    t.run_gauss_case(128, 6, 9, 5, 3, T, dst3=planes[0], sum_plane=planes[1], seed=T, expect_cmb=False)
t.run_gauss_case(128, 10, 4, 9, 1, 36, deconv=True, toff=1, c0=6, seed=3, expect_cmb=False)
print('CMB0 OK', max(t.RATIO.values()))
"""


@pytest.mark.gpu
def test_three_product_without_the_combine_epilogue():
    """SE_GAUSS_CMB=0 (read once per process): co = 128 through the Z = 3 launch and gauss_combine_kernel, in one fresh child"""
    need_gpu()
    env = dict(os.environ, SE_GAUSS_CMB='0')
    r = subprocess.run([sys.executable, '-c', _CMB0_CHILD.format(tests=os.path.dirname(os.path.abspath(__file__)))], env=env,
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and 'CMB0 OK' in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
@pytest.mark.parametrize('CP', [4, 5, 7, 1020, 1023, 1024, 1025, 1027, 2052])
def test_sum_and_planes23_kernels(CP):
    """S = R + I and [R | I] -> [S | R | I] are exact to one rounding; CP % 4 in {0, 1, 3}, around one block's span of 1024"""
    need_gpu()
    dev = 'cuda'
    lib = Lib.get()
    gen = torch.Generator(device=dev)
    gen.manual_seed(CP)
    for B in (1, 3):
        t3 = Buf((B, 3, CP), dev)
        t3.t[:, 1:] = torch.randn((B, 2, CP), generator=gen, device=dev)
        want = t3.t[:, 1:].clone()
        assert lib.epp_gauss_sum(t3.ptr(), B, 1, 1, CP) == 0, Lib.error()
        assert torch.equal(t3.t[:, 0], want[:, 0] + want[:, 1]) and torch.equal(t3.t[:, 1:], want)
        assert bool(torch.isnan(t3.flat[t3.n:]).all())
        x2 = Buf((B, 2, CP), dev, 0.0)
        x2.t[:] = torch.randn((B, 2, CP), generator=gen, device=dev)
        x3 = Buf((B, 3, CP), dev)
        assert lib.epp_gauss_planes23(x2.ptr(), x3.ptr(), B, CP) == 0, Lib.error()
        assert torch.equal(x3.t[:, 0], x2.t[:, 0] + x2.t[:, 1]) and torch.equal(x3.t[:, 1:], x2.t)
        assert bool(torch.isnan(x3.flat[x3.n:]).all()) and bool((x2.flat[x2.n:] == 0).all())
    REACHED.setdefault(('sum / planes23', CP % 4), CP)


TARGETS = [(bm, e, 'plain') for bm in (32, 64, 128, 'direct') for e in (EPI_ACT, EPI_ADD, EPI_MUL)] + \
          [(bm, EPI_GLU, 'plain') for bm in (32, 64, 128)] + \
          [(bm, e, 'fz') for bm in (32, 64, 128) for e in (EPI_ACT, EPI_ADD)] + \
          [(bm, EPI_CMB, k) for bm in (64, 128) for k in ('pair', 'sum')] + \
          [(s, e) for s in ('vector store', 'tail store') for e in (EPI_ACT, EPI_ADD, EPI_MUL, EPI_GLU)] + \
          [('combine kernel', 'vector'), ('combine kernel', 'scalar'), ('sum / planes23', 0), ('sum / planes23', 1), ('sum / planes23', 3)]


@pytest.mark.gpu
def test_every_targeted_form_is_reached():
    """Runs last in this file: every (tile height, epilogue, plain / FZ) the models use, both store paths of each epilogue, the
    combine epilogue with and without the sum plane on both tile heights, both branches of the elementwise kernels."""
    need_gpu()
    for k, v in sorted(RATIO.items()):
        print(f'worst err / bound [{k}]: {v:.3f}')
    missing = [t for t in TARGETS if t not in REACHED]
    assert not missing, f'not reached: {missing}'


# ------------------------------------------------------------------------------------------------ CPU parts
def test_reference_matches_torch_and_the_oracle():
    """the float64 complex layer of gauss_reference against the reference's four-conv form (oracle/nnops.py) and against torch, on one
    encoder and one decoder layer"""
    sys.path.insert(0, ROOT)
    from oracle import nnops
    co, ci, B, T = 4, 3, 2, 7
    gp = gauss_params(co, ci, 1)
    g = np.random.default_rng(2)
    d = lambda k: torch.from_numpy(gp[k]).double()
    sl = gp['slope'].astype(np.float64)
    for deconv, Fin, Fout, toff in ((False, 9, 5, 0), (True, 4, 8, 1)):
        R, I = g.standard_normal((B, ci, Fin, T)), g.standard_normal((B, ci, Fin, T))
        x3 = torch.from_numpy(np.concatenate([R + I, R, I], 1))
        y, _ = gauss_reference([x3], d('wr'), d('wi'), d('bias'), d('bn'), d('slope'), T, Fout, deconv=deconv, toff=toff, dst3=False,
                               sum_plane=False)
        wr, wi = gp['wr'].astype(np.float64), gp['wi'].astype(np.float64)
        br, bi = gp['br'].astype(np.float64), gp['bi'].astype(np.float64)
        if not deconv:
            pad = lambda a: np.pad(a, ((0, 0), (0, 0), (0, 0), (1, 0)))
            cv = lambda a, w, b: nnops.conv2d(pad(a), w, b, stride=(2, 1), padding=(2, 0))
            tc = lambda a, w, b: torch.nn.functional.conv2d(torch.from_numpy(pad(a)), torch.from_numpy(w), torch.from_numpy(b), stride=(2, 1),
                                                            padding=(2, 0)).numpy()
        else:
            wt = lambda w: np.ascontiguousarray(w.transpose(1, 0, 2, 3))
            crop = lambda a: a[:, :, :Fout, toff:toff + T]
            cv = lambda a, w, b: crop(nnops.conv_transpose2d(a, wt(w), b, stride=(2, 1), padding=(2, 0), output_padding=(1, 0)))
            tc = lambda a, w, b: crop(torch.nn.functional.conv_transpose2d(torch.from_numpy(a), torch.from_numpy(wt(w)), torch.from_numpy(b),
                                                                           stride=(2, 1), padding=(2, 0), output_padding=(1, 0)).numpy())
        for f in (cv, tc):
            # complexnn: real = real_conv(real) - imag_conv(imag), imag = real_conv(imag) + imag_conv(real), each conv with its own bias
            out = np.concatenate([f(R, wr, br) - f(I, wi, bi), f(I, wr, br) + f(R, wi, bi)], 1)
            z = nnops.batchnorm(out, gp['bn'][0].astype(np.float64), gp['bn'][1].astype(np.float64), gp['bn'][2].astype(np.float64),
                                gp['bn'][3].astype(np.float64))
            z = np.where(z >= 0, z, sl[None, :, None, None] * z)
            # fold_tail rounds scale and shift to fp32, and the bias enters as fp32(br -+ bi): 3 roundings of O(1) values
            assert np.abs(z - y.numpy()).max() < 16 * U24 * max(1.0, np.abs(z).max()), (deconv, np.abs(z - y.numpy()).max())


def _small_case(kind, seed=0):
    """the smallest shapes of the GPU matrix, on the CPU: sources, weights, reference keyword arguments"""
    g = torch.Generator()
    g.manual_seed(seed)
    if kind == 'gauss':
        co, ci, B, T, Fin, Fout = 32, 6, 3, 5, 9, 5
        gp = gauss_params(co, ci, seed)
        x = torch.randn((B, 2 * ci, Fin, T), generator=g).double()
        x3 = torch.cat([(x[:, :ci].float() + x[:, ci:].float()).double(), x], 1)
        d = lambda k: torch.from_numpy(gp[k]).double()
        return lambda fault=None: gauss_reference([x3], d('wr'), d('wi'), d('bias'), d('bn'), d('slope'), T, Fout, tlen=torch.tensor([5, 1, 4]),
                                                  fault=fault)
    epi, taps, M, act = dict(glu=(EPI_GLU, 'c32', 24, ACT_PRELU), fz=(EPI_ACT, 'c32', 24, ACT_NONE), pad=(EPI_ACT, 'dcp', 40, ACT_PRELU))[kind]
    sh = layer_shape(taps, M, 6)
    p = make_weights(sh, seed, epi, act)
    B, T = 3, 33
    x = torch.randn((B, 6, sh['Fin'], T), generator=g).double()
    dC = M // 2 if epi == EPI_GLU else M
    fz = torch.randn((B, 3 * dC, sh['Fout'], T), generator=g).double()
    d = lambda k: None if p[k] is None else torch.from_numpy(p[k]).double()
    kw = dict(act=act, epi=epi, slope=d('slope'), post=None if p['post'] is None else post_scale_shift(p['post'], 'cpu'), bias_pad=d('bias_pad'),
              tlen=torch.tensor([33, 7, 32]), elu=epi == EPI_GLU, stats=epi == EPI_GLU, cstats=epi == EPI_GLU,
              fz=fz if kind == 'fz' else None, fz_planes=3)
    return lambda fault=None: epi_reference(sh, x, d('w'), d('bias'), T, sh['Fout'], fault=fault, **kw)


FAULTS = [('gauss', 'cmb_neg', None), ('gauss', 'planes_swapped', None), ('gauss', 'ps_z', None), ('glu', 'glu_swap', 'dst'),
          ('glu', 'slope_row', 'dst'), ('glu', 'elu_premask', 'dst_elu'), ('fz', 'fz_twice', 'fz'), ('fz', 'fz_s_stale', 'fz'),
          ('glu', 'stats_shift', 'stats'), ('glu', 'cstats_ragged', 'cstats'), ('pad', 'bias_pad', 'dst')]


@pytest.mark.parametrize('kind,fault,key', FAULTS)
def test_bound_catches_plausible_faults(kind, fault, key):
    """each defect, put into the float64 reference alone, moves some element by more than its bound (and by much more: the bound
    is no slack a real defect could hide in)"""
    ref = _small_case(kind)
    good, bad = ref(), ref(fault)
    if kind == 'gauss':
        (y, e), (yb, _) = good, bad
    else:
        (y, e), (yb, _) = good[key], bad[key]
    over = ((yb - y).abs() / e.clamp(min=1e-300))
    assert float(over.max()) > 100.0, f'{fault}: the largest deviation is {float(over.max()):.3g} bounds'


def test_reference_riders_and_masks_on_the_cpu():
    """the reference's own bookkeeping: ragged frames are zeros in dst / dst_elu, the riders count exactly the stored values"""
    out = _small_case('glu')()
    y = out['dst'][0]
    assert bool((y[1, :, :, 7:] == 0).all()) and bool((out['dst_elu'][0][1, :, :, 7:] == 0).all()) and bool((y[0] != 0).any())
    assert torch.allclose(out['cstats'][0][..., 0], y.sum(1)) and torch.allclose(out['stats'][0][..., 0].sum(-1), y.sum(-1))
