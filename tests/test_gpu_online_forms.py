"""The frame-online layer path against float64, chunk by chunk.  A stream of at most 3 rows is pushed in chunks through the code a
frame-online model runs between its STFT and its iSTFT (csrc/tests/online_probe.hip -> libse_onlineprobe.so): the chain kernel of
the cLN TCM blocks (csrc/k_tcm_stream.hip tcm_chain_kernel<3 | 5> through blocks.h run_tcm_chain), one conv / transposed-conv layer
on a window of H history columns + n new frames (layers.hip run_conv / run_deconv under a published StreamScope, or with explicit
t_base / t_out / tb_soft), and the history movers (k_misc.hip stream_exchange, stream_exchange_pair, launch_hist_*).  Every chunk's
new frames are compared, element by element, with a float64 computation of the WHOLE sequence at once.

References and bounds are those of the sibling suites: conv_f64 / deconv_f64 and the 4 u K (sum |w| |x| + |bias|) bound of
tests/test_gpu_gemmconv_geometry.py; the cumulative-LayerNorm / FIR / dilated-conv error model of tests/test_gpu_norm_forms.py
(affine_bound, fir_apply, dconv and its constants U, C_DOT, Q_PROP, ACT_ULP).  Streaming adds no arithmetic of its own, so no
tolerance constant is introduced here.  Two things the offline model had no need for are derived from its own terms:
  * block_ref carries an error field Ein of the block's INPUT (a chain hands block i + 1 the fp32 output of block i): it goes through
    the in-conv in quadrature with Q_PROP, as every carried error goes through a matrix there, and through the residual add as it is;
  * the carried cLN sums S = sum v, Q = sum v^2 (float64 on the device, of fp32 values with error field dv) are bounded by what
    ref_cln charges the mean and the variance for them: dS = Q_PROP sqrt(sum dv^2) + C_DOT 2^-53 sqrt(cnt) sum |v|,
    dQ = 2 Q_PROP sqrt(sum (v dv)^2) + C_DOT 2^-53 sqrt(cnt) sum v^2.
block_ref is ref_tcm(cum=True) restated with a carried state (sums, FIR / conv history) so that a stream can start at frame
2^24 + 3; test_references_agree (CPU) pins it, and the plain chunked numpy restatement of the kernel's ring / carry arithmetic, to
ref_tcm.  test_bound_catches_streaming_faults (CPU) shows that each plausible streaming fault exceeds the bound on the inputs the GPU
cases use, and that a plain fp32 evaluation in two summation orders stays inside it.

Every case also checks ownership (outputs are pre-filled with NaN: only the new frames may be written), that NaN poison in the
history columns of a source is gone after its exchange (and stays where no exchange reaches), that no NaN reaches an output (nothing
reads stale memory as history), and the kernels that ran from the launch logs; test_every_form_reached asserts the table."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'sixty-years-of-frequency-domain-monaural-speech-enhancement_amd')
PROBE_LIB = os.environ.get('SE_ONLINEPROBE_LIB') or os.path.join(PKG, 'libse_onlineprobe.so')
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from test_gpu_gemmconv_geometry import FAM_DIRECT, FAM_DIRECT_LDS, FAM_THIN, FAM_THIN_PAIR, FAM_TILE, U24, conv_f64, deconv_f64  # noqa: E402
from test_gpu_norm_forms import (ACT_ULP, C_DOT, EPS, F64, Q_PROP, U, Buf, affine_bound, dconv, fir_apply, make, prelu,  # noqa: E402
                                 ref_cln, ref_tcm, tcm_params)

gpu = pytest.mark.gpu
NAN = float('nan')
ACT_NONE, ACT_PRELU = 0, 1
EPI_ACT, EPI_GLU, EPI_ADD, EPI_MUL = 0, 2, 3, 4
REACHED = {}        # form -> the case that reached it
WORST = {}          # family -> (worst error / bound, case)


def note(form, case, ratio=None, family=None):
    REACHED.setdefault(form, case)
    if ratio is not None and ratio > WORST.get(family or form, (0.0, ''))[0]:
        WORST[family or form] = (ratio, case)


# ------------------------------------------------------------------------------------------------ float64 reference with a carried state
def ring_of(need):
    """k_tcm_stream.hip ring_of: columns of a history ring (frame t at t mod R)"""
    r = 16
    while r < need + 1:
        r <<= 1
    return r


def cln_carry(v, dv, gain, bias, S0, Q0, n0):
    """ref_cln's cumulative LayerNorm on v [B][C][T] (already PReLU'd, error field dv) whose statistics continue sums S0, Q0 [B] over
    n0 earlier frames.  Returns z, dz and the running sums with their bounds (module docstring)."""
    B, C_, T = v.shape
    s = S0[:, None] + v.sum(1).cumsum(-1)
    q = Q0[:, None] + (v * v).sum(1).cumsum(-1)
    cnt = C_ * (float(n0) + torch.arange(1, T + 1, dtype=F64))
    mu = s / cnt
    msq = q / cnt
    var = torch.clamp((q - 2 * mu * s) / cnt + mu * mu, min=0.0)
    mu, var, msq = mu[:, None, :], var[:, None, :], msq[:, None, :]
    rs = 1.0 / torch.sqrt(var + EPS)
    e1 = torch.sqrt((dv * dv).sum(1).cumsum(-1))
    d_mu = U * mu.abs() + Q_PROP * e1[:, None, :] / cnt
    e_rs = U + C_DOT * 2.0 ** -53 * torch.sqrt(cnt) * msq / (var + EPS) + \
        Q_PROP * torch.sqrt((((v - mu) * dv) ** 2).sum(1).cumsum(-1))[:, None, :] / cnt / (var + EPS)
    sh = (1, C_, 1)
    z, dz = affine_bound(v, mu, rs, gain.view(sh), bias.view(sh), None, None, d_mu, e_rs)
    dz = dz + (rs * gain.view(sh)).abs() * dv
    f64t = C_DOT * 2.0 ** -53 * torch.sqrt(cnt)
    dS = Q_PROP * e1 + f64t * (S0.abs()[:, None] + v.abs().sum(1).cumsum(-1))
    dQ = 2 * Q_PROP * torch.sqrt(((v * dv) ** 2).sum(1).cumsum(-1)) + f64t * q
    return z, dz, (s, q, dS, dQ)


def block_ref(x, p, dil, K, gated, Ein=None, carry=None):
    """ref_tcm(cum=True) on x [B][256][T] with (a) an error field Ein of x and (b) a carried state: carry = {'n0': frames before x,
    hd: {'S', 'Q' [B], 'z' [B][64][K - 1] (FIR history), 'a' [B][64][(ks - 1) dil] (dilated conv history)}}.  Returns y, bound, mid
    (per head: running sums S, Q with bounds dS, dQ; the normalised values z that enter the FIR ring; the values a that enter the conv
    ring; their bounds)."""
    B, _, T = x.shape
    ks = p['w_l'].shape[2]
    KH, CH = max(K - 1, 0), (ks - 1) * dil
    n0 = carry['n0'] if carry else 0
    zero = lambda *s: torch.zeros(s, dtype=F64)
    w1 = p['w_in'][:, :, 0]
    h = torch.einsum('oc,bct->bot', w1, x)
    Eh = C_DOT * U * math.sqrt(256) * torch.einsum('oc,bct->bot', w1.abs(), x.abs())
    if Ein is not None:
        Eh = Eh + Q_PROP * torch.sqrt(torch.einsum('oc,bct->bot', w1 ** 2, Ein ** 2))
    mid = {}

    def head(v, Ev, hd, fir):
        c = carry[hd] if carry else {}
        sl = p['s' + hd].view(1, 64, 1)
        a = prelu(v, sl)
        da = U * a.abs() + torch.clamp(sl.abs(), min=1.0) * Ev
        z, dz, (s, q, dS, dQ) = cln_carry(a, da, p['g' + hd], p['b' + hd], c.get('S', zero(B)), c.get('Q', zero(B)), n0)
        mid[hd] = dict(S=s, Q=q, dS=dS, dQ=dQ, z=z, dz=dz)
        if fir is not None:
            zz, dzz = fir_apply(torch.cat([c.get('z', zero(B, 64, KH)), z], -1), torch.cat([zero(B, 64, KH), dz], -1), fir)
            z, dz = zz[..., KH:], dzz[..., KH:]
        mid[hd].update(a=z, da=dz)
        return z, dz

    def conv(a, Ea, hd, w):
        c = carry[hd] if carry else {}
        m, Em = dconv(torch.cat([c.get('a', zero(B, 64, CH)), a], -1), torch.cat([zero(B, 64, CH), Ea], -1), w, dil)
        return m[..., CH:], Em[..., CH:]

    a, Ea = head(h, Eh, 'L', p.get('firL'))
    m, Em = conv(a, Ea, 'L', p['w_l'])
    if gated:
        r, Er = head(h, Eh, 'R', p.get('firR'))
        gte, Eg = conv(r, Er, 'R', p['w_r'])
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
    bd = Ey + U * y.abs()
    if Ein is not None:
        bd = bd + Ein
    return y, bd, mid


def chain_ref(x, blocks, carries=None):
    """blocks = [(p, dil, K, gated)] feeding each other; returns y, bound, [mid per block]"""
    E, mids = None, []
    for i, (p, dil, K, gated) in enumerate(blocks):
        x, E, mid = block_ref(x, p, dil, K, gated, E, carries[i] if carries else None)
        mids.append(mid)
    return x, E, mids


# ------------------------------------------------------------------------------------------------ the kernel's arithmetic, restated
class StreamChain:
    """tcm_chain_kernel in plain numpy (float64, or fp32 products with dtype=np.float32): one frame at a time, per block the six
    carried sums, the FIR ring and the dilated-conv ring (frame t in column t mod R, zeros before the stream).  fault: one of FAULTS."""

    def __init__(self, blocks, B, dtype=np.float64, fault=None, order=0):
        self.blocks, self.B, self.dt, self.fault, self.order = blocks, B, dtype, fault, order
        self.q = [{k: v.numpy().astype(dtype) for k, v in p.items()} for p, _, _, _ in blocks]
        self.state = []
        for p, dil, K, gated in blocks:
            ks = p['w_l'].shape[2]
            KH, CH, nb = max(K - 1, 0), (ks - 1) * dil, 2 if gated else 1
            self.state.append(dict(sums=np.zeros((B, 6)), fir=np.zeros((nb, B, 64, ring_of(KH)), dtype), cv=np.zeros((nb, B, 64, ring_of(CH)), dtype)))
        self.chunks = 0
        self.prev = None

    def mm(self, w, v):      # w [o][c], v [B][c]
        if self.order == 0:
            return (v @ w.T).astype(self.dt)
        hlf = w.shape[1] // 2
        return (v[:, hlf:] @ w[:, hlf:].T + v[:, :hlf] @ w[:, :hlf].T).astype(self.dt)

    def push(self, xs, t0):
        """xs [B][256][n]: the new frames of one chunk, first frame t0 -> [B][256][n]"""
        n = xs.shape[-1]
        out = np.zeros((self.B, 256, n), self.dt)
        saved = [s['sums'].copy() for s in self.state]
        for c in range(n):
            t = t0 + c
            x = xs[:, :, c].astype(self.dt)
            if self.fault == 't_base_low':        # the window read one column too low: the frame before (zeros before the stream)
                x = self.prev if self.prev is not None else np.zeros_like(x)
                self.prev = xs[:, :, c].astype(self.dt)
            for bi, (p, dil, K, gated) in enumerate(self.blocks):
                q, st = self.q[bi], self.state[bi]
                ks = q['w_l'].shape[2]
                KH = max(K - 1, 0)
                RF, RC = st['fir'].shape[-1], st['cv'].shape[-1]
                h = self.mm(q['w_in'][:, :, 0], x)

                def cln(v, hd, which):
                    v = np.where(v >= 0, v, q['s' + hd][None, :] * v).astype(self.dt)
                    drop = self.fault == 'first_frame_dropped' and c == 0 and self.chunks > 0
                    if not drop:
                        st['sums'][:, 2 * which] += v.astype(np.float64).sum(1)
                        st['sums'][:, 2 * which + 1] += (v.astype(np.float64) ** 2).sum(1)
                    s, qq = st['sums'][:, 2 * which], st['sums'][:, 2 * which + 1]
                    cnt = 64.0 * (t + 1)
                    m = s / cnt
                    var = (qq - 2 * m * s) / cnt + m * m
                    rs = 1.0 / np.sqrt(var + 1e-5)
                    return ((v - m.astype(self.dt)[:, None]) * rs.astype(self.dt)[:, None] * q['g' + hd][None, :] + q['b' + hd][None, :]).astype(self.dt)

                def branch(br):
                    hd = 'LR'[br]
                    a = cln(h, hd, br)
                    nbr = np.roll if self.fault == 'neighbour_row' and self.B > 1 else (lambda r_, *_a, **_k: r_)
                    if K > 0:
                        wr = (t + 1 if self.fault == 'ring_off_by_one' else t) & (RF - 1)
                        if KH > 0:
                            st['fir'][br][:, :, wr] = a
                        ring = nbr(st['fir'][br], 1, axis=0)
                        acc = q['fir' + hd][K - 1] * a
                        for k in range(KH):
                            acc = acc + q['fir' + hd][k] * ring[:, :, (t - KH + k) & (RF - 1)]
                        a = acc.astype(self.dt)
                    st['cv'][br][:, :, t & (RC - 1)] = a
                    ring = nbr(st['cv'][br], 1, axis=0)
                    acc = self.mm(q['w_l' if br == 0 else 'w_r'][:, :, ks - 1], a)
                    for tap in range(ks - 1):
                        back = (ks - 1 - tap) * dil + (1 if self.fault == 'stale_tap' else 0)
                        acc = acc + self.mm(q['w_l' if br == 0 else 'w_r'][:, :, tap], ring[:, :, (t - back) & (RC - 1)])
                    return acc.astype(self.dt)

                if gated:
                    g = branch(1)
                    m = (branch(0) * (1.0 / (1.0 + np.exp(-g)))).astype(self.dt)
                else:
                    m = branch(0)
                o = cln(m, 'O', 2)
                x = (self.mm(q['w_out'][:, :, 0], o) + x).astype(self.dt)
            out[:, :, c] = x
        if self.fault == 'carry_head' and self.chunks == 1:      # one head's sums not stored at the end of the second chunk
            for st, old in zip(self.state, saved):
                st['sums'][:, 4:6] = old[:, 4:6]
        self.chunks += 1
        return out

    def run(self, x, sched, t0=0):
        x = x.numpy() if torch.is_tensor(x) else x
        outs, c, i = [], 0, 0
        while c < x.shape[-1]:
            n = min(sched[i % len(sched)], x.shape[-1] - c)
            outs.append(self.push(x[:, :, c:c + n], t0 + c))
            c, i = c + n, i + 1
        return np.concatenate(outs, -1)


FAULTS = ('ring_off_by_one', 'stale_tap', 'carry_head', 'neighbour_row', 'first_frame_dropped', 't_base_low')

# ------------------------------------------------------------------------------------------------ the chain cases
MIXED = (1, 2, 3, 8, 1, 5)
# name -> (ks, [(dil, K, gated)], B, frames, chunk schedule, H); ring sizes and frame counts are in the names
CHAIN_CASES = {
    'ks3_gated_K7_dil1_ring16_T48_ones': (3, [(1, 7, True)], 2, 48, (1,), 0),
    'ks3_single_K0_dil1_ring16_T48_mixed': (3, [(1, 0, False)], 3, 48, MIXED, 5),
    'ks3_gated_K1_dil2_ring16_T41_n40': (3, [(2, 1, True)], 1, 41, (40, 1), 1),
    'ks5_gated_K2_dil4_ring32_T40_mixed': (5, [(4, 2, True)], 2, 40, MIXED, 16),
    'ks5_single_K63_dil1_firring64_T140_mixed': (5, [(1, 63, False)], 1, 140, MIXED, 3),
    'ks3_gated_K64_dil8_firring64_T140_n40': (3, [(8, 64, True)], 2, 140, (40, 3, 1), 2),
    'ks5_gated_K0_dil32_ring256_T300_mixed': (5, [(32, 0, True)], 1, 300, (8, 1, 40, 5), 4),
    'ks3_chain2_mixedK_ring16_T44_mixed': (3, [(1, 7, True), (2, 2, True)], 2, 44, MIXED, 0),
    'ks3_chain6_dil1to32_ring16to128_T150_mixed': (3, [(1 << i, 0, False) for i in range(6)], 1, 150, (8, 40, 1, 5), 2),
    'ks5_chain8_dil1to128_ring16to1024_T40_ones': (5, [(1 << i, 2 if i % 2 else 0, i < 2) for i in range(8)], 1, 40, (1, 2), 7),
}
FAULT_CASES = ('ks3_chain2_mixedK_ring16_T44_mixed', 'ks5_gated_K2_dil4_ring32_T40_mixed')
_cache = {}


def chain_inputs(name):
    """(blocks, x, y, bound, mids) of a case, computed once"""
    if name not in _cache:
        ks, spec, B, T, _, _ = CHAIN_CASES[name]
        seed = 1000 + 17 * sorted(CHAIN_CASES).index(name)
        blocks = [(tcm_params(seed + i, ks, gated, True, K), dil, K, gated) for i, (dil, K, gated) in enumerate(spec)]
        x = make((B, 256, T), 'normal', seed + 99)
        _cache[name] = (blocks, x) + chain_ref(x, blocks)
    return _cache[name]


def ratio(got, ref, bound):
    r = (torch.as_tensor(np.asarray(got, dtype=np.float64)) - ref).abs() / bound
    assert torch.isfinite(r).all(), 'non-finite output or zero bound'
    return float(r.max())


# ------------------------------------------------------------------------------------------------ CPU tests
def test_references_agree():
    """block_ref without carry or input error is ref_tcm(cum=True), value and bound; split in two with the carried state handed over
    it gives the same values; the chunked restatement of the kernel equals both in float64"""
    for name in FAULT_CASES + ('ks3_single_K0_dil1_ring16_T48_mixed',):
        blocks, x, y, bd, mids = chain_inputs(name)
        v = x
        for p, dil, K, gated in blocks:
            want, wb = ref_tcm(v, p, dil, K, gated, True)
            got, gb, _ = block_ref(v, p, dil, K, gated)
            assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
            assert float((gb - wb).abs().max()) <= 1e-9 * float(wb.abs().max())
            v = want
        assert float((v - y).abs().max()) <= 1e-12 * float(y.abs().max())
        sched = CHAIN_CASES[name][4]
        z = StreamChain(blocks, x.shape[0]).run(x, sched)
        assert float(np.abs(z - y.numpy()).max()) <= 1e-11 * float(y.abs().max()), name
        # the carried form: the second half from the state the first half leaves
        p, dil, K, gated = blocks[0]
        ks = p['w_l'].shape[2]
        KH, CH, T = max(K - 1, 0), (ks - 1) * dil, x.shape[-1]
        c = T // 2
        assert c >= KH and c >= CH
        full, _, mid = block_ref(x, p, dil, K, gated)
        carry = {'n0': c}
        for hd in mid:
            carry[hd] = dict(S=mid[hd]['S'][:, c - 1], Q=mid[hd]['Q'][:, c - 1], z=mid[hd]['z'][..., c - KH:c], a=mid[hd]['a'][..., c - CH:c])
        tail, _, _ = block_ref(x[..., c:], p, dil, K, gated, None, carry)
        assert float((tail - full[..., c:]).abs().max()) <= 1e-11 * float(full.abs().max())
    # the cLN inside block_ref is ref_cln
    v = make((2, 64, 1, 30), 'offset', 5)
    g, b, sl = make((64,), 'normal', 6), make((64,), 'normal', 7), make((64,), 'normal', 8).abs() * 0.3
    want, wb = ref_cln(v, g, b, pre=sl, Ein=torch.zeros_like(v))
    a = prelu(v[:, :, 0, :], sl.view(1, 64, 1))
    got, gb, _ = cln_carry(a, U * a.abs(), g, b, torch.zeros(2, dtype=F64), torch.zeros(2, dtype=F64), 0)
    assert float((got - want[:, :, 0]).abs().max()) <= 1e-12 * float(want.abs().max())
    assert float((gb - wb[:, :, 0]).abs().max()) <= 1e-9 * float(wb.abs().max())


def test_bound_catches_streaming_faults():
    """(i) the kernel's arithmetic in plain fp32 (two summation orders) stays inside the bound; (ii) each streaming fault exceeds it,
    on the inputs of the GPU cases"""
    inside, caught = {}, {}
    for name in FAULT_CASES:
        blocks, x, y, bd, _ = chain_inputs(name)
        sched = CHAIN_CASES[name][4]
        for order in (0, 1):
            inside[name, order] = ratio(StreamChain(blocks, x.shape[0], np.float32, order=order).run(x, sched), y, bd)
        for f in FAULTS:
            caught[name, f] = ratio(StreamChain(blocks, x.shape[0], fault=f).run(x, sched), y, bd)
    print('fp32 restatement: worst error / bound %s' % {k: round(v, 3) for k, v in inside.items()})
    print('faults: error / bound %s' % {k: round(v, 1) for k, v in caught.items()})
    assert max(inside.values()) <= 1.0, inside
    assert min(caught.values()) > 1.0, caught


# ------------------------------------------------------------------------------------------------ the probe
_lib = None
I, P, LL = C.c_int, C.c_void_p, C.c_longlong
SIGS = {
    'op_stream_begin': [P], 'op_slot_read': [P, I, P, LL], 'op_slot_write': [P, I, P, LL], 'op_scope_open': [P, I, I, LL],
    'op_tcm_chain_run': [P, I, P, P, P, I, I, P], 'op_tcm_chain_launch': [P, I, P, P],
    'op_exchange': [P, LL, LL, LL, I, I, I, I], 'op_exchange_pair': [P, LL, LL, LL, I, I, P, LL, LL, LL, I, I, I, I],
    'op_hist_restore': [P, P, I, LL, I, I], 'op_hist_save': [P, P, I, LL, I, I], 'op_hist_batch': [P, P, P, I, I, I, I, I],
    'op_layer_run': [P, P, P, I, P, I, I, P, I, I, I, I, I, I],
}
NREC = ('W', 'VPT', 'KS', 'GATED', 'CUM', 'strip', 'ragged', 'c0', 'WP', 'grid', 'block', 'shmem', 'res')
GREC = ('family', 'BM', 'BN', 'flat_upr', 'upt', 'flat_rows', 'qt2', 'nrm', 'res', 'trim', 'stats', 'ragged', 'flat_nrm_refused', 'nblk', 'epi')


def lib():
    global _lib
    if _lib is None:
        assert os.path.exists(PROBE_LIB), 'libse_onlineprobe.so is missing: run build() (make -C csrc)'
        L = C.CDLL(PROBE_LIB)
        for name, sig in SIGS.items():
            getattr(L, name).argtypes = sig
            getattr(L, name).restype = I
        L.op_last_error.restype = C.c_char_p
        L.op_launch_kernel.restype = C.c_char_p
        L.op_launch_kernel.argtypes = [I]
        L.op_launch_get.argtypes = [I, C.POINTER(LL), I]
        L.op_gc_launch_get.argtypes = [I, C.POINTER(LL), I]
        L.op_stream_create.restype = P
        L.op_stream_create.argtypes = [I]
        L.op_stream_destroy.argtypes = [P]
        L.op_slot_count.argtypes = [P]
        L.op_slot_bytes.argtypes = [P, I]
        L.op_slot_bytes.restype = LL
        L.op_sd_create.restype = P
        L.op_sd_destroy.argtypes = [P]
        L.op_sd_put.argtypes = [P, C.c_char_p, P, C.POINTER(LL), I]
        L.op_tcm_create.restype = P
        L.op_tcm_create.argtypes = [P, C.c_char_p, I, C.c_char_p, C.c_char_p, I, I, I, I]
        L.op_tcm_destroy.argtypes = [P]
        for f in ('op_conv_create', 'op_deconv_create'):
            getattr(L, f).restype = P
        L.op_conv_create.argtypes = [P, P, P] + [I] * 12
        L.op_deconv_create.argtypes = [P, P, P] + [I] * 10
        L.op_plan_destroy.argtypes = [P]
        L.op_plan_info.argtypes = [P, C.POINTER(I), I]
        L.op_register_overread.argtypes = [P, C.c_size_t]
        L.op_unregister_overread.argtypes = [P]
        _lib = L
    return _lib


def ptr(a):
    return a.ptr if isinstance(a, Buf) else (a.data_ptr() if torch.is_tensor(a) else a)


def logs():
    L = lib()
    nrm, gc = [], []
    for i in range(L.op_launch_count()):
        v = (LL * len(NREC))()
        L.op_launch_get(i, v, len(NREC))
        nrm.append(dict(zip(NREC, list(v)), kernel=L.op_launch_kernel(i).decode()))
    for i in range(L.op_gc_launch_count()):
        v = (LL * len(GREC))()
        L.op_gc_launch_get(i, v, len(GREC))
        gc.append(dict(zip(GREC, list(v))))
    return nrm, gc


def call(name, *args):
    """one probe call on cleared logs -> (norm records, conv records)"""
    L = lib()
    torch.cuda.synchronize()
    L.op_log_clear()
    rc = getattr(L, name)(*[ptr(a) for a in args])
    assert rc == 0, '%s: %s' % (name, L.op_last_error().decode())
    return logs()


def refused(msg, name, *args):
    """a host-side refusal: error with this text, nothing launched"""
    L = lib()
    torch.cuda.synchronize()
    L.op_log_clear()
    rc = getattr(L, name)(*[ptr(a) for a in args])
    nrm, gc = logs()
    err = L.op_last_error().decode()
    assert rc != 0 and msg in err and not nrm and not gc, (rc, err, nrm, gc)


class Stream:
    def __init__(self, B):
        self.L, self.B = lib(), B
        self.h = self.L.op_stream_create(B)
        assert self.h, self.L.op_last_error().decode()

    def open(self, H, n, t0):
        assert self.L.op_scope_open(self.h, H, n, t0) == 0, self.L.op_last_error().decode()

    def close(self):
        self.L.op_scope_close()

    def slots(self):
        return [self.L.op_slot_bytes(self.h, i) for i in range(self.L.op_slot_count(self.h))]

    def read(self, i):
        a = np.zeros(self.slots()[i], np.uint8)
        assert self.L.op_slot_read(self.h, i, a.ctypes.data, a.nbytes) == 0, self.L.op_last_error().decode()
        return a

    def write(self, i, a):
        a = np.ascontiguousarray(a).view(np.uint8)
        assert self.L.op_slot_write(self.h, i, a.ctypes.data, a.nbytes) == 0, self.L.op_last_error().decode()

    def begin(self):
        assert self.L.op_stream_begin(self.h) == 0

    def destroy(self):
        self.L.op_scope_close()
        self.L.op_stream_destroy(self.h)


def tcm_block(p, dil, K, ks, gated):
    """the block's state dict in torch layout, cLN `gain` keys -> TcmBlock::load"""
    L = lib()
    sd = L.op_sd_create()
    keep = []

    def put(key, t, shape):
        a = np.ascontiguousarray(t.numpy().astype(np.float32))
        keep.append(a)
        L.op_sd_put(sd, ('blk.' + key).encode(), a.ctypes.data, (LL * len(shape))(*shape), len(shape))

    put('in_conv.weight', p['w_in'], (64, 256, 1))
    put('out_conv.2.weight', p['w_out'], (256, 64, 1))
    for hd, name in (('L', 'left_conv'), ('R', 'right_conv')) if gated else (('L', 'left_conv'),):
        put(name + '.0.weight', p['s' + hd], (64,))
        put(name + '.1.gain', p['g' + hd], (64,))
        put(name + '.1.bias', p['b' + hd], (64,))
        if K > 0:
            put(name + '.2.weight', p['fir' + hd], (1, 1, K))
        put(name + ('.4' if K > 0 else '.3') + '.weight', p['w_l' if hd == 'L' else 'w_r'], (64, 64, ks))
    put('out_conv.0.weight', p['sO'], (64,))
    put('out_conv.1.gain', p['gO'], (64,))
    put('out_conv.1.bias', p['bO'], (64,))
    h = L.op_tcm_create(sd, b'blk.', dil, b'left_conv', b'right_conv' if gated else b'left_conv', 4 if K > 0 else 3, K, ks, int(gated))
    L.op_sd_destroy(sd)
    assert h, L.op_last_error().decode()
    return h


def parse_slot(raw, B, K, ks, dil, gated):
    """one block's state slot (k_tcm_stream.hip launch_tcm_chain): per row 6 float64 sums in 64 bytes, the FIR rings [nb][64][RF],
    the dilated-conv rings [nb][64][RC]"""
    KH, CH, nb = max(K - 1, 0), (ks - 1) * dil, 2 if gated else 1
    RF, RC = ring_of(KH), ring_of(CH)
    stride = 64 + nb * 64 * ((RF if KH else 0) + RC) * 4
    assert raw.nbytes == B * stride, (raw.nbytes, B, stride)
    rows = raw.reshape(B, stride)
    sums = np.ascontiguousarray(rows[:, :48]).view(np.float64).reshape(B, 6)
    body = np.ascontiguousarray(rows[:, 64:]).view(np.float32).reshape(B, -1)
    nf = nb * 64 * RF if KH else 0
    fir = body[:, :nf].reshape(B, nb, 64, RF) if KH else None
    cv = body[:, nf:].reshape(B, nb, 64, RC)
    return sums, fir, cv


def build_slot(B, K, ks, dil, gated, sums, fir, cv):
    KH, CH, nb = max(K - 1, 0), (ks - 1) * dil, 2 if gated else 1
    RF, RC = ring_of(KH), ring_of(CH)
    stride = 64 + nb * 64 * ((RF if KH else 0) + RC) * 4
    raw = np.zeros((B, stride), np.uint8)
    raw[:, :48] = np.ascontiguousarray(sums, dtype=np.float64).view(np.uint8).reshape(B, 48)
    parts = ([np.asarray(fir, np.float32).reshape(B, -1)] if KH else []) + [np.asarray(cv, np.float32).reshape(B, -1)]
    raw[:, 64:] = np.ascontiguousarray(np.concatenate(parts, 1)).view(np.uint8).reshape(B, -1)
    return raw


def push_chain(st, handles, x, sched, H, t_start, case):
    """x [B][256][T] through op_tcm_chain_run in chunks -> the new frames of every chunk [B][256][T] (fp32), the chain kernels seen"""
    B, _, T = x.shape
    L = lib()
    arr = (P * len(handles))(*handles)
    got = torch.full(x.shape, NAN, dtype=torch.float32, device='cuda')
    c, i, seen = 0, 0, []
    which = I(-1)
    while c < T:
        n = min(sched[i % len(sched)], T - c)
        i += 1
        win = torch.full((B, 256, H + n), NAN, dtype=torch.float32)      # history columns: poison - the chain keeps its own
        win[..., H:] = x[..., c:c + n].to(torch.float32)
        xb, y0, y1 = Buf(win.numel(), 0, win.cuda()), Buf(win.numel(), 0), Buf(win.numel(), 0)
        st.open(H, n, t_start + c)
        nrm, gc = call('op_tcm_chain_run', arr, len(handles), xb, y0, y1, B, H + n, C.addressof(which))
        st.close()
        assert [r['kernel'] for r in nrm] == ['tcm_chain'] and not gc and nrm[0]['grid'] == B, (nrm, gc)
        seen.append(nrm[0]['KS'])
        out, other = (y0, y1) if which.value == 0 else (y1, y0)
        assert which.value == (len(handles) - 1) & 1
        yw = out.v.reshape(B, 256, H + n)
        assert out.untouched() and other.untouched() and torch.isnan(other.v).all() and torch.isnan(yw[..., :H]).all(), \
            '%s: the chunk wrote outside its new frames' % case
        assert xb.untouched() and torch.isnan(xb.v.reshape(win.shape)[..., :H]).all()
        got[..., c:c + n] = yw[..., H:]
        c += n
    return got.cpu(), seen


def check(case, family, got, ref, bound):
    got = torch.as_tensor(np.asarray(got.cpu() if torch.is_tensor(got) else got, dtype=np.float64)).reshape(ref.shape)
    assert torch.isfinite(got).all(), '%s: non-finite output (poison read as history?)' % case
    r = (got - ref).abs() / bound
    k = int(r.argmax())
    rt = float(r.reshape(-1)[k])
    print('%s [%s]: worst error / bound %.3f at %s (got %.9g, want %.9g, bound %.3g)' %
          (case, family, rt, tuple(int(i) for i in np.unravel_index(k, ref.shape)), float(got.reshape(-1)[k]), float(ref.reshape(-1)[k]),
           float(bound.reshape(-1)[k])))
    if rt > WORST.get(family, (0.0, ''))[0]:
        WORST[family] = (rt, case)
    assert rt <= 1.0, '%s: error %.3f of the bound' % (case, rt)


# ------------------------------------------------------------------------------------------------ GPU: the chain
@gpu
@pytest.mark.parametrize('name', sorted(CHAIN_CASES))
def test_tcm_chain(name):
    """a stream pushed through run_tcm_chain in chunks: every new frame against the float64 chain on the whole sequence; after the
    last chunk the state slots - the six carried sums of each block against the float64 running sums, the ring columns of the most
    recent K - 1 / (ks - 1) dil frames against the reference's normalised branch values; then a second stream on the same slots
    (StreamSlots::begin) must reproduce the first from zero state"""
    ks, spec, B, T, sched, H = CHAIN_CASES[name]
    blocks, x, y, bd, mids = chain_inputs(name)
    handles = [tcm_block(p, dil, K, ks, gated) for p, dil, K, gated in blocks]
    st = Stream(B)
    try:
        got, seen = push_chain(st, handles, x, sched, H, 0, name)
        assert set(seen) == {ks}
        note('tcm_chain<%d>' % ks, name)
        check(name, 'tcm_chain<%d> output' % ks, got, y, bd)
        assert len(st.slots()) == len(blocks)
        for i, ((p, dil, K, gated), mid) in enumerate(zip(blocks, mids)):
            sums, fir, cv = parse_slot(st.read(i), B, K, ks, dil, gated)
            KH, CH = max(K - 1, 0), (ks - 1) * dil
            for w, hd in enumerate('LRO'):
                if hd == 'R' and not gated:
                    continue
                for j, key in enumerate('SQ'):
                    check('%s block %d sum %s%s' % (name, i, key, hd), 'tcm_chain carried sums', sums[:, 2 * w + j], mid[hd][key][:, -1],
                          mid[hd]['d' + key][:, -1])
            for br, hd in enumerate('LR' if gated else 'L'):
                for ring, key, dk, depth in ((fir, 'z', 'dz', KH), (cv, 'a', 'da', CH)):
                    ts = list(range(max(T - depth, 0), T))
                    if ts:
                        R = ring.shape[-1]
                        check('%s block %d ring %s%s' % (name, i, key, hd), 'tcm_chain ring columns', ring[:, br][:, :, [t & (R - 1) for t in ts]],
                              mid[hd][key][..., ts], mid[hd][dk][..., ts])
        st.begin()      # a second stream: zero state again, same slots
        n2 = min(T, 12)
        again, _ = push_chain(st, handles, x[..., :n2], sched, H, 0, name + ' second stream')
        assert len(st.slots()) == len(blocks)
        check(name + ' second stream', 'tcm_chain<%d> output' % ks, again, y[..., :n2], bd[..., :n2])
    finally:
        st.destroy()
        for h in handles:
            lib().op_tcm_destroy(h)


@gpu
@pytest.mark.parametrize('ks,dil,K', [(3, 2, 7), (5, 4, 2)])
def test_tcm_chain_mid_stream_start(ks, dil, K):
    """a stream that is 2^24 + 3 frames old (a float32 frame count would lose its + 1): every earlier frame was zero input, so the
    state has a closed form - both branch heads have zero sums and normalise 0 to their bias, which the FIR and the dilated conv turn
    into one steady column after K - 1 + (ks - 1) dil frames; the out head's sums are the transient frames' plus (t0 - transient)
    steady ones.  That state is written into the slot, 8 real frames are pushed, and compared with the float64 continuation.  One
    block per chain: the second block of a chain sees a cLN output that keeps converging, which has no closed form."""
    B, t0, n = 2, 2 ** 24 + 3, 8
    p = tcm_params(4000 + ks, ks, True, True, K)
    blocks = [(p, dil, K, True)]
    KH, CH = K - 1, (ks - 1) * dil
    ntr = KH + CH + 1
    sc = StreamChain(blocks, B)
    before = []
    for t in range(ntr + 1):
        sc.push(np.zeros((B, 256, 1)), t)
        before.append(sc.state[0]['sums'].copy())
    inc = before[-1] - before[-2]
    assert np.allclose(inc, before[-2] - before[-3], rtol=0, atol=1e-12 * np.abs(inc).max()), 'not steady yet'
    sums = before[-1] + (t0 - (ntr + 1)) * inc
    zst = np.stack([p['b' + hd].numpy() for hd in 'LR'])                                  # [2][64]: cLN of zeros is the bias
    ast = np.stack([zst[i] * p['fir' + hd].numpy().sum() for i, hd in enumerate('LR')])
    RF, RC = ring_of(KH), ring_of(CH)
    fir = np.broadcast_to(zst[None, :, :, None], (B, 2, 64, RF))
    cv = np.broadcast_to(ast[None, :, :, None], (B, 2, 64, RC))
    carry = {'n0': t0}
    for i, hd in enumerate('LR'):
        carry[hd] = dict(S=torch.zeros(B, dtype=F64), Q=torch.zeros(B, dtype=F64), z=torch.from_numpy(np.ascontiguousarray(fir[:, i, :, :KH])),
                         a=torch.from_numpy(np.ascontiguousarray(cv[:, i, :, :CH])))
    carry['O'] = dict(S=torch.from_numpy(sums[:, 4].copy()), Q=torch.from_numpy(sums[:, 5].copy()))
    x = make((B, 256, n), 'normal', 4100 + ks)
    y, bd, _ = block_ref(x, p, dil, K, True, None, carry)
    h = tcm_block(p, dil, K, ks, True)
    st = Stream(B)
    name = 'mid-stream ks%d t0=2^24+3' % ks
    try:
        # the first launch sizes the slot; it runs on zero input at t0 - 1 and its state is then replaced
        push_chain(st, [h], torch.zeros((B, 256, 1), dtype=F64), (1,), 2, t0 - 1, name)
        st.write(0, build_slot(B, K, ks, dil, True, sums, fir, cv))
        got, _ = push_chain(st, [h], x, (3, 1, 4), 2, t0, name)
        check(name, 'tcm_chain<%d> output' % ks, got, y, bd)
        note('tcm_chain<%d> mid-stream' % ks, name)
    finally:
        st.destroy()
        lib().op_tcm_destroy(h)


# ------------------------------------------------------------------------------------------------ GPU: causal convs in a window
# w [M][Cin][nkf][nkt] (frequency taps first); conv: out[f][t] = sum w x[f sf - pf + kf][t - pt + kt dil_t]
LAYERS = {
    't2f3_m9_c16': dict(kind='conv', M=9, Cin=16, nkf=3, nkt=2, sf=1, pf=1, pt=1, dt=1, c0=-1, Fin=6, Fout=6, epi=EPI_ACT),          # lookback 1, 4 chunks: resident
    't1f3_m8_c5': dict(kind='conv', M=8, Cin=5, nkf=3, nkt=1, sf=1, pf=1, pt=0, dt=1, c0=-1, Fin=7, Fout=7, epi=EPI_ADD),            # no look-back
    't2f5_m64_c8': dict(kind='conv', M=64, Cin=8, nkf=5, nkt=2, sf=2, pf=2, pt=1, dt=1, c0=-1, Fin=10, Fout=5, epi=EPI_ACT),         # strided in frequency
    'pw_m3_c9': dict(kind='conv', M=3, Cin=9, nkf=1, nkt=1, sf=1, pf=0, pt=0, dt=1, c0=-1, Fin=5, Fout=5, epi=EPI_ACT),              # pointwise, direct
    't3_m4_c7': dict(kind='conv', M=4, Cin=7, nkf=1, nkt=3, sf=1, pf=0, pt=2, dt=1, c0=-1, Fin=3, Fout=3, epi=EPI_MUL),              # lookback 2, direct
    't3d2_m9_c24': dict(kind='conv', M=9, Cin=24, nkf=1, nkt=3, sf=1, pf=0, pt=4, dt=2, c0=-1, Fin=4, Fout=4, epi=EPI_MUL),          # lookback 4 = H
    'cat_m16_c4_12': dict(kind='conv', M=16, Cin=16, nkf=3, nkt=2, sf=1, pf=1, pt=1, dt=1, c0=4, Fin=5, Fout=5, epi=EPI_GLU),        # two sources, gated
    'dec_m9_c16': dict(kind='deconv', M=9, Cin=16, nkf=3, nkt=2, sf=2, pf=0, toff=0, c0=-1, Fin=5, Fout=11, epi=EPI_ACT),            # two parity classes
    'dec_m3_c6_cat': dict(kind='deconv', M=3, Cin=6, nkf=3, nkt=2, sf=2, pf=0, toff=0, c0=3, Fin=4, Fout=9, epi=EPI_ACT),
}
CHUNKS = (1, 2, 3, 4, 5, 8, 9, 64, 65)
_layers = {}


def layer_data(name):
    if name not in _layers:
        sh = LAYERS[name]
        g = np.random.default_rng(7000 + sorted(LAYERS).index(name))
        K = sh['Cin'] * sh['nkf'] * sh['nkt']
        w = torch.from_numpy((g.uniform(-1, 1, (sh['M'], sh['Cin'], sh['nkf'], sh['nkt'])) / math.sqrt(K)).astype(np.float32)).to(F64)
        bias = torch.from_numpy(g.uniform(-0.3, 0.3, sh['M']).astype(np.float32)).to(F64)
        slope = torch.from_numpy(g.uniform(0.05, 0.45, sh['M']).astype(np.float32)).to(F64)
        _layers[name] = (w, bias, slope)
    return _layers[name]


def make_plan(name):
    sh = LAYERS[name]
    w, bias, slope = layer_data(name)
    L = lib()
    f = lambda a: np.ascontiguousarray(a.numpy(), dtype=np.float32)
    wa, ba = f(w), f(bias)
    prelu_on = sh['epi'] != EPI_GLU
    sa = f(slope) if prelu_on else None
    act = ACT_PRELU if prelu_on else ACT_NONE
    sp = sa.ctypes.data if prelu_on else None
    if sh['kind'] == 'conv':
        h = L.op_conv_create(wa.ctypes.data, ba.ctypes.data, sp, sh['M'], sh['Cin'], sh['nkf'], sh['nkt'], sh['sf'], sh['pf'], sh['pt'], 1, sh['dt'], act,
                             sh['epi'], sh['c0'])
    else:
        h = L.op_deconv_create(wa.ctypes.data, ba.ctypes.data, sp, sh['M'], sh['Cin'], sh['nkf'], sh['nkt'], sh['sf'], sh['pf'], sh['toff'], act, sh['epi'],
                               sh['c0'])
    assert h, L.op_last_error().decode()
    out = (I * 6)()
    L.op_plan_info(h, out, 6)
    return h, dict(zip(('nplans', 'lookback', 'cic', 'direct', 'BM', 'pair'), out))


def layer_ref(name, x, aux):
    """float64 output of the layer on the whole sequence x [B][Cin][Fin][T] and the bound of its fp32 form (the geometry suite's
    4 u K (sum |w| |x| + |bias|) for the accumulation; the epilogues as test_gpu_norm_forms chains them)"""
    sh = LAYERS[name]
    w, bias, slope = layer_data(name)
    if sh['kind'] == 'conv':
        f = lambda a, ww: conv_f64(a, ww, sh['sf'], sh['pf'], sh['pt'], 1, sh['dt'], Fout=sh['Fout'])
    else:
        f = lambda a, ww: deconv_f64(a, ww, sh['sf'], sh['pf'], sh['toff'], sh['Fout'])
    y = f(x, w) + bias[None, :, None, None]
    K = w.shape[1] * w.shape[2] * w.shape[3]
    bd = 4.0 * U24 * K * (f(x.abs(), w.abs()) + bias.abs()[None, :, None, None])
    if sh['epi'] == EPI_GLU:
        a, g, ba, bg = y[:, 0::2], y[:, 1::2], bd[:, 0::2], bd[:, 1::2]
        sg = torch.sigmoid(g)
        y = a * sg
        return y, sg * ba + a.abs() * (sg * (1 - sg) * bg + ACT_ULP) + U * y.abs()
    s = slope[None, :, None, None]
    y = torch.where(y >= 0, y, s * y)
    if sh['epi'] == EPI_ADD:
        y = y + aux
        bd = bd + U * y.abs()
    elif sh['epi'] == EPI_MUL:
        y = y * aux
        bd = bd * aux.abs() + U * y.abs()
    return y, bd


def family_of(r, direct):
    if r['family'] == FAM_TILE:
        return 'tile resident' if r['res'] else 'tile plain'
    return {FAM_THIN: 'thin', FAM_THIN_PAIR: 'thin pair', FAM_DIRECT: 'direct', FAM_DIRECT_LDS: 'direct'}[r['family']]


def split_src(sh, t):
    c0 = sh['Cin'] if sh['c0'] < 0 else sh['c0']
    return [t[:, :c0]] + ([t[:, c0:]] if c0 < sh['Cin'] else [])


def run_layer_chunk(L, h, sh, info, srcs, aux, B, H, n, case, tb=None):
    """one layer call on a window: srcs / aux are [B][C][F][H + n] float32 CPU tensors (history columns as the caller wants them).
    Returns the output window, the source windows after the call, and the launch records."""
    T = H + n
    dstC = sh['M'] // 2 if sh['epi'] == EPI_GLU else sh['M']
    sb = [Buf(s.numel(), 0, s.cuda()) for s in srcs]
    for b_ in sb:
        L.op_register_overread(b_.t.data_ptr(), b_.t.numel() * 4)
    ab = Buf(aux.numel(), 0, aux.cuda()) if aux is not None else None
    ob = Buf(B * dstC * sh['Fout'] * T, 0)
    t_base, t_out, soft = tb if tb else (0, -1, 0)
    try:
        nrm, gc = call('op_layer_run', h, sb[0], sb[1] if len(sb) > 1 else None, sh['Fin'], ob, dstC, sh['Fout'], ab, B, T, T, t_base, t_out, soft)
    finally:
        for b_ in sb:
            L.op_unregister_overread(b_.t.data_ptr())
    assert ob.untouched() and all(b_.untouched() for b_ in sb), '%s: wrote outside its tensors' % case
    return ob.v.reshape(B, dstC, sh['Fout'], T).cpu(), [b_.v.reshape(s.shape).cpu() for b_, s in zip(sb, srcs)], nrm, gc


@gpu
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('Hk', [4, 8, 'odd'])
@pytest.mark.parametrize('name', sorted(LAYERS))
def test_conv_in_a_stream_window(name, Hk, B):
    """frames pushed as chunks of 1, 2, 3, 4, 5, 8, 9, 64 and 65 new frames under a StreamScope with H = 4 or 8 history columns (the
    look-backs are 0, 1, 2 and 4 = H itself), through run_conv / run_deconv: gc_launch_prof exchanges the history and sets
    t_base = H.  gc_select wants a first frame that is a multiple of 4 except on the thin path, which takes any: 'odd' is the
    smallest odd H that holds the look-back, with the chunks of up to 8 frames.  New frames against float64 on the whole sequence; the
    rest of the output window keeps its NaN; the source's history columns the taps reach lose their NaN in the exchange, the others
    keep it."""
    sh = LAYERS[name]
    L = lib()
    h, info = make_plan(name)
    need = info['lookback']
    H = (need | 1) if Hk == 'odd' else Hk
    chunks = tuple(n for n in CHUNKS if n <= 8) if Hk == 'odd' else CHUNKS
    T = sum(chunks)
    x = make((B, sh['Cin'], sh['Fin'], T), 'normal', 7100 + B)
    dstC = sh['M'] // 2 if sh['epi'] == EPI_GLU else sh['M']
    aux = make((B, dstC, sh['Fout'], T), 'normal', 7200 + B) if sh['epi'] in (EPI_ADD, EPI_MUL) else None
    y, bd = layer_ref(name, x, aux)
    st = Stream(B)
    got = torch.full(y.shape, NAN, dtype=torch.float32)
    fams = set()
    try:
        c = 0
        for n in chunks:
            case = '%s B%d H%d n%d' % (name, B, H, n)
            win = torch.full((B, sh['Cin'], sh['Fin'], H + n), NAN, dtype=torch.float32)
            win[..., H:] = x[..., c:c + n].to(torch.float32)
            aw = None
            if aux is not None:
                aw = torch.full((B, dstC, sh['Fout'], H + n), NAN, dtype=torch.float32)
                aw[..., H:] = aux[..., c:c + n].to(torch.float32)
            st.open(H, n, c)
            out, after, nrm, gc = run_layer_chunk(L, h, sh, info, split_src(sh, win), aw, B, H, n, case)
            st.close()
            hist = [r['kernel'] for r in nrm]
            two = len(after) > 1
            assert hist == ([] if need == 0 else ['stream_hist_pair' if two else 'stream_hist']), (case, hist)      # (one exchange serves both parity classes)
            for k_ in hist:
                note(k_, case)
            assert len(st.slots()) == (0 if need == 0 else (2 if two else 1))
            assert torch.isnan(out[..., :H]).all() and not torch.isnan(out[..., H:]).any(), '%s: output outside the new frames / poison inside' % case
            for a_ in after:
                assert torch.isnan(a_[..., :H - need]).all() and not torch.isnan(a_[..., H - need:]).any(), '%s: history columns' % case
            if need:
                want = x[..., max(c - need, 0):c].to(torch.float32)
                want = torch.cat([torch.zeros(x.shape[:-1] + (need - want.shape[-1],)), want], -1)      # zeros before the stream
                assert torch.equal(torch.cat(after, 1)[..., H - need:H], want), '%s: restored history' % case
            got[..., c:c + n] = out[..., H:]
            for r in gc:
                fm = family_of(r, info['direct'])
                fams.add(fm)
                assert Hk != 'odd' or fm in ('thin', 'thin pair'), (case, fm)
                note(fm + ' at t_base > 0', case)
            c += n
    finally:
        st.destroy()
        L.op_plan_destroy(h)
    check('%s B%d H%d' % (name, B, H), 'conv in a window: ' + '/'.join(sorted(fams)), got, y, bd)


@gpu
@pytest.mark.parametrize('n', [4, 9])
def test_parity_classes_share_one_exchange(n):
    """the two parity classes of a transposed conv read the same source with the same look-back: one state slot, one exchange
    (StreamCtx::memo_src); a following layer on another source takes its own slot and exchange.  One chunk after a first one, so that
    the history is real."""
    L = lib()
    B, H = 2, 4
    hd, idec = make_plan('dec_m9_c16')
    hc, icnv = make_plan('t2f3_m9_c16')
    sd, sc = LAYERS['dec_m9_c16'], LAYERS['t2f3_m9_c16']
    xd = make((B, sd['Cin'], sd['Fin'], 2 * n), 'normal', 7301)
    xc = make((B, sc['Cin'], sc['Fin'], 2 * n), 'normal', 7302)
    yd, bdd = layer_ref('dec_m9_c16', xd, None)
    yc, bdc = layer_ref('t2f3_m9_c16', xc, None)
    st = Stream(B)
    try:
        for c in (0, n):
            wins = []
            for x, sh in ((xd, sd), (xc, sc)):
                w = torch.full((B, sh['Cin'], sh['Fin'], H + n), NAN, dtype=torch.float32)
                w[..., H:] = x[..., c:c + n].to(torch.float32)
                wins.append(w)
            st.open(H, n, c)
            od, _, nrm1, gc1 = run_layer_chunk(L, hd, sd, idec, [wins[0]], None, B, H, n, 'memo deconv')
            assert [r['kernel'] for r in nrm1] == ['stream_hist'] and len(st.slots()) == (1 if c == 0 else 2) and L.op_scope_cursor() == 1
            assert len(gc1) == (1 if n <= 8 else 2) and (gc1[0]['family'] == FAM_THIN_PAIR) == (n <= 8), gc1
            oc, _, nrm2, gc2 = run_layer_chunk(L, hc, sc, icnv, [wins[1]], None, B, H, n, 'memo conv')
            assert [r['kernel'] for r in nrm2] == ['stream_hist'] and len(st.slots()) == 2 and L.op_scope_cursor() == 2
            st.close()
            check('memo n%d deconv chunk at %d' % (n, c), 'conv in a window: memo', od[..., H:], yd[..., c:c + n], bdd[..., c:c + n])
            check('memo n%d conv chunk at %d' % (n, c), 'conv in a window: memo', oc[..., H:], yc[..., c:c + n], bdc[..., c:c + n])
        note('memo: one exchange for two parity classes', 'n%d' % n)
    finally:
        st.destroy()
        L.op_plan_destroy(hd)
        L.op_plan_destroy(hc)


@gpu
@pytest.mark.parametrize('mover', ['single', 'batch'])
@pytest.mark.parametrize('name', ['dec_m9_c16', 't2f3_m9_c16', 'dec_m3_c6_cat'])
def test_explicit_t_base(name, mover):
    """no stream context: the caller keeps HC history columns itself (launch_hist_restore / launch_hist_save, or launch_hist_batch)
    and passes t_base; run_deconv also with tb_soft (the up to 3 frames below t_base may be rewritten, with correct values only) and
    with t_out below T (frames from t_out on are not produced).  t_base in {1, 2, 3, 4, 5, 7, 8}, 3 and 9 new frames, on one running
    sequence."""
    sh = LAYERS[name]
    L = lib()
    h, info = make_plan(name)
    B = 2
    dec = sh['kind'] == 'deconv'
    # 3 new frames: the thin path, any first frame; 9: the tile / direct path - a multiple of 4, or any first frame under tb_soft
    cases = [(tb, soft, cut, n) for n in (3, 9) for tb in (1, 2, 3, 4, 5, 7, 8) for soft in ((0, 1) if dec else (0,))
             for cut in ((0, 1) if dec and tb in (3, 8) else (0,)) if n == 3 or soft or tb % 4 == 0]
    T = 8 + sum(c_[3] for c_ in cases)
    x = make((B, sh['Cin'], sh['Fin'], T), 'normal', 7400)
    y, bd = layer_ref(name, x, None)
    rows = sh['Cin'] * sh['Fin']
    fams = set()
    try:
        c = 8
        for tb, soft, cut, n in cases:
            case = '%s t_base %d soft %d cut %d n %d (%s)' % (name, tb, soft, cut, n, mover)
            Tw = tb + n
            state = x[..., c - tb:c].to(torch.float32).reshape(B, rows, tb).contiguous().cuda()      # what a save left after the last chunk
            win = torch.full((B, sh['Cin'], sh['Fin'], Tw), NAN, dtype=torch.float32)
            win[..., tb:] = x[..., c:c + n].to(torch.float32)
            wb = Buf(win.numel(), 0, win.cuda())
            if mover == 'single':
                nrm, _ = call('op_hist_restore', wb, state, B, rows, Tw, tb)
                assert [r['kernel'] for r in nrm] == ['hist']
            else:
                nrm, _ = call('op_hist_batch', (P * 1)(wb.ptr), (P * 1)(state.data_ptr()), (LL * 1)(rows), 1, B, Tw, tb, 0)
                assert [r['kernel'] for r in nrm] == ['hist_batch']
            note(nrm[0]['kernel'], case)
            full = wb.v.reshape(win.shape).cpu()
            assert wb.untouched() and torch.equal(full, x[..., c - tb:c + n].to(torch.float32)), '%s: restored window' % case
            t_out = Tw - 1 if cut else -1
            out, _, _, gc = run_layer_chunk(L, h, sh, info, split_src(sh, full), None, B, tb, n, case, (tb, t_out, soft))
            # the direct (<= 4 channel) kernel has no first frame: it produces every frame below t_out again, those below t_base
            # "without their own history" (kernels.h, launch_hist_restore) - its callers restore them afterwards.  Held to the rule
            # of tb_soft here: a rewritten frame whose taps lie inside the window must be correct
            direct = any(r['family'] in (FAM_DIRECT, FAM_DIRECT_LDS) for r in gc)
            lo = 0 if direct else ((tb & ~3) if soft else tb)
            hi = Tw - 1 if cut else Tw
            assert torch.isnan(out[..., :lo]).all() and torch.isnan(out[..., hi:]).all() and not torch.isnan(out[..., tb:hi]).any(), case
            # frames the soft start may rewrite: NaN or correct (their taps' history must be in the window: tb - lo <= 3, look-back 1)
            ref_w, bd_w = y[..., c - tb:c + n], bd[..., c - tb:c + n]
            for t in range(max(lo, info['lookback']), hi):
                col = out[..., t]
                if t < tb and torch.isnan(col).all():
                    continue
                check(case + ' col %d' % t, 'conv explicit t_base', col, ref_w[..., t], bd_w[..., t])
            # the caller's save: the last tb columns of the window into the state
            st2 = torch.full_like(state, NAN)
            if mover == 'single':
                call('op_hist_save', wb, st2, B, rows, Tw, tb)
            else:
                call('op_hist_batch', (P * 1)(wb.ptr), (P * 1)(st2.data_ptr()), (LL * 1)(rows), 1, B, Tw, tb, 1)
            assert torch.equal(st2.cpu().reshape(B, sh['Cin'], sh['Fin'], tb), full[..., Tw - tb:]), '%s: saved state' % case
            for r in gc:
                fams.add(family_of(r, info['direct']))
            c += n
        print('%s explicit t_base: families %s' % (name, sorted(fams)))
        for f in fams:
            note(f + ' explicit t_base', name)
    finally:
        L.op_plan_destroy(h)


# ------------------------------------------------------------------------------------------------ GPU: the history movers alone
def exchange_model(win, state, H, n, need):
    """columns [H - need, H) <- state; state <- the last `need` columns of the window (after the restore)"""
    win = win.copy()
    win[..., H - need:H] = state
    return win, win[..., H + n - need:H + n].copy()


EXCH = [(need, ns) for need in (1, 2, 3, 5, 8, 128, 256) for ns in ((max(need - 1, 1), 1, need, need + 3),)]


@gpu
@pytest.mark.parametrize('need,ns', EXCH)
@pytest.mark.parametrize('layout', ['dense', 'strided', 'f1_sf0'])
def test_stream_exchange_is_a_bitwise_copy(need, ns, layout):
    """stream_exchange over four consecutive chunks with n below, equal to and above `need` (n < need: the new state begins with the
    tail of the old one), row counts that are no multiple of 256 / KP, non-contiguous batch / channel strides, and the F = 1, sf = 0
    form; integer-exact: the window and the state slot are compared bit for bit, everything else keeps its NaN"""
    B, Cc, F_ = 3, 5, (1 if layout == 'f1_sf0' else 3)
    H = need + (2 if need < 128 else 0)
    g = np.random.default_rng(need)
    st = Stream(B)
    state = np.zeros((B, Cc, F_, need), np.float32)
    try:
        for i, n in enumerate(ns):
            T = H + n
            pc, pb = (F_ * T + 7, Cc * (F_ * T + 7) + 11) if layout == 'strided' else (F_ * T, Cc * F_ * T)
            full = np.full((B, pb), np.nan, np.float32)
            view = np.lib.stride_tricks.as_strided(full, (B, Cc, F_, T), (pb * 4, pc * 4, T * 4, 4))
            view[..., :H] = np.nan
            view[..., H:] = g.standard_normal((B, Cc, F_, n)).astype(np.float32)
            want, state = exchange_model(view, state, H, n, need)
            buf = Buf(full.size, 0, torch.from_numpy(full).cuda())
            st.open(H, n, 100 * i)
            nrm, gc = call('op_exchange', buf, pb, pc, 0 if layout == 'f1_sf0' else T, B, Cc, F_, need)
            st.close()
            assert [r['kernel'] for r in nrm] == ['stream_hist'] and not gc
            got = np.lib.stride_tricks.as_strided(buf.v.cpu().numpy().reshape(B, pb), (B, Cc, F_, T), (pb * 4, pc * 4, T * 4, 4))
            ref = full.copy()
            np.lib.stride_tricks.as_strided(ref, (B, Cc, F_, T), (pb * 4, pc * 4, T * 4, 4))[...] = want
            assert buf.untouched() and np.array_equal(buf.v.cpu().numpy().view(np.uint32), ref.reshape(-1).view(np.uint32)), (need, n, layout)
            assert not np.isnan(got[..., H - need:]).any()
            assert st.slots() == [B * Cc * F_ * need * 4]
            assert np.array_equal(st.read(0).view(np.uint32), np.ascontiguousarray(state).reshape(-1).view(np.uint32)), (need, n, layout)
        note('stream_hist', 'need %d %s' % (need, layout))
    finally:
        st.destroy()


@gpu
@pytest.mark.parametrize('dims', [((2, 7), (9, 1)), ((9, 1), (2, 7)), ((3, 4), (3, 4))])
@pytest.mark.parametrize('need', [1, 3, 128])
def test_stream_exchange_pair_equals_two_single_calls(dims, need):
    """two sources whose C, F and row counts differ in both directions: windows, slot order and slot contents identical to two
    stream_exchange calls, over three chunks"""
    B, H = 3, need + 1
    g = np.random.default_rng(need + dims[0][0])
    sp, ss = Stream(B), Stream(B)
    try:
        for i, n in enumerate((max(need - 1, 1), need, need + 2)):
            T = H + n
            wins = []
            for Cc, F_ in dims:
                w = np.full((B, Cc, F_, T), np.nan, np.float32)
                w[..., H:] = g.standard_normal((B, Cc, F_, n)).astype(np.float32)
                wins.append(w)
            pb = [Buf(w.size, 0, torch.from_numpy(w).cuda()) for w in wins]
            sb = [Buf(w.size, 0, torch.from_numpy(w).cuda()) for w in wins]
            (C0, F0), (C1, F1) = dims
            sp.open(H, n, i)
            nrm, _ = call('op_exchange_pair', pb[0], C0 * F0 * T, F0 * T, T, C0, F0, pb[1], C1 * F1 * T, F1 * T, T, C1, F1, B, need)
            sp.close()
            assert [r['kernel'] for r in nrm] == ['stream_hist_pair']
            ss.open(H, n, i)
            for b_, (Cc, F_) in zip(sb, dims):
                call('op_exchange', b_, Cc * F_ * T, F_ * T, T, B, Cc, F_, need)
            ss.close()
            for a, b_ in zip(pb, sb):
                assert a.untouched() and np.array_equal(a.v.cpu().numpy().view(np.uint32), b_.v.cpu().numpy().view(np.uint32))
                assert not torch.isnan(a.v.reshape(B, -1, T)[..., H - need:]).any()
            assert sp.slots() == ss.slots() == [B * Cc * F_ * need * 4 for Cc, F_ in dims]
            for k in range(2):
                assert np.array_equal(sp.read(k), ss.read(k))
        note('stream_hist_pair', 'need %d dims %s' % (need, dims))
    finally:
        sp.destroy()
        ss.destroy()


@gpu
@pytest.mark.parametrize('save', [0, 1])
def test_hist_batch_sixteen_tensors(save):
    """launch_hist_batch on 16 tensors of different row counts, one above 65 536 elements per tensor so that the grid-stride loop
    runs (its grid stops at 256 workgroups of 256 threads), against plain indexing, bit for bit; no tensors: a no-op"""
    B, Tw, hc = 2, 11, 3
    rows = [1, 2, 3, 5, 7, 16, 31, 33, 64, 100, 127, 129, 255, 257, 12001, 4]
    assert B * max(rows) * hc > 65536
    g = np.random.default_rng(5 + save)
    bufs = [torch.from_numpy(g.standard_normal((B, r, Tw)).astype(np.float32)).cuda() for r in rows]
    states = [torch.from_numpy(g.standard_normal((B, r, hc)).astype(np.float32)).cuda() for r in rows]
    b0, s0 = [b_.clone() for b_ in bufs], [s.clone() for s in states]
    nrm, gc = call('op_hist_batch', (P * 16)(*[b_.data_ptr() for b_ in bufs]), (P * 16)(*[s.data_ptr() for s in states]), (LL * 16)(*rows), 16, B, Tw, hc, save)
    assert [r['kernel'] for r in nrm] == ['hist_batch'] and not gc
    for b_, s, bo, so in zip(bufs, states, b0, s0):
        if save:
            assert torch.equal(b_, bo) and torch.equal(s, bo[..., Tw - hc:])
        else:
            assert torch.equal(s, so) and torch.equal(b_[..., :hc], so) and torch.equal(b_[..., hc:], bo[..., hc:])
    nrm, gc = call('op_hist_batch', None, None, None, 0, B, Tw, hc, save)
    assert not nrm and not gc
    note('hist_batch grid-stride', 'save %d' % save)


# ------------------------------------------------------------------------------------------------ refusals
@gpu
def test_refusals_launch_nothing():
    """host checks: refused by message, nothing launched (both launch logs stay empty)"""
    L = lib()
    B = 1
    x = torch.zeros(B * 2 * 300, dtype=torch.float32, device='cuda')
    big = torch.zeros(B * 256 * 8, dtype=torch.float32, device='cuda')
    out = torch.full_like(big, NAN)
    blocks = {}
    for key, (ks, K) in dict(a=(3, 0), b=(5, 0), c=(3, 65)).items():
        blocks[key] = tcm_block(tcm_params(1, ks, False, True, K), 1, K, ks, False)
    h, info = make_plan('t2f3_m9_c16')
    sh = LAYERS['t2f3_m9_c16']
    src = torch.zeros(B * sh['Cin'] * sh['Fin'] * 8, dtype=torch.float32, device='cuda')
    dst = torch.full((B * sh['M'] * sh['Fout'] * 8,), NAN, dtype=torch.float32, device='cuda')
    cases = [
        ((2, 1), 'history deeper than the window keeps', 'op_exchange', (x, 6, 3, 3, B, 2, 1, 3)),                       # need > H
        ((258, 1), 'more than 256 history columns', 'op_exchange', (x, 2 * 259, 259, 259, B, 2, 1, 257)),                # need > 256
        ((1, 1), '1..8 blocks', 'op_tcm_chain_launch', ((P * 9)(*[blocks['a']] * 9), 9, big, out)),
        ((1, 1), "share the dilated conv's tap count", 'op_tcm_chain_launch', ((P * 2)(blocks['a'], blocks['b']), 2, big, out)),
        ((1, 1), 'FIR longer than 64 taps', 'op_tcm_chain_launch', ((P * 1)(blocks['c']), 1, big, out)),
        ((2, 3), 'not a window of the current chunk', 'op_layer_run', (h, src, None, sh['Fin'], dst, sh['M'], sh['Fout'], None, B, 6, 6, 0, -1, 0)),
    ]
    try:
        for (H, n), msg, fn, args in cases:
            st = Stream(B)      # (a refusal may have taken a slot: every case gets its own stream)
            try:
                st.open(H, n, 0)
                refused(msg, fn, *args)
            finally:
                st.destroy()
        assert torch.isnan(out).all() and torch.isnan(dst).all()
    finally:
        L.op_plan_destroy(h)
        for h_ in blocks.values():
            L.op_tcm_destroy(h_)


# ------------------------------------------------------------------------------------------------ coverage
TARGET_FORMS = ['tcm_chain<3>', 'tcm_chain<5>', 'tcm_chain<3> mid-stream', 'tcm_chain<5> mid-stream', 'thin at t_base > 0', 'thin pair at t_base > 0',
                'tile resident at t_base > 0', 'tile plain at t_base > 0', 'direct at t_base > 0', 'stream_hist', 'stream_hist_pair', 'hist',
                'hist_batch', 'hist_batch grid-stride', 'memo: one exchange for two parity classes']


@gpu
def test_every_form_reached():
    """every kernel form this file is about was seen in a launch log by the cases above (runs last: pytest keeps file order)"""
    print('worst error / bound by family:')
    for k in sorted(WORST):
        print('  %-60s %.3f  (%s)' % (k, WORST[k][0], WORST[k][1]))
    missing = [f for f in TARGET_FORMS if f not in REACHED]
    assert not missing, missing
