"""One recurrent layer (or stack) at a time against a float64 LSTM / GRU.  The recurrent kernels pick among a dozen forms by hidden
size, sequence count, LSTMs per launch, CU count, an LDS budget and 32-bit offset bounds (csrc/lstm_select.h: lstm_coop_select, the
support queries and the chunk pipeline's plan, which `expected_coop` ... `chunk_plan` below mirror; the one-sequence stack kernel,
k_lstm.hip's persistent kernels, k_lstm_short.hip, and the per-step EPI_LSTM epilogue of gemmconv.hip); they exchange h_t across
workgroups through tagged or flagged slabs.  The whole-model suites
reach a few of those forms at a few (S, T).  Here every case is one layer of torch.nn tensors, turned into an engine layer by the
engine's own loaders and run through the entry points the models call (csrc/tests/lstm_probe.hip -> libse_lstmprobe.so); every
stored h_t is checked against float64, every element the layer does not own must still hold its NaN sentinel, and the form the
launch log reports must be the one `expected_forms` (a mirror of the launchers' selection) predicts for this device's CU count.

Error bound (`reference`), per stored element, carried step by step beside the float64 recurrence (u = 2^-24):
  * gate pre-activation a = W_ih x + b + W_hh h_{t-1}, a sum of K = I + H products (plus the bias) in fp32, whichever way the
    kernel splits or orders it.  The worst case is u K (sum |W_ih| |x| + |b| + sum |W_hh| |h_{t-1}|); it assumes every rounding of
    the sum has the same sign and is never approached (an exact fp32 evaluation stays below 5e-4 of it at H = 1024).  The K
    roundings have independent signs, each at most u times the magnitude above: the bound takes
        |da| <= c u sqrt(K) (sum |W_ih| |x| + |b| + sum |W_hh| |h_{t-1}|),   c = 4  (~7 standard deviations of their sum),
    plus the error e_{t-1} of h_{t-1} (and, in a stack, of the layer's input) carried through the matrix.  Its components are
    sums of H terms of independent rounding origin; the bound takes Q sqrt(sum_k W_jk^2 E_k^2) with Q = 3.  (The worst case
    sum_k |W_jk| E_k grows ~2.5x per step at H = 1024 with the weights below and would be useless after a dozen steps; in the
    quadrature form the recurrence contracts - about 0.3x per step in the ordinary regime.)
  * each hardware sigmoid / tanh (v_exp_f32 + v_rcp_f32, 1 ulp each, plus the roundings around them): D = 8u absolute; an input
    error da moves it by at most s'(a) da (linearised at the float64 point: da is < 1e-2 where s' is not tiny).
  * cell c_t = f c_{t-1} + i g and h_t = o tanh(c_t): first-order propagation of the above, the carried cell error f E_c, 2u for
    the products and the sum; h_t gets 4u |h_t| for its own rounding and for the tagged exchange, whose 1-bit step tag replaces
    the lowest mantissa bit of h_t (<= 1 ulp per step).
  * GRU: the same for r, z, n = tanh(a_n + r (W_hn h + b_hn)) and h' = (1 - z) n + z h (carried error z E_h).
test_bound_catches_plausible_faults (CPU) shows the bound is tight enough to see the faults these kernels could have; each GPU
case prints its worst error as a fraction of the bound.

Forms that only a tuning switch selects (SE_COOP16=0, SE_COOP4=0) run in one child process per switch
(test_switch_only_forms)."""
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
PROBE_LIB = os.environ.get('SE_LSTMPROBE_LIB') or os.path.join(PKG, 'libse_lstmprobe.so')      # (as SE_ENGINE_LIB: A/B another build)

U = 2.0 ** -24
ACT_ULP = 8 * U            # absolute error of one fast-math sigmoid / tanh
C_DOT = 4.0                # the dot products' rounding: C_DOT u sqrt(K) of the magnitude sum
Q_PROP = 3.0               # quadrature factor of the error carried through W_hh / W_ih
EPI_LSTM = 1
CHUNK_T = 48               # rnn.h lstm_stack_chunked_fm: steps per chunk


# ------------------------------------------------------------------------------------------------ float64 reference
def layer_params(H, I, seed, gru=False, regime='ordinary', dtype=torch.float64):
    """torch.nn.LSTM / GRU tensors of one layer.  ordinary: torch's default init U(+-1/sqrt(H)) times 1/2 (the recurrence
    contracts); saturating: input weights x8 and biases U(+-6) (+6 on the forget gate): many gates sit at 0 / 1 and c grows."""
    g = np.random.default_rng(seed)
    G = 3 if gru else 4
    k = 1.0 / math.sqrt(H)
    p = {'wih': g.uniform(-k, k, (G * H, I)) * 0.5, 'whh': g.uniform(-k, k, (G * H, H)) * 0.5,
         'bih': g.uniform(-k, k, G * H) * 0.5, 'bhh': g.uniform(-k, k, G * H) * 0.5}
    if regime == 'saturating':
        p['wih'] *= 8.0
        p['bih'] = g.uniform(-6.0, 6.0, G * H)
        if not gru:
            p['bih'][H:2 * H] += 6.0
    # the values the kernels see are fp32: the reference starts from exactly those
    return {n: torch.from_numpy(v.astype(np.float32)).to(dtype) for n, v in p.items()}


def make_input(T, S, I, seed, regime='ordinary'):
    g = np.random.default_rng(seed)
    x = g.standard_normal((T, S, I)) * (2.0 if regime == 'saturating' else 1.0)
    return torch.from_numpy(x.astype(np.float32)).to(torch.float64)


def reference(x, p, gru=False, h0=None, c0=None, reverse=False, Ex=None, fault=None):
    """float64 LSTM (gate rows i, f, g, o) / GRU (r, z, n) over x [T][S][I] from (h0, c0) (default zeros), and the elementwise error
    bound of its fp32 form (module docstring).  Returns h [T][S][H], bound [T][S][H], the final (h, c) and their bounds.
    Ex: bound of x itself (an upper layer of a stack).  fault: test_bound_catches_plausible_faults's injected defects."""
    T, S, I = x.shape
    H = p['whh'].shape[1]
    dev = x.device
    wih, whh, bih, bhh = (p[n].to(dev, torch.float64) for n in ('wih', 'whh', 'bih', 'bhh'))
    if fault and fault['kind'] == 'gate_swap':          # rows of gates a and b of unit u trade places
        a, b = fault['gates'][0] * H + fault['u'], fault['gates'][1] * H + fault['u']
        perm = torch.arange(wih.shape[0], device=dev)
        perm[a], perm[b] = b, a
        wih, whh, bih, bhh = wih[perm], whh[perm], bih[perm], bhh[perm]
    awih, awhh = wih.abs(), whh.abs()
    wih2, whh2 = wih * wih, whh * whh
    K = H + I
    z = lambda: torch.zeros((S, H), dtype=torch.float64, device=dev)
    h = z() if h0 is None else h0.to(dev, torch.float64).clone()
    c = z() if c0 is None else c0.to(dev, torch.float64).clone()
    h_prev = h.clone()
    Eh, Ec = z(), z()
    out = torch.empty((T, S, H), dtype=torch.float64, device=dev)
    E = torch.empty_like(out)
    dsig = lambda s: s * (1 - s)
    for n_step, t in enumerate(range(T - 1, -1, -1) if reverse else range(T)):
        hu = h
        if fault and fault['kind'] == 'stale_h' and n_step == fault['step']:
            hu = h.clone()
            hu[fault['seq']] = h_prev[fault['seq']]          # one sequence reads h_{t-2}
        if fault and fault['kind'] == 'c_reset' and n_step == fault['step']:
            c = z()                                          # the cell state lost at a chunk boundary
        xt = x[t]
        mag = xt.abs() @ awih.T + bih.abs() + bhh.abs() + hu.abs() @ awhh.T
        ep = U * C_DOT * math.sqrt(K) * mag + Q_PROP * torch.sqrt((Eh * Eh) @ whh2.T)
        if Ex is not None:
            ep = ep + Q_PROP * torch.sqrt((Ex[t] * Ex[t]) @ wih2.T)
        gx = xt @ wih.T + bih
        gh = hu @ whh.T + bhh
        if gru:
            r = torch.sigmoid(gx[:, :H] + gh[:, :H])
            zz = torch.sigmoid(gx[:, H:2 * H] + gh[:, H:2 * H])
            hw = gh[:, 2 * H:]
            nn_ = torch.tanh(gx[:, 2 * H:] + r * hw)
            hn = (1 - zz) * nn_ + zz * hu
            e_r, e_z, e_n = ep[:, :H], ep[:, H:2 * H], ep[:, 2 * H:]
            en = (1 - nn_ * nn_) * (e_n * (1 + r) + hw.abs() * (dsig(r) * e_r + ACT_ULP)) + ACT_ULP
            Eh = (nn_ - hu).abs() * (dsig(zz) * e_z + ACT_ULP) + (1 - zz) * en + zz * Eh + 4 * U * (hn.abs() + nn_.abs() + hu.abs())
            cn = hn
        else:
            a = gx + gh
            si, sf = torch.sigmoid(a[:, :H]), torch.sigmoid(a[:, H:2 * H])
            tg, so = torch.tanh(a[:, 2 * H:3 * H]), torch.sigmoid(a[:, 3 * H:])
            e_i, e_f, e_g, e_o = ep[:, :H], ep[:, H:2 * H], ep[:, 2 * H:3 * H], ep[:, 3 * H:]
            cn = sf * c + si * tg
            Ec = sf * Ec + c.abs() * (dsig(sf) * e_f + ACT_ULP) + tg.abs() * (dsig(si) * e_i + ACT_ULP) + \
                si * ((1 - tg * tg) * e_g + ACT_ULP) + 2 * U * ((sf * c).abs() + (si * tg).abs())
            tc = torch.tanh(cn)
            hn = so * tc
            Eh = tc.abs() * (dsig(so) * e_o + ACT_ULP) + so * ((1 - tc * tc) * Ec + ACT_ULP) + 4 * U * hn.abs()
        h_prev, h, c = h, hn, cn
        out[t] = h
        E[t] = Eh
    if fault and fault['kind'] == 'neighbour':                # a ragged tile's last sequence taken from its neighbour
        out[:, fault['seq']] = out[:, fault['seq'] - 1]
    return out, E, (h, c, Eh, Ec)


def ratio(got, want, bound):
    """Worst |got - want| / bound (NaN / inf in `got` count as infinitely wrong)."""
    err = (got.to(torch.float64) - want).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float('inf')))
    return float((err / bound).max())


# ------------------------------------------------------------------------------------------------ the launchers' selection
def expected_coop(H, S, Z, n_cu, gx_row, out_row, coop16=True, coop4=True):
    """The kernel launch_lstm_coop (k_lstm_coop.hip) runs for one call, as a form string (see `form_of`)."""
    US = H // 16
    if H == 256:                                             # opt-in width: lstm_coop256_supported -> launch_c16<256>
        return 'coop16<256>'
    # launch_lstm_coop: the K-split form for one tile (S <= 16 at 1024, <= 4 at 512, at most two LSTMs at 512)
    if S <= (16 if H == 1024 else 4) and (H == 1024 or Z <= 2) and (H // 4) * Z <= n_cu and (H // 4) * Z <= 256:
        ns, tag = (1, 1) if S <= 1 else (4, 1) if S <= 4 else (16, 0)            # launch_ks_n
        return f'ks<{H},{ns},{tag}>'
    bounds_ok = S * H * 8 < 2 ** 31 and gx_row * 4 * H * 4 < 4.0e9 and out_row * H < 4.0e9

    def c16():                                               # launch_c16
        if not coop16 or S < 17 or US * Z > n_cu or not bounds_ok:
            return None
        nt = -(-S // 16)
        ss = max(1, min(nt, n_cu // (US * Z)))
        ntl = -(-nt // ss)
        return f'coop16<{H}>' if (2 * 16 * (H + 4) + 2 * 4 * 256 + 4 * ntl * 64) * 4 <= 160 * 1024 else None

    def c4():                                                # launch_c4_n
        if not coop4 or S < 17 or US * Z > n_cu or not bounds_ok:
            return None
        ns4 = -(-S // 4)
        ss = max(1, min(ns4, n_cu // (US * Z)))
        if -(-ns4 // ss) * 256 > 24 * 1024:
            return None
        nsub_min = ns4 // ss
        lead = min(3, nsub_min)
        if 3 <= nsub_min < 6:
            lead = 2
        return f'coop8<{H},{max(lead, 1)},4>'

    us_z, nt16 = US * Z, -(-S // 16)
    sub4 = H == 1024 and us_z <= n_cu and nt16 <= n_cu // us_z and S * us_z < 60 * n_cu // 4
    for f in ((c4,) if sub4 else ()) + (c16, c4):
        r = f()
        if r:
            return r
    return f'coop<{H}>'                                      # launch_t: the flag-barrier form


def coop256_supported(S, n_cu, coop16=True):
    """lstm_coop256_supported (k_lstm_coop.hip)."""
    H, US = 256, 16
    if not coop16 or S < 17 or S > 4096 or US > n_cu or S * H * 8 >= 2 ** 31 or S * 4 * H * 4 >= 4.0e9:
        return False
    nt = -(-S // 16)
    ss = max(1, min(nt, n_cu // US))
    return (2 * 16 * (H + 4) + 2 * 4 * 256 + 4 * -(-nt // ss) * 64) * 4 <= 160 * 1024


def coop_supported(H, S, Z):
    """lstm_coop_supported (k_lstm_coop.hip)."""
    return H in (512, 1024) and (H // 16) * Z <= 256 and S <= 4096


def chunk_supported(H, S, L, T, n_cu):
    """lstm_coop_chunk_supported (k_lstm_coop.hip) and the further conditions of rnn.h lstm_stack_chunked_fm."""
    if H not in (512, 1024) or not 2 <= L <= 4 or S < 17:
        return False
    US, NT = H // 16, -(-S // 16)
    if not (US * L <= n_cu and NT <= n_cu // US and S * H * 8 < 2 ** 31):
        return False
    if T * S * 4 * H * 4 >= 4.0e9 or T * S * H >= 4.0e9:
        return False
    tc = max(2, min(CHUNK_T, T)) & ~1
    return T >= 2 * tc


def chunk_plan(T, L):
    """(lz, t0, Tz) of every z of every launch of rnn.h lstm_stack_chunked_fm."""
    nc = -(-T // CHUNK_T)
    plan = []
    for s in range(nc + L - 1):
        plan.append([(l, (s - l) * CHUNK_T, min(CHUNK_T, T - (s - l) * CHUNK_T)) for l in range(L) if 0 <= s - l < nc])
    return plan


def expected_forms(case, n_cu, coop16=True, coop4=True):
    """The recurrent dispatches case `case` makes, as a list of form strings ('step' / 'step gru' / 'step_x': the EPI_LSTM GEMM
    launches of a layer that runs one step per launch, listed once)."""
    k, H, S, T = case['kind'], case['H'], case['S'], case['T']
    if k == 'cols':
        whole = case.get('c0', 0) == 0 and case.get('Sn', S) == S and not case.get('gru')
        if whole and H == 256 and case.get('coop256') and coop256_supported(S, n_cu, coop16):
            return ['coop16<256>']
        if whole and H in (512, 1024) and coop_supported(H, S, 1):
            return [expected_coop(H, S, 1, n_cu, S, case.get('out_rs', 1) * S, coop16, coop4)]
        return ['step gru' if case.get('gru') else 'step']
    if k == 'fm':
        return [expected_coop(H, S, 1, n_cu, T * S, T * S, coop16, coop4)]
    if k == 'pair':
        if coop_supported(H, S, 2):
            return [expected_coop(H, S, 2, n_cu, S, 2 * S, coop16, coop4)]
        return [expected_coop(H, S, 1, n_cu, S, 2 * S, coop16, coop4)] * 2 if coop_supported(H, S, 1) else ['step']
    if k == 'stack':
        return [f"stack<{H},{case['L']}>"]
    if k == 'chunk':
        L = case['L']
        if not chunk_supported(H, S, L, T, n_cu):
            return None
        return [f'chunk coop16<{H}>'] * len(chunk_plan(T, L))
    if k == 'stream':
        return ['step gru' if case.get('gru') else 'step']
    if k == 'cols_x':
        return ['step_x']
    if k == 'persist':
        if H == 128 and not case.get('carry') and -(-S // 16) * case['Z'] * case['O'] <= 128:
            return ['persist4<128>']
        return [f'persist<{H}>']
    if k == 'short':
        return ['short']
    raise ValueError(k)


def form_of(name, r):
    """Form string of one launch-log record."""
    if name == 'ks':
        return f"ks<{r['H']},{r['NS']},{r['TAG']}>"
    if name == 'coop8':
        return f"coop8<{r['H']},{r['LEAD']},{r['NW']}>"
    if name == 'coop16':
        return f"{'chunk ' if r['chunk'] else ''}coop16<{r['H']}>"
    if name == 'stack':
        return f"stack<{r['H']},{r['L']}>"
    if name == 'short':
        return 'short'
    return f"{name}<{r['H']}>"            # coop, persist, persist4


# ------------------------------------------------------------------------------------------------ the probe
class Probe:
    REC = ('H', 'NS', 'TAG', 'LEAD', 'NW', 'L', 'Z', 'SS', 'chunk', 'grid', 'shmem', 'lz0', 'lz1', 'lz2', 'lz3', 't00', 't01', 't02',
           't03', 'Tz0', 'Tz1', 'Tz2', 'Tz3')
    _lib = None

    @classmethod
    def lib(cls):
        if cls._lib is None:
            assert os.path.exists(PROBE_LIB), f'{PROBE_LIB} is not built (make -C {PKG}/csrc)'
            lib = C.CDLL(PROBE_LIB)      # (after torch: one HIP runtime per process, see se_amd/_lib.py)
            vp, i32, i64, fp = C.c_void_p, C.c_int, C.c_long, C.POINTER(C.c_float)
            lib.lsp_last_error.restype = C.c_char_p
            lib.lsp_layer_create.restype = vp
            lib.lsp_layer_create.argtypes = [fp, fp, fp, fp] + [i32] * 6
            lib.lsp_layer_destroy.argtypes = [vp]
            lib.lsp_run_cols.argtypes = [vp, vp, i64, vp, vp, vp, i64, i32, i32, i32, i32, i32]
            lib.lsp_run_fm.argtypes = [vp, vp, vp, vp, vp, i32, i32]
            lib.lsp_run_stream.argtypes = [vp, vp, i64, vp, vp, vp, vp, i64, i32, i32, i32, i32]
            lib.lsp_run_cols_x.argtypes = [vp, vp, i64, vp, vp, vp, i64, i32, i32, i32, i32, i32]
            lib.lsp_run_pair.argtypes = [vp, vp, vp, vp, i64, vp, vp, vp, i64, i64, i32, i32, i32]
            lib.lsp_stack_fm.argtypes = [C.POINTER(vp), i32, vp, vp, vp, i32, C.POINTER(i32)]
            lib.lsp_stack_chunked_fm.argtypes = [C.POINTER(vp), i32, vp, vp, vp, C.POINTER(vp), i32, i32, C.POINTER(i32)]
            lib.lsp_persist.argtypes = [C.POINTER(vp), i32, vp, i64, i64, i32, vp, vp, i64, i64, i64, i64, i32, i32, i32, vp, vp]
            lib.lsp_short.argtypes = [C.POINTER(vp), i32, vp, i64, i64, i64, vp, i64, i64, i64, i64, i32, i32, i32, i32]
            lib.lsp_launch_kernel.restype = C.c_char_p
            lib.lsp_launch_kernel.argtypes = [i32]
            lib.lsp_launch_get.argtypes = [i32, C.POINTER(C.c_longlong), i32]
            lib.lsp_gc_get.argtypes = [i32, C.POINTER(C.c_longlong), i32]
            lib.lsp_register_overread.argtypes = [vp, C.c_size_t]
            lib.lsp_unregister_overread.argtypes = [vp]
            cls._lib = lib
        return cls._lib

    def __init__(self):
        self.layers, self.bufs = [], []

    def layer(self, p, I, H, gru=False, fuse_x=False, coop256=False, s_hint=64):
        f32 = [np.ascontiguousarray(p[n].cpu().numpy(), dtype=np.float32) for n in ('wih', 'whh', 'bih', 'bhh')]
        ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        h = self.lib().lsp_layer_create(*(ptr(a) for a in f32), I, H, int(gru), int(fuse_x), int(coop256), s_hint)
        assert h, self.lib().lsp_last_error().decode()
        self.layers.append(h)
        return h

    def buf(self, n, fill=float('nan'), register=False):
        """A device tensor of n fp32 values (+ 16 B of slack, as the engine's arenas have) filled with `fill`."""
        t = torch.full((n + 4,), fill, dtype=torch.float32, device='cuda')
        self.bufs.append(t)
        if register:
            self.lib().lsp_register_overread(t.data_ptr(), (n + 4) * 4)
            self.registered = getattr(self, 'registered', []) + [t.data_ptr()]
        return t[:n]

    def check(self, rc):
        assert rc == 0, self.lib().lsp_last_error().decode()

    def log(self):
        lib = self.lib()
        recs = []
        for i in range(lib.lsp_launch_count()):
            out = (C.c_longlong * len(self.REC))()
            lib.lsp_launch_get(i, out, len(self.REC))
            r = dict(zip(self.REC, out))
            recs.append((lib.lsp_launch_kernel(i).decode(), r))
        gc = []
        for i in range(lib.lsp_gc_count()):
            out = (C.c_longlong * 3)()
            lib.lsp_gc_get(i, out, 3)
            gc.append(dict(epi=out[0], gru=out[1], nblk=out[2]))
        return recs, gc

    def close(self):
        torch.cuda.synchronize()
        for p in getattr(self, 'registered', []):
            self.lib().lsp_unregister_overread(p)
        for h in self.layers:
            self.lib().lsp_layer_destroy(h)
        self.layers, self.bufs, self.registered = [], [], []


def forms_logged(recs, gc, T, fused=False):
    """The recurrent forms a run dispatched; the per-step launches of the gemmconv log as one 'step' / 'step gru' / 'step_x', once
    there are at least T of them (one or more per step)."""
    forms = [form_of(n, r) for n, r in recs]
    steps = [g for g in gc if g['epi'] == EPI_LSTM]
    if steps:
        kinds = sorted({'step_x' if fused else 'step gru' if g['gru'] else 'step' for g in steps})
        forms += kinds if len(steps) >= T else [f'{kinds} x {len(steps)} launches for {T} steps']
    return forms


def dev(t):
    return t.to('cuda', torch.float32).contiguous()


def n_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ------------------------------------------------------------------------------------------------ one case
def check_owned(out, idx, want, bound, what):
    """Elements `idx` of the flat device tensor `out` against (want, bound); every other element must still be NaN."""
    got = out[idx.reshape(-1)].reshape(idx.shape)
    r = ratio(got, want, bound)
    rest = out.clone()
    rest[idx.reshape(-1)] = float('nan')
    assert bool(torch.isnan(rest).all()), f'{what}: {int((~torch.isnan(rest)).sum())} elements outside the layer written'
    return r


def out_index(T, S, H, out_t, row, n0=0, Sn=None, base=0):
    """Flat indices [T][Sn][H] of h_t (sequence n0 + n, unit j) at base + t out_t + j row + n0 + n."""
    Sn = S if Sn is None else Sn
    t = torch.arange(T, device='cuda')[:, None, None]
    n = torch.arange(Sn, device='cuda')[None, :, None] + n0
    j = torch.arange(H, device='cuda')[None, None, :]
    return base + t * out_t + j * row + n


def run_case(case, coop16=True, coop4=True):
    """Builds, runs and checks one case.  Returns (worst error / bound, forms logged, forms expected)."""
    k, H, S, T = case['kind'], case['H'], case['S'], case['T']
    gru = case.get('gru', False)
    I = case.get('I', H)
    regime = case.get('regime', 'ordinary')
    seed = case.get('seed', 1)
    n_cu = n_cus()
    want_forms = expected_forms(case, n_cu, coop16, coop4)
    pr = Probe()
    lib = pr.lib()
    worst = 0.0
    try:
        if k in ('cols', 'fm', 'stream', 'cols_x'):
            p = layer_params(H, I, seed, gru, regime)
            x = make_input(T, S, I, seed + 100, regime).cuda()
            h = pr.layer(p, I, H, gru=gru, fuse_x=(k == 'cols_x'), coop256=case.get('coop256', False), s_hint=S)
            out_rs = case.get('out_rs', 1)
            c0, Sn = case.get('c0', 0), case.get('Sn', S)
            if k == 'fm':
                xd = pr.buf(I * T * S, register=True)
                xd.copy_(dev(x.permute(2, 0, 1)).reshape(-1))                 # [I][T][S]
                out = pr.buf(H * T * S, register=True)
                G, cell = pr.buf(4 * H * T * S, 0.0), pr.buf(H * S, 0.0)
                pr.check(lib.lsp_run_fm(h, xd.data_ptr(), G.data_ptr(), cell.data_ptr(), out.data_ptr(), T, S))
                want, bound, _ = reference(x, p, gru)
                idx = out_index(T, S, H, S, T * S)                          # [H][T][S]
                worst = check_owned(out, idx, want, bound, 'out')
            else:
                xd = pr.buf(T * I * S, register=True)
                xd.copy_(dev(x.permute(0, 2, 1)).reshape(-1))                 # [T][I][S]
                out_t = H * S * out_rs
                out = pr.buf(T * out_t, register=True)
                cell = pr.buf(H * S, 0.0)
                if k == 'cols':
                    G = pr.buf(T * 4 * H * S, 0.0)
                    pr.check(lib.lsp_run_cols(h, xd.data_ptr(), I * S, G.data_ptr(), cell.data_ptr(), out.data_ptr(), out_t, out_rs,
                                              T, S, c0, Sn))
                    want, bound, _ = reference(x[:, c0:c0 + Sn], p, gru)
                    worst = check_owned(out, out_index(T, S, H, out_t, out_rs * S, c0, Sn), want, bound, 'out')
                elif k == 'cols_x':
                    hz = pr.buf(H * S, 0.0, register=True)
                    pr.check(lib.lsp_run_cols_x(h, xd.data_ptr(), I * S, cell.data_ptr(), hz.data_ptr(), out.data_ptr(), out_t, out_rs,
                                                T, S, c0, Sn))
                    want, bound, _ = reference(x[:, c0:c0 + Sn], p, gru)
                    worst = check_owned(out, out_index(T, S, H, out_t, out_rs * S, c0, Sn), want, bound, 'out')
                else:           # stream: T1 steps from the stream's start, then T - T1 more from the state they left
                    T1 = case['T1']
                    G = pr.buf(T * 4 * H * S, 0.0)
                    hs = pr.buf(H * S, 0.0, register=True)
                    pr.check(lib.lsp_run_stream(h, xd.data_ptr(), I * S, G.data_ptr(), cell.data_ptr(), hs.data_ptr(), out.data_ptr(),
                                                out_t, out_rs, T1, S, 1))
                    want, bound, (hT, cT, EhT, EcT) = reference(x[:T1], p, gru)
                    worst = check_owned(out[:T1 * out_t], out_index(T1, S, H, out_t, out_rs * S), want, bound, 'out (first part)')
                    state_h = hs.reshape(H, S).T
                    state_c = cell.reshape(H, S).T
                    worst = max(worst, ratio(state_h, hT, EhT), ratio(state_c, cT, EcT if not gru else EhT))
                    h0, cc0 = state_h.to(torch.float64).clone(), state_c.to(torch.float64).clone()
                    recs1, gc1 = pr.log()
                    pr.check(lib.lsp_run_stream(h, xd[T1 * I * S:].data_ptr(), I * S, G.data_ptr(), cell.data_ptr(), hs.data_ptr(),
                                                out[T1 * out_t:].data_ptr(), out_t, out_rs, T - T1, S, 0))
                    want, bound, (hT, cT, EhT, EcT) = reference(x[T1:], p, gru, h0=h0, c0=cc0)
                    worst = max(worst, check_owned(out[T1 * out_t:], out_index(T - T1, S, H, out_t, out_rs * S), want, bound,
                                                   'out (continued)'))
                    worst = max(worst, ratio(hs.reshape(H, S).T, hT, EhT), ratio(cell.reshape(H, S).T, cT, EcT if not gru else EhT))
                    recs2, gc2 = pr.log()
                    got_forms = forms_logged(recs1 + recs2, gc1 + gc2, T)
                    return worst, got_forms, want_forms
        elif k == 'pair':               # GCRN's grouped LSTM: x [T][2I][S] (group z: features z I ...), h interleaved (out_rs = 2)
            ps = [layer_params(H, I, seed + z, False, regime) for z in range(2)]
            x = make_input(T, S, 2 * I, seed + 100, regime).cuda()
            hs_ = [pr.layer(p, I, H, s_hint=S) for p in ps]
            xd = pr.buf(T * 2 * I * S, register=True)
            xd.copy_(dev(x.permute(0, 2, 1)).reshape(-1))
            out_t = 2 * H * S
            out = pr.buf(T * out_t, register=True)
            G, cell = pr.buf(2 * T * 4 * H * S, 0.0), pr.buf(2 * H * S, 0.0)
            pr.check(lib.lsp_run_pair(hs_[0], hs_[1], xd.data_ptr(), xd[I * S:].data_ptr(), 2 * I * S, G.data_ptr(), cell.data_ptr(),
                                      out.data_ptr(), S, out_t, 2, T, S))
            idx, wants, bounds = [], [], []
            for z in range(2):
                w_, b_, _ = reference(x[:, :, z * I:(z + 1) * I], ps[z], False)
                idx.append(out_index(T, S, H, out_t, 2 * S, base=z * S))
                wants.append(w_)
                bounds.append(b_)
            worst = check_owned(out, torch.stack(idx), torch.stack(wants), torch.stack(bounds), 'out')
        elif k in ('stack', 'chunk'):
            L = case['L']
            ps = [layer_params(H, I if l == 0 else H, seed + l, False, regime) for l in range(L)]
            x = make_input(T, S, I, seed + 100, regime).cuda()
            hs_ = [pr.layer(ps[l], I if l == 0 else H, H, s_hint=S) for l in range(L)]
            arr = (C.c_void_p * L)(*hs_)
            xd = pr.buf(I * T * S, register=True)
            xd.copy_(dev(x.permute(2, 0, 1)).reshape(-1))                     # [I][T][S]
            G = pr.buf(4 * H * T * S, 0.0)
            ran = C.c_int(-1)
            wants, bounds, Ex, xin = [], [], None, x
            for l in range(L):
                w_, b_, _ = reference(xin, ps[l], False, Ex=Ex)
                wants.append(w_)
                bounds.append(b_)
                xin, Ex = w_, b_
            if k == 'stack':
                out = pr.buf(H * T, register=True)
                pr.check(lib.lsp_stack_fm(arr, L, xd.data_ptr(), G.data_ptr(), out.data_ptr(), T, C.byref(ran)))
                assert ran.value == 1, 'lstm_stack_fm refused'
                worst = check_owned(out, out_index(T, 1, H, 1, T), wants[-1], bounds[-1], 'out')
            else:
                # outs[l] aliases outs[l - 2], as CRN / LSTM pass them
                nb = min(L, 2)
                obufs = [pr.buf(H * T * S, register=True) for _ in range(nb)]
                outs = (C.c_void_p * L)(*[obufs[l % 2].data_ptr() for l in range(L)])
                cells = pr.buf(L * H * S, 0.0)
                pr.check(lib.lsp_stack_chunked_fm(arr, L, xd.data_ptr(), G.data_ptr(), cells.data_ptr(), outs, T, S, C.byref(ran)))
                if want_forms is None:
                    recs, gc = pr.log()
                    assert ran.value == 0 and not recs, 'lstm_stack_chunked_fm ran where its conditions say it does not apply'
                    return 0.0, [], []
                assert ran.value == 1, 'lstm_stack_chunked_fm refused'
                for l in range(max(0, L - 2), L):                          # the last two layers' outputs survive the aliasing
                    worst = max(worst, check_owned(obufs[l % 2], out_index(T, S, H, S, T * S), wants[l], bounds[l], f'out of layer {l}'))
                recs, gc = pr.log()
                plan = chunk_plan(T, L)
                assert len(recs) == len(plan), (len(recs), len(plan))
                for (_, r), launch in zip(recs, plan):
                    got = [(r[f'lz{z}'], r[f't0{z}'], r[f'Tz{z}']) for z in range(r['Z'])]
                    assert got == launch, f'chunk launch {got} != {launch}'
        elif k == 'persist':            # Z LSTMs x O items; z walks backwards when bit z of `reverse` is set
            Z, O, rev = case['Z'], case['O'], case.get('reverse', 0)
            ps = [layer_params(H, I, seed + z, False, regime) for z in range(Z)]
            x = make_input(O * T, S, I, seed + 100, regime).cuda().reshape(O, T, S, I)
            hs_ = [pr.layer(p, I, H, s_hint=S) for p in ps]
            arr = (C.c_void_p * Z)(*hs_)
            xd = pr.buf(O * T * I * S, register=True)
            xd.copy_(dev(x.permute(0, 1, 3, 2)).reshape(-1))               # [O][T][I][S]
            G = pr.buf(O * Z * T * 4 * H * S, 0.0)
            # out [O][T][Z][H][S]: the layers of one step side by side (DCCRN's two real LSTMs: z stride H S, t stride Z H S)
            out_z, out_t, out_o = H * S, Z * H * S, T * Z * H * S
            out = pr.buf(O * out_o, register=True)
            carry = case.get('carry', False)
            st_h = st_c = None
            h0 = c0_ = None
            if carry:
                g = torch.Generator().manual_seed(seed)
                h0 = (torch.rand((Z, S, H), generator=g, dtype=torch.float64) - 0.5).float().double().cuda()
                c0_ = (torch.rand((Z, S, H), generator=g, dtype=torch.float64) * 2 - 1).float().double().cuda()
                st_h, st_c = pr.buf(Z * H * S), pr.buf(Z * H * S)
                st_h.copy_(dev(h0.permute(0, 2, 1)).reshape(-1))
                st_c.copy_(dev(c0_.permute(0, 2, 1)).reshape(-1))
            pr.check(lib.lsp_persist(arr, Z, xd.data_ptr(), T * I * S, I * S, O, G.data_ptr(), out.data_ptr(), out_o, out_z, out_t, S,
                                     T, S, rev, st_h.data_ptr() if carry else None, st_c.data_ptr() if carry else None))
            idx, wants, bounds = [], [], []
            for o in range(O):
                for z in range(Z):
                    w_, b_, (hT, cT, EhT, EcT) = reference(x[o], ps[z], False, reverse=bool((rev >> z) & 1),
                                                           h0=None if not carry else h0[z], c0=None if not carry else c0_[z])
                    idx.append(out_index(T, S, H, out_t, S, base=o * out_o + z * out_z))
                    wants.append(w_)
                    bounds.append(b_)
                    if carry:
                        worst = max(worst, ratio(st_h[z * H * S:(z + 1) * H * S].reshape(H, S).T, hT, EhT),
                                    ratio(st_c[z * H * S:(z + 1) * H * S].reshape(H, S).T, cT, EcT))
            worst = max(worst, check_owned(out, torch.stack(idx), torch.stack(wants), torch.stack(bounds), 'out'))
        elif k == 'short':              # DPCRN's intra-frame BiLSTM: x (o, c, t, n), out (z, o, u, t, n)
            Z, O, rev = case['Z'], case['O'], case.get('reverse', 0)
            ps = [layer_params(H, I, seed + z, False, regime) for z in range(Z)]
            x = make_input(O * T, S, I, seed + 100, regime).cuda().reshape(O, T, S, I)
            hs_ = [pr.layer(p, I, H, s_hint=S) for p in ps]
            arr = (C.c_void_p * Z)(*hs_)
            xd = pr.buf(O * I * T * S, register=True)
            xd.copy_(dev(x.permute(0, 3, 1, 2)).reshape(-1))               # [O][I][T][S]
            out_t, out_row = S, T * S
            out_o = 2 * H * T * S                                           # (channels of both directions per item, as DPCRN)
            out_z = H * T * S
            out = pr.buf(O * out_o, register=True)
            pr.check(lib.lsp_short(arr, Z, xd.data_ptr(), I * T * S, T * S, S, out.data_ptr(), out_o, out_z, out_t, out_row, T, S, O, rev))
            idx, wants, bounds = [], [], []
            for o in range(O):
                for z in range(Z):
                    w_, b_, _ = reference(x[o], ps[z], False, reverse=bool((rev >> z) & 1))
                    idx.append(out_index(T, S, H, out_t, out_row, base=o * out_o + z * out_z))
                    wants.append(w_)
                    bounds.append(b_)
            worst = check_owned(out, torch.stack(idx), torch.stack(wants), torch.stack(bounds), 'out')
        else:
            raise ValueError(k)
        recs, gc = pr.log()
        return worst, forms_logged(recs, gc, T, fused=(k == 'cols_x')), want_forms
    finally:
        pr.close()


# ------------------------------------------------------------------------------------------------ cases
def C_(kind, H, S, T, **kw):
    return dict(kind=kind, H=H, S=S, T=T, **kw)


CASES = [
    # H = 1024, time-major run_cols: the K-split form by NS, the sub-tile form by LEAD, 16-sequence tiles, sub-tiles again, the
    # flag-barrier form; ragged tiles / sub-tiles; T = 1 ... 5 (tags repeat every 4 steps, slabs every 2), odd T, 401
    C_('cols', 1024, 1, 401), C_('cols', 1024, 1, 1), C_('cols', 1024, 2, 5), C_('cols', 1024, 4, 3), C_('cols', 1024, 5, 2),
    C_('cols', 1024, 16, 4), C_('cols', 1024, 17, 5), C_('cols', 1024, 28, 33), C_('cols', 1024, 29, 3), C_('cols', 1024, 59, 401),
    C_('cols', 1024, 60, 1), C_('cols', 1024, 61, 7), C_('cols', 1024, 1472, 9), C_('cols', 1024, 1473, 5), C_('cols', 1024, 1536, 2),
    C_('cols', 1024, 1537, 3), C_('cols', 1024, 4096, 3),
    C_('cols', 1024, 17, 4, out_rs=2), C_('cols', 1024, 100, 2, out_rs=2),
    # H = 512: K-split (tagged) up to 4, the flag-barrier form at 5 - 16, 16-sequence tiles from 17
    C_('cols', 512, 1, 5), C_('cols', 512, 4, 401), C_('cols', 512, 5, 4), C_('cols', 512, 16, 33), C_('cols', 512, 17, 2),
    C_('cols', 512, 333, 5), C_('cols', 512, 4096, 2),
    # H = 256: DCCRN's opt-in 16-sequence tiles from 17 sequences, the per-step GEMM below and without the opt-in
    C_('cols', 256, 16, 5, coop256=True), C_('cols', 256, 17, 401, coop256=True), C_('cols', 256, 4096, 3, coop256=True),
    C_('cols', 256, 40, 7),
    # feature-major (gx_row = T S): the same kernels on the other strides, and the 32-bit-offset refusal either side of T S 16 KB = 4 GB
    C_('fm', 1024, 1, 3), C_('fm', 1024, 17, 48), C_('fm', 1024, 64, 5), C_('fm', 512, 100, 33),
    C_('fm', 1024, 992, 246), C_('fm', 1024, 992, 247),
    # GCRN's pair (Z = 2, out_rs = 2)
    C_('pair', 512, 1, 5), C_('pair', 512, 3, 4), C_('pair', 512, 4, 1), C_('pair', 512, 5, 3), C_('pair', 512, 16, 401),
    C_('pair', 512, 17, 2), C_('pair', 512, 100, 33),
    # one sequence, a whole stack (T < L: the layer lag is longer than the utterance)
    C_('stack', 1024, 1, 1, L=2), C_('stack', 1024, 1, 2, L=2), C_('stack', 1024, 1, 401, L=2), C_('stack', 1024, 1, 2, L=3),
    C_('stack', 1024, 1, 97, L=3), C_('stack', 512, 1, 5, L=2), C_('stack', 512, 1, 33, L=3),
    # the chunk pipeline: T = 96 (the minimum) ... 145 end on chunks of every parity; state carried across launches
    C_('chunk', 1024, 17, 96, L=2), C_('chunk', 1024, 64, 97, L=3), C_('chunk', 1024, 33, 143, L=4), C_('chunk', 512, 128, 144, L=2),
    C_('chunk', 512, 100, 145, L=3), C_('chunk', 512, 17, 97, L=4),
    C_('chunk', 1024, 17, 95, L=2), C_('chunk', 1024, 65, 96, L=2), C_('chunk', 512, 129, 96, L=2),
    # the per-step EPI_LSTM GEMM: column ranges, streaming with carried state, the fused input projection, the GRU cell
    C_('cols', 1024, 40, 5, c0=8, Sn=20), C_('cols', 512, 37, 6, c0=5, Sn=31), C_('cols', 384, 50, 9, c0=7, Sn=33, I=256),
    C_('stream', 1024, 3, 9, T1=4), C_('stream', 256, 18, 7, T1=5), C_('stream', 384, 5, 6, T1=1, I=96),
    C_('cols_x', 384, 50, 7, c0=10, Sn=33, I=32), C_('cols_x', 384, 19, 5, I=384),
    C_('cols', 384, 20, 7, gru=True, I=64), C_('cols', 128, 33, 5, gru=True, I=128, c0=3, Sn=17),
    C_('stream', 384, 21, 6, T1=2, gru=True, I=64),
    # the persistent kernels: 4-sequence tiles, 16-sequence tiles past 128 tiles, H = 64, reverse bits, carried state
    C_('persist', 128, 20, 33, Z=2, O=1, I=128), C_('persist', 128, 7, 5, Z=1, O=3, I=64, reverse=1),
    C_('persist', 128, 1040, 4, Z=2, O=1, I=128, reverse=2), C_('persist', 64, 35, 4, Z=2, O=3, I=128, reverse=2),
    C_('persist', 128, 40, 6, Z=2, O=1, I=128, carry=True), C_('persist', 64, 17, 401, Z=1, O=1, I=64),
    # the short-sequence kernel (H = 64, I = 128, T <= 16): one tile per workgroup and many, both directions
    C_('short', 64, 20, 4, Z=2, O=3, I=128, reverse=2), C_('short', 64, 100, 4, Z=2, O=60, I=128, reverse=2),
    C_('short', 64, 33, 16, Z=1, O=2, I=128), C_('short', 64, 16, 1, Z=2, O=1, I=128, reverse=1),
    # saturating gates and large cells at the fast-math activations' ends, one case per family
    C_('cols', 1024, 1, 33, regime='saturating'), C_('cols', 1024, 17, 33, regime='saturating'),
    C_('cols', 1024, 60, 33, regime='saturating'), C_('cols', 1024, 1537, 5, regime='saturating'),
    C_('cols', 512, 9, 33, regime='saturating'), C_('pair', 512, 5, 401, regime='saturating'),
    C_('cols', 256, 17, 33, coop256=True, regime='saturating'), C_('stack', 1024, 1, 33, L=2, regime='saturating'),
    C_('chunk', 1024, 17, 97, L=2, regime='saturating'), C_('cols', 1024, 40, 9, c0=8, Sn=20, regime='saturating'),
    C_('persist', 128, 20, 33, Z=2, O=1, I=128, regime='saturating'), C_('short', 64, 20, 4, Z=2, O=3, I=128, reverse=2, regime='saturating'),
]
# forms that only a tuning switch selects: one child process per switch
SWITCH_CASES = {
    'SE_COOP16': [C_('cols', 512, 17, 5), C_('cols', 512, 100, 4), C_('cols', 512, 200, 3), C_('cols', 512, 3073, 2),
                  C_('cols', 1024, 92, 3), C_('cols', 1024, 93, 5), C_('cols', 1024, 1473, 2), C_('cols', 256, 17, 3, coop256=True),
                  C_('pair', 512, 17, 3)],
    'SE_COOP4': [C_('cols', 1024, 17, 5), C_('cols', 1024, 59, 3), C_('cols', 1024, 1473, 2)],
}


def case_id(c):
    extra = ','.join(f'{k}={v}' for k, v in c.items() if k not in ('kind', 'H', 'S', 'T'))
    return f"{c['kind']}-H{c['H']}-S{c['S']}-T{c['T']}" + (f'-{extra}' if extra else '')


def reached_key(form, case):
    return form + (' saturating' if case.get('regime') == 'saturating' else '')


REACHED = {}        # form -> the (kind, S, T) that reached it (test_every_form_is_reached)
RATIOS = {}         # form -> worst error / bound over its cases


def record(case, got, worst):
    for f in sorted(set(got)):
        REACHED.setdefault(reached_key(f, case), (case['kind'], case['S'], case['T']))
        RATIOS[f] = max(RATIOS.get(f, 0.0), worst)


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_layer_matches_float64(case):
    worst, got, want = run_case(case)
    print(f'{case_id(case)}: forms {sorted(set(got))}, worst error / bound {worst:.3g}')
    assert got == want, f'forms {got} != expected {want}'
    assert worst < 1.0, f'error exceeds the bound: {worst:.3g} of it'
    record(case, got, worst)


@pytest.mark.gpu
@pytest.mark.parametrize('switch', sorted(SWITCH_CASES))
def test_switch_only_forms(switch):
    """The forms only SE_COOP16=0 / SE_COOP4=0 reach (kept for measurements), all cases of one switch in one child."""
    env = dict(os.environ, **{switch: '0'})
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', switch], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    res = [json.loads(l[len('CASE '):]) for l in r.stdout.splitlines() if l.startswith('CASE ')]
    assert len(res) == len(SWITCH_CASES[switch]), r.stdout[-4000:] + r.stderr[-4000:]
    bad = []
    for case, (worst, got, want) in zip(SWITCH_CASES[switch], res):
        print(f'{switch}=0 {case_id(case)}: forms {sorted(set(got))}, worst error / bound {worst:.3g}')
        if got != want or not worst < 1.0:
            bad.append((case_id(case), got, want, worst))
        else:
            record(case, got, worst)
    assert not bad, bad


# every form of the launchers' tables (a CU count other than 256 moves some boundaries: expected_forms follows it, and the targets
# that no case reaches on such a device are listed by the test)
TARGETS = ['ks<1024,1,1>', 'ks<1024,4,1>', 'ks<1024,16,0>', 'coop8<1024,1,4>', 'coop8<1024,2,4>', 'coop8<1024,3,4>', 'coop16<1024>',
           'coop<1024>', 'ks<512,1,1>', 'ks<512,4,1>', 'coop<512>', 'coop16<512>', 'coop8<512,1,4>', 'coop8<512,2,4>', 'coop8<512,3,4>',
           'coop16<256>', 'chunk coop16<1024>', 'chunk coop16<512>', 'stack<1024,2>', 'stack<1024,3>', 'stack<512,2>', 'stack<512,3>',
           'persist4<128>', 'persist<128>', 'persist<64>', 'short', 'step', 'step gru', 'step_x']


@pytest.mark.gpu
def test_every_form_is_reached():
    """Runs last in this file: the cases above together reach every form (a moved threshold must not quietly turn them into cases
    of some other form), and the worst error / bound of each."""
    for f in TARGETS:
        print(f'{f:22s} first reached by {REACHED.get(f)}  worst error / bound {RATIOS.get(f, float("nan")):.3g}')
    missing = [t for t in TARGETS if t not in REACHED]
    assert not missing, f'not reached: {missing}; reached: {sorted(REACHED)}'
    assert max(RATIOS.values()) > 1e-3, f'no case comes within 1e-3 of the bound: {RATIOS}'


# ------------------------------------------------------------------------------------------------ CPU: the reference and its bound
def test_selection_mirror_matches_the_launchers_table():
    """expected_coop at 256 CUs gives the table the launchers were written to (k_lstm_coop.hip launch_lstm_coop)."""
    tm = lambda H, S, Z=1, **kw: expected_coop(H, S, Z, 256, S, S, **kw)
    assert [tm(1024, s) for s in (1, 2, 4, 5, 16)] == ['ks<1024,1,1>', 'ks<1024,4,1>', 'ks<1024,4,1>', 'ks<1024,16,0>', 'ks<1024,16,0>']
    assert [tm(1024, s) for s in (17, 28, 29, 59)] == ['coop8<1024,1,4>'] * 2 + ['coop8<1024,2,4>'] * 2
    assert [tm(1024, s) for s in (60, 1472)] == ['coop16<1024>'] * 2
    assert [tm(1024, s) for s in (1473, 1536)] == ['coop8<1024,3,4>'] * 2
    assert [tm(1024, s) for s in (1537, 4096)] == ['coop<1024>'] * 2
    assert expected_coop(1024, 992, 1, 256, 992 * 246, 992 * 246) == 'coop16<1024>'
    assert expected_coop(1024, 992, 1, 256, 992 * 247, 992 * 247) == 'coop<1024>'
    for Z in (1, 2):
        assert [tm(512, s, Z) for s in (1, 4, 5, 16, 17, 4096)] == ['ks<512,1,1>', 'ks<512,4,1>', 'coop<512>', 'coop<512>',
                                                                    'coop16<512>', 'coop16<512>']
    assert [tm(512, s, coop16=False) for s in (17, 100, 200, 3073)] == ['coop8<512,1,4>', 'coop8<512,2,4>', 'coop8<512,3,4>',
                                                                        'coop<512>']
    assert [tm(1024, s, coop4=False) for s in (17, 1473)] == ['coop16<1024>', 'coop<1024>']
    assert [coop256_supported(s, 256) for s in (16, 17, 4096, 4097)] == [False, True, True, False]
    assert [chunk_supported(1024, s, 2, 96, 256) for s in (16, 17, 64, 65)] == [False, True, True, False]
    assert [chunk_supported(512, s, 2, 96, 256) for s in (17, 128, 129)] == [True, True, False]
    assert [chunk_supported(1024, 17, 2, t, 256) for t in (95, 96)] == [False, True]
    assert chunk_plan(97, 2) == [[(0, 0, 48)], [(0, 48, 48), (1, 0, 48)], [(0, 96, 1), (1, 48, 48)], [(1, 96, 1)]]


def test_reference_matches_torch_and_the_oracle_in_float64():
    """The float64 reference the GPU cases rest on, against torch.nn.LSTM / torch.nn.GRU (float64; initial state, reverse via flip)
    and oracle/nnops.lstm_layer / gru_layer."""
    sys.path.insert(0, ROOT)
    from oracle import nnops
    T, S, I, H = 7, 3, 5, 6
    for gru in (False, True):
        p = layer_params(H, I, 5, gru)
        x = make_input(T, S, I, 6)
        m = (torch.nn.GRU if gru else torch.nn.LSTM)(I, H).double()
        with torch.no_grad():
            m.weight_ih_l0.copy_(p['wih'])
            m.weight_hh_l0.copy_(p['whh'])
            m.bias_ih_l0.copy_(p['bih'])
            m.bias_hh_l0.copy_(p['bhh'])
            want, _ = m(x)
            got, bound, (hT, cT, _, _) = reference(x, p, gru)
            assert torch.allclose(got, want, rtol=0, atol=1e-13)
            assert bool((bound > 0).all()) and torch.equal(hT, got[-1])
            fn = nnops.gru_layer if gru else nnops.lstm_layer
            ora = fn(x.numpy(), *(p[n].numpy() for n in ('wih', 'whh', 'bih', 'bhh')))
            assert np.allclose(got.numpy(), ora, rtol=0, atol=1e-13)
            h0 = torch.randn(1, S, H, dtype=torch.float64)
            if gru:
                want, hN = m(x, h0)
                got, _, (hT, _, _, _) = reference(x, p, True, h0=h0[0])
            else:
                c0 = torch.randn(1, S, H, dtype=torch.float64)
                want, (hN, cN) = m(x, (h0, c0))
                got, _, (hT, cT, _, _) = reference(x, p, False, h0=h0[0], c0=c0[0])
                assert torch.allclose(cT, cN[0], rtol=0, atol=1e-13)
            assert torch.allclose(got, want, rtol=0, atol=1e-13) and torch.allclose(hT, hN[0], rtol=0, atol=1e-13)
            if not gru:
                want, _ = m(x.flip(0))
                got, _, _ = reference(x, p, False, reverse=True)
                assert torch.allclose(got, want.flip(0), rtol=0, atol=1e-13)
                ora = nnops.lstm_layer(x.numpy(), *(p[n].numpy() for n in ('wih', 'whh', 'bih', 'bhh')), reverse=True)
                assert np.allclose(got.numpy(), ora, rtol=0, atol=1e-13)


@pytest.mark.parametrize('fault', ['stale_h', 'c_reset', 'gate_swap', 'neighbour'])
def test_bound_catches_plausible_faults(fault):
    """The bound has teeth: at a shape of the GPU cases (H = 1024, S = 17: a ragged 16-sequence tile and a ragged 4-sequence
    sub-tile; T = 97: a chunk boundary at step 48), each fault a recurrent kernel could plausibly have moves some stored h_t by at
    least 10x the bound of the correct computation:
      stale_h    one sequence reads h_{t-2} instead of h_{t-1} at one step (an exchange slab of the wrong parity)
      c_reset    the cell state restarts from zero at a chunk boundary (state not carried across launches)
      gate_swap  two gates of one unit trade places (a wrong gate interleave)
      neighbour  the last sequence of a ragged tile is stored from its neighbour's lane"""
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    H, S, T = 1024, 17, 97
    p = layer_params(H, H, 11)
    x = make_input(T, S, H, 12)
    f = {'stale_h': dict(kind='stale_h', step=5, seq=16), 'c_reset': dict(kind='c_reset', step=CHUNK_T),
         'gate_swap': dict(kind='gate_swap', gates=(0, 1), u=517), 'neighbour': dict(kind='neighbour', seq=16)}[fault]
    good, bound, _ = reference(x, p)
    bad, _, _ = reference(x, p, fault=f)
    r = ratio(bad, good, bound)
    assert r >= 10.0, f'{fault}: the fault moves h by only {r:.3g}x the bound'
    # ... and the bound is not so loose that it is never approached: a correct fp32 evaluation of the same recurrence is within it
    p32 = {n: v.float() for n, v in p.items()}
    h = torch.zeros((S, H))
    c = torch.zeros((S, H))
    out = torch.empty((T, S, H))
    for t in range(T):
        a = x[t].float() @ p32['wih'].T + p32['bih'] + p32['bhh'] + h @ p32['whh'].T
        i, fg, g, o = a[:, :H].sigmoid(), a[:, H:2 * H].sigmoid(), a[:, 2 * H:3 * H].tanh(), a[:, 3 * H:].sigmoid()
        c = fg * c + i * g
        h = o * c.tanh()
        out[t] = h
    r32 = ratio(out, good, bound)
    assert 1e-3 < r32 < 1.0, r32


# ------------------------------------------------------------------------------------------------ child (test_switch_only_forms)
if __name__ == '__main__' and len(sys.argv) > 2 and sys.argv[1] == '--child':
    sw = sys.argv[2]
    for case in SWITCH_CASES[sw]:
        worst, got, want = run_case(case, coop16=(sw != 'SE_COOP16'), coop4=(sw != 'SE_COOP4'))
        print('CASE ' + json.dumps([worst, got, want]), flush=True)
