"""One conv launch at a time against float64: the tap-table conv (csrc/gemmconv.hip) picks among a dozen tile geometries by batch
size, frequency rows, frame count and launch-size thresholds, and each can carry on-the-fly InstanceNorm (NRM), the statistics
rider and ragged rows.  The whole-model suites reach most geometries at one or two (B, T) points; here every case is a single
layer of the engine's own shapes, built and launched as the engine does it (csrc/tests/gc_probe.hip -> libse_gcprobe.so), checked
element by element against a float64 reference, and checked for the geometry it was meant to reach."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'sixty-years-of-frequency-domain-monaural-speech-enhancement_amd')
PROBE_LIB = os.environ.get('SE_GCPROBE_LIB') or os.path.join(PKG, 'libse_gcprobe.so')      # (as SE_ENGINE_LIB: A/B another build)

ACT_NONE, ACT_PRELU = 0, 1
EPI_ACT = 0
FAM_TILE, FAM_THIN, FAM_THIN_PAIR, FAM_DIRECT, FAM_DIRECT_LDS = 0, 1, 2, 3, 4
# gc_launch's thresholds at the time of writing (gemmconv.hip: SE_GC_ALT_N64, SE_GC_QT2_MIN, SE_GC_WIDE_MIN, SE_GC_WIDE_FILL) - the
# cases below are placed just below and just above them, and assert the geometry each side selects
ALT_N64, QT2_MIN, WIDE_MIN, WIDE_FILL = 4096, 4096, 6144, 75
T_SWEEP = (1, 2, 3, 4, 5, 31, 32, 33, 64, 65, 96, 97, 101, 128, 129, 150, 160, 161, 192, 257, 401)
U24 = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ float64 reference
def normalise(x, nrm):
    """The consumer-side InstanceNorm + PReLU of gc_kernel NRM: y = x * scale + shift; y += (slope - 1) * min(y, 0).
    x [B][C][F][T], nrm [B][C][4] = {scale, shift, slope - 1, x0}.  Also returns the magnitude its fp32 form is exact to."""
    if nrm is None:
        return x, x.abs()
    s, h, sm1 = (nrm[:, :, i, None, None] for i in range(3))
    y = x * s + h
    y = y + sm1 * torch.clamp(y, max=0.0)
    return y, x.abs() * s.abs() + h.abs() + y.abs()


def conv_f64(x, w, sf, pf, pt_left, dil_f=1, dil_t=1, Fout=None):
    """out[b][m][f][t] = sum w[m][c][kf][kt] x[b][c][f sf - pf + kf dil_f][t - pt_left + kt dil_t], zero outside the plane - the
    convention of layers.h make_conv_plan, as oracle/nnops.conv2d computes it (one contraction per tap over a zero-padded input)."""
    B, Cin, Fin, T = x.shape
    M, _, nkf, nkt = w.shape
    if Fout is None:
        Fout = (Fin + 2 * pf - dil_f * (nkf - 1) - 1) // sf + 1
    padr_f = max(0, (Fout - 1) * sf - pf + (nkf - 1) * dil_f - Fin + 1)
    padr_t = max(0, (nkt - 1) * dil_t - pt_left)
    xp = torch.nn.functional.pad(x, (pt_left, padr_t, pf, padr_f))
    out = torch.zeros((B, M, Fout, T), dtype=torch.float64, device=x.device)
    for kf in range(nkf):
        for kt in range(nkt):
            patch = xp[:, :, kf * dil_f: kf * dil_f + (Fout - 1) * sf + 1: sf, kt * dil_t: kt * dil_t + T]
            out += torch.einsum('oc,bcft->boft', w[:, :, kf, kt], patch)
    return out


def deconv_f64(x, w, sf, pf, toff, Fout):
    """out[b][m][fo][to] = sum_{(fo + pf - kf) % sf == 0} w[m][c][kf][kt] x[b][c][(fo + pf - kf) / sf][to + toff - kt] - the
    convention of layers.h make_deconv_plan, i.e. oracle/nnops.conv_transpose2d (frequency stride sf, padding pf) cropped."""
    assert pf >= 0 and toff >= 0
    B, Cin, Fin, T = x.shape
    M, _, nkf, nkt = w.shape
    Ff, Tf = (Fin - 1) * sf + nkf, T + nkt - 1
    full = torch.zeros((B, M, max(Ff, pf + Fout), max(Tf, toff + T)), dtype=torch.float64, device=x.device)
    for kf in range(nkf):
        for kt in range(nkt):
            full[:, :, kf: kf + (Fin - 1) * sf + 1: sf, kt: kt + T] += torch.einsum('oc,bcft->boft', w[:, :, kf, kt], x)
    return full[:, :, pf: pf + Fout, toff: toff + T]


def reference(sh, xs, nrms, w, bias, slope, T, Fout, tlen=None):
    """float64 output of one layer and the per-output error bound c * 2^-24 * K * (sum |w| |x| + |bias|) of its fp32 form."""
    ys, mags = zip(*(normalise(x, n) for x, n in zip(xs, nrms)))
    x = torch.cat(ys, dim=1)
    mag = torch.cat(mags, dim=1)
    if sh['kind'] == 'conv':
        f = lambda a, ww: conv_f64(a, ww, sh['sf'], sh['pf'], sh['pt'], Fout=Fout)
    else:
        f = lambda a, ww: deconv_f64(a, ww, sh['sf'], sh['pf'], sh['toff'], Fout)
    y = f(x, w) + bias[None, :, None, None]
    bound = f(mag, w.abs()) + bias.abs()[None, :, None, None]
    if slope is not None:
        s = slope[None, :, None, None]
        y = torch.where(y >= 0, y, s * y)
    if tlen is not None:
        t = torch.arange(T, device=y.device)
        y = y * (t[None, :] < tlen[:, None]).to(y.dtype)[:, None, None, :]
    K = w.shape[1] * w.shape[2] * w.shape[3]
    return y, 4.0 * U24 * K * bound


# ------------------------------------------------------------------------------------------------ the probe
class Probe:
    FACTS = ('BM', 'BN', 'nplans', 'nrm_ok', 'stats_ok', 'flat_uw', 'direct', 'flat128', 'flat256', 'wide', 'qt2', 'alt64',
             'tail32', 'cic', 'nrows', 'wide_wp', 'tail_split', 'po', 'so')
    REC = ('family', 'BM', 'BN', 'flat_upr', 'upt', 'flat_rows', 'qt2', 'nrm', 'res', 'trim', 'stats', 'ragged', 'flat_nrm_refused',
           'nblk')
    _lib = None

    @classmethod
    def lib(cls):
        if cls._lib is None:
            assert os.path.exists(PROBE_LIB), f'{PROBE_LIB} is not built (make -C {PKG}/csrc)'
            lib = C.CDLL(PROBE_LIB)      # (after torch: one HIP runtime per process, see se_amd/_lib.py)
            vp, i32, fp = C.c_void_p, C.c_int, C.POINTER(C.c_float)
            lib.gcp_last_error.restype = C.c_char_p
            lib.gcp_conv_create.restype = vp
            lib.gcp_conv_create.argtypes = [fp, fp, fp] + [i32] * 12
            lib.gcp_deconv_create.restype = vp
            lib.gcp_deconv_create.argtypes = [fp, fp, fp] + [i32] * 10
            lib.gcp_destroy.argtypes = [vp]
            lib.gcp_info.argtypes = [vp, i32, C.POINTER(i32), i32]
            lib.gcp_run.argtypes = [vp, vp, vp, vp, vp, i32, vp, i32, i32, i32, i32, i32, vp, vp]
            lib.gcp_launch_get.argtypes = [i32, C.POINTER(C.c_longlong), i32]
            lib.gcp_flat_rows_spanned.argtypes = [i32, i32, i32]
            lib.gcp_register_overread.argtypes = [vp, C.c_size_t]
            lib.gcp_unregister_overread.argtypes = [vp]
            cls._lib = lib
        return cls._lib

    def __init__(self, sh, w, bias, slope):
        lib = self.lib()
        self.sh = sh
        f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
        self._keep = [f32(w), f32(bias), f32(slope)]
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
        wp, bp, sp = (ptr(a) for a in self._keep)
        M, Cin, nkf, nkt = w.shape
        act = ACT_PRELU if slope is not None else ACT_NONE
        if sh['kind'] == 'conv':
            self.h = lib.gcp_conv_create(wp, bp, sp, M, Cin, nkf, nkt, sh['sf'], sh['pf'], sh['pt'], 1, 1, act, EPI_ACT, sh['c0'])
        else:
            self.h = lib.gcp_deconv_create(wp, bp, sp, M, Cin, nkf, nkt, sh['sf'], sh['pf'], sh['toff'], act, EPI_ACT, sh['c0'])
        assert self.h, lib.gcp_last_error().decode()
        self.plans = [self.info(0)]
        for c in range(1, self.plans[0]['nplans']):
            self.plans.append(self.info(c))

    def info(self, cls):
        out = (C.c_int * len(self.FACTS))()
        assert self.lib().gcp_info(self.h, cls, out, len(self.FACTS)) == len(self.FACTS)
        return dict(zip(self.FACTS, out))

    def close(self):
        if self.h:
            self.lib().gcp_destroy(self.h)
            self.h = None

    def run(self, xs, nrms, dst, Fin, Fout, B, T, Tp, stats=None, tlen=None):
        p = lambda t: None if t is None else t.data_ptr()
        x1 = xs[1] if len(xs) > 1 else None
        n1 = nrms[1] if len(nrms) > 1 else None
        torch.cuda.synchronize()
        rc = self.lib().gcp_run(self.h, p(xs[0]), p(nrms[0]), p(x1), p(n1), Fin, p(dst), dst.shape[1], Fout, B, T, Tp, p(stats), p(tlen))
        assert rc == 0, self.lib().gcp_last_error().decode()
        recs = []
        for i in range(self.lib().gcp_launch_count()):
            out = (C.c_longlong * len(self.REC))()
            self.lib().gcp_launch_get(i, out, len(self.REC))
            recs.append(dict(zip(self.REC, out)))
        return recs


def rows_spanned(B, upr, upt):
    """Most batch rows one flattened tile of `upt` 32-frame units touches (B rows of `upr` units end to end)."""
    units = B * upr
    most = 0
    for k in range(min((units + upt - 1) // upt, upr)):
        u0 = k * upt
        u1 = min(u0 + upt, units) - 1
        most = max(most, u1 // upr - u0 // upr + 1)
    return most


# ------------------------------------------------------------------------------------------------ layer shapes of the engine
# w [M][Cin][nkf][nkt]; conv: out[f][t] = sum w x[f sf - pf + kf][t - pt + kt]; deconv: make_deconv_plan(sf, pf, toff)
SHAPES = {
    # a G2Net U^2-Net level: 64 -> 64, (1, 3) taps (no extent in time), frequency stride 2, sources normalised on the fly
    'g2net_level': dict(kind='conv', M=64, Cin=64, nkf=3, nkt=1, sf=2, pf=0, pt=0, c0=-1, Fin=79, Fout=39, nrm=True),
    # its decoder: the two-source ('cat') transposed conv, 64 + 64 = GC_NRM_MAXC input channels, two parity classes
    'g2net_deconv': dict(kind='deconv', M=64, Cin=128, nkf=3, nkt=1, sf=2, pf=0, toff=0, c0=64, Fin=39, Fout=79, nrm=True),
    # TaylorSENet's (2, 3) level (SE_IN_FOLD=2 normalises its sources on the fly): one frame of look-back
    'taylor_level': dict(kind='conv', M=64, Cin=64, nkf=3, nkt=2, sf=2, pf=0, pt=1, c0=-1, Fin=79, Fout=39, nrm=True),
    # a strided complex encoder conv of DCCRN in its real block form (5 x 2 taps, stride 2, 128-row tiles)
    'dccrn_enc': dict(kind='conv', M=128, Cin=64, nkf=5, nkt=2, sf=2, pf=2, pt=1, c0=-1, Fin=64, Fout=32, nrm=False),
    # a pointwise 64 -> 256 layer (the TCM blocks' input projection) on 64-row tiles
    'pw_1x1': dict(kind='conv', M=256, Cin=64, nkf=1, nkt=1, sf=1, pf=0, pt=0, c0=-1, Fin=4, Fout=4, nrm=False),
    # a layer back to two channels (the direct path; its LDS-tiled form from 1 024 eight-row workgroups on)
    'direct_2ch': dict(kind='conv', M=2, Cin=32, nkf=3, nkt=2, sf=1, pf=1, pt=1, c0=-1, Fin=64, Fout=64, nrm=False),
}


def plan_q(pl, sh):
    """Output rows of one launch of plan `pl` (layers.hip run_conv / run_deconv)."""
    if sh['kind'] == 'conv':
        return sh['Fout']
    return (sh['Fout'] - pl['po'] + pl['so'] - 1) // pl['so']


def expected(pl, sh, B, T, nrm, stats):
    """The geometry gc_launch selects for one launch of plan `pl` at these thresholds (None: not asserted - thin / resident forms
    of tiny launches), as a dict of record fields."""
    if pl['direct']:
        return None
    Q = plan_q(pl, sh)
    nt = -(-T // pl['BN'])
    nm = -(-sh['M'] // pl['BM'])
    nblk = B * Q * nt * nm
    if T <= 8:
        return None
    if pl['alt64'] == 64 and nblk < (ALT_N64 if pl['BM'] == 64 else 256):
        return None if pl['BM'] == 128 else dict(BM=64, BN=64, flat_upr=0)
    if pl['BM'] == 64 and pl['flat_uw'] and B > 1:
        wide = pl['flat256'] == 256 and nblk >= WIDE_MIN
        upt = 8 if wide else 4
        upr = -(-T // 32)
        tiles_plain = B * -(-T // (32 * upt))
        tiles_flat = -(-(B * upr) // upt)
        if (pl['flat256'] if wide else pl['flat128']) and tiles_flat * 100 <= tiles_plain * 94:
            span = rows_spanned(B, upr, upt)
            if not nrm or span <= 2:
                return dict(BM=64, BN=32 * upt, flat_upr=upr, upt=upt, nrm=int(nrm))
            refused = span
        else:
            refused = 0
    else:
        refused = 0
    nt2 = -(-T // 256)
    if pl['wide'] == 256 and pl['BM'] == 64 and nblk >= WIDE_MIN and T * 100 >= nt2 * 256 * WIDE_FILL and \
            pl['cic'] * pl['nrows'] * pl['wide_wp'] <= 4608:
        return dict(BM=64, BN=256, flat_upr=0, qt2=0, flat_nrm_refused=refused)
    if pl['qt2'] == 64 and pl['BN'] == 128 and Q >= 2 and not stats and not nrm and nblk >= QT2_MIN:
        return dict(BM=pl['BM'], BN=128, qt2=1, flat_upr=0)
    return dict(BM=pl['BM'], BN=pl['BN'], flat_upr=0, qt2=0, flat_nrm_refused=refused)


def b_points(pl, sh, T):
    """Batch sizes just below and just above each workgroup threshold of plan `pl` at T frames."""
    Q = plan_q(pl, sh)
    per_b = Q * -(-T // pl['BN']) * -(-sh['M'] // pl['BM'])
    thr = (256, QT2_MIN) if pl['BM'] == 128 else (ALT_N64, WIDE_MIN)
    if pl['direct']:
        per_b = -(-T // 256) * -(-Q // 8)
        thr = (1024,)
    pts = set()
    for t in thr:
        pts.add(max(1, (t - 1) // per_b))
        pts.add(-(-t // per_b))
    return sorted(pts)


# ------------------------------------------------------------------------------------------------ one case
def make_layer(sh, seed, prelu):
    g = np.random.default_rng(seed)
    w = g.standard_normal((sh['M'], sh['Cin'], sh['nkf'], sh['nkt'])) / math.sqrt(sh['Cin'] * sh['nkf'] * sh['nkt'])
    bias = 0.1 * g.standard_normal(sh['M'])
    slope = g.uniform(0.05, 0.4, sh['M']) if prelu else None
    return w.astype(np.float32), bias.astype(np.float32), None if slope is None else slope.astype(np.float32)


def make_nrm(B, Cn, gen, dev):
    scale = torch.rand((B, Cn), generator=gen, device=dev) * 1.5 + 0.5
    shift = torch.randn((B, Cn), generator=gen, device=dev)
    sm1 = torch.rand((B, Cn), generator=gen, device=dev) * 0.3 - 1.0        # PReLU slopes 0 .. 0.3
    return torch.stack([scale, shift, sm1, -shift / scale], dim=-1).contiguous()


def run_case(probe, sh, w, bias, slope, B, T, *, nrm=False, stats=False, tlen=None, Tp=None, seed=0):
    """Launch the layer once on random sources and compare every stored value (and statistic) with float64.  Returns the
    geometry records of the launch."""
    dev = 'cuda'
    gen = torch.Generator(device=dev)
    gen.manual_seed(1000 + seed)
    Tp = Tp or T
    Fin, Fout, M = sh['Fin'], sh['Fout'], sh['M']
    C0 = sh['Cin'] if sh['c0'] < 0 else sh['c0']
    chans = [C0] + ([sh['Cin'] - C0] if C0 < sh['Cin'] else [])
    slack = 4096
    xs, bufs = [], []
    for Cn in chans:
        n = B * Cn * Fin * Tp
        buf = torch.randn(n + slack, generator=gen, device=dev)
        x = buf[:n].view(B, Cn, Fin, Tp)
        if Tp > T:
            x[..., T:] = 1.0e3      # frames of the row pitch behind the row: must never reach a stored value
        probe.lib().gcp_register_overread(buf.data_ptr(), buf.numel() * 4)
        xs.append(x)
        bufs.append(buf)
    nrms = [make_nrm(B, Cn, gen, dev) if nrm else None for Cn in chans]      # (two sources: parameters drawn apart)
    dst = torch.full((B, M, Fout, Tp), float('nan'), device=dev)
    ns = -(-T // 32)
    st = torch.zeros((B, M, Fout, ns, 2), device=dev) if stats else None
    tl = None if tlen is None else torch.as_tensor(tlen, dtype=torch.int32, device=dev)
    try:
        recs = probe.run(xs, nrms, dst, Fin, Fout, B, T, Tp, st, tl)
    finally:
        for buf in bufs:
            probe.lib().gcp_unregister_overread(buf.data_ptr())
    w64 = torch.from_numpy(w).double().to(dev)
    b64 = torch.from_numpy(bias).double().to(dev)
    s64 = None if slope is None else torch.from_numpy(slope).double().to(dev)
    xs64 = [x[..., :T].double() for x in xs]
    nr64 = [None if n is None else n.double() for n in nrms]
    ref, bound = reference(sh, xs64, nr64, w64, b64, s64, T, Fout, None if tl is None else tl.long())
    y = dst[..., :T].double()
    err = (y - ref).abs()
    bad = ~(err <= bound)                # (NaN: a value that was never stored)
    what = f'{sh} B={B} T={T} nrm={nrm} stats={stats} ragged={tlen is not None} geometry={recs}'
    if bad.any():
        idx = bad.nonzero()[:5].tolist()
        raise AssertionError(f'{int(bad.sum())} of {bad.numel()} outputs out of bound, first at [b, m, f, t] {idx} '
                             f'(err {err[bad].max().item():.3e}); rows hit {sorted(set(bad.nonzero()[:, 0].tolist()))[:16]}; {what}')
    if stats:
        pad = ns * 32 - T
        yr = torch.nn.functional.pad(ref, (0, pad)).view(B, M, Fout, ns, 32)
        br = torch.nn.functional.pad(bound, (0, pad)).view(B, M, Fout, ns, 32)
        s_ref, q_ref = yr.sum(-1), (yr * yr).sum(-1)
        s_tol = (br + 4 * U24 * 32 * yr.abs()).sum(-1)
        q_tol = (2 * yr.abs() * br + br * br + 4 * U24 * 32 * yr * yr).sum(-1)
        ds = (st[..., 0].double() - s_ref).abs()
        dq = (st[..., 1].double() - q_ref).abs()
        assert bool((ds <= s_tol).all()), f'statistics rider (sums) off by up to {ds.max().item():.3e}; {what}'
        assert bool((dq <= q_tol).all()), f'statistics rider (sums of squares) off by up to {dq.max().item():.3e}; {what}'
    return recs


def check_geometry(probe, sh, recs, B, T, nrm, stats):
    tiles = [r for r in recs if r['family'] == FAM_TILE]
    for pl in probe.plans:
        exp = expected(pl, sh, B, T, nrm, stats)
        if exp is None:
            continue
        hit = [r for r in tiles if all(r.get(k) == v for k, v in exp.items())]
        assert hit, f'{sh} B={B} T={T} nrm={nrm} stats={stats}: expected a launch with {exp}, got {recs}'


# ------------------------------------------------------------------------------------------------ tests
REACHED = {}        # coverage target -> the case that reached it (test_every_targeted_geometry_is_reached)


def note(recs, B, T, ragged=False, two_src_nrm=False):
    for r in recs:
        if r['family'] == FAM_DIRECT_LDS:
            REACHED.setdefault('direct_lds', (B, T))
        if r['family'] != FAM_TILE:
            continue
        if r['flat_upr']:
            kind = 'wide' if r['upt'] == 8 else 'narrow'
            REACHED.setdefault(f"flat{'+nrm' if r['nrm'] else ''} {kind} upr {r['flat_upr']}", (B, T))
            if ragged:
                REACHED.setdefault('flat ragged', (B, T))
        if r['qt2']:
            REACHED.setdefault('qt2', (B, T))
        if r['BN'] == 256 and not r['flat_upr']:
            REACHED.setdefault('plain wide', (B, T))
        if r['stats']:
            REACHED.setdefault('stats', (B, T))
        if two_src_nrm and r['nrm']:
            REACHED.setdefault('nrm two sources 128 channels', (B, T))


_probes = {}


def probe_for(name, prelu=False):
    key = (name, prelu)
    if key not in _probes:
        sh = SHAPES[name]
        w, bias, slope = make_layer(sh, sorted(SHAPES).index(name) + 10 * prelu, prelu)
        _probes[key] = (Probe(sh, w, bias, slope), w, bias, slope)
    return _probes[key]


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(SHAPES))
@pytest.mark.parametrize('T', T_SWEEP)
def test_layer_matches_float64_at_threshold_batches(name, T):
    """Every shape x every frame count x a batch just below and just above each workgroup threshold (NRM and the statistics rider
    where the layer has them in the engine)."""
    assert torch.cuda.is_available()
    sh = SHAPES[name]
    probe, w, bias, slope = probe_for(name, prelu=not sh['nrm'])
    nrm = sh['nrm']
    stats = bool(probe.plans[0]['stats_ok']) and sh['nrm']
    for B in sorted({b for pl in probe.plans for b in b_points(pl, sh, T)}):
        recs = run_case(probe, sh, w, bias, slope, B, T, nrm=nrm, stats=stats, seed=B * 1000 + T)
        check_geometry(probe, sh, recs, B, T, nrm, stats)
        note(recs, B, T, two_src_nrm=nrm and sh['c0'] >= 0 and sh['Cin'] == 128)


# flat+NRM: units per row and the tile (8 units wide / 4 narrow).  Rows shorter than a tile put three or more rows into one
# tile for upr 1, 2, 3, 5 (wide) and 1 (narrow) - the flattened tile holds two rows' norm parameters, so gc_launch refuses it
FLAT_CASES = [('wide', u) for u in (1, 2, 3, 5, 4, 6, 7, 13)] + [('narrow', u) for u in (1, 2)]


def flat_batch(sh, upt, T, nrm):
    """A batch that selects the flattened tile of `upt` units at T frames (its nblk lies on the right side of the thresholds)."""
    Q = sh['Fout']
    per_b = Q * -(-T // 128)
    if upt == 8:
        return -(-WIDE_MIN // per_b) + 3
    return -(-ALT_N64 // per_b) + 3 if -(-ALT_N64 // per_b) + 3 < WIDE_MIN / per_b else None


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['g2net_level', 'taylor_level'])
@pytest.mark.parametrize('nrm', [True, False])
@pytest.mark.parametrize('kind,upr', FLAT_CASES)
def test_flattened_tiles_by_units_per_row(name, nrm, kind, upr):
    assert torch.cuda.is_available()
    sh = SHAPES[name]
    probe, w, bias, slope = probe_for(name, prelu=not nrm)
    upt = 8 if kind == 'wide' else 4
    T = 32 * upr - 3 if upr > 1 else 29
    B = flat_batch(sh, upt, T, nrm)
    assert B is not None and B * sh['Fout'] * -(-T // 128) >= ALT_N64
    recs = run_case(probe, sh, w, bias, slope, B, T, nrm=nrm, seed=upr * 7 + upt)
    span = rows_spanned(B, upr, upt)
    tiles = [r for r in recs if r['family'] == FAM_TILE]
    flat = [r for r in tiles if r['flat_upr'] == upr and r['upt'] == upt]
    if nrm and span > 2:
        assert not flat and any(r['flat_nrm_refused'] == span for r in tiles), (span, recs)
    else:
        assert flat and flat[0]['nrm'] == int(nrm) and flat[0]['flat_rows'] == span, (span, recs)
    note(recs, B, T)
    REACHED.setdefault(f"case flat{'+nrm' if nrm else ''} {kind} upr {upr}", (B, T))


@pytest.mark.gpu
@pytest.mark.parametrize('upr', [3, 4, 13])
def test_flattened_tiles_with_ragged_rows(upr):
    """Ragged rows (se_enhance_ragged, PadFrames): frames >= tlen[b] leave as zeros from every unit of a flattened tile."""
    sh = SHAPES['g2net_level']
    probe, w, bias, slope = probe_for('g2net_level')
    T = 32 * upr
    B = -(-WIDE_MIN // (sh['Fout'] * -(-T // 128))) + 1
    g = np.random.default_rng(upr)
    tlen = g.integers(max(1, T - 40), T + 1, B)
    tlen[0] = T
    recs = run_case(probe, sh, w, bias, slope, B, T, nrm=True, stats=True, tlen=tlen, seed=upr)
    assert all(r['ragged'] for r in recs if r['family'] == FAM_TILE)
    note(recs, B, T, ragged=True)


@pytest.mark.gpu
@pytest.mark.parametrize('T', [256, 500])
def test_plain_wide_tiles(T):
    """Rows that fill whole 256-frame tiles (flattening would save nothing): the plain 64 x 256 tile, with NRM and statistics."""
    for name in ('g2net_level', 'taylor_level'):
        sh = SHAPES[name]
        probe, w, bias, slope = probe_for(name)
        B = -(-WIDE_MIN // (sh['Fout'] * -(-T // 128)))
        recs = run_case(probe, sh, w, bias, slope, B, T, nrm=True, stats=True, seed=T)
        assert any(r['BN'] == 256 and not r['flat_upr'] and r['nrm'] and r['stats'] for r in recs), recs
        note(recs, B, T)


@pytest.mark.gpu
def test_row_pitch_frames_never_reach_the_output():
    """Sources whose row pitch is wider than the row (the frames behind it hold 1e3): no geometry may read them into a stored value."""
    for name, T, Tp in (('g2net_level', 150, 160), ('taylor_level', 97, 100), ('dccrn_enc', 101, 104)):
        sh = SHAPES[name]
        probe, w, bias, slope = probe_for(name, prelu=not sh['nrm'])
        for pl in probe.plans:
            for B in b_points(pl, sh, T):
                run_case(probe, sh, w, bias, slope, B, T, nrm=sh['nrm'], Tp=Tp, seed=B + T)


# (the flat+NRM cases of upr 1, 2, 3, 5 wide and 1 narrow reach gc_launch's refusal: test_flattened_tiles_by_units_per_row asserts it)
TARGETS = ['flat+nrm wide upr %d' % u for u in (4, 6, 7, 13)] + ['flat+nrm narrow upr 2'] + \
          ['case flat+nrm wide upr %d' % u for u in (1, 2, 3, 5, 4, 6, 7, 13)] + \
          ['case flat+nrm narrow upr %d' % u for u in (1, 2)] + \
          ['flat wide upr %d' % u for u in (1, 2, 3, 5, 4, 6, 7, 13)] + ['flat narrow upr %d' % u for u in (1, 2)] + \
          ['flat ragged', 'nrm two sources 128 channels', 'qt2', 'plain wide', 'direct_lds', 'stats']


@pytest.mark.gpu
def test_every_targeted_geometry_is_reached():
    """Runs last in this file: the cases above together reach every geometry they were written for (a retuned threshold must not
    quietly turn them into cases of some other geometry)."""
    missing = [t for t in TARGETS if t not in REACHED]
    assert not missing, f'not reached: {missing}; reached: {sorted(REACHED)}'


# ------------------------------------------------------------------------------------------------ CPU: the reference itself
def test_reference_matches_torch_and_the_oracle_in_float64():
    """The float64 reference the GPU cases rest on: its normalisation, its zero padding (outside the plane AFTER normalisation,
    i.e. a padded tap contributes 0, not norm(0)) and its frame / row conventions against torch's F.conv2d / F.conv_transpose2d
    and oracle/nnops, and ragged rows stored as zeros from tlen[b] on."""
    sys.path.insert(0, ROOT)
    from oracle import nnops
    g = np.random.default_rng(3)
    B, Cin, M, Fin, T = 3, 5, 4, 9, 11
    x = torch.from_numpy(g.standard_normal((B, Cin, Fin, T)))
    scale = torch.from_numpy(g.uniform(0.5, 2.0, (B, Cin)))
    shift = torch.from_numpy(g.standard_normal((B, Cin)))
    slope = torch.from_numpy(g.uniform(0.0, 0.3, (B, Cin)))
    nrm = torch.stack([scale, shift, slope - 1, -shift / scale], -1)
    xn, _ = normalise(x, nrm)
    pre = x * scale[:, :, None, None] + shift[:, :, None, None]
    assert torch.allclose(xn, torch.where(pre >= 0, pre, slope[:, :, None, None] * pre), rtol=0, atol=1e-14)
    # conv: frequency stride 2, pad 1 both sides, causal time taps (pt_left = nkt - 1, the engine's causal pad)
    w = torch.from_numpy(g.standard_normal((M, Cin, 3, 2)))
    sh = dict(kind='conv', sf=2, pf=1, pt=1)
    Fout = (Fin + 2 - 3) // 2 + 1
    bias = torch.from_numpy(g.standard_normal(M))
    y, bound = reference(sh, [x], [nrm], w, bias, None, T, Fout)
    xp = torch.nn.functional.pad(xn, (1, 0, 0, 0))           # time: causal left pad of the NORMALISED input
    want = torch.nn.functional.conv2d(xp, w, bias, stride=(2, 1), padding=(1, 0))
    assert want.shape == y.shape and torch.allclose(y, want, rtol=0, atol=1e-12)
    assert torch.allclose(y, torch.from_numpy(nnops.conv2d(xp.numpy(), w.numpy(), bias.numpy(), stride=(2, 1), padding=(1, 0))),
                          rtol=0, atol=1e-12)
    assert bool((bound > 0).all())
    # two sources with different norm parameters are one channel concat
    y2, _ = reference(sh, [x[:, :2], x[:, 2:]], [nrm[:, :2], nrm[:, 2:]], w, bias, None, T, Fout)
    assert torch.allclose(y, y2, rtol=0, atol=1e-12)
    # transposed conv (U^2-Net decoder: frequency stride 2, no pad; time taps reach back)
    wd = torch.from_numpy(g.standard_normal((M, Cin, 3, 2)))
    shd = dict(kind='deconv', sf=2, pf=0, toff=0)
    Fo = (Fin - 1) * 2 + 3
    yd, _ = reference(shd, [x], [None], wd, bias, None, T, Fo)
    wt = wd.permute(1, 0, 2, 3).contiguous()                     # torch layout [Cin][M][kf][kt]
    full = torch.nn.functional.conv_transpose2d(x, wt, bias, stride=(2, 1))
    assert torch.allclose(yd, full[..., :T], rtol=0, atol=1e-12)
    assert torch.allclose(yd, torch.from_numpy(nnops.conv_transpose2d(x.numpy(), wt.numpy(), bias.numpy(), stride=(2, 1)))[..., :T],
                          rtol=0, atol=1e-12)
    # PReLU epilogue and ragged rows
    sl = torch.from_numpy(g.uniform(0.1, 0.3, M))
    tlen = torch.tensor([T, 4, 1])
    yr, _ = reference(sh, [x], [nrm], w, bias, sl, T, Fout, tlen)
    full_act = torch.where(want >= 0, want, sl[None, :, None, None] * want)
    for b in range(B):
        assert torch.allclose(yr[b, ..., :tlen[b]], full_act[b, ..., :tlen[b]], rtol=0, atol=1e-12)
        assert bool((yr[b, ..., tlen[b]:] == 0).all())
    # the flattened tiles' row span, as gc_launch computes it
    assert rows_spanned(256, 3, 8) == 4 and rows_spanned(256, 13, 8) == 2 and rows_spanned(256, 1, 4) == 4
    assert rows_spanned(256, 5, 8) == 3 and rows_spanned(256, 4, 8) == 2 and rows_spanned(256, 2, 4) == 2
