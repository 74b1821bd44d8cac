"""Edge-row classes of the tap-table conv (csrc/gemmconv.hip, gc_select.h: gc_edge_classes): output rows whose frequency taps partly
lie outside the input plane run on K tables and packed weights of the live K rows only.  The skipped terms were w * 0, so a plan
with classes has to give, value for value, what the same plan built with SE_GC_EDGE=0 gives - and both stay inside the float64
bound of tests/test_gpu_gemmconv_geometry.py.  Single layers of DCCRN's (5, 2) conv / transposed conv through the probe library
(csrc/tests/gc_probe.hip: gcp_edge_create), the grouped three-product launches through gauss::run_layer (csrc/tests/epi_probe.hip:
epp_gauss_create_edge); the class builder itself on a CPU (csrc/tests/gc_select_probe.cpp: gcs_edge_classes).

Shapes: B = 2 rows of T = 40 frames (one partly filled time tile), Cin = 7 (the last K chunk is a partial one), planned for rows of
40 frames so that the launches take the plan's own one-row tiles in the plain form - the form that reads the classes."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import test_gpu_conv_epilogues as E
from test_gpu_gemmconv_geometry import FAM_TILE, PKG, Probe, reference

GSPROBE_LIB = os.path.join(PKG, 'libse_gcselprobe.so')
B, T, CIN = 2, 40, 7
MAX_KCP, EDGE_MAX = 48, 2


class env_edge:
    """SE_GC_EDGE for the plans built inside the block (gc_make_plan reads it at every call)."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get('SE_GC_EDGE')
        if self.value is None:
            os.environ.pop('SE_GC_EDGE', None)
        else:
            os.environ['SE_GC_EDGE'] = self.value

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop('SE_GC_EDGE', None)
        else:
            os.environ['SE_GC_EDGE'] = self.old


# ------------------------------------------------------------------------------------------------ single layers
class EdgeProbe(Probe):
    """One (5, 2) layer built by gcp_edge_create; run and read like the geometry test's probe."""

    def __init__(self, sh, w, bias, slope, edge_Fin):
        lib = self.lib()
        vp, i32, fp = C.c_void_p, C.c_int, C.POINTER(C.c_float)
        lib.gcp_edge_create.restype = vp
        lib.gcp_edge_create.argtypes = [fp, fp, fp] + [i32] * 8
        lib.gcp_edge_info.argtypes = [vp, i32, C.POINTER(i32), i32]
        self.sh = sh
        f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
        self._keep = [f32(w), f32(bias), f32(slope)]
        ptr = lambda a: None if a is None else a.ctypes.data_as(fp)
        wp, bp, sp = (ptr(a) for a in self._keep)
        M, Cin = w.shape[:2]
        deconv = sh['kind'] == 'deconv'
        self.h = lib.gcp_edge_create(wp, bp, sp, M, Cin, int(deconv), sh.get('toff', 0), 1 if slope is not None else 0, sh['c0'], T, edge_Fin)
        assert self.h, lib.gcp_last_error().decode()
        self.plans = [self.info(0)]
        for c in range(1, self.plans[0]['nplans']):
            self.plans.append(self.info(c))

    def edge(self, cls):
        out = (C.c_int * 8)()
        assert self.lib().gcp_edge_info(self.h, cls, out, 8) == 8
        return dict(zip(('nclass', 'lo', 'hi', 'Fin', 'Q', 'KCp', 'KCp1', 'KCp2'), out))


def shape(kind, M, Fin):
    if kind == 'conv':
        return dict(kind='conv', M=M, Cin=CIN, nkf=5, nkt=2, sf=2, pf=2, pt=1, c0=-1, Fin=Fin, Fout=Fin // 2)
    return dict(kind='deconv', M=M, Cin=CIN, nkf=5, nkt=2, sf=2, pf=2, toff=1, c0=4, Fin=Fin, Fout=2 * Fin)


def launch(probe, sh, xs):
    dst = torch.full((B, sh['M'], sh['Fout'], T), float('nan'), device='cuda')
    recs = probe.run(xs, [None] * len(xs), dst, sh['Fin'], sh['Fout'], B, T, T)
    return dst, recs


# (kind, M, Fin) -> per plan the classes that have to be built: (classes, class of row 0, class of row Q - 1)
SINGLE = [
    ('conv', 128, 8, [(2, 1, 2)]),                    # 8 -> 4 rows: two one-row edge classes and an interior
    ('conv', 128, 4, [(2, 1, 2)]),                    # 4 -> 2 rows: both rows are edges
    ('conv', 128, 2, [(0, 0, 0)]),                    # 2 -> 1 row: low and high edge at once - nothing is built
    ('conv', 64, 8, [(2, 1, 2)]),                     # the 64-row tile
    ('deconv', 128, 4, [(2, 1, 2), (1, 0, 1)]),       # 4 -> 8 rows, even / odd output rows, two sources (4 + 3 channels)
    ('deconv', 128, 2, [(2, 1, 2), (1, 0, 1)]),       # 2 -> 4 rows
    ('deconv', 64, 4, [(2, 1, 2), (1, 0, 1)]),
]


@pytest.mark.gpu
@pytest.mark.parametrize('kind,M,Fin,classes', SINGLE, ids=[f'{k}-M{m}-Fin{f}' for k, m, f, _ in SINGLE])
def test_edge_rows_equal_the_full_table_and_float64(kind, M, Fin, classes):
    assert torch.cuda.is_available()
    sh = shape(kind, M, Fin)
    g = np.random.default_rng(100 * Fin + M + (kind == 'deconv'))
    w = (g.standard_normal((M, CIN, 5, 2)) / np.sqrt(CIN * 10)).astype(np.float32)
    bias = (0.1 * g.standard_normal(M)).astype(np.float32)
    slope = g.uniform(0.05, 0.4, M).astype(np.float32)
    with env_edge(None):
        on = EdgeProbe(sh, w, bias, slope, Fin)
    with env_edge('0'):
        off = EdgeProbe(sh, w, bias, slope, Fin)
    try:
        for c, (n, lo, hi) in enumerate(classes):
            e = on.edge(c)
            assert (e['nclass'], e['lo'], e['hi']) == (n, lo, hi), e
            assert all(0 < e[k] < e['KCp'] and e[k] % 4 == 0 for k in ('KCp1', 'KCp2')[:n]), e
            assert off.edge(c)['nclass'] == 0
        gen = torch.Generator(device='cuda')
        gen.manual_seed(Fin * 1000 + M)
        C0 = CIN if sh['c0'] < 0 else sh['c0']
        xs = [torch.randn((B, cn, Fin, T), generator=gen, device='cuda') for cn in ([C0] + ([CIN - C0] if C0 < CIN else []))]
        y_on, r_on = launch(on, sh, xs)
        y_off, r_off = launch(off, sh, xs)
    finally:
        on.close()
        off.close()
    # the same dispatches, and the plan's own one-row tiles in the plain form (no resident-K, no two-row tile)
    assert r_on == r_off and len(r_on) == len(classes), (r_on, r_off)
    for r in r_on:
        assert r['family'] == FAM_TILE and r['BM'] == (128 if M == 128 else 64) and r['BN'] == 64 and not r['qt2'] and not r['res'], r
    w64 = torch.from_numpy(w).double().cuda()
    ref, bound = reference(sh, [x.double() for x in xs], [None] * len(xs), w64, torch.from_numpy(bias).double().cuda(),
                           torch.from_numpy(slope).double().cuda(), T, sh['Fout'])
    for name, y in (('edge classes', y_on), ('SE_GC_EDGE=0', y_off)):
        err = (y.double() - ref).abs()
        bad = ~(err <= bound)
        print(f'{kind} M={M} Fin={Fin} {name}: max err / bound {float((err / bound).max()):.3f}')
        assert not bad.any(), f'{name}: {int(bad.sum())} outputs out of bound, first {bad.nonzero()[:4].tolist()}'
    assert np.array_equal(y_on.cpu().numpy(), y_off.cpu().numpy()), \
        f'rows differ: {sorted(set((y_on != y_off).nonzero()[:, 2].tolist()))}'


# ------------------------------------------------------------------------------------------------ the grouped launches of gauss.h
def gauss_edge_lib():
    L = E.Lib.get()
    vp, i32, fp = C.c_void_p, C.c_int, C.POINTER(C.c_float)
    L.epp_gauss_create_edge.restype = vp
    L.epp_gauss_create_edge.argtypes = [fp] * 5 + [i32] * 7
    L.epp_gauss_edge_info.argtypes = [vp, i32, C.POINTER(i32)]
    return L


@pytest.mark.gpu
@pytest.mark.parametrize('co,sum_plane', [(128, False), (64, True)])
def test_grouped_three_product_launches_with_edge_rows(co, sum_plane):
    """gauss::run_layer at 8 -> 4 rows: k1 alone (EPI_ACT), then k2 and k3 with the combine epilogue (EPI_CMB) - as one grouped launch
    (Z = 2), or with a sum plane as two - each on the plan's weights moved along z: the classes' weights have to move with them.
    Reference and bound: gauss_reference of tests/test_gpu_conv_epilogues.py."""
    assert torch.cuda.is_available()
    L = gauss_edge_lib()
    ci, Fin, Fout = CIN, 8, 4
    gp = E.gauss_params(co, ci, 70 + co)
    gen = torch.Generator(device='cuda')
    gen.manual_seed(11 + co)
    src = E.three_planes(B, ci, Fin, T, gen, 'cuda')
    outs, recs = [], []
    for value in (None, '0'):
        with env_edge(value):
            h = L.epp_gauss_create_edge(E.fptr(gp['wr']), E.fptr(gp['wi']), E.fptr(gp['bias']), E.fptr(gp['bn']), E.fptr(gp['slope']), co, ci,
                                        0, 0, -1, T, Fin)
        assert h, E.Lib.error()
        try:
            info = (C.c_int * 3)()
            assert L.epp_gauss_edge_info(h, 0, info) == 3
            assert tuple(info) == ((2, 1, 2) if value is None else (0, 0, 0)), tuple(info)
            dst = E.Buf((B, 3 * co, Fout, T), 'cuda')
            K = E.Buf((3, B, co, Fout, T), 'cuda')
            torch.cuda.synchronize()
            rc = L.epp_gauss_run(h, src.ptr(), None, Fin, Fout, B, T, dst.ptr(), 1, int(sum_plane), K.ptr(), None)
            assert rc == 0, E.Lib.error()
            recs.append(E.Lib.records())
            dst.assert_unowned(T, 'dst')
            outs.append(dst.t.clone())
        finally:
            L.epp_gauss_destroy(h)
    assert recs[0] == recs[1], recs
    assert [r['Z'] for r in recs[0]] == ([1, 1, 1] if sum_plane else [1, 2]), recs[0]
    assert [r['epi'] for r in recs[0]] == ([E.EPI_ACT, E.EPI_CMB, E.EPI_CMB] if sum_plane else [E.EPI_ACT, E.EPI_CMB]), recs[0]
    assert all(r['family'] == FAM_TILE and r['BM'] == (128 if co == 128 else 64) and r['BN'] == 64 and not r['qt2'] and not r['res'] and
               r['form'] == 0 for r in recs[0]), recs[0]
    d = lambda k: torch.from_numpy(gp[k]).double().cuda()
    ref, bound = E.gauss_reference([src.t.double()], d('wr'), d('wi'), d('bias'), d('bn'), d('slope'), T, Fout, dst3=True, sum_plane=sum_plane)
    for name, got in (('edge classes', outs[0]), ('SE_GC_EDGE=0', outs[1])):
        if not sum_plane:
            assert bool(torch.isnan(got[:, :co]).all()), 'the S plane was written without sum_plane'
            got = got[:, co:]
        err = (got.double() - ref).abs()
        print(f'three-product layer co={co} sum={sum_plane} {name}: max err / bound {float((err / bound).max()):.3f}')
        assert bool((err <= bound).all()), name
    assert np.array_equal(outs[0].cpu().numpy(), outs[1].cpu().numpy(), equal_nan=True)


# ------------------------------------------------------------------------------------------------ CPU: the class builder
def edge_classes(df, cic, si, Fin, Q):
    assert os.path.exists(GSPROBE_LIB), 'libse_gcselprobe.so is missing: run build() (make -C csrc)'
    L = C.CDLL(GSPROBE_LIB)
    n = 3 + EDGE_MAX * (3 + MAX_KCP)
    out = (C.c_int * n)()
    assert L.gcs_edge_classes(len(df), (C.c_int * len(df))(*df), cic, si, Fin, Q, out) == n
    cls = []
    for c in range(EDGE_MAX):
        o = 3 + c * (3 + MAX_KCP)
        dead, kc, kcp = out[o: o + 3]
        cls.append(dict(dead=dead, KC=kc, KCp=kcp, live=list(out[o + 3: o + 3 + kc])))
    return dict(nclass=out[0], lo=out[1], hi=out[2], cls=cls[: out[0]])


def by_hand(df, cic, si, Fin, q):
    """The K rows (cil * ntaps + j) of a chunk whose tap lies inside the plane for output row q, ascending."""
    return [cil * len(df) + j for cil in range(cic) for j, d in enumerate(df) if 0 <= q * si + d < Fin]


CONV_DF = [kf - 2 for kf in range(5) for _ in range(2)]          # gauss.h conv52_taps
DEC_DF = {0: [1, 1, 0, 0, -1, -1], 1: [1, 1, 0, 0]}                # gauss.h deconv52_taps, even / odd output rows


@pytest.mark.parametrize('Fin', [32, 16, 8, 4])
def test_class_builder_conv(Fin):
    """(5, 2) conv, stride 2, pad 2, 2-channel chunks: row 0 loses two frequency taps, row Q - 1 one, every other row none - from
    F_out = 16 down to 2 exactly two classes, each the live K rows of its row in class 0's order, padded to a multiple of 4."""
    Q = Fin // 2
    e = edge_classes(CONV_DF, 2, 2, Fin, Q)
    assert (e['nclass'], e['lo'], e['hi']) == (2, 1, 2)
    assert e['cls'][0]['dead'] == 0b0000001111 and e['cls'][1]['dead'] == 0b1100000000
    for c, q in ((0, 0), (1, Q - 1)):
        assert e['cls'][c]['live'] == by_hand(CONV_DF, 2, 2, Fin, q)
        assert e['cls'][c]['KC'] == len(e['cls'][c]['live']) and e['cls'][c]['KCp'] == -(-e['cls'][c]['KC'] // 4) * 4
    assert [e['cls'][0]['KCp'], e['cls'][1]['KCp']] == [12, 16]
    for q in range(1, Q - 1):
        assert len(by_hand(CONV_DF, 2, 2, Fin, q)) == 20


def test_class_builder_refuses_what_the_row_rule_cannot_name():
    assert edge_classes(CONV_DF, 2, 2, 2, 1)['nclass'] == 0              # one row: low and high edge at once
    assert edge_classes([0], 8, 1, 4, 4)['nclass'] == 0                  # pointwise: nothing dead
    assert edge_classes([-2, -1, 0, 1, 2], 4, 1, 8, 8)['nclass'] == 0    # stride 1, pad 2: rows 1 and Q - 2 have dead taps too
    assert edge_classes(CONV_DF, 2, 2, 0, 4)['nclass'] == 0


@pytest.mark.parametrize('Fin', [2, 4, 8])
def test_class_builder_deconv(Fin):
    """Parity classes of the transposed (5, 2) layer, F -> 2 F: the even rows lose the tap below row 0 and the tap above row F - 1 (two
    classes of 16 of 24 K rows), the odd rows only the tap above (one class, row 0 stays whole)."""
    e = edge_classes(DEC_DF[0], 4, 1, Fin, Fin)
    assert (e['nclass'], e['lo'], e['hi']) == (2, 1, 2) and [c['KCp'] for c in e['cls']] == [16, 16]
    assert e['cls'][0]['live'] == by_hand(DEC_DF[0], 4, 1, Fin, 0) and e['cls'][1]['live'] == by_hand(DEC_DF[0], 4, 1, Fin, Fin - 1)
    o = edge_classes(DEC_DF[1], 8, 1, Fin, Fin)
    assert (o['nclass'], o['lo'], o['hi']) == (1, 0, 1) and o['cls'][0]['KCp'] == 16
    assert o['cls'][0]['live'] == by_hand(DEC_DF[1], 8, 1, Fin, Fin - 1) and len(by_hand(DEC_DF[1], 8, 1, Fin, 0)) == 32
