"""GPU: the FullSubNet launchers that take the model's shape at run time (csrc/k_fullsubnet.hip), one launch at a time through
csrc/tests/fsn_shape_probe.hip (libse_fsnshapeprobe.so), in the manner of tests/test_gpu_fullsubnet_norm_kernels.py.  The cLN and
Gaussian references, their derived bounds and the guarded buffers are imported from that file; the cumulative Laplace norm has no
float64 reference there, so `ref_cum` below is this file's own, with a bound derived here in the same way (stated next to it).

  fsn_build_sb   the sub-band unfold: (2 sbn + 1) rows of the noisy magnitudes then (2 fbn + 1) rows of the full-band output per sub band,
                 time-major [steps][W][257 * B], the frequency axis reflect-padded by sbn / fbn bins (BaseModel.unfold,
                 FullSubNet/fullsubnet_net_sa/base_model.py:13-42; num_neighbor = 0 returns the input, :25-27).  A pure gather: EQUAL
                 to a numpy gather on np.pad(mode='reflect').  (sbn, fbn) in (0, 0), (15, 0), (7, 2), (15, 15) x B in 1, 3 x 1 and 5
                 steps: both reflected edges, a width that is no multiple of 4 (20), the sequence index n * B + b with B > 1.
  fsn_cum_sb     cumulative_laplace_norm of a [n][W][S] tensor at W = 2 and 18 (the run-time form; W = 32 is the register form the
                 existing files cover): x / (S1 / (W frames) + EPS), float32 running sum.  Bound, derived as the cLN's in the imported
                 docstring: a1 = (W + frames + 1) U S1 on the sum, one rounding each for the division by the count, the + EPS and the
                 final division: |dy| <= |y| (a1 / (cnt d) + 3 U), d = mean + EPS.
  fsn_cln_sb     cumulative_layer_norm at W = 2 and 18 against ref_cln (tree = W sequential additions), chunked runs and rows with a
                 frame origin held to bit identity as there.  Data: `spread_data`, whose rows are well apart, because with W = 2 the
                 imported `cln_data` brings sequences whose two values nearly coincide and ref_cln refuses the whole case as
                 ill-conditioned.  So that W = 2 is not checked on separated rows alone, the kernel also runs on `cln_data` as it is and is held to ref_cln's
                 bound on the sequences whose running variance stays above 1e-4 mean^2 - a hundred times the (W + frames + 2) U mean^2 its rounding can reach.
  fsn_moments / fsn_finish_gauss  at frame_rows = W * 257 for W = 2, 18 and a look-ahead of 0 and 3 in the ragged row count
                 (tlen[b] + la) * frame_rows, against ref_moments / ref_finish."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('fsn_norm_kernels_ref', os.path.join(HERE, 'test_gpu_fullsubnet_norm_kernels.py'))
K = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(K)

PROBE_LIB = os.environ.get('SE_FSNSHAPEPROBE_LIB') or os.path.join(K.PKG, 'libse_fsnshapeprobe.so')
U, TINY, NBIN, f32, d64, Buf = K.U, K.TINY, K.NBIN, K.f32, K.d64, K.Buf
EPS32 = K.EPS32
WIDTHS = (2, 18)
gpu = pytest.mark.gpu

CT = {'p': C.c_void_p, 'i': C.c_int, 'l': C.c_long}
SIGS = {'fsp_build_sb': 'pppiiii', 'fsp_cum_sb': 'piipipi', 'fsp_cln_sb': 'piippipi', 'fsp_moments': 'plippili',
        'fsp_finish_gauss': 'pplipili', 'fsp_gauss_apply': 'pplip'}
_lib = None


def lib():
    global _lib
    if _lib is None:
        assert os.path.exists(PROBE_LIB), 'libse_fsnshapeprobe.so is missing: run build() (make -C csrc)'
        L = C.CDLL(PROBE_LIB)
        for name, sig in SIGS.items():
            getattr(L, name).argtypes = [CT[c] for c in sig]
            getattr(L, name).restype = C.c_int
        L.fsp_last_error.restype = C.c_char_p
        _lib = L
    return _lib


def call(name, *args):
    L = lib()
    rc = getattr(L, name)(*[a.ptr if isinstance(a, Buf) else a for a in args])
    assert rc == 0, '%s: %s' % (name, L.fsp_last_error().decode())


# ------------------------------------------------------------------------------------------------ the unfold
def ref_unfold(magT, fbo, sbn, fbn):
    """[steps][257][B] x 2 -> [steps][W][257][B]: BaseModel.unfold of each, noisy rows first (model.py:88-96)"""
    parts = []
    for a, n in ((magT, sbn), (fbo, fbn)):
        p = np.pad(a, ((0, 0), (n, n), (0, 0)), mode='reflect') if n > 0 else a          # base_model.py:25-33
        idx = np.arange(NBIN)[None, :] + np.arange(2 * n + 1)[:, None]                    # [2n+1][257]: window k of sub band f
        parts.append(p[:, idx, :])                                                        # [steps][2n+1][257][B]
    return np.concatenate(parts, axis=1)


@gpu
@pytest.mark.parametrize('steps', [1, 5])
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('sbn,fbn', [(0, 0), (15, 0), (7, 2), (15, 15)])
def test_unfold_equals_a_reflect_padded_gather(sbn, fbn, B, steps):
    g = np.random.default_rng(1000 * sbn + 100 * fbn + 10 * B + steps)
    magT = np.abs(g.standard_normal((steps, NBIN, B))).astype(f32)
    fbo = np.abs(g.standard_normal((steps, NBIN, B))).astype(f32) + f32(10)             # (never equal to a magnitude: a row from the wrong source shows)
    W = (2 * sbn + 1) + (2 * fbn + 1)
    bm, bf, bs = Buf(magT.size, magT), Buf(fbo.size, fbo), Buf(steps * W * NBIN * B)
    call('fsp_build_sb', bm, bf, bs, B, steps, sbn, fbn)
    assert bs.untouched() and bm.untouched() and bf.untouched()
    assert np.array_equal(bm.np(*magT.shape), magT) and np.array_equal(bf.np(*fbo.shape), fbo)
    got = bs.np(steps, W, NBIN, B)
    want = ref_unfold(magT, fbo, sbn, fbn)
    assert want.shape == got.shape
    assert np.array_equal(got, want), ('first mismatch at', np.argwhere(got != want)[:1])
    # the edges by hand: sub band 0 reads bins sbn .. 0 .. sbn, sub band 256 reads 256 - sbn .. 256 .. 256 - sbn
    assert np.array_equal(got[:, :2 * sbn + 1, 0, :], magT[:, np.abs(np.arange(-sbn, sbn + 1)), :])
    assert np.array_equal(got[:, :2 * sbn + 1, 256, :], magT[:, 256 - np.abs(np.arange(-sbn, sbn + 1)), :])
    assert np.array_equal(got[:, 2 * sbn + 1:, 256, :], fbo[:, 256 - np.abs(np.arange(-fbn, fbn + 1)), :])


def test_reference_gather_is_the_torch_unfold():
    """(CPU) ref_unfold is BaseModel.unfold: reflect pad, then torch's unfold of windows (base_model.py:29-42), restated with torch ops"""
    from torch.nn import functional as Fn
    g = np.random.default_rng(3)
    x = np.abs(g.standard_normal((2, NBIN, 1))).astype(f32)            # [steps = T][F][B = 1]
    for n in (0, 2, 15):
        inp = torch.from_numpy(x[:, :, 0].T.copy())[None, None]        # [1][1][F][T]
        if n < 1:
            out = inp.permute(0, 2, 1, 3).reshape(1, NBIN, 1, 1, 2)
        else:
            o = Fn.pad(inp.reshape(1, 1, NBIN, 2), [0, 0, n, n], mode='reflect')
            o = Fn.unfold(o, (2 * n + 1, 2))
            out = o.reshape(1, 1, 2 * n + 1, 2, NBIN).permute(0, 4, 1, 2, 3)
        want = out.reshape(NBIN, 2 * n + 1, 2).numpy()                 # [F][2n+1][T]
        mine = ref_unfold(x, x, n, 0)[:, :2 * n + 1, :, 0]             # [T][2n+1][F]
        assert np.array_equal(np.transpose(mine, (2, 1, 0)), want), n


# ------------------------------------------------------------------------------------------------ cumulative Laplace norm, any width
def ref_cum(x, t_first=0, run0=None):
    """cumulative_laplace_norm of x [n][W][S] in float64 -> y, its bound, S1 after the last frame, its bound (module docstring)"""
    x = d64(x)
    n, W, S = x.shape
    S1 = np.cumsum(x.sum(1), 0) + (0.0 if run0 is None else d64(run0)[None])
    frames = (np.zeros(S) + t_first)[None] + np.arange(n)[:, None] + 1.0
    cnt = W * frames
    a1 = (W + frames + 1) * U * np.abs(S1)
    d = S1 / cnt + EPS32
    y = x / d[:, None]
    e_y = np.abs(y) * ((a1 / (cnt * d))[:, None] + 3 * U) + TINY
    return y, e_y, S1[-1], a1[-1] + TINY


def run_cum(x, cs=None, t_first=0, origin=None):
    n, W, S = x.shape
    bx = Buf(x.size, x)
    call('fsp_cum_sb', bx, n, S, cs, t_first, origin, W)
    assert bx.untouched() and (cs is None or cs.untouched())
    return bx.np(n, W, S)


@gpu
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('W', WIDTHS)
def test_cumulative_laplace_norm_at_other_widths(W, B):
    S = NBIN * B
    x = K.cln_data(9, W, S, 40 * W + B)
    y, ybd, run, rbd = ref_cum(x)
    cs1 = Buf(S)                                          # NaN in it: a first chunk must not read the carry
    one = run_cum(x, cs1, 0)
    K.verify('fsn_cum_sb W%d B%d one shot' % (W, B), 'fsn_cum_sb', one, y, ybd)
    K.verify('fsn_cum_sb W%d B%d carried sum' % (W, B), 'fsn_cum_sb', cs1.np(S), run, rbd)
    assert np.array_equal(one, run_cum(x))
    cs, t0, outs = Buf(S), 0, []
    for c in K.CLN_CHUNKS:
        outs.append(run_cum(np.ascontiguousarray(x[t0:t0 + c]), cs, t0))
        t0 += c
    assert np.array_equal(np.concatenate(outs), one) and np.array_equal(cs.np(S), cs1.np(S))
    # rows with a frame origin: each equals the row run alone at its own t_first
    if B == 3:
        carry = np.full(S, np.nan, f32)
        for r, o in enumerate(K.ORIGINS):
            if 2 - o > 0:
                carry[r::B] = np.abs(np.random.default_rng(r).standard_normal(NBIN)).astype(f32) * W * (2 - o)
        cso = Buf(S, carry)
        got = run_cum(x[:4].copy(), cso, 2, Buf(B, np.asarray(K.ORIGINS, np.int32), torch.int32))
        for b, o in enumerate(K.ORIGINS):
            ca = Buf(NBIN, carry[b::B])
            alone = run_cum(np.ascontiguousarray(x[:4, :, b::B]), ca, 2 - o)
            assert np.array_equal(got[:, :, b::B], alone) and np.array_equal(cso.np(S)[b::B], ca.np(NBIN)), (b, o)


# ------------------------------------------------------------------------------------------------ cumulative LayerNorm, any width
def spread_data(n, W, S, seed, zero_first=False):
    """[n][W][S] >= 0 whose W values of a frame are at least one scale apart: (min(|N(0,1)|, 1) + 2 k) scale for row k.  With two rows
    cln_data's independent draws bring, among 771 sequences, pairs that nearly coincide - a first-frame variance at the size of its own
    rounding, which ref_cln refuses as ill-conditioned; here var >= scale^2 / 4 against mean^2 of a few scale^2 at every width"""
    g = np.random.default_rng(seed)
    x = np.minimum(np.abs(g.standard_normal((n, W, S))), 1.0) + 2.0 * np.arange(W)[None, :, None]
    x = (x * np.exp(g.uniform(-3, 1, (n, 1, S)))).astype(f32)
    if zero_first:
        x[0] = 0
    return x


def run_cln(x, B, cs=None, t_first=0, origin=None):
    n, W, S = x.shape
    bx = Buf(x.size, x)
    c1, c2 = cs if cs is not None else (None, None)
    call('fsp_cln_sb', bx, n, S, c1, c2, t_first, origin, W)
    assert bx.untouched() and (cs is None or (c1.untouched() and c2.untouched()))
    return bx.np(n, W, S)


@gpu
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('W', WIDTHS)
def test_cumulative_layer_norm_at_other_widths(W, B):
    S = NBIN * B
    name = 'fsn_cln_sb'
    for n in K.CLN_N:
        x = spread_data(n, W, S, 100 * n + B + W, zero_first=(n == 2))
        got = run_cln(x, B)
        y, ybd, _, _ = K.ref_cln(x, W)
        K.verify('%s W%d B%d n%d' % (name, W, B, n), name, got, y, ybd)
        if n == 2:
            assert (got[0] == 0).all() and np.isfinite(got).all()
    x = spread_data(9, W, S, 900 + B + W)
    y, ybd, run, rbd = K.ref_cln(x, W)
    cs1 = (Buf(S), Buf(S))
    one = run_cln(x, B, cs1, 0)
    K.verify('%s W%d B%d one shot with carry' % (name, W, B), name, one, y, ybd)
    K.verify('%s W%d B%d carried sums' % (name, W, B), name, np.stack([cs1[0].np(S), cs1[1].np(S)]), run, rbd)
    cs, t0, outs = (Buf(S), Buf(S)), 0, []
    for c in K.CLN_CHUNKS:
        outs.append(run_cln(np.ascontiguousarray(x[t0:t0 + c]), B, cs, t0))
        t0 += c
    assert np.array_equal(np.concatenate(outs), one), 'chunked outputs differ from the one-shot run'
    assert np.array_equal(cs[0].np(S), cs1[0].np(S)) and np.array_equal(cs[1].np(S), cs1[1].np(S))
    # the imported generator as it is: the well-conditioned sequences inside ref_cln's bound (where var + EPS is at the size of its
    # rounding the reference's own float32 expression is noise, and nothing is asserted)
    x = K.cln_data(9, W, S, 300 + B + W)
    got = run_cln(x, B)
    xd = d64(x)
    cnt = W * (np.arange(9)[:, None] + 1.0)
    mean = np.cumsum(xd.sum(1), 0) / cnt
    var = np.cumsum((xd * xd).sum(1), 0) / cnt - mean * mean
    sel = np.flatnonzero((var > 1e-4 * mean * mean).all(0))
    assert sel.size >= S // 2, 'the criterion keeps most sequences'
    y, ybd, _, _ = K.ref_cln(x[:, :, sel], W)
    K.verify('%s W%d B%d cln_data, %d of %d sequences' % (name, W, B, sel.size, S), name, got[:, :, sel], y, ybd)
    if B == 3:
        t_first = 2
        carry = np.full((2, S), np.nan, f32)
        for r, o in enumerate(K.ORIGINS):
            if t_first - o > 0:
                carry[:, r::B] = K.eval_cln32(spread_data(t_first - o, W, NBIN, 60 + r), 'sb')[1]
        cso = (Buf(S, carry[0]), Buf(S, carry[1]))
        got = run_cln(x[:4].copy(), B, cso, t_first, Buf(B, np.asarray(K.ORIGINS, np.int32), torch.int32))
        for b, o in enumerate(K.ORIGINS):
            ca = (Buf(NBIN, carry[0][b::B]), Buf(NBIN, carry[1][b::B]))
            alone = run_cln(np.ascontiguousarray(x[:4, :, b::B]), 1, ca, t_first - o)
            assert np.array_equal(got[:, :, b::B], alone), ('row', b, 'origin', o)
            assert np.array_equal(cso[0].np(S)[b::B], ca[0].np(NBIN)) and np.array_equal(cso[1].np(S)[b::B], ca[1].np(NBIN))


# ------------------------------------------------------------------------------------------------ Gaussian moments: width and look-ahead
@gpu
@pytest.mark.parametrize('la', [0, 3])
@pytest.mark.parametrize('W', WIDTHS)
def test_gaussian_moments_count_a_ragged_rows_own_look_ahead(W, la):
    B, Tp = 3, 7
    frame_rows = W * NBIN
    rows, T = Tp * frame_rows, Tp - la
    tlen = [T, 1, max(1, T // 2)]
    rmax = [min(rows, (t + la) * frame_rows) for t in tlen]
    g = np.random.default_rng(10 * W + la)
    x = (np.abs(g.standard_normal((rows, B))) * np.exp(g.uniform(-2, 1, (1, B)))).astype(f32)
    for b, r in enumerate(rmax):
        x[r:, b] = np.nan                                  # what a ragged row must not read
    rb, MB = K.rows_buf(tlen)
    bx, bpart, bstat = Buf(x.size, x), Buf(K.SUM_BLOCKS * 2 * B, dtype=torch.float64), Buf(2 * B)
    call('fsp_moments', bx, rows, B, bpart, rb, MB, frame_rows, la)
    assert bpart.untouched() and bx.untouched()
    rp, pbd = K.ref_moments(x, B, rmax)
    case = 'W%d la%d' % (W, la)
    K.verify('fsn_moments ' + case, 'fsn_moments', bpart.np(K.SUM_BLOCKS, 2, B), rp, pbd)
    call('fsp_finish_gauss', bpart, bstat, rows, B, rb, MB, frame_rows, la)
    assert bstat.untouched() and rb.untouched()
    rs, sbd = K.ref_finish(rp, rmax, 1030 + 256 // B + -(-rows // (K.SUM_BLOCKS * (256 // B))) + 1)
    K.verify('fsn_finish_gauss ' + case, 'fsn_finish_gauss', bstat.np(2, B), rs, sbd)
    by = Buf(x.size)
    call('fsp_gauss_apply', bx, by, x.size, B, bstat)
    live = np.stack([np.arange(rows) < r for r in rmax], 1)
    ry, ybd = K.ref_apply(np.where(live, x, 0), bstat.np(2, B))
    K.verify('fsn_gauss_apply ' + case, 'fsn_gauss_apply', np.where(live, by.np(*x.shape), 0), np.where(live, ry, 0), ybd)
