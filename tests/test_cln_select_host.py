"""The cumulative LayerNorm's kernel selection on a CPU: cln_select (csrc/cln_select.h, through the host-only probe
csrc/tests/cln_select_probe.cpp -> libse_clnselprobe.so)
  * its kernel names against the Python mirror of tests/test_gpu_norm_forms.py (cln_forms, stream_form and the pair of
    test_cln_parts: an independent statement of the ladder, written from the launcher the selection replaced and asserted by the GPU
    tests against real launches), over chunk widths 1..64, rows either side of both thresholds, channels either side of 256, FIR
    lengths, pre-slope, residual and both values of the two switches;
  * every launch's grid and LDS, c0, WP and W / VPT against formulas written out here from that launcher;
  * one predicate: takes_res is "the register form and SE_CLN_STREAM_RES on", and a residual on any other chunk is refused;
  * every refusal with its message and no launch."""
import ctypes as C
import os

import test_gpu_norm_forms as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_LIB = os.path.join(ROOT, 'sixty-years-of-frequency-domain-monaural-speech-enhancement_amd', 'libse_clnselprobe.so')

CHOICE = ('form', 'n_launch', 'c0', 'back', 'WP', 'W', 'VPT', 'takes_res', 'scratch')
LAUNCH = ('kernel', 'gx', 'gy', 'gz', 'block', 'lds', 'res')
IN = ('B', 'C', 'F', 'T', 'K', 'pre', 'post', 'res', 'parts', 'ragged', 'stream', 'H', 'n', 'sB')
RES_PLAIN = 'cLN: the residual rides on the plain 2-D form only'
TOO_LONG = 'utterance too long for the LDS-resident cLN scan'
NOT_WINDOW = 'cLN: tensor is not a window of the current chunk'
FIR_LONG = "cLN FIR longer than the window's history"
RES_REG = 'frame-online cLN: the residual rides on the register form only (ask cln_stream_takes_res first)'
PARTS_OFFLINE = 'cLN from epilogue statistics: offline equal-length batches only'
_lib = None
_in = (C.c_int * len(IN))()
_out = (C.c_longlong * (len(CHOICE) + 3 * len(LAUNCH)))()


def lib():
    global _lib
    if _lib is None:
        assert os.path.exists(PROBE_LIB), 'libse_clnselprobe.so is missing: run build() (make -C csrc)'
        L = C.CDLL(PROBE_LIB)
        L.css_form_name.restype = L.css_kernel_name.restype = L.css_select.restype = C.c_char_p
        L.css_select.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_longlong)]
        assert L.css_choice_fields() == len(CHOICE) and L.css_launch_fields() == len(LAUNCH)
        _lib = L
    return _lib


def select(plane=True, stream_res=True, **kw):
    """cln_select of a call as a dict; 'launches': its n_launch entries, 'kernels': their log names"""
    L = lib()
    args = dict(B=2, F=1, K=0, pre=0, post=0, res=0, parts=0, ragged=0, stream=0, H=0, n=0, sB=0)
    args.update(kw)
    for i, k in enumerate(IN):
        _in[i] = int(args[k])
    refusal = L.css_select(_in, int(plane), int(stream_res), _out).decode()
    c = dict(zip(CHOICE, _out))
    c['launches'] = [dict(zip(LAUNCH, _out[len(CHOICE) + len(LAUNCH) * i:])) for i in range(c['n_launch'])]
    c['kernels'] = [L.css_kernel_name(l['kernel']).decode() for l in c['launches']]
    c['name'] = L.css_form_name(c['form']).decode()
    c['refusal'] = refusal
    assert (c['name'] == 'refused') == bool(refusal) and (not refusal or (c['n_launch'] == 0 and not c['takes_res'])), c
    return c


def chunk(Cc, Fq, H, n, B=2, **kw):
    return select(B=B, C=Cc, F=Fq, T=H + n, stream=1, H=H, n=n, sB=B, **kw)


def cdiv(a, b):
    return (a + b - 1) // b


def grids(c):
    return [(l['gx'], l['gy'], l['gz'], l['lds'], l['res']) for l in c['launches']]


# rows R = C * F either side of 256 * 41 (C <= 256 and C > 256), and with T - c0 columns either side of 32768 elements
STREAM_SHAPES = [(4, 7), (64, 161), (64, 164), (64, 165), (256, 41), (257, 1), (257, 40), (512, 1), (66, 161), (600, 1), (64, 1), (8, 20),
                 (64, 8), (64, 33), (3, 171), (1, 32768), (1, 32769), (205, 1), (206, 1)]


def test_stream_forms_equal_the_mirror_and_one_predicate_takes_the_residual():
    seen, n_cases = set(), 0
    for Cc, Fq in STREAM_SHAPES:
        R = Cc * Fq
        for n in range(1, 65):
            for K in (0, 2, 5, 63):
                for pre in (0, 1):
                    if K and Fq != 1 and n % 7:      # (the models' FIR heads are 1-D; keep some 2-D ones)
                        continue
                    H = max(8, K - 1)
                    back = K - 1 if K else 0
                    c0, T = H - back, H + n
                    Wn = T - c0
                    want = G.stream_form(n, R, Cc, K, bool(pre), Wn, T)
                    for stream_res in (True, False):
                        for res in (0, 1):
                            c = chunk(Cc, Fq, H, n, K=K, pre=pre, post=1 - pre, res=res, stream_res=stream_res)
                            n_cases += 1
                            if res and (K or pre):
                                assert c['refusal'] == RES_PLAIN
                                continue
                            reg = want == ['cln_window_reg']
                            if res and not (reg and stream_res):
                                assert c['refusal'] == RES_REG, (Cc, Fq, n, K, pre, c)
                                continue
                            assert c['kernels'] == want, (Cc, Fq, n, K, pre, c)
                            assert c['takes_res'] == (c['name'] == 'stream_reg' and stream_res) and (c['name'] == 'stream_reg') == reg
                            assert (c['c0'], c['back'], c['scratch']) == (c0, back, 2 * T * 24)
                            # grids, LDS, WP, W from the launcher this selection replaced
                            if reg:
                                assert grids(c) == [(2, 1, 1, 0, 1)] and (c['W'], c['VPT'], c['WP']) == (n, 41 * n, 0)
                            elif want == ['cln_window']:
                                assert grids(c) == [(2, 1, 1, 24 * T + (4 * R * Wn if K else 0), 0)] and (c['W'], c['VPT'], c['WP']) == (0, 0, 0)
                            else:
                                WP = 1
                                while WP < Wn and WP < 64:
                                    WP *= 2
                                assert WP >= min(Wn, 64) and (WP == 1 or WP // 2 < Wn) and WP & (WP - 1) == 0
                                assert grids(c) == [(cdiv(Wn, WP), 2, 1, 0, 0), (2, 1, 1, 16 * T, 0), (cdiv(n, 256), cdiv(R, 8), 2, 0, 0)]
                                assert (c['W'], c['VPT'], c['WP']) == (0, 0, WP)
                            seen.add((c['name'], bool(K)))
    assert seen == {('stream_reg', False), ('stream_window', False), ('stream_window', True), ('stream_rows', False), ('stream_rows', True)}
    assert n_cases > 20000


def test_chunk_query_is_the_same_predicate():
    """cln_stream_takes_res (blocks.h asks it before it hands launch_cln a residual) is cln_select's takes_res of the plain 2-D call"""
    L = lib()
    for Cc, Fq in STREAM_SHAPES:
        for n in (1, 2, 3, 64):
            for stream_res in (True, False):
                c = chunk(Cc, Fq, 8, n, post=1, stream_res=stream_res)
                assert bool(L.css_chunk_takes_res(2, Cc, Fq, 8, n, int(stream_res))) == bool(c['takes_res'])
                with_res = chunk(Cc, Fq, 8, n, post=1, res=1, stream_res=stream_res)
                assert (with_res['refusal'] == '') == bool(c['takes_res']) and with_res['refusal'] in ('', RES_REG)


def test_offline_forms_equal_the_mirror():
    n_cases = 0
    for B in (1, 2, 5):
        for Cc, Fq in ((1, 1), (4, 1), (5, 7), (3, 171), (64, 161), (257, 3)):
            R = Cc * Fq
            for T in G.CLN_T + [255, 256, 257, 3749]:      # up to the LDS limit of the scan, 16 T <= 60000
                for K in (0, 2, 5, 63):
                    for pre in (0, 1):
                        for res in (0, 1):
                            for plane in (True, False):
                                c = select(B=B, C=Cc, F=Fq, T=T, K=K, pre=pre, post=1 - pre, res=res, plane=plane)
                                n_cases += 1
                                if res and (K or pre):
                                    assert c['refusal'] == RES_PLAIN
                                    continue
                                want = G.cln_forms(K, bool(pre), bool(res), plane)
                                assert c['kernels'] == want, (B, Cc, Fq, T, K, pre, res, plane, c)
                                assert (c['c0'], c['back'], c['WP'], c['W'], c['VPT'], c['scratch']) == (0, 0, 64, 0, 0, B * T * 24)
                                assert c['takes_res'] == (not K and not pre)
                                stats, scan = (cdiv(T, 64), B, 1, 0, 0), (B, 1, 1, 16 * T, 0)
                                if want[2] == 'cln_apply_plane':
                                    assert c['name'] == 'plane' and grids(c) == [stats, scan, (B * Cc, 1, 1, 8 * T, 1)]
                                else:
                                    assert c['name'] == 'rows' and grids(c) == [stats, scan, (cdiv(T, 256), cdiv(R, 8), B, 0, 0)]
                                assert all(l['block'] == 256 for l in c['launches'])
    assert n_cases > 5000


def test_parts_form():
    for plane in (True, False):
        for Fq, T, _ in G.PARTS_CASES:
            for res in (0, 1):
                c = select(B=2, C=6, F=Fq, T=T, post=1, res=res, parts=1, plane=plane)
                assert c['name'] == 'parts' and c['kernels'] == ['cln_scan_parts', 'cln_apply_plane'] and c['takes_res']
                assert grids(c) == [(2, 1, 1, 16 * T, 0), (12, 1, 1, 8 * T, 1)] and (c['c0'], c['WP'], c['scratch']) == (0, 0, 2 * T * 24)


def test_refusals():
    # a residual behind a FIR or a pre-slope, offline and on a chunk
    assert select(C=1, T=8, K=3, res=1)['refusal'] == RES_PLAIN
    assert select(C=1, T=8, pre=1, res=1)['refusal'] == RES_PLAIN
    assert chunk(4, 1, 8, 1, K=3, pre=1, res=1)['refusal'] == RES_PLAIN
    # T * 16 > 60000
    assert select(C=1, T=3750)['refusal'] == '' and select(C=1, T=3751)['refusal'] == TOO_LONG
    assert select(C=6, F=7, T=3751, parts=1)['refusal'] == TOO_LONG and chunk(4, 7, 3750, 1)['refusal'] == TOO_LONG
    # the tensor against the open chunk
    assert select(C=4, F=7, T=10, stream=1, H=8, n=1, sB=2)['refusal'] == NOT_WINDOW
    assert select(C=4, F=7, T=9, stream=1, H=8, n=1, sB=3)['refusal'] == NOT_WINDOW
    assert select(C=4, F=7, T=9, stream=1, H=8, n=1, sB=2)['refusal'] == ''
    # FIR against the history
    assert chunk(64, 1, 8, 1, K=9, pre=1)['refusal'] == '' and chunk(64, 1, 8, 1, K=10, pre=1)['refusal'] == FIR_LONG
    # a residual on a chunk outside the register form, or with the switch off
    assert chunk(4, 7, 8, 3, res=1)['refusal'] == RES_REG and chunk(66, 161, 8, 1, res=1)['refusal'] == RES_REG
    assert chunk(4, 7, 8, 2, res=1)['refusal'] == '' and chunk(4, 7, 8, 2, res=1, stream_res=False)['refusal'] == RES_REG
    assert chunk(4, 7, 8, 2, stream_res=False)['name'] == 'stream_reg'      # (the switch takes the residual off the form, not the form)
    # the epilogue sums on a chunk or on a ragged batch
    assert select(C=6, F=7, T=40, parts=1)['refusal'] == ''
    assert select(C=6, F=7, T=40, parts=1, ragged=1)['refusal'] == PARTS_OFFLINE
    assert chunk(6, 7, 8, 1, parts=1)['refusal'] == PARTS_OFFLINE
