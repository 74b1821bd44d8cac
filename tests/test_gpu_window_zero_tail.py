"""GPU: the window-relative zero tail of chunk tensors (csrc/window_rows.h, k_rows.hip: launch_window_zero_tail and its batched form),
one launch at a time through the test-only probe csrc/tests/wzt_probe.hip, against a numpy statement for EXACT equality: for row b
of a tensor [B][rows][Tw] whose column c holds frame t0 - HC + c, columns [cut_b, Tw) become 0 with
cut_b = clamp(tlen[b] - (t0 - HC), 0, Tw), and every other float - the guard words in front of and behind every tensor included -
keeps its bits.  The kernels only store zeros, so there is no rounding to allow for.

Shapes: B = 3; Tw = 13, 19, 28 (HC + 1, + 7, + 16: no multiple of four, so the tails start at every 16 B phase) and 300 (a tail longer
than the 64 lanes of a row cover in one pass); 1, 5 and 1024 rows (one lane group, an odd count, more than one block); tensors placed
behind 5 guard floats, so their bases are not 16 B aligned either.  tlen puts the cut below the window, at column 0, inside, at Tw - 1,
at Tw and beyond it, and into the first window, whose history columns are frames below 0."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'sixty-years-of-frequency-domain-monaural-speech-enhancement_amd')
PROBE_LIB = os.path.join(PKG, 'libse_wztprobe.so')

pytestmark = pytest.mark.gpu

HC, B, GUARD = 12, 3, 5
GUARD_BITS = 0x7FC0BEEF              # a NaN pattern: a guard that is read and compared as a float would not even equal itself


@pytest.fixture(scope='module')
def lib():
    assert os.path.exists(PROBE_LIB), f'{PROBE_LIB} is not built (make -C {PKG}/csrc)'
    L = C.CDLL(PROBE_LIB)
    L.wz_last_error.restype = C.c_char_p
    L.wz_window_cut.argtypes = [C.c_int] * 4
    L.wz_zero_tail.argtypes = [C.c_void_p, C.c_int, C.c_longlong, C.c_int, C.c_void_p, C.c_int, C.c_int]
    L.wz_zero_tail_batch.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_longlong), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
    return L


def _tlen_sets(t0, Tw):
    """frame counts for the three rows: the window holds frames [t0 - HC, t0 - HC + Tw)"""
    f0 = t0 - HC
    if f0 < 0:          # the first window: columns 0 .. HC - 1 are frames below 0; cuts HC + 1, inside, beyond
        return [(1, min(5, Tw - HC), 100)]
    return [(5, f0 + 3, f0 + Tw),                      # below the window (everything cleared) | inside | at Tw (untouched)
            (f0, f0 + Tw - 1, 1000)]                   # at column 0 (everything cleared) | at Tw - 1 (one column) | beyond (untouched)


def _cut(tlen, t0, Tw):
    return int(np.clip(tlen - (t0 - HC), 0, Tw))


def _arena(rows_list, Tw, tlen, t0, seed):
    """one flat buffer: [guard | tensor 0 | guard | tensor 1 | ... | guard]; -> (uint32 image, float offsets of the tensors, expected image)"""
    rng = np.random.default_rng(seed)
    sizes = [B * r * Tw for r in rows_list]
    total = GUARD * (len(sizes) + 1) + sum(sizes)
    img = np.full(total, GUARD_BITS, dtype=np.uint32)
    want = img.copy()
    offs, o = [], GUARD
    for r, n in zip(rows_list, sizes):
        x = rng.standard_normal((B, r, Tw)).astype(np.float32)      # NaN-free ...
        for b in range(B):
            cut = _cut(tlen[b], t0, Tw)
            if cut < Tw:                                            # ... plus a few NaNs and an inf in the tail, which must disappear
                x[b, rng.integers(0, r, size=3), rng.integers(cut, Tw, size=3)] = np.nan
                x[b, r - 1, Tw - 1] = np.inf
        ref = x.copy()
        for b in range(B):
            ref[b, :, _cut(tlen[b], t0, Tw):] = 0.0
        img[o:o + n] = x.reshape(-1).view(np.uint32)
        want[o:o + n] = ref.reshape(-1).view(np.uint32)
        offs.append(o)
        o += n + GUARD
    return img, offs, want


def _run(lib, rows_list, Tw, tlen, t0, seed, batched):
    img, offs, want = _arena(rows_list, Tw, tlen, t0, seed)
    for b in range(B):
        assert lib.wz_window_cut(int(tlen[b]), t0, HC, Tw) == _cut(tlen[b], t0, Tw)
    dev = torch.from_numpy(img.view(np.int32)).cuda()
    dt = torch.tensor(list(tlen), dtype=torch.int32).cuda()
    base = dev.data_ptr()
    if batched:
        ptrs = (C.c_void_p * len(offs))(*[base + 4 * o for o in offs])
        rws = (C.c_longlong * len(offs))(*rows_list)
        rc = lib.wz_zero_tail_batch(ptrs, rws, len(offs), B, Tw, dt.data_ptr(), t0, HC)
        assert rc == 0, lib.wz_last_error()
    else:
        for o, r in zip(offs, rows_list):
            assert lib.wz_zero_tail(base + 4 * o, B, r, Tw, dt.data_ptr(), t0, HC) == 0, lib.wz_last_error()
    got = dev.cpu().numpy().view(np.uint32)
    diff = np.flatnonzero(got != want)
    assert diff.size == 0, (rows_list, Tw, tlen, t0, 'floats that differ', diff.size, 'first at', diff[:8])
    for k in range(len(offs) + 1):      # (covered by the comparison above; said on its own because it is the point)
        g0 = 0 if k == 0 else offs[k - 1] + B * rows_list[k - 1] * Tw
        assert (got[g0:g0 + GUARD] == GUARD_BITS).all(), ('guard', k)


@pytest.mark.parametrize('Tw', [13, 19, 28])
@pytest.mark.parametrize('rows', [1, 5, 1024])
def test_single_launch_equals_the_numpy_statement(lib, Tw, rows):
    for t0 in (40, 0):
        for k, tlen in enumerate(_tlen_sets(t0, Tw)):
            _run(lib, [rows], Tw, tlen, t0, 100 * Tw + rows + k, batched=False)


def test_a_tail_longer_than_one_pass_of_a_row(lib):
    """Tw = 300: a cleared row is 300 floats, more than the 64 lanes of a row store in one pass (256)"""
    for tlen in _tlen_sets(500, 300):
        _run(lib, [5], 300, tlen, 500, 7, batched=False)


@pytest.mark.parametrize('Tw', [13, 19, 28])
def test_batched_launch_equals_the_numpy_statement(lib, Tw):
    """seven tensors with the row counts of DCCRN's E[0..5] and D[0] in a chunk (4096 x 4, 2048, 1024 x 2), divided by 16, and the
    shape set of the single launch as seven tensors of 1, 5 and 1024 rows"""
    for rows_list in ([256, 256, 256, 256, 128, 64, 64], [1, 5, 1024, 5, 1, 1024, 1]):
        for t0 in (40, 0):
            for k, tlen in enumerate(_tlen_sets(t0, Tw)):
                _run(lib, rows_list, Tw, tlen, t0, 1000 + Tw + k, batched=True)


def test_bad_arguments_are_errors(lib):
    dt = torch.zeros(3, dtype=torch.int32).cuda()
    x = torch.zeros(64, dtype=torch.float32).cuda()
    ptrs = (C.c_void_p * 9)(*[x.data_ptr()] * 9)
    rws = (C.c_longlong * 9)(*[1] * 9)
    assert lib.wz_zero_tail_batch(ptrs, rws, 9, 1, 13, dt.data_ptr(), 0, HC) != 0 and b'0..8 tensors' in lib.wz_last_error()
    assert lib.wz_zero_tail(x.data_ptr(), 1, 1, 8, dt.data_ptr(), 0, HC) != 0 and b'bad window' in lib.wz_last_error()      # HC > Tw
    assert lib.wz_zero_tail(x.data_ptr(), 1, 1, 13, None, 0, HC) != 0 and b'bad window' in lib.wz_last_error()
