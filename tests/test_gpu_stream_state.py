"""GPU: parking and resuming frame-online streams (se_stream_save / se_stream_restore, `Engine.stream_save` / `stream_restore`).

The contract under test: save a stream between any two calls on it, let anything else happen on the engine, restore it there or
on another engine of the same configuration and weights - the outputs of every later push and of the flush then equal those of
the uninterrupted stream bit for bit, n_out included.  Every comparison is np.array_equal, call by call, against the
uninterrupted stream on the same engine configuration.  Engines of max_samples = 4000 with 2 rows (FullSubNet: 1), the models
and weight seeds of tests/test_gpu_sliding_stream.py, signals of 3700 samples pushed in uneven pieces so that save points fall
before the first complete frame (100 samples), mid-frame, behind a chunk boundary and after the last push.  The copy kernel
itself is run alone through a probe library against numpy."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import se_amd  # noqa: F401
from se_amd import synth
from se_amd.engine import EngineError, StreamSnapshot
from test_gpu_sliding_stream import ALL, DCCRN_CL, _make, _rows

pytestmark = pytest.mark.gpu

MS, L = 4000, 3700
PUSHES = [100, 333, 1, 800, 160, 7, 1200, 1099]          # 3700 in all
CHUNK = 4                                                # frames per step: the 800- and 1200-sample pushes cross chunk boundaries
assert sum(PUSHES) == L


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@functools.lru_cache(maxsize=None)
def _signal(B, seed, n=L):
    x = np.stack([synth.synth_clip(seed + b, 'speech' if b % 2 == 0 else 'white', n) for b in range(B)])
    x.setflags(write=False)
    return x


_ENGINES = {}


def _engine(name, kind='bounded'):
    """one engine per (model, kind) for the whole module"""
    key = (name, kind)
    if key not in _ENGINES:
        kw = {'bounded': dict(max_samples=MS), 'sliding': dict(max_samples=MS, sliding_stream=True)}[kind]
        _ENGINES[key] = _make(name, _rows(name), **kw).engine
    return _ENGINES[key]


@pytest.fixture(scope='module', autouse=True)
def _release_engines():
    yield
    for eng in _ENGINES.values():
        eng.close()
    _ENGINES.clear()
    _reference.cache_clear()


def _begin(eng, B, running=False, chunk=CHUNK):
    torch = _torch()
    if running:
        eng.stream_begin(B, max_chunk_frames=chunk, running_rms=True)
    else:
        eng.stream_begin(B, c=torch.full((B,), 3.0, device='cuda'), max_chunk_frames=chunk)


def _pieces(x, pushes):
    torch = _torch()
    xt, pos, out = torch.from_numpy(np.ascontiguousarray(x)).cuda(), 0, []
    for n in pushes:
        out.append(xt[:, pos:pos + n].contiguous())
        pos += n
    return out


def _run(eng, x, pushes=PUSHES, running=False, between=None):
    """the outputs of every push and of the flush; between(k): called after push k (k = len(pushes) - 1: before the flush)"""
    _begin(eng, x.shape[0], running)
    outs = []
    for k, p in enumerate(_pieces(x, pushes)):
        outs.append(eng.stream_push(p).cpu().numpy())
        if between:
            between(k)
    outs.append(eng.stream_flush().cpu().numpy())
    return outs


@functools.lru_cache(maxsize=None)
def _reference(name, kind='bounded', running=False):
    """the uninterrupted stream on this engine configuration: computed once, never written to"""
    outs = _run(_engine(name, kind), _signal(_rows(name), 800), running=running)
    for o in outs:
        o.setflags(write=False)
    return tuple(outs)


def _same(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape, (what, 'call', k, g.shape, w.shape)
        assert np.array_equal(g, w), (what, 'call', k, float(np.abs(g - w).max()))


def _other_stream(eng, name):
    """an unrelated stream on the same handle: another signal, another batch size where the model allows, left running"""
    B = 1
    y = _signal(B, 950, 1500)
    _begin(eng, B, chunk=7)
    for p in _pieces(y, [700, 800]):
        eng.stream_push(p)


# ------------------------------------------------------------------------------------------------ 1. another stream in between
@pytest.mark.parametrize('name', ALL)
def test_save_restore_with_another_stream_in_between(name):
    eng = _engine(name)
    want = _reference(name)
    snap = StreamSnapshot()

    def between(k):
        eng.stream_save(snap)
        _other_stream(eng, name)
        eng.stream_restore(snap)
    got = _run(eng, _signal(_rows(name), 800), between=between)
    snap.close()
    assert sum(o.shape[1] for o in want) >= L
    _same(got, want, name)


# ------------------------------------------------------------------------------------------------ 2. an engine that never streamed
@pytest.mark.parametrize('name', ['crn', 'dccrn', 'g2net_new', 'fullsubnet_cum'])
def test_restore_on_a_second_engine_that_has_never_streamed(name):
    src = _engine(name, 'sliding')
    want = _reference(name, 'sliding')
    x = _signal(_rows(name), 800)
    for label, kw in (('same configuration', dict(max_samples=MS, sliding_stream=True)), ('bounded, larger max_samples', dict(max_samples=6000))):
        dst = _make(name, _rows(name), **kw).engine         # its state buffers and slots do not exist yet
        for cut in (4, 1):                                # behind a chunk boundary; mid-frame (then into an engine that has streamed)
            _begin(src, x.shape[0])
            pieces = _pieces(x, PUSHES)
            got = [src.stream_push(p).cpu().numpy() for p in pieces[:cut]]
            snap = src.stream_save()
            dst.stream_restore(snap)
            got += [dst.stream_push(p).cpu().numpy() for p in pieces[cut:]]
            got.append(dst.stream_flush().cpu().numpy())
            snap.close()
            _same(got, want, (name, label, cut))
        dst.close()


# ------------------------------------------------------------------------------------------------ 3. offline calls in between
def _offline_between(names):
    torch = _torch()
    for name in names:
        eng = _engine(name)
        x = _signal(_rows(name), 800)
        want = _run(eng, x)
        clip = torch.from_numpy(np.ascontiguousarray(_signal(_rows(name), 970, MS))).cuda()
        long_clip = torch.from_numpy(np.ascontiguousarray(_signal(_rows(name), 980, 9000))).cuda()
        snap = StreamSnapshot()

        def between(k):
            eng.stream_save(snap)
            eng.enhance_batch(clip)
            if k % 2:
                eng.enhance_long(long_clip, max_chunk_frames=6)         # ends the stream
                with pytest.raises(EngineError, match='without se_stream_begin'):
                    eng.stream_push(clip[:, :160].contiguous())
                eng._stream_batch = x.shape[0]
            eng.stream_restore(snap)
        got = _run(eng, x, between=between)
        snap.close()
        assert all(np.isfinite(o).all() for o in got), name
        _same(got, want, name)


def test_offline_calls_between_save_and_restore():
    _offline_between(['crn', 'dccrn', 'ctsnet_new'])


def test_offline_calls_between_save_and_restore_with_a_poisoned_arena():
    """SE_ARENA_POISON=1 (read once per process: a child process): nothing a resumed stream reads comes from the arena"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = ("import sys; sys.path[:0] = [sys.argv[1], sys.argv[1] + '/tests']\n"
              "import test_gpu_stream_state as t\n"
              "t._offline_between(['crn', 'dccrn', 'ctsnet_new'])\nprint('STATE-POISON-OK')\n")
    r = subprocess.run([sys.executable, '-c', script, root], env=dict(os.environ, SE_ARENA_POISON='1'), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and 'STATE-POISON-OK' in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


# ------------------------------------------------------------------------------------------------ 4. running scale, sliding
@pytest.mark.parametrize('name', ['crn', 'dccrn', 'g2net_new'])
def test_running_scale_stream(name):
    eng = _engine(name)
    want = _reference(name, running=True)
    snap = StreamSnapshot()

    def between(k):
        eng.stream_save(snap)
        _other_stream(eng, name)
        eng.stream_restore(snap)
    got = _run(eng, _signal(_rows(name), 800), running=True, between=between)
    snap.close()
    _same(got, want, name)


@pytest.mark.parametrize('name', ['crn', 'dccrn_snr', 'taylorsenet_new'])
def test_sliding_stream_saved_after_a_slide(name):
    """3 x max_samples through a window of max_samples + n_fft + hop: the window has slid (w0 > 0) when the stream is parked"""
    eng = _engine(name, 'sliding')
    B = _rows(name)
    x = _signal(B, 820, 3 * MS)
    pushes = [3000, 2999, 1, 2500, 3500]
    want = _run(eng, x, pushes)
    snap = StreamSnapshot()

    def between(k):
        if k >= 1:                                        # 5999 samples and more have gone into a window of < 4700
            eng.stream_save(snap)
            _other_stream(eng, name)
            eng.stream_restore(snap)
    got = _run(eng, x, pushes, between=between)
    assert snap.nbytes > 0
    snap.close()
    _same(got, want, name)


# ------------------------------------------------------------------------------------------------ 5. time-slicing
@pytest.mark.parametrize('name', ['crn', 'g2net_new'])
def test_two_groups_alternate_on_one_engine(name):
    torch = _torch()
    eng = _engine(name)
    B = _rows(name)
    xs = [_signal(B, 800), _signal(B, 900)]
    wants = [_reference(name), tuple(_run(eng, xs[1]))]
    pieces = [_pieces(x, PUSHES) for x in xs]
    snaps = [StreamSnapshot(), StreamSnapshot()]
    for g in range(2):                                    # both groups begin, neither has pushed
        _begin(eng, B)
        eng.stream_save(snaps[g])
    gots, marks = [[], []], []
    for k in range(len(PUSHES)):
        for g in range(2):
            eng.stream_restore(snaps[g])
            gots[g].append(eng.stream_push(pieces[g][k]).cpu().numpy())
            eng.stream_save(snaps[g])
        torch.cuda.synchronize()
        marks.append((snaps[0].nbytes, snaps[1].nbytes, torch.cuda.mem_get_info()[0]))
    for g in range(2):
        eng.stream_restore(snaps[g])
        gots[g].append(eng.stream_flush().cpu().numpy())
    for g in range(2):
        _same(gots[g], wants[g], (name, 'group', g))
    print(name, 'nbytes, nbytes, free device memory after every round:', marks)
    assert len(set(marks[1:])) == 1, marks               # after the first round nothing is allocated or released
    for s in snaps:
        s.close()


# ------------------------------------------------------------------------------------------------ 6. no disturbance, forking
@pytest.mark.parametrize('name', ['crn', 'ctsnet_new'])
def test_a_save_does_not_disturb_and_a_snapshot_forks(name):
    eng = _engine(name)
    want = _reference(name)
    x = _signal(_rows(name), 800)
    snaps = {}
    got = _run(eng, x, between=lambda k: snaps.__setitem__(k, eng.stream_save(snaps.get(k - 2))) if k in (1, 3) else eng.stream_save().close())
    _same(got, want, (name, 'saved after every call'))
    assert snaps[3] is snaps[1]                           # the object given was reused
    pieces = _pieces(x, PUSHES)
    for again in range(2):                                # the same snapshot, twice: the same continuation
        eng.stream_restore(snaps[3])
        tail = [eng.stream_push(p).cpu().numpy() for p in pieces[4:]] + [eng.stream_flush().cpu().numpy()]
        _same(tail, want[4:], (name, 'fork', again))
    snaps[3].close()


# ------------------------------------------------------------------------------------------------ 7. through host memory
@pytest.mark.parametrize('name', ['crn', 'dccrn', 'g2net_new'])
def test_to_bytes_from_bytes_round_trip(name):
    eng = _engine(name)
    want = _reference(name)
    images = []

    def between(k):
        with eng.stream_save() as snap:
            images.append(snap.to_bytes())
        _other_stream(eng, name)
        with StreamSnapshot.from_bytes(images[-1]) as back:
            assert back.batch == _rows(name) and back.to_bytes() == images[-1]
            eng.stream_restore(back)
    got = _run(eng, _signal(_rows(name), 800), between=between)
    _same(got, want, name)
    assert len(images[0]) < len(images[-1]) + 4 * _rows(name) * 700       # compact: the window part is the live samples only


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_leave_the_running_stream_as_it_was():
    eng = _engine('crn')
    want = _reference('crn')
    x = _signal(2, 800)
    idle = _make('crn', 2, MS).engine
    with pytest.raises(EngineError, match='stream_save without stream_begin'):
        idle.stream_save()
    h = C.c_void_p()
    assert idle._lib.se_stream_state_create(C.byref(h)) == 0
    assert idle._lib.se_stream_save(idle._h, h, None) != 0 and b'se_stream_save without se_stream_begin' in idle._lib.se_last_error(idle._h)
    assert idle._lib.se_stream_state_bytes(h) == 0
    idle._lib.se_stream_state_destroy(h)
    idle.close()

    # snapshots the target has to refuse
    _begin(eng, 2)
    pieces = _pieces(x, PUSHES)
    for p in pieces[:2]:
        eng.stream_push(p)
    crn2 = eng.stream_save()
    gcrn = _engine('gcrn')
    _begin(gcrn, 2)
    gcrn.stream_push(pieces[0])
    other_model = gcrn.stream_save()
    dccrn_plain = _engine('dccrn')
    _begin(dccrn_plain, 2)
    dccrn_plain.stream_push(pieces[0])
    other_flags = dccrn_plain.stream_save()
    long_eng = _make('crn', 2, 8000).engine
    _begin(long_eng, 2)
    for p in _pieces(_signal(2, 820, 6000), [3000, 3000]):
        long_eng.stream_push(p)
    too_long = long_eng.stream_save()
    long_eng.close()
    empty = StreamSnapshot()

    small = _make('crn', 1, MS).engine
    causal = _engine('dccrn_snr')
    cases = [(eng, empty, 'empty'), (eng, other_model, 'model id'), (causal, other_flags, 'flags differ'),
             (small, crn2, 'exceeds max_batch'), (eng, too_long, 'more than max_samples')]
    for target, snap, reason in cases:
        B = 1 if target is small else 2
        xs = _signal(B, 800)
        ref = _run(target, xs)

        def between(k):
            with pytest.raises(EngineError, match=reason):
                target.stream_restore(snap)
        got = _run(target, xs, between=between)
        _same(got, ref, reason)
    small.close()
    _same(_run(eng, x), want, 'afterwards')
    for s in (crn2, other_model, other_flags, too_long, empty):
        s.close()


# ------------------------------------------------------------------------------------------------ 9. the copy kernel alone
def _probe():
    from se_amd import _lib
    lib = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), 'libse_stateprobe.so'))
    lib.sp_last_error.restype = C.c_char_p
    lib.sp_copy.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int,
                            C.c_long, C.c_long, C.c_long, C.c_long, C.POINTER(C.c_long)]
    return lib


@pytest.mark.parametrize('direction', ['save', 'restore'])
def test_copy_kernel_alone(direction):
    """20 flat segments of 0, 1, 3, 4, 5, 4099 ... floats at 16 B aligned AND at odd float offsets, and a window of 2 rows whose pitch
    (1003) and origin (column 5) are no multiples of 4 floats against compact rows: one launch, against numpy, guard words around
    every destination untouched."""
    torch = _torch()
    lib = _probe()
    tile = lib.sp_tile()
    lens = [0, 1, 3, 4, 5, 4099, 7, 0, tile, tile + 1, 2 * tile - 1, 16, 33, 2, 4099, 1, 64, 255, 257, 6]
    assert len(lens) > 16
    G = 8                                                  # guard floats on either side of every destination
    rng = np.random.default_rng(3)
    src_off, dst_off, so, do = [], [], 0, G
    for i, n in enumerate(lens):
        so += i % 3                                        # some sources start off 16 B alignment ...
        src_off.append(so)
        so += (n + 3) // 4 * 4
        dst_off.append(do + (1 if i % 5 == 4 else 0))      # ... and some destinations
        do += (n + 3) // 4 * 4 + 4 + 2 * G
    rows, wlen, pitch, origin = 2, 777, 1003, 5
    src = rng.standard_normal(so + 8).astype(np.float32)
    win_wide = rng.standard_normal(rows * pitch + 16).astype(np.float32)
    win_compact = rng.standard_normal(rows * wlen).astype(np.float32)
    dst0 = rng.standard_normal(do + G).astype(np.float32)
    if direction == 'save':                                # wide engine rows -> compact payload rows
        wsrc, wdst0 = win_wide, rng.standard_normal(rows * wlen + 2 * G).astype(np.float32)
        args = (origin, G, pitch, wlen)
    else:
        wsrc, wdst0 = win_compact, rng.standard_normal(rows * pitch + 16).astype(np.float32)
        args = (0, origin, wlen, pitch)
    d_src, d_dst = torch.from_numpy(src).cuda(), torch.from_numpy(dst0.copy()).cuda()
    d_wsrc, d_wdst = torch.from_numpy(wsrc).cuda(), torch.from_numpy(wdst0.copy()).cuda()
    n = len(lens)
    sp = (C.c_void_p * (n + 1))(*[d_src.data_ptr() + 4 * o for o in src_off], d_wsrc.data_ptr())
    dp = (C.c_void_p * (n + 1))(*[d_dst.data_ptr() + 4 * o for o in dst_off], d_wdst.data_ptr())
    tiles = C.c_long(0)
    rc = lib.sp_copy(sp, dp, (C.c_int * n)(*lens), n, 1, rows, wlen, args[0], args[1], args[2], args[3], C.byref(tiles))
    assert rc == 0, lib.sp_last_error()
    assert tiles.value == sum((m + tile - 1) // tile for m in lens) + rows * ((wlen + tile - 1) // tile)
    want = dst0.copy()
    for o_s, o_d, m in zip(src_off, dst_off, lens):
        want[o_d:o_d + m] = src[o_s:o_s + m]
    wwant = wdst0.copy()
    for r in range(rows):
        wwant[args[1] + r * args[3]:args[1] + r * args[3] + wlen] = wsrc[args[0] + r * args[2]:args[0] + r * args[2] + wlen]
    assert np.array_equal(d_dst.cpu().numpy(), want)       # every segment, and every word between two of them as it was
    assert np.array_equal(d_wdst.cpu().numpy(), wwant)
    assert not np.array_equal(want, dst0) and not np.array_equal(wwant, wdst0)
    # no segment at all, and a window alone
    assert lib.sp_copy(sp, dp, (C.c_int * n)(*lens), 0, 0, 0, 0, 0, 0, 0, 0, C.byref(tiles)) == 0 and tiles.value == 0
    assert np.array_equal(d_dst.cpu().numpy(), want)
