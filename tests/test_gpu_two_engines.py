"""GPU: two pieces of the library in flight at once on two hipStreams, driven by ONE host thread.

Contract (include/se_engine.h): whatever a handle returns for a call made alone - the device idle before and after - it returns
bit for bit while another handle's call is in flight on another stream, and se_resample likewise for two calls of two ratios.  The
reference is always the same engine's (the same call's) own solo result, computed first in this process; a concurrent run is
never a reference.

Making "in flight at once" real: an 8000-sample decode is bound by launch submission, so two calls made one after the other
hardly overlap by themselves.  Every round therefore parks both caller streams behind an event that a device-side sleep of
GATE_MS on a third stream releases, enqueues both calls and then synchronises - all of both calls is queued before either
starts.  Begin / end events on both streams give the two intervals; a case in which NO round's intervals overlap has proved
nothing and fails.  Rounds are fixed (ROUNDS), nothing is retried, a mismatch is an ordinary failure.

What the cases are after:
  * the scratch of work a model forks onto the PROCESS-wide auxiliary streams, whose address a captured hipGraph keeps: replayed
    nodes do not run on the stream they were captured on, so nothing orders them against another engine's use of the same slot;
  * se_resample's tables, once rewritten in place by every call of a new ratio behind a wait for the caller's stream alone.
The timing cases can pass by luck; test_captured_scratch_is_the_engines_own reads the record of scratch hand-outs instead and
needs none.

SE_TWO_ENGINES_REPORT=<file>: one JSON line per case (overlap fractions, rounds that differed) is appended there - the figures of
profiles/two_engines.md."""
import ctypes as C
import gc
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import se_amd  # noqa: F401
from se_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'sixty-years-of-frequency-domain-monaural-speech-enhancement_amd')
SCRATCH_PROBE = os.environ.get('SE_SCRATCHPROBE_LIB') or os.path.join(PKG, 'libse_scratchprobe.so')   # (as SE_ENGINE_LIB: A/B a build)

L = 8000                 # max_samples of every engine here: 51 frames
ROUNDS = 8
GATE_MS = 40.0           # the device-side sleep both streams wait behind; bounded by GATE_MAX_MS in every round
GATE_MAX_MS = 90.0

_state = {}


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _report(rec):
    print('two_engines', json.dumps(rec))
    path = os.environ.get('SE_TWO_ENGINES_REPORT')
    if path:
        with open(path, 'a') as f:
            f.write(json.dumps(rec) + '\n')


def _streams():
    """three caller streams (a round takes two of them, in turn: whatever the runtime's mapping of streams onto hardware queues,
    not every pair shares one) and the gate's stream"""
    torch = _torch()
    if 'streams' not in _state:
        _state['streams'] = [torch.cuda.Stream() for _ in range(3)]
        _state['gate'] = torch.cuda.Stream()
    return _state['streams'], _state['gate']


def _gate_cycles():
    """torch.cuda._sleep counts device clock ticks: measured once, so that the gate is GATE_MS whatever that clock is"""
    torch = _torch()
    if 'cycles' not in _state:
        def timed(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            torch.cuda._sleep(n)
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b)
        timed(1000)                              # (the first launch loads the kernel)
        n, ms = 100_000, 0.0
        for _ in range(5):                       # at most 5 probes, each 10 x the last, until one lasts a millisecond
            ms = timed(n)
            if ms >= 1.0:
                break
            n *= 10
        assert 1.0 <= ms < GATE_MAX_MS, (n, ms)
        n = int(n * GATE_MS / ms)
        ms = timed(n)
        assert GATE_MS / 2 < ms < GATE_MAX_MS, (n, ms)
        _state['cycles'] = n
    return _state['cycles']


class _Side:
    """one engine with one input: its solo result is taken on the third call of the shape (a graph engine replays from there
    on), then the shape is run once on every caller stream so that the gated phase allocates nothing"""

    def __init__(self, name, seed, batch, graphs, clip0, max_batch=None):
        torch = _torch()
        from se_amd import models_new  # noqa: F401
        from se_amd.models import MODEL_CLASSES, CTSNet
        kw = dict(max_batch=max_batch or batch, max_samples=L, graphs=graphs)
        self.m = CTSNet(**kw).load_synthetic(seed, seed + 1) if name == 'ctsnet' else MODEL_CLASSES[name](**kw).load_synthetic(seed)
        self.tag = f"{name}{'/graph' if graphs else ''}[{batch}]"
        self.x = torch.from_numpy(np.stack([synth.synth_clip(clip0 + b, 'speech' if b % 2 == 0 else 'white', L)
                                            for b in range(batch)])).cuda()
        self.out = torch.empty((batch, self.m.engine.output_samples(L)), dtype=torch.float32, device='cuda')
        self.want = None

    def run(self):
        self.m.engine.enhance_batch(self.x, out=self.out)

    def solo(self):
        torch = _torch()
        torch.cuda.synchronize()
        self.out.fill_(float('nan'))
        torch.cuda.synchronize()
        self.run()
        torch.cuda.synchronize()
        return self.out.clone()

    def warm(self):
        torch = _torch()
        for _ in range(3):
            self.want = self.solo()
        assert bool(torch.isfinite(self.want).all()), self.tag
        for s in _streams()[0]:
            with torch.cuda.stream(s):
                assert torch.equal(self.solo(), self.want), (self.tag, 'solo on another stream')
        return self


def _gated_round(a, b, sa, sb):
    """both calls queued behind the gate -> (overlap fraction of the two intervals, a differed, b differed, all was queued before
    the gate opened, gate ms)"""
    torch = _torch()
    _, sg = _streams()
    ev = {k: torch.cuda.Event(enable_timing=True) for k in ('ref', 'gate', 'a0', 'a1', 'b0', 'b1')}
    for side in (a, b):
        side.out.fill_(float('nan'))
    torch.cuda.synchronize()
    with torch.cuda.stream(sg):
        ev['ref'].record()
        torch.cuda._sleep(_gate_cycles())
        ev['gate'].record()
    for side, st, k in ((a, sa, 'a'), (b, sb, 'b')):
        with torch.cuda.stream(st):
            st.wait_event(ev['gate'])
            ev[k + '0'].record()
            side.run()
            ev[k + '1'].record()
    queued = not ev['gate'].query()
    torch.cuda.synchronize()
    t = {k: ev['ref'].elapsed_time(e) for k, e in ev.items() if k != 'ref'}
    assert GATE_MS / 2 < t['gate'] < GATE_MAX_MS, t
    both = min(t['a1'], t['b1']) - max(t['a0'], t['b0'])
    frac = max(0.0, both) / max(min(t['a1'] - t['a0'], t['b1'] - t['b0']), 1e-6)
    return frac, not torch.equal(a.out, a.want), not torch.equal(b.out, b.want), queued, t['gate']


def _fly(case, a, b):
    torch = _torch()
    streams, _ = _streams()
    _gate_cycles()
    a.warm()
    b.warm()
    rounds = [_gated_round(a, b, streams[r % 3], streams[(r + 1) % 3]) for r in range(ROUNDS)]
    # no state was damaged: each engine alone again
    after = [not torch.equal(s.solo(), s.want) for s in (a, b)]
    rec = {'case': case, 'a': a.tag, 'b': b.tag, 'overlap': [round(r[0], 3) for r in rounds], 'queued': [int(r[3]) for r in rounds],
           'rounds_a_differed': sum(r[1] for r in rounds), 'rounds_b_differed': sum(r[2] for r in rounds),
           'rounds_queued_before_release': sum(r[3] for r in rounds), 'gate_ms': round(max(r[4] for r in rounds), 1),
           'solo_after_differed': after}
    _report(rec)
    assert rec['rounds_a_differed'] == 0 and rec['rounds_b_differed'] == 0, rec
    assert after == [False, False], rec
    assert any(r[3] and r[0] > 0.0 for r in rounds), \
        ('no round had both calls queued behind the gate and then in flight at once: the case proved nothing', rec)


# (case, A: name, seed, batch, graphs; B: the same) - the models that fork offline but make no cooperative launch; ctsnet is the
# zoo's TCM network that stays on one stream offline.  Different weights and different clips on the two sides.
CASES = [
    ('eager_eager_same', ('taylorsenet', 19, 2, False), ('taylorsenet', 23, 3, False)),
    ('eager_eager_taylor_g2net', ('taylorsenet', 19, 4, False), ('g2net', 20, 2, False)),
    ('eager_eager_taylor_new_ctsnet', ('taylorsenet_new', 21, 2, False), ('ctsnet', 17, 3, False)),
    ('eager_eager_g2net_big', ('g2net', 20, 8, False), ('taylorsenet_new', 21, 5, False)),
    ('graph_eager_taylor', ('taylorsenet', 19, 2, True), ('taylorsenet', 23, 3, False)),
    ('graph_eager_g2net_taylor_new', ('g2net', 20, 3, True), ('taylorsenet_new', 21, 2, False)),
    ('graph_graph_taylor', ('taylorsenet', 19, 2, True), ('taylorsenet', 23, 2, True)),
    ('graph_graph_taylor_new_g2net', ('taylorsenet_new', 21, 3, True), ('g2net', 20, 2, True)),
]


@pytest.mark.parametrize('case,a,b', CASES, ids=[c[0] for c in CASES])
def test_two_engines_in_flight_equal_each_one_alone(case, a, b):
    sa = _Side(a[0], a[1], a[2], a[3], clip0=500)
    sb = _Side(b[0], b[1], b[2], b[3], clip0=600)
    _fly(case, sa, sb)


def test_scratch_growth_under_flight_keeps_the_running_call():
    """The retire rule of the scratch pool (csrc/common.h) with two engines: A's call of a small shape is enqueued, then B's FIRST
    call of a larger batch outgrows the slots both engines' forked work shares, then A runs again.  Ungated (the growth is a
    hipMalloc); both of A's results must be A's solo result.  B's in-flight first call is held to the solo result B gives
    afterwards - asking B first would grow the slots before the flight."""
    torch = _torch()
    gc.collect()                                  # engines of earlier tests: the device's last engine takes the slots with it
    streams, _ = _streams()
    a = _Side('taylorsenet', 19, 2, False, clip0=500).warm()
    b = _Side('taylorsenet', 23, 8, False, clip0=600)
    out2 = torch.empty_like(a.out)
    differed = []
    torch.cuda.synchronize()
    with torch.cuda.stream(streams[0]):
        a.run()
    with torch.cuda.stream(streams[1]):
        b.run()
    with torch.cuda.stream(streams[0]):
        a.m.engine.enhance_batch(a.x, out=out2)
    torch.cuda.synchronize()
    differed += [not torch.equal(a.out, a.want), not torch.equal(out2, a.want)]
    got_b = b.out.clone()
    differed.append(not torch.equal(b.solo(), got_b))
    differed.append(not torch.equal(a.solo(), a.want))
    _report({'case': 'scratch_growth_under_flight', 'a': a.tag, 'b': b.tag, 'differed': differed})
    assert differed == [False] * 4, differed


# ---- the deterministic witness: the record of scratch hand-outs, read in a process that loads the probe build as the engine

WITNESS = r"""
import ctypes as C, json, sys
import numpy as np, torch
sys.path.insert(0, %(root)r)
import se_amd
from se_amd import synth, _lib, models_new
from se_amd.models import MODEL_CLASSES
lib = _lib.load()
lib.scp_get.argtypes = [C.c_int, C.POINTER(C.c_longlong)]
x = torch.from_numpy(np.stack([synth.synth_clip(500 + b, 'speech', 8000) for b in range(2)])).cuda()
engines = [(name, graphs, MODEL_CLASSES[name](max_batch=2, max_samples=8000, graphs=graphs).load_synthetic(seed))
           for name, graphs, seed in %(engines)r]
marks = []
lib.scp_begin()
for name, graphs, m in engines:
    for _ in range(3):                    # eager warm-up, capture, first replay
        y = m.enhance_batch(x)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all())
    marks.append(lib.scp_count())
lib.scp_end()
recs, row = [], (C.c_longlong * 5)()
for i in range(lib.scp_count()):
    assert lib.scp_get(i, row) == 0
    recs.append(list(row))
print('WITNESS ' + json.dumps({'marks': marks, 'recs': recs}))
"""


def _witness(engines):
    code = WITNESS % {'root': ROOT, 'engines': engines}
    env = dict(os.environ, SE_ENGINE_LIB=SCRATCH_PROBE, SE_GRAPH_DEBUG='1')
    r = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('WITNESS ')][-1]
    return json.loads(line[len('WITNESS '):]), r.stderr


def test_captured_scratch_is_the_engines_own():
    """Three engines decode one shape three times each in one process - TaylorSENet with graphs (its separate encoder is captured
    with its fork), TaylorSENet eager (the same fork, on the process-wide auxiliary stream), G2Net with graphs - under the record
    of every device_scratch hand-out: (purpose, key of the slot, stream, buffer, was the stream capturing).  The invariant
    (DESIGN.md 4.5): a buffer handed out while its stream was capturing - its address is in a graph's kernel nodes from then on -
    is never handed to another engine, and its slot is not keyed by a stream that more than one engine works on.  Also what the
    graph cases above rely on: both graph engines really captured (SE_GRAPH_DEBUG), and TaylorSENet's capture really held forked
    work - hand-outs on two different capturing streams."""
    engines = [('taylorsenet', True, 19), ('taylorsenet', False, 23), ('g2net', True, 20)]
    w, err = _witness(engines)
    assert err.count('se_graph: captured') == 2 and 'se_graph: capture failed' not in err, err[-2000:]
    marks, recs = w['marks'], w['recs']
    seg = [recs[lo:hi] for lo, hi in zip([0] + marks[:-1], marks)]
    assert all(seg), [len(s) for s in seg]
    streams_of = [{r[2] for r in s} for s in seg]
    shared = {st for i, si in enumerate(streams_of) for j, sj in enumerate(streams_of) if i != j for st in si & sj}
    assert shared, 'the forking engines no longer share an auxiliary stream: the witness watches nothing'
    cap0 = [r for r in seg[0] if r[4]]
    assert len({r[2] for r in cap0}) >= 2, 'TaylorSENet captured no forked work'
    bad = []
    for i, s in enumerate(seg):
        baked = {r[3] for r in s if r[4]}
        for j, other in enumerate(seg):
            if j != i:
                bad += [('buffer of engine %d captured, handed to engine %d' % (i, j), r) for r in other if r[3] in baked]
        bad += [('captured under a process-wide key', r) for r in s if r[4] and r[1] in shared]
    _report({'case': 'witness', 'hand_outs': [len(s) for s in seg], 'captured_hand_outs': [sum(r[4] for r in s) for s in seg],
             'violations': len(bad)})
    assert not bad, bad[:6]


# ---- se_resample on two streams

# The first call's row: 2^25 input samples, the smallest power of two at which resample_kernel runs for more than 3 ms on an MI355X
# at both of the first calls' ratios (3.7 ms at 48 kHz, 5.9 ms at 44.1 kHz; 2^24: 1.9 and 3.0 ms - profiles/two_engines.md has the
# sweep).  The second call is made - and on the parent rewrote the tables - while that kernel is queued behind the gate.
RS_LONG = 1 << 25
RS_SHORT = 1 << 20
RS_CASES = [((48000, 16000, RS_LONG), (44100, 16000, 1 << 22)),        # integer decimation first: only the filter table is shared
            ((44100, 16000, RS_LONG), (22050, 16000, RS_SHORT))]       # the second row is shorter: the position table does not grow
ORACLE_BOUND = 2e-7      # tests/test_resample.py::test_hip_resampler_matches_oracle: fp32 output of a float64 accumulation


def _se_resample(x, sr_in, sr_out, y):
    torch = _torch()
    from se_amd import _lib
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    n = x.shape[0]
    rc = lib.se_resample(C.c_void_p(x.data_ptr()), n, 1, n, int(sr_in), int(sr_out), C.c_void_p(y.data_ptr()), y.shape[0], st)
    assert rc == 0, lib.se_last_error(None).decode()


def _oracle_places(n_out, n_calc):
    """output samples the float64 oracle is read at (its loop is a Python step per sample): both ends, the fix_length tail, and
    blocks spread over the row"""
    blocks = [np.arange(0, 48), np.arange(n_calc - 48, n_calc)] + [np.arange(k, k + 16) for k in np.linspace(48, n_calc - 64, 9).astype(int)]
    return np.unique(np.concatenate(blocks))


@pytest.mark.parametrize('first,second', RS_CASES, ids=['48k_then_44k1', '44k1_then_22k05'])
def test_se_resample_on_two_streams_equals_each_call_alone(first, second):
    torch = _torch()
    from se_amd import resample as HR
    from oracle import resample as R
    streams, sg = _streams()
    _gate_cycles()
    g = torch.Generator(device='cuda').manual_seed(5)
    calls = []
    for sr_in, sr_out, n in (first, second):
        x = 0.1 * torch.randn(n, generator=g, device='cuda', dtype=torch.float32)
        y = torch.empty(HR.resample_samples(n, sr_in, sr_out), dtype=torch.float32, device='cuda')
        calls.append([sr_in, sr_out, x, y, None])
    for c in calls:                                # each call alone, the device idle before and after
        torch.cuda.synchronize()
        _se_resample(c[2], c[0], c[1], c[3])
        torch.cuda.synchronize()
        c[4] = c[3].clone()
    differed, in_flight = [], []
    for rnd in range(3):
        for c in calls:
            c[3].fill_(float('nan'))
        done = torch.cuda.Event()
        torch.cuda.synchronize()
        with torch.cuda.stream(sg):
            torch.cuda._sleep(_gate_cycles())
            gate = torch.cuda.Event()
            gate.record()
        with torch.cuda.stream(streams[0]):
            streams[0].wait_event(gate)
            _se_resample(calls[0][2], calls[0][0], calls[0][1], calls[0][3])
            done.record()
        with torch.cuda.stream(streams[1]):        # not gated: whatever this call waits for, it is not the first call
            _se_resample(calls[1][2], calls[1][0], calls[1][1], calls[1][3])
        in_flight.append(not done.query())
        torch.cuda.synchronize()
        differed.append([not torch.equal(c[3], c[4]) for c in calls])
    _report({'case': 'se_resample %s -> %s' % (first, second), 'differed': differed, 'first_call_in_flight': in_flight})
    assert all(in_flight), 'the first call had finished before the second was made: the case proved nothing'
    assert differed == [[False, False]] * 3, differed
    for sr_in, sr_out, x, y, want in calls:
        n = x.shape[0]
        n_calc = int(n * (float(sr_out) / sr_in))
        ts = _oracle_places(want.shape[0], n_calc)
        ref = R.resample_at(x.cpu().numpy().astype(np.float64), sr_in, sr_out, ts)
        got = want.cpu().numpy()
        assert np.abs(got[ts] - ref).max() < ORACLE_BOUND, (sr_in, np.abs(got[ts] - ref).max())
        assert not got[n_calc:].any()              # librosa's fix_length tail
