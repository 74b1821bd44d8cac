"""Record what gemmconv's tile selection does on the cases of tests/test_gpu_gemmconv_geometry.py, one JSON line per case: the case
key, the gcp_info facts of each plan, the launch records and - where the probe library has gc_set_select_log - the GCSelIn of
every gc_launch call.

    SE_GCPROBE_LIB=<probe of the parent build> python tools/gc_select_record.py record parent.jsonl
    python tools/gc_select_record.py record new.jsonl
    python tools/gc_select_record.py join parent.jsonl new.jsonl tests/golden/gc_select_parent.jsonl.gz

`join` writes the fixture tests/test_gc_select_host.py and tests/test_gpu_gc_select_replay.py read (gzip'ed JSON lines: 265 KB of
integers as text, 9 KB packed): per case the GCSelIn of the new build with the facts and records of the PARENT build.  A case whose two builds dispatch a different number of launches is an
error, not something to drop.  Each `record` run is its own process; nothing is compared with float64 here (the geometry test does)."""
import ctypes as C
import gzip
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import test_gpu_gemmconv_geometry as G      # noqa: E402


def cases():
    """(group, shape name, prelu, B, T, nrm, stats, tlen or None): the launches of the geometry test's cases, in its order.
    Needs the probe (the batch points depend on each plan's tile)."""
    for name in sorted(G.SHAPES):       # test_layer_matches_float64_at_threshold_batches
        sh = G.SHAPES[name]
        probe = G.probe_for(name, prelu=not sh['nrm'])[0]
        stats = bool(probe.plans[0]['stats_ok']) and sh['nrm']
        for T in G.T_SWEEP:
            for B in sorted({b for pl in probe.plans for b in G.b_points(pl, sh, T)}):
                yield ('sweep', name, not sh['nrm'], B, T, sh['nrm'], stats, None)
    for name in ('g2net_level', 'taylor_level'):        # test_flattened_tiles_by_units_per_row
        for nrm in (True, False):
            for kind, upr in G.FLAT_CASES:
                T = 32 * upr - 3 if upr > 1 else 29
                B = G.flat_batch(G.SHAPES[name], 8 if kind == 'wide' else 4, T, nrm)
                yield ('flat', name, not nrm, B, T, nrm, False, None)
    sh = G.SHAPES['g2net_level']
    for upr in (3, 4, 13):      # test_flattened_tiles_with_ragged_rows
        T = 32 * upr
        B = -(-G.WIDE_MIN // (sh['Fout'] * -(-T // 128))) + 1
        tlen = np.random.default_rng(upr).integers(max(1, T - 40), T + 1, B)
        tlen[0] = T
        yield ('ragged', 'g2net_level', False, B, T, True, True, [int(t) for t in tlen])
    for T in (256, 500):        # test_plain_wide_tiles
        for name in ('g2net_level', 'taylor_level'):
            B = -(-G.WIDE_MIN // (G.SHAPES[name]['Fout'] * -(-T // 128)))
            yield ('wide', name, False, B, T, True, True, None)


def case_key(c):
    return list(c[:7]) + [c[7] is not None]


def launch(probe, sh, B, T, nrm, stats, tlen):
    """One launch of the layer on sources laid out and registered as the geometry test's run_case does it (the values do not
    matter here).  Returns (launch records, GCSelIn rows or None)."""
    import torch
    lib = probe.lib()
    dev = 'cuda'
    C0 = sh['Cin'] if sh['c0'] < 0 else sh['c0']
    chans = [C0] + ([sh['Cin'] - C0] if C0 < sh['Cin'] else [])
    bufs = [torch.zeros(B * Cn * sh['Fin'] * T + 4096, device=dev) for Cn in chans]
    xs = [b[:B * Cn * sh['Fin'] * T].view(B, Cn, sh['Fin'], T) for b, Cn in zip(bufs, chans)]
    nrms = [torch.ones((B, Cn, 4), device=dev) if nrm else None for Cn in chans]
    dst = torch.zeros((B, sh['M'], sh['Fout'], T), device=dev)
    st = torch.zeros((B, sh['M'], sh['Fout'], -(-T // 32), 2), device=dev) if stats else None
    tl = None if tlen is None else torch.as_tensor(tlen, dtype=torch.int32, device=dev)
    for b in bufs:
        lib.gcp_register_overread(b.data_ptr(), b.numel() * 4)
    try:
        recs = probe.run(xs, nrms, dst, sh['Fin'], sh['Fout'], B, T, T, st, tl)
    finally:
        for b in bufs:
            lib.gcp_unregister_overread(b.data_ptr())
    sel = None
    if hasattr(lib, 'gcp_select_get'):
        lib.gcp_select_get.argtypes = [C.c_int, C.POINTER(C.c_longlong), C.c_int]
        sel = []
        for i in range(lib.gcp_select_count()):
            out = (C.c_longlong * 128)()
            n = lib.gcp_select_get(i, out, 128)
            assert n > 0
            sel.append(list(out[:n]))
    return [[r[k] for k in G.Probe.REC] for r in recs], sel


def run_case(c):
    _, name, prelu, B, T, nrm, stats, tlen = c
    probe = G.probe_for(name, prelu=prelu)[0]
    recs, sel = launch(probe, G.SHAPES[name], B, T, nrm, stats, tlen)
    line = dict(key=case_key(c), facts=[[pl[k] for k in G.Probe.FACTS] for pl in probe.plans], recs=recs)
    if tlen is not None:
        line['tlen'] = tlen
    if sel is not None:
        line['selin'] = sel
    return line


def record(path):
    with open(path, 'w') as f:
        for c in cases():
            f.write(json.dumps(run_case(c), separators=(',', ':')) + '\n')
            f.flush()
    print('recorded', path)


def join(parent, new, out):
    load = lambda p: [json.loads(l) for l in open(p)]
    a, b = load(parent), load(new)
    assert [x['key'] for x in a] == [x['key'] for x in b], 'the two runs recorded different cases'
    with gzip.GzipFile(out, 'wb', 9, mtime=0) as f:
        for x, y in zip(a, b):
            assert len(x['recs']) == len(y['recs']), f"{x['key']}: {len(x['recs'])} launches in the parent, {len(y['recs'])} now"
            line = dict(key=x['key'], facts=x['facts'], recs=x['recs'], selin=y['selin'])
            f.write((json.dumps(line, separators=(',', ':')) + '\n').encode())
    print('joined', len(a), 'cases ->', out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    if sys.argv[1] == 'record':
        record(sys.argv[2])
    else:
        join(*sys.argv[2:5])
