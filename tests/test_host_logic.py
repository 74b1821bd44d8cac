"""CPU: host-side logic - library symbols, WAV I/O, sharding + gather over gloo (world_size 2)."""
import os
import re

import numpy as np
import pytest
import torch

import se_amd
from se_amd import _lib, wavio, shard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, 'include', 'se_engine.h')).read()
    declared = set(re.findall(r'\b(se_[a-z0-9_]+)\s*\(', hdr))
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    lib = _lib.load()
    for s in declared:
        assert hasattr(lib, s), s
    assert lib.se_abi_version() == 5


def test_engine_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from se_amd.engine import Engine, EngineError
    with pytest.raises(EngineError):
        Engine('dccrn')


def test_wav_roundtrip(tmp_path):
    rng = np.random.default_rng(0)
    y = np.clip(0.3 * rng.standard_normal(1234), -1, 1)
    p = str(tmp_path / 'a.wav')
    wavio.write_wav_pcm16(p, y, 16000)
    x, fs = wavio.read_wav(p)
    assert fs == 16000 and x.shape == y.shape
    # written with libsndfile's 0x7FFF scale, read back with 1 / 0x8000: |y| / 32768 of level change + half an LSB of rounding
    assert np.max(np.abs(x - y)) <= (0.5 + np.abs(y).max()) / 32768 + 1e-12
    assert np.array_equal(wavio.pcm16_bytes(y), np.rint(y * 32767.0).astype('<i2'))
    wavio.write_wav_pcm16(p, np.array([2.0, -2.0, 0.0]), 16000)           # clipping like PCM_16
    x, _ = wavio.read_wav(p)
    assert x[0] == 32767 / 32768 and x[1] == -1.0 and x[2] == 0.0


def test_shard_ranges_cover():
    for n in (0, 1, 7, 256, 257):
        for w in (1, 2, 3, 8):
            spans = [shard.shard_range(n, r, w) for r in range(w)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            sizes = [b - a for a, b in spans]
            assert max(sizes) - min(sizes) <= 1


def _worker(rank, world, port, n_items, tmp):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    wav = torch.arange(n_items * 5, dtype=torch.float32).reshape(n_items, 5)
    out = shard.run_sharded(lambda x: x * 2.0 + 1.0, wav)
    if rank == 0:
        torch.save(out, os.path.join(tmp, 'out.pt'))
    else:
        assert out is None
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize('world,n_items', [(2, 6), (2, 7), (4, 8), (4, 11), (8, 16), (8, 21), (8, 5)])
def test_sharded_decode_gather_gloo(tmp_path, world, n_items):
    """The N > 1 path of bench.py / decode: contiguous utterance shards, gather to rank 0 - even and uneven shards at 2, 4 and
    8 ranks (the driver's scaling run launches N = 1, 2, 4, 8), and fewer items than ranks (empty shards)."""
    import torch.multiprocessing as mp
    port = 29500 + (os.getpid() % 1000) + 3 * n_items + world
    mp.spawn(_worker, args=(world, port, n_items, str(tmp_path)), nprocs=world, join=True)
    out = torch.load(os.path.join(str(tmp_path), 'out.pt'))
    ref = torch.arange(n_items * 5, dtype=torch.float32).reshape(n_items, 5) * 2.0 + 1.0
    assert torch.equal(out, ref)


def _pipe_worker(rank, world, port, tmp):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    pipe = shard.GatherPipe(3, 4, torch.device('cpu'))
    for k in range(5):                                   # 5 batches through 2 send slots: slot reuse + async overlap
        out = pipe.slot()
        out.copy_(torch.full((3, 4), float(100 * k + rank)))
        pipe.submit()
    rows = pipe.finish()
    if rank == 0:
        torch.save(torch.stack(rows), os.path.join(tmp, 'pipe.pt'))
    else:
        assert rows is None
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize('world', [2, 4, 8])
def test_gather_pipe_gloo(tmp_path, world):
    """bench.py's steady-state gather (double-buffered, asynchronous; 5 batches, so both send slots wrap twice): rank 0 holds
    every rank's rows of the last batch - at the 2, 4 and 8 ranks of the driver's scaling run."""
    import torch.multiprocessing as mp
    port = 30500 + (os.getpid() % 1000) + world
    mp.spawn(_pipe_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    rows = torch.load(os.path.join(str(tmp_path), 'pipe.pt'))
    assert rows.shape == (world, 3, 4)
    for r in range(world):
        assert torch.equal(rows[r], torch.full((3, 4), 400.0 + r))


def test_decode_driver_batch_plan():
    """se_amd/decode.py:plan_batches - ragged: sorted runs bounded by count and padded size; not ragged: equal lengths."""
    from se_amd.decode import plan_batches
    lens = [5000, 3210, 4444, 6100, 3999, 5001, 4800, 3210]
    b = plan_batches(lens, 3, 10 ** 9, True)
    assert sorted(i for g in b for i in g) == list(range(len(lens))) and max(len(g) for g in b) <= 3 and len(b) == 3
    flat = [lens[i] for g in b for i in g]
    assert flat == sorted(lens)                                  # runs of neighbouring lengths: little padding
    b = plan_batches(lens, 8, 2 * 5001, True)                    # padded-size budget: count x longest <= 10 002
    assert all(len(g) * max(lens[i] for i in g) <= 10002 for g in b)
    b = plan_batches([70000], 4, 64000, True)                    # a clip longer than the budget still gets its own call
    assert b == [[0]]
    b = plan_batches(lens, 8, 10 ** 9, False)                    # non-ragged plan: only exactly equal lengths share a call
    assert sorted(map(sorted, b)) == sorted([[1, 7], [0], [2], [3], [4], [5], [6]])


def test_decode_driver_padding_cap_and_rank_shards():
    """the plan's padding stays ~15 % for any max_batch (it was 42 % at 256 on a VoiceBank+DEMAND-like
    length distribution), and the ranks get disjoint, complete, equally loaded shares of the clip list."""
    from se_amd.decode import plan_batches, shard_clips
    rng = np.random.default_rng(2024)
    lens = [int(v * 16000) for v in np.clip(np.exp(rng.normal(np.log(2.6), 0.45, 824)), 1.2, 9.8)]
    for mb in (16, 64, 256):
        plan = plan_batches(lens, mb, mb * 64000, True)
        assert sorted(i for b in plan for i in b) == list(range(len(lens)))
        for b in plan:                                         # every call by itself: <= 15 % of its frames are padding
            padded, use = len(b) * max(lens[i] for i in b), sum(lens[i] for i in b)
            assert len(b) <= mb and padded <= max(mb * 64000, max(lens[i] for i in b)) and (padded - use) <= 0.15 * padded + 1
    loose = plan_batches(lens, 256, 256 * 64000, True, max_pad=1.0)
    waste = lambda plan: sum(len(b) * max(lens[i] for i in b) for b in plan) / sum(lens) - 1.0
    assert waste(loose) > 0.30 > 0.18 > waste(plan_batches(lens, 256, 256 * 64000, True))
    world = 8
    shares = [shard_clips(lens, r, world) for r in range(world)]
    assert sorted(i for s in shares for i in s) == list(range(len(lens)))
    frames = [sum(lens[i] for i in s) for s in shares]
    assert max(len(s) for s in shares) - min(len(s) for s in shares) <= 1
    assert max(frames) < 1.03 * min(frames)                    # same length distribution on every rank


def test_bench_roofline_inputs():
    """bench.py's algorithmic figures: 53.4 GFLOP per DCCRN utterance is SURVEY 8(d)'s number; the algorithmic HBM bytes of
    the 20 tap-table GEMM launches of a step are what `roofline.traffic` (PMC) is compared with; the committed PMC
    summary carries the traffic figure bench.py reports."""
    import sys
    sys.path.insert(0, ROOT)
    import bench
    rd, wr = bench.dccrn_conv_bytes(256)
    per_launch = (rd + wr) / 1e9 / 20
    assert 3.8 < per_launch < 4.0, per_launch
    assert rd > wr > 0
    pmc = bench.pmc_traffic()
    # round 5: 11 plain GEMM launches; per three-product conv / parity class k1 alone, then k2 and k3 with the combine epilogue -
    # as two launches where the layer's output has a sum plane (k3's epilogue writes it: encoder layers 4-6, decoder layers 1-2:
    # 7 x 3 = 21), as one grouped launch else (decoder layer 3: 2 x 2 = 4); 2 sum passes behind block-form layers - which the
    # engine's profiler and tools/pmc_summary.py count in the family
    assert pmc is not None and pmc["launches_per_step"] == 38.0
    # the counters were taken on THESE kernel sources (bench.py quotes them only then: `traffic_stale`)
    assert pmc['csrc_sha16'] == bench.dccrn_csrc_sha16() and not pmc['stale']
    # measured traffic can only exceed the algorithmic bytes; with the block form everywhere it was 1.14x (halo rows / columns
    # of neighbouring tiles).  The three-product layers write and re-read their k1 tensor and the x_r + x_i planes:
    # 1.56x per step, the price of 16 % fewer matrix flops at 1.3 TB/s of the 8 TB/s roof
    step_traffic = pmc['traffic_GB_per_launch'] * pmc['launches_per_step']
    assert (rd + wr) / 1e9 <= step_traffic < 1.75 * (rd + wr) / 1e9
    assert 0.80 * 256 * 53.4e-3 < pmc['executed_mfma_tflop_per_step'] < 0.90 * 256 * 53.4e-3
    assert bench.DCCRN_GFLOP_PER_UTT == 53.4 and bench.F32_MFMA_PEAK_TFLOPS == 157.3


def test_bench_dump_outputs_caps_size_with_a_fixed_row_sample(tmp_path):
    """bench.py --dump-outputs: a last step that fits the budget is written whole, in rank order; a larger one as the same
    seeded sample of whole rows, ascending, on every call - so that two builds can be compared output for output."""
    import sys
    sys.path.insert(0, ROOT)
    import bench
    small = [torch.arange(6 * 5, dtype=torch.float32).view(6, 5), -torch.ones(2, 5)]
    bench.dump_outputs(str(tmp_path / 's'), small)
    y = np.load(tmp_path / 's' / 'enhanced.npy')
    assert y.dtype == np.float32 and np.array_equal(y, torch.cat(small).numpy())
    n = 256
    big = [torch.arange(n, dtype=torch.float32)[:, None].expand(n, 64000).contiguous()]
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), big)
    a, b = (np.load(tmp_path / d / 'enhanced.npy') for d in ('a', 'b'))
    assert a.nbytes <= bench.DUMP_BUDGET_BYTES < 64e6 and a.shape[1] == 64000 and a.shape[0] > n // 2
    rows = a[:, 0]
    assert np.array_equal(a, b) and np.all(np.diff(rows) > 0) and np.array_equal(a, rows[:, None] * np.ones((1, 64000)))
