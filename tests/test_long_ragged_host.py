"""CPU: the host side of the windowed decode of long clips of different lengths (se_enhance_long_ragged) - the planner that groups
the clips above the driver's bound, the Python wrapper's refusals before the library is called, the binding, `--long-batch`."""
import random

import pytest

import se_amd  # noqa: F401
from se_amd import _lib, decode
from se_amd.engine import EngineError
from test_long_decode_host import _FakeCuda, _engine


def _pad_share(lens):
    return sum(max(lens) - n for n in lens) / (len(lens) * max(lens))


@pytest.mark.parametrize('long_batch,max_pad', [(2, 0.15), (4, 0.15), (8, 0.05), (64, 0.15), (3, 0.0)])
def test_groups_partition_the_clips_within_size_and_padding(long_batch, max_pad):
    rng = random.Random(7)
    lens = [rng.randrange(64001, 40 * 16000) for _ in range(41)] + [64001, 64001, 64001]      # (equal clips among them)
    groups = decode.plan_long_groups(lens, long_batch, max_pad)
    assert sorted(i for g in groups for i in g) == list(range(len(lens)))
    for g in groups:
        assert 1 <= len(g) <= long_batch
        assert _pad_share([lens[i] for i in g]) <= max_pad + 1e-12, (g, _pad_share([lens[i] for i in g]))
    # (sorted by length: a group is a run of the sorted order, so the cap costs as few calls as a greedy pass can)
    flat = [lens[i] for g in groups for i in g]
    assert flat == sorted(lens)
    if long_batch == 3 and max_pad == 0.0:
        assert [64001] * 3 in [[lens[i] for i in g] for g in groups]          # no padding allowed: only equal clips share a call


def test_one_row_per_call_keeps_the_order_given():
    lens = [90000, 70000, 80000, 70000]
    assert decode.plan_long_groups(lens, 1, 0.15) == [[0], [1], [2], [3]]
    assert decode.plan_long_groups(lens, 0, 0.15) == [[0], [1], [2], [3]]
    assert decode.plan_long_groups([], 4, 0.15) == []


def test_an_outlier_goes_alone():
    lens = [100000, 101000, 99000, 30 * 60 * 16000, 102000]                  # half an hour among clips of six seconds
    groups = decode.plan_long_groups(lens, 8, 0.15)
    assert [3] in groups and sorted(map(sorted, groups)) == [[0, 1, 2, 4], [3]]
    # the cap is on the group's padding share: a clip 15 % longer than three equal ones still joins them (a share of 9.8 %) ...
    assert decode.plan_long_groups([100000, 100000, 100000, 115000], 8, 0.15) == [[0, 1, 2, 3]]
    # ... one 30 % longer does not (17.3 %)
    assert decode.plan_long_groups([100000, 100000, 100000, 130000], 8, 0.15) == [[0, 1, 2], [3]]


@pytest.mark.parametrize('lengths,why', [
    ([9000], '1 lengths for a batch of 2'),
    ([9000, 9000, 9000], '3 lengths for a batch of 2'),
    ([], '0 lengths for a batch of 2'),
])
def test_enhance_long_ragged_refuses_a_lengths_list_of_another_size(lengths, why):
    with pytest.raises(EngineError, match=why):
        _engine().enhance_long_ragged(_FakeCuda((2, 9000), (9000, 1)), lengths)


@pytest.mark.parametrize('wav,lengths,kw,why', [
    (_FakeCuda((3, 9000), (9000, 1)), [9000] * 3, {}, 'max_batch'),
    (_FakeCuda((2, 9000), (9000, 1)), [9000, 9001], {}, 'outside rows of 9000'),
    (_FakeCuda((2, 9000), (9000, 1)), [9000, 0], {}, 'outside rows of 9000'),
    (_FakeCuda((2, 9000), (8000, 1)), [9000, 5000], {}, 'overlap'),
    (_FakeCuda((2, 9000), (9000, 2)), [9000, 5000], {}, 'unit inner stride'),
    (_FakeCuda((2, 9000), (9000, 1)), [9000, 5000], {'max_chunk_frames': -1}, 'max_chunk_frames'),
])
def test_enhance_long_ragged_refuses_bad_input_before_calling_the_library(wav, lengths, kw, why):
    with pytest.raises(EngineError, match=why):
        _engine().enhance_long_ragged(wav, lengths, **kw)


def test_model_wrappers_pass_enhance_long_ragged_through():
    from se_amd import models, models_new
    seen = []

    class _Eng:
        def enhance_long_ragged(self, wav, lengths, max_chunk_frames=0, out=None):
            seen.append((wav, lengths, max_chunk_frames, out))
            return 'y'

    for net in (models.crn_net(), models.CTSNet(), models_new.CTSNet()):
        net.engine = _Eng()
        assert net.enhance_long_ragged('x', [1, 2], max_chunk_frames=7) == 'y' and seen[-1] == ('x', [1, 2], 7, None)


def test_binding_declares_the_entry_point():
    assert 'se_enhance_long_ragged' in _lib.SYMBOLS
    lib = _lib.load()
    assert len(lib.se_enhance_long_ragged.argtypes) == 9
    assert lib.se_abi_version() == 5                  # an added entry point: the number stays


def test_long_batch_argument_parses():
    base = ['--mix_file_path', 'a', '--esti_clean_file_path', 'b']
    p = decode.build_parser()
    assert p.parse_args(base).long_batch == 1
    assert p.parse_args(base + ['--long-batch', '4']).long_batch == 4
    assert p.parse_args(base + ['--long_batch', '8']).long_batch == 8
    with pytest.raises(SystemExit):
        p.parse_args(base + ['--long-batch', 'many'])


def test_models_whose_long_clips_may_share_a_walk():
    assert decode.LONG_RAGGED_MODELS == decode.LONG_MODELS - {'dccrn'}
    assert {'crn', 'dccrn_snr', 'g2net_new'} <= decode.LONG_RAGGED_MODELS
