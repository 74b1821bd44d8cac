"""CPU: how se_enhance_batch cuts a batch into the parts that decode side by side (csrc/batch_parts.h) is host arithmetic alone and
runs under the host sanitizers in a stand-alone program (csrc/tests/batch_parts_check.cpp); the cuts it prints are checked once more
against the rule as DESIGN.md 3.9 words it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'sixty-years-of-frequency-domain-monaural-speech-enhancement_amd', 'csrc')


@pytest.fixture(scope='module')
def check_program(tmp_path_factory):
    src = open(os.path.join(CSRC, 'batch_parts.h')).read()
    assert '#include' not in src, 'batch_parts.h is plain arithmetic: no header of its own, none of HIP'
    cxx = shutil.which(os.environ.get('CXX', 'g++')) or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('parts') / 'batch_parts_check')
    subprocess.run([cxx, '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                    os.path.join(CSRC, 'tests', 'batch_parts_check.cpp'), '-o', exe], check=True)
    return exe


def test_cut_is_host_only_and_clean_under_the_host_sanitizers(check_program):
    r = subprocess.run([check_program], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


def _cut(check_program, parts, lead, batches):
    r = subprocess.run([check_program, 'cut', str(parts), str(lead)] + [str(b) for b in batches], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    rows = [[int(v) for v in line.split()] for line in r.stdout.split('\n') if line]
    assert len(rows) == len(batches)
    return rows


@pytest.mark.parametrize('parts', [2, 3])
def test_equal_parts_are_ceil_batch_over_parts(check_program, parts):
    batches = list(range(64, 300))
    for b, rows in zip(batches, _cut(check_program, parts, 8, batches)):
        bp = -(-b // parts)
        assert rows == [bp] * (parts - 1) + [b - bp * (parts - 1)], (b, rows)


@pytest.mark.parametrize('parts,lead', [(2, 9), (2, 10), (2, 12), (2, 6), (3, 10), (3, 9)])
def test_unequal_parts_keep_whole_groups_of_four_in_every_part_but_the_last(check_program, parts, lead):
    batches = list(range(64, 300))
    for b, rows in zip(batches, _cut(check_program, parts, lead, batches)):
        assert len(rows) == parts and sum(rows) == b and min(rows) >= 4, (b, rows)
        assert all(r % 4 == 0 for r in rows[:-1]), (b, rows)
        left = b
        for k, r in zip(range(parts, 1, -1), rows):        # the first of k parts: the whole group nearest to lead / (8 k) of what is left
            assert abs(r - left * lead / (8 * k)) <= 2, (b, rows)
            left -= r
    assert _cut(check_program, 2, 10, [256, 67]) == [[160, 96], [40, 27]]
