"""The cases of tests/golden/gc_select_parent.jsonl.gz launched again on the built probe (libse_gcprobe.so): the plan facts and the
launch records have to equal the ones the commit before gc_select.h produced (the fixture's `facts` / `recs`), and the GCSelIn this
build's gc_launch hands to gc_select has to equal the fixture's - which shows that the fixture test_gc_select_host.py rests on is
not stale.  No numerical comparison here: tests/test_gpu_gemmconv_geometry.py checks the same launches against float64."""
import gzip
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'gc_select_parent.jsonl.gz')

GROUPS = ['sweep direct_2ch', 'sweep dccrn_enc', 'sweep g2net_deconv', 'sweep g2net_level', 'sweep pw_1x1', 'sweep taylor_level',
          'flat', 'ragged', 'wide']


def group_of(key):
    return f'{key[0]} {key[1]}' if key[0] == 'sweep' else key[0]


@pytest.mark.gpu
@pytest.mark.parametrize('group', GROUPS)
def test_launches_equal_the_parent_commits(group):
    import torch
    import gc_select_record as R
    assert torch.cuda.is_available()
    want = {json.dumps(c['key']): c for c in map(json.loads, gzip.open(FIXTURE, 'rt'))}
    assert sorted({group_of(c['key']) for c in want.values()}) == sorted(GROUPS)
    ran = 0
    for c in R.cases():
        if group_of(R.case_key(c)) != group:
            continue
        key = json.dumps(R.case_key(c))
        assert key in want, f'case {key} is not in the fixture'
        got = R.run_case(c)
        assert got['facts'] == want[key]['facts'], (key, got['facts'], want[key]['facts'])
        assert got['recs'] == want[key]['recs'], (key, got['recs'], want[key]['recs'])
        assert got['selin'] == want[key]['selin'], (key, got['selin'], want[key]['selin'])
        ran += 1
    assert ran == sum(1 for c in want.values() if group_of(c['key']) == group) and ran > 0
