"""Record what the recurrent kernels' selection does on the cases of tests/test_gpu_lstm_forms.py (CASES, then SWITCH_CASES in one
child process per switch, as the test runs them), one JSON line per case: the case, the CU count of the device, every
LstmLaunchRec field of every recurrent dispatch in launch order, and the SHA-1 of each output buffer the case checks.

    SE_LSTMPROBE_LIB=<probe of the parent build> python tools/lstm_select_record.py record parent.jsonl
    python tools/lstm_select_record.py record new.jsonl
    python tools/lstm_select_record.py compare parent.jsonl new.jsonl            # launches (and hashes) must be equal
    python tools/lstm_select_record.py fixture parent.jsonl [parent2.jsonl] tests/golden/lstm_select_parent.jsonl.gz

`fixture` writes what tests/test_lstm_select_host.py reads.  The hashes are kept only when a second run of the same build is
given and agrees with the first on every case; otherwise they are left out (and `fixture` says so).  Each `record` run is its own
process; the float64 comparison of the test runs too (a case that fails it fails the recording)."""
import gzip
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import test_gpu_lstm_forms as G      # noqa: E402


def run(case, switch=None):
    """One case through the test's run_case with the launch log read after every probe call and every checked buffer hashed."""
    recs, hashes = [], []
    check, owned = G.Probe.check, G.check_owned

    def check_and_log(self, rc):
        check(self, rc)
        recs.extend([name] + [int(r[k]) for k in G.Probe.REC] for name, r in self.log()[0])

    def owned_and_hash(out, *a):
        hashes.append(hashlib.sha1(out.contiguous().cpu().numpy().tobytes()).hexdigest())
        return owned(out, *a)

    G.Probe.check, G.check_owned = check_and_log, owned_and_hash
    try:
        worst, got, want = G.run_case(case, coop16=(switch != 'SE_COOP16'), coop4=(switch != 'SE_COOP4'))
    finally:
        G.Probe.check, G.check_owned = check, owned
    assert got == want and worst < 1.0, (G.case_id(case), got, want, worst)
    return dict(id=G.case_id(case), switch=switch, case=case, n_cu=G.n_cus(), recs=recs, sha1=hashes)


def record(path):
    with open(path, 'w') as f:
        for case in G.CASES:
            f.write(json.dumps(run(case), separators=(',', ':')) + '\n')
            f.flush()
    for switch in sorted(G.SWITCH_CASES):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), 'child', switch, path], env=dict(os.environ, **{switch: '0'}), cwd=ROOT,
                           timeout=600)
        assert r.returncode == 0, f'{switch}=0 child: exit status {r.returncode}'
    print('recorded', path)


def child(switch, path):
    with open(path, 'a') as f:
        for case in G.SWITCH_CASES[switch]:
            f.write(json.dumps(run(case, switch), separators=(',', ':')) + '\n')
            f.flush()


def load(path):
    return [json.loads(l) for l in open(path)]


def same(a, b, what=('recs', 'sha1')):
    """Cases of two recordings that differ in one of `what` (the case lists themselves must be equal)."""
    assert [(x['id'], x['switch'], x['n_cu']) for x in a] == [(x['id'], x['switch'], x['n_cu']) for x in b], 'the two runs recorded different cases'
    return [(x['id'], x['switch'], k) for x, y in zip(a, b) for k in what if x[k] != y[k]]


def compare(p, q):
    a, b = load(p), load(q)
    bad = same(a, b)
    print(f'{len(a)} cases, {sum(len(x["recs"]) for x in a)} dispatches:', 'identical' if not bad else f'DIFFERENT {bad}')
    return 1 if bad else 0


def fixture(paths, out):
    a = load(paths[0])
    keep = len(paths) > 1 and not same(a, load(paths[1]))
    print('output hashes', 'kept: two runs agree' if keep else 'left out: ' + ('two runs disagree' if len(paths) > 1 else 'one run only'))
    with gzip.GzipFile(out, 'wb', 9, mtime=0) as f:
        for x in a:
            if not keep:
                del x['sha1']
            f.write((json.dumps(x, separators=(',', ':')) + '\n').encode())
    print('wrote', len(a), 'cases ->', out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    cmd = sys.argv[1]
    if cmd == 'record':
        record(sys.argv[2])
    elif cmd == 'child':
        child(sys.argv[2], sys.argv[3])
    elif cmd == 'compare':
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        fixture(sys.argv[2:-1], sys.argv[-1])
