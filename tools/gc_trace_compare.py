"""Same launches, two builds: from two `rocprofv3 --kernel-trace --output-format csv` output directories of the SAME program (one run
with SE_ENGINE_LIB pointing at another build's libse_engine.so, one with this tree's), compare the multiset of (kernel name, grid
size, workgroup size, LDS bytes) over every kernel whose name contains `gc_`.

    python tools/gc_trace_compare.py <dir of build A> <dir of build B> [label]

Prints one line - the number of gc_ launches, of distinct (kernel, grid, workgroup, LDS) keys, and `identical` or the first keys
that differ - and exits 1 when the multisets differ."""
import collections
import csv
import glob
import os
import sys


def launches(d):
    files = glob.glob(os.path.join(d, '**', '*kernel_trace.csv'), recursive=True)
    assert files, f'no kernel trace under {d}'
    c = collections.Counter()
    for f in files:
        for r in csv.DictReader(open(f)):
            if 'gc_' not in r['Kernel_Name']:
                continue
            grid = tuple(r.get(k, '') for k in ('Grid_Size_X', 'Grid_Size_Y', 'Grid_Size_Z')) if 'Grid_Size_X' in r else r.get('Grid_Size')
            wg = tuple(r.get(k, '') for k in ('Workgroup_Size_X', 'Workgroup_Size_Y', 'Workgroup_Size_Z')) if 'Workgroup_Size_X' in r \
                else r.get('Workgroup_Size')
            c[(r['Kernel_Name'], grid, wg, r.get('LDS_Block_Size', r.get('LDS_Block_Size_v', '')))] += 1
    return c


def main():
    a, b = launches(sys.argv[1]), launches(sys.argv[2])
    label = sys.argv[3] if len(sys.argv) > 3 else ''
    diff = {k: (a.get(k, 0), b.get(k, 0)) for k in set(a) | set(b) if a.get(k, 0) != b.get(k, 0)}
    forms = collections.Counter(k[0].split('(')[0].replace('void ', '') for k in a.elements())
    print(label, 'gc_ launches', sum(a.values()), sum(b.values()), 'distinct keys', len(a), len(b), 'kernel instances', len(forms),
          'identical' if not diff else f'DIFFERENT: {list(diff.items())[:5]}')
    if not diff:
        for k, n in sorted(forms.items()):
            print('   ', n, k)
    sys.exit(1 if diff else 0)


if __name__ == '__main__':
    main()
