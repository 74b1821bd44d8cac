"""Exposed recurrence time of a split DCCRN decode, from a `rocprofv3 --kernel-trace` CSV of a few `bench.py` steps (a run of its
own, no counters in it): per step, the time during which a `lstm_persist4_kernel` launch runs with no `gc_kernel` of ANOTHER
hardware queue in flight - the parts of a split decode run on different queues, an unsplit decode has one queue and all of its
recurrence is exposed.  Also prints, per step, when each queue's recurrence starts and when each queue's last kernel ends,
relative to the step's first kernel (which part ends the step).

    python tools/split_trace.py <kernel_trace.csv> [steps to skip at the front, default 2]
"""
import csv
import sys
from collections import defaultdict


def union_len(ivs, lo, hi):
    """length of [lo, hi) covered by the intervals"""
    tot, cur = 0, lo
    for s, e in sorted(ivs):
        s, e = max(s, cur), min(e, hi)
        if e > s:
            tot += e - s
            cur = e
    return tot


def main():
    path = sys.argv[1]
    skip = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    rows = []
    for r in csv.DictReader(open(path)):
        n = r['Kernel_Name']
        kind = 'lstm' if 'lstm_persist4_kernel' in n else 'gc' if 'gc_kernel' in n else 'rms' if 'rms_partial_kernel' in n else 'other'
        rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp']), int(r['Queue_Id']), kind))
    rows.sort()
    # a step begins with the first rms_partial_kernel after an lstm launch (every part starts with one; a call's parts are forked
    # behind the previous call's join)
    steps, cur, seen_lstm = [], [], False
    for r in rows:
        if r[3] == 'rms' and seen_lstm:
            steps.append(cur)
            cur, seen_lstm = [], False
        if cur or r[3] == 'rms':
            cur.append(r)
        seen_lstm = seen_lstm or r[3] == 'lstm'
    if seen_lstm:
        steps.append(cur)
    print('%d steps in %s, the first %d skipped' % (len(steps), path, skip))
    exp_all = []
    for i, st in enumerate(steps[skip:]):
        t0 = st[0][0]
        gc = defaultdict(list)
        for s, e, q, k in st:
            if k == 'gc':
                gc[q].append((s, e))
        exposed, total, lines = 0, 0, []
        for s, e, q, k in st:
            if k != 'lstm':
                continue
            other = [iv for qq, ivs in gc.items() if qq != q for iv in ivs]
            cov = union_len(other, s, e)
            exposed += (e - s) - cov
            total += e - s
            lines.append('q%d lstm %.2f-%.2f ms (%.2f exposed)' % (q, (s - t0) / 1e6, (e - t0) / 1e6, ((e - s) - cov) / 1e6))
        ends = defaultdict(int)
        for s, e, q, k in st:
            ends[q] = max(ends[q], e)
        span = (max(ends.values()) - t0) / 1e6
        exp_all.append(exposed / 1e6)
        print('step %d: span %.2f ms, lstm %.2f ms in %d launches, exposed %.2f ms; queue ends %s' %
              (i, span, total / 1e6, len(lines), exposed / 1e6, ', '.join('q%d %.2f' % (q, (e - t0) / 1e6) for q, e in sorted(ends.items()))))
        for ln in lines:
            print('    ' + ln)
    if exp_all:
        print('exposed lstm per step: mean %.2f ms' % (sum(exp_all) / len(exp_all)))


if __name__ == '__main__':
    main()
