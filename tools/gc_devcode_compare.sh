#!/bin/bash
# The device code of one object file, two builds: bash tools/gc_devcode_compare.sh <X.o of build A> <X.o of build B>
# Written for gemmconv.o (hence the name) but not specific to it: any object of csrc/ with gfx950 kernels compares the same way
# (k_lstm_coop.o: profiles/lstm_select.md).  Unbundles the gfx950 code object of each, and compares per kernel the disassembly (llvm-objdump -d) and the metadata (llvm-readelf
# --notes: register counts, LDS, scratch, workgroup size).  Kernels may be emitted in another order; padding after a section's last
# kernel is ignored.  Prints the number of kernels and `identical`, or the kernels that differ (exit status 1).
set -e
L=${ROCM_LLVM:-/opt/rocm/llvm/bin}
T=$(mktemp -d)
for t in a b; do
  o=$1; [ $t = b ] && o=$2
  $L/llvm-objcopy --dump-section .hip_fatbin=$T/$t.fat "$o"
  $L/clang-offload-bundler --type=o --unbundle --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input=$T/$t.fat --output=$T/$t.co
  $L/llvm-objdump -d --no-show-raw-insn $T/$t.co | sed -E 's#//.*##; s/^ +//' > $T/$t.dis
  $L/llvm-readelf --notes $T/$t.co > $T/$t.meta
done
python - $T <<'PY'
import re, sys
T = sys.argv[1]
def funcs(path):
    d, cur = {}, None
    for line in open(path):
        m = re.match(r'^[0-9a-f]+ <(.+)>:', line)
        if m:
            cur = m.group(1); d[cur] = []
        elif cur is not None and line.strip() not in ('', '...'):
            d[cur].append(line.rstrip())
    return d
KEYS = ('.name:', 'vgpr_count', 'agpr_count', 'sgpr_count', 'group_segment_fixed_size', 'private_segment_fixed_size', 'max_flat_workgroup_size')
def meta(path):
    d, blk = {}, []
    for line in open(path):
        if any(k in line for k in KEYS):
            blk.append(line.strip().lstrip('- '))
        if '.vgpr_count' in line:
            d[[b for b in blk if b.startswith('.name:')][0].split()[-1]] = sorted(blk); blk = []
    return d
a, b, ma, mb = funcs(T + '/a.dis'), funcs(T + '/b.dis'), meta(T + '/a.meta'), meta(T + '/b.meta')
bad = sorted(set(a) ^ set(b)) + [k for k in a if k in b and a[k] != b[k]] + [k for k in ma if ma[k] != mb.get(k)]
print('kernels', len(ma), len(mb), 'identical' if not bad and len(ma) == len(mb) else 'DIFFERENT: %s' % bad[:8])
sys.exit(1 if bad else 0)
PY
rm -rf $T
