#!/bin/bash
# full GPU suite + the driver's full bench line (bench.py --full) into OUTDIR: bash tools/full_gpu_check.sh OUTDIR
set -u
OUT=$(realpath -m "${1:?usage: bash tools/full_gpu_check.sh OUTDIR}")
ROOT=${GRAFT_REPO_ROOT:-/root/repo}
cd $ROOT
mkdir -p "$OUT"
timeout 1200 python -m pytest tests -x -q -m gpu 2>&1 | tail -6
timeout 600 python bench.py --full --steps 10 --warmup 3 > "$OUT/bench.json" 2> "$OUT/bench.err"
python - "$OUT/bench.json" <<'PY'
import json,sys
d=json.load(open(sys.argv[1]))
print('value',d['value'],'frac',d['roofline']['frac'],'whole',d['roofline_whole_path']['frac'])
for r in d['roofline'].get('configs',[])+d['roofline'].get('zoo',[]): print(r['model'],r['batch'],r['utt_s'],r['frac'])
print('cpu',d.get('cpu_baseline',{}).get('value'))
for s in d.get('roofline_stages',[]): print(s['stage'],s['ms_per_step'],s['frac'])
PY
