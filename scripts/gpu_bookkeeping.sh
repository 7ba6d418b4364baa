#!/bin/bash
# tracker bookkeeping kernels: parity tests, C3 bench line (with end-to-end), e2e GPU-time traces
# (outputs of the first two under $OUT_DIR, bench_out/ by default)
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT_DIR:-bench_out}
mkdir -p "$OUT"
timeout -k 10 600 python -u -m pytest -x -v --timeout 300 --timeout-method thread tests/test_gpu_encoder.py tests/test_gpu_tracker.py > "$OUT/t_bk.log" 2>&1 || { tail -30 "$OUT/t_bk.log"; exit 1; }
tail -3 "$OUT/t_bk.log"
timeout -k 10 400 python bench.py --full --steps 20 --warmup 3 --no-cpu-baseline > "$OUT/bench_bk.json" 2> "$OUT/bench_bk.err" || { tail -20 "$OUT/bench_bk.err"; exit 1; }
python -c "
import json; d=json.loads(open('$OUT/bench_bk.json').read().strip().splitlines()[-1])
print(d['value'], d['ms_per_step'], json.dumps(d.get('end_to_end')))"
bash scripts/gpu_e2e_time.sh
