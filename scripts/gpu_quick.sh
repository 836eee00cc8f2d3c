#!/bin/bash
# parity tests + one bench line (no profiling). Usage: scripts/gpu_quick.sh TAG -> $TMVS_OUT_ROOT/TAG
# (default root: profiles/runs)
TAG=${1:-dev}
cd "$(dirname "$0")/.." || exit 1
O=${TMVS_OUT_ROOT:-profiles/runs}/$TAG
mkdir -p $O
timeout -k 10 900 python -m pytest tests/ -m gpu -q -rA --timeout=300 > $O/pytest_gpu.log 2>&1
rc=$?
echo "pytest rc=$rc"; grep -E "^(FAILED|ERROR)|passed|failed" $O/pytest_gpu.log | tail -8
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
timeout -k 10 400 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline > $O/bench.json 2> $O/bench.err
rc=$?
python - "$O" <<'PY'
import json, sys
try:
    d = json.loads(open(f"{sys.argv[1]}/bench.json").read().strip().splitlines()[-1])
    print("value", d["value"], "ms", d["ms_per_step"], {k: v for k, v in d["kernel_ms_per_depth_map"].items()})
    for k in d["roofline_kernels"]:
        print(k["kernel"], k["achieved"], k["unit"], k["frac"], k["per_stage_ms"])
except Exception as e:
    print("bench parse failed", e)
PY
exit $rc
