#!/bin/bash
# On a GPU: inference parity tests, then a rocprofv3 kernel trace of a short bench (no training, no
# e2e). Usage: bash scripts/gpu/parity_prof.sh TAG -> $TMVS_OUT_ROOT/TAG (default root: profiles/runs)
TAG=$1
cd "$(dirname "$0")/../.." || exit 1
export TMPDIR=/tmp
O=${TMVS_OUT_ROOT:-profiles/runs}/$TAG
mkdir -p $O
timeout -k 10 300 python -u -m pytest -x -q --timeout 200 --timeout-method thread tests/test_gpu_parity.py \
  > $O/pytest.log 2>&1 || exit $?
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/prof -o run -- python3 bench.py --full --steps 10 \
  --warmup 3 --no-cpu-baseline --e2e-steps 0 --train-steps 0 > $O/bench.json 2> $O/bench.err
