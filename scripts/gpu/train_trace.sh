#!/bin/bash
# rocprofv3 kernel trace + stats of the C5 training step (bench.py's train_depth_stages, graph replay):
# bash scripts/gpu/train_trace.sh TAG -> $TMVS_OUT_ROOT/TAG/train_kernel_stats.csv (default root: profiles/runs)
TAG=$1
ROOT=$(cd "$(dirname "$0")/../.." && pwd) || exit 1
O=${TMVS_OUT_ROOT:-$ROOT/profiles/runs}/$TAG; mkdir -p $O
T=$(mktemp -d) && cd $T || exit 1
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $T/trprof -o tr --output-format csv -- python \
  $ROOT/bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --e2e-steps 0 --train-steps 5 --profile-steps 0 \
  > $O/train_trace.log 2>&1 || exit $?
f=$(find $T/trprof -name "*kernel_stats.csv" | head -1)
cp "$f" $O/train_kernel_stats.csv && head -25 $O/train_kernel_stats.csv | cut -d, -f1-4
