#!/bin/bash
# Same-box A/B of the combined store of the first VectorMLP block (DC_VN_STORE_Y) on the bench line, beside another build of the
# library (the parent commit's): <rounds> alternating runs of  parent | DC_VN_STORE_Y=0 | DC_VN_STORE_Y=1,  then one kernel trace of
# the step for the parent and for the new default, reduced to ordered timelines and their launch-by-launch diff.
# usage: bash tools/vn_store_y_ab.sh <out-dir> <parent-lib.so> [rounds=6]       (from the repository root; profiles/vn_store_y_ab.txt)
set -o pipefail
OUT=$(realpath -m $1); PARENT=$(realpath $2); ROUNDS=${3:-6}
ROOT=$PWD; mkdir -p $OUT
FLAGS="--no-cpu-baseline --no-exact-chain --no-in-step-stamps"
spec() {
  case $1 in
    parent) echo "DELTACONV_HIP_LIB=$PARENT DC_VN_STORE_Y=0";;
    off) echo "DC_VN_STORE_Y=0";;
    on) echo "DC_VN_STORE_Y=1";;
  esac
}
for round in $(seq $ROUNDS); do
  for var in parent off on; do
    env $(spec $var) timeout -k 10 240 python bench.py --gpus 1 --steps 200 --warmup 20 $FLAGS > $OUT/bench_${var}_$round.log 2>&1 || { echo "bench $var $round failed"; exit 1; }
    tail -1 $OUT/bench_${var}_$round.log | python -c "
import json, sys
print('$var round $round ms_per_step', round(json.loads(sys.stdin.read())['ms_per_step'], 4))" | tee -a $OUT/ab.txt
  done
done
export TMPDIR=/tmp
for var in parent on; do
  (cd /tmp && env $(spec $var) timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$var -o bench -- python $ROOT/bench.py --steps 10 --warmup 3 $FLAGS > $OUT/rocprof_$var.log 2>&1) || { echo "trace $var failed"; exit 1; }
  python tools/step_timeline.py $OUT/prof_$var > $OUT/step_timeline_$var.txt 2>&1
  tail -1 $OUT/step_timeline_$var.txt
  rm -rf $OUT/prof_$var
done
python tools/timeline_diff.py $OUT/step_timeline_parent.txt $OUT/step_timeline_on.txt > $OUT/timeline_diff.txt 2>&1
tail -1 $OUT/timeline_diff.txt
