#!/bin/bash
# Same-box A/B of the one-launch form of a block's weight- and input-gradient products (gemm_dual_kernel; option 14) on the bench
# line, beside a built checkout of the parent commit: <rounds> alternating runs of  parent | this tree | this tree with 14=1  at the
# defaults of bench.py, the step's outputs of the three (cmp), then one kernel trace of the step for the parent and for this tree,
# reduced to ordered timelines and their launch-by-launch diff.
# usage: bash tools/gemm_dual_ab.sh <out-dir> <built parent checkout> [rounds=6] [phase=all|bench|trace]   (from the repository root;
#        profiles/gemm_dual_ab.txt)
set -o pipefail
OUT=$(realpath -m $1); PARENT=$(realpath $2); ROUNDS=${3:-6}; PHASE=${4:-all}
ROOT=$PWD; mkdir -p $OUT
FLAGS="--no-in-step-stamps"
tree() { [ $1 = parent ] && echo $PARENT || echo $ROOT; }
opts() { [ $1 = off ] && echo "DC_OPTIONS=14=1" || echo "DC_OPTIONS="; }
if [ $PHASE = all ] || [ $PHASE = bench ]; then
  for round in $(seq $ROUNDS); do
    for var in parent on off; do
      (cd $(tree $var) && env $(opts $var) timeout -k 10 240 python bench.py --gpus 1 > $OUT/bench_${var}_$round.log 2>&1) || { echo "bench $var $round failed"; tail -5 $OUT/bench_${var}_$round.log; exit 1; }
      tail -1 $OUT/bench_${var}_$round.log | python -c "
import json, sys
print('$var round $round ms_per_step', round(json.loads(sys.stdin.read())['ms_per_step'], 4))" | tee -a $OUT/ab.txt
    done
  done
  for var in parent on off; do
    (cd $(tree $var) && env $(opts $var) timeout -k 10 240 python bench.py --gpus 1 --steps 3 --warmup 2 --dump-outputs $OUT/dump_$var > $OUT/dump_$var.log 2>&1) || { echo "dump $var failed"; tail -5 $OUT/dump_$var.log; exit 1; }
  done
  for var in on off; do
    n=0; bad=0
    for f in $OUT/dump_parent/*.npy; do n=$((n + 1)); cmp -s $f $OUT/dump_$var/$(basename $f) || bad=$((bad + 1)); done
    echo "outputs parent vs $var: $n files, $bad differ" | tee -a $OUT/ab.txt
  done
  rm -rf $OUT/dump_parent $OUT/dump_on $OUT/dump_off
fi
if [ $PHASE = all ] || [ $PHASE = trace ]; then
  export TMPDIR=/tmp
  for var in parent on; do
    (cd /tmp && env $(opts $var) timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$var -o bench -- python $(tree $var)/bench.py --steps 10 --warmup 3 $FLAGS > $OUT/rocprof_$var.log 2>&1) || { echo "trace $var failed"; tail -5 $OUT/rocprof_$var.log; exit 1; }
    python tools/step_timeline.py $OUT/prof_$var > $OUT/step_timeline_$var.txt 2>&1
    tail -1 $OUT/step_timeline_$var.txt
    rm -rf $OUT/prof_$var
  done
  python tools/timeline_diff.py $OUT/step_timeline_parent.txt $OUT/step_timeline_on.txt > $OUT/timeline_diff.txt 2>&1
  tail -1 $OUT/timeline_diff.txt
fi
