#!/bin/bash
# fp32 parity mode, the plane-kernel engine (UMR_X3_ALL=1, default) against round 3's form (UMR_X3_ALL=0) on ONE box:
# the reference recipe's train step, the cfg5 sweep, and a rocprofv3 kernel-stats pass of the ref step.
# Every output (bench lines, their stderr, the profile and its kernel-stats table) goes to $OUT.
ROOT=$(pwd)
export TMPDIR=/tmp
OUT=${OUT:-/tmp/r4_fp32_ab}; mkdir -p $OUT && OUT=$(cd $OUT && pwd)      # absolute: the profile pass runs from /tmp
for v in 1 0; do
  UMR_X3_ALL=$v python bench.py --full --workload ref --dtype fp32 --no-cpu-baseline --no-alt --steps 8 > $OUT/ref_fp32_x3all$v.json 2> $OUT/ref_fp32_x3all$v.err
  UMR_X3_ALL=$v python bench.py --full --workload cfg5 --no-cpu-baseline --no-alt --steps 2 --warmup 1 > $OUT/cfg5_fp32_x3all$v.json 2> $OUT/cfg5_fp32_x3all$v.err
done
cd /tmp
rocprofv3 --kernel-trace --stats -d $OUT/prof_ref_fp32 -o run --output-format csv -- python3 $ROOT/bench.py --full --workload ref --dtype fp32 --steps 3 --warmup 2 --no-cpu-baseline --no-alt --graphs off > $OUT/prof_ref_fp32.log 2>&1
cd $ROOT
cp $(find $OUT/prof_ref_fp32 -name '*kernel_stats.csv' | head -1) $OUT/ref_fp32_kernel_stats.csv
for f in $OUT/ref_fp32_x3all*.json $OUT/cfg5_fp32_x3all*.json; do python -c "
import json,sys
r=json.load(open('$f')); print('$f', round(r['value'],3), round(r['ms_per_step'],2), r['roofline']['achieved'])"; done
