#!/bin/bash
# rocprofv3 kernel-trace summary of the bench command (bench.py --full) -> $OUT/kernel_stats.csv (copy it into profiles/)
# OUT defaults to prof_out/ in the repository.   bash tools/prof_step.sh [bench.py args]
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/prof_out}; mkdir -p "$OUT"; OUT=$(cd "$OUT" && pwd)
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/prof
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -- python $R/bench.py --full --steps 4 --warmup 2 --no-cpu-baseline "$@" > $OUT/prof_bench.log 2>&1
f=$(ls $OUT/prof/*/*kernel_stats.csv | head -1)
cp $f $OUT/kernel_stats.csv
rm -rf $OUT/prof
head -30 $OUT/kernel_stats.csv | cut -c1-150
tail -1 $OUT/prof_bench.log | cut -c1-200
