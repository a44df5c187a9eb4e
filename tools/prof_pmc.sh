#!/bin/bash
# HBM traffic counters (separate passes, kernel-trace only -- never combined with sys/hip/hsa traces) of `bench.py --full`, the
# command whose roofline quotes them (it only does so for the kernels its own run launched).
# Writes $OUT/pmc_summary.json (tools/pmc_summary.py over the per-dispatch rows); OUT defaults to prof_out/ in the repository.
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/prof_out}; mkdir -p "$OUT"; OUT=$(cd "$OUT" && pwd)
cd /tmp && export TMPDIR=/tmp
for c in FETCH_SIZE WRITE_SIZE; do
  rm -rf $OUT/pmc_$c
  timeout 900 rocprofv3 --pmc $c --kernel-trace --output-format csv -d $OUT/pmc_$c -- python $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $OUT/pmc_$c.log 2>&1
  f=$(ls $OUT/pmc_$c/*/*counter_collection.csv 2>/dev/null | head -1)
  if [ -n "$f" ]; then cp $f $OUT/pmc_$c.csv; fi
  rm -rf $OUT/pmc_$c
done
python $R/tools/pmc_summary.py $OUT/pmc_FETCH_SIZE.csv $OUT/pmc_WRITE_SIZE.csv > $OUT/pmc_summary.json
rm -f $OUT/pmc_FETCH_SIZE.csv $OUT/pmc_WRITE_SIZE.csv      # per-dispatch tables are large; keep the summary
head -c 1500 $OUT/pmc_summary.json
