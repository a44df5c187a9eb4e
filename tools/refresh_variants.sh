#!/bin/bash
# bench lines (--full) + rocprofv3 kernel summaries of the other workloads (SE-DiCoW, CTC recipe, preheat phase, whisper-base B=8 eager / graph)
# -> $OUT (defaults to prof_out/ in the repository)
R=$(cd "$(dirname "$0")/.." && pwd); cd $R
export OUT=${OUT:-$R/prof_out}; mkdir -p "$OUT"; OUT=$(cd "$OUT" && pwd)
for v in se ctc preheat; do
  python bench.py --$v --steps 8 --warmup 3 --full --no-cpu-baseline > $OUT/r02w_bench_$v.json 2> $OUT/r02w_bench_$v.err
  bash tools/prof_step.sh --$v > /dev/null 2>&1; cp $OUT/kernel_stats.csv $OUT/r02w_kernel_stats_$v.csv
done
python bench.py --model whisper-base --batch 8 --full --no-cpu-baseline > $OUT/r02w_bench_base_b8.json 2> $OUT/r02w_base.err
python bench.py --model whisper-base --batch 8 --graph --full --no-cpu-baseline > $OUT/r02w_bench_base_b8_graph.json 2> $OUT/r02w_baseg.err
bash tools/prof_step.sh --model whisper-base --batch 8 > /dev/null 2>&1; cp $OUT/kernel_stats.csv $OUT/r02w_base_b8_kernel_stats.csv
python bench.py --steps 10 --warmup 3 --full --no-cpu-baseline > $OUT/r02w_bench_default_samebox.json 2>/dev/null
for f in $OUT/r02w_bench_*.json; do python -c "
import json,sys; d=json.loads(open('$f').read().strip().splitlines()[-1]); print('$f', d['value'], d['ms_per_step_median'], d.get('power'))"; done
