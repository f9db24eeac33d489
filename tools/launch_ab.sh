#!/bin/bash
# per-launch HIP-event profiles of one workload under several environments, in one script run:
#   OUT=<dir> tools/launch_ab.sh <tag> "<bench args>" "<env 0>" "<env 1>" ...   -> <dir>/launches_<tag>_v<i>.csv
# (OUT defaults to bench_runs/)
tag=$1; args=$2; shift 2
out=${OUT:-bench_runs}
mkdir -p "$out"
i=0
for v in "$@"; do
  f=$out/launches_${tag}_v${i}
  env $v python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-bf16-line $args --launch-csv $f.csv \
      > $f.json 2> $f.err || { echo "variant $i failed"; tail -5 $f.err; exit 1; }
  echo "variant $i [$v] done"
  i=$((i+1))
done
