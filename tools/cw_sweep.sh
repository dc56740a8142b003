#!/bin/bash
# first-round width of the line search (TRAJOPT_LS_CANDIDATES) on the Quadrotor workloads: bench lines under $OUT_DIR/cw_sweep/ (default results/)
out=${OUT_DIR:-results}/cw_sweep; mkdir -p "$out"
for cw in 16 8 4; do
  for w in quadrotor quadrotor_altro; do
    steps=3; [ $w = quadrotor_altro ] && steps=1
    TRAJOPT_LS_CANDIDATES=$cw python bench.py --full --workload $w --steps $steps --no-cpu-baseline --no-extra --throughput-probe 0 > "$out/${w}_cw$cw.json" 2>/dev/null
  done
done
