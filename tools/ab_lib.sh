#!/bin/bash
# A/B of library variants on the GPU box: tools/ab_lib.sh <tag> <lib1.so> <lib2.so> ... ; bench lines under $OUT_DIR/<tag>/ (default results/)
tag=$1; shift
out=${OUT_DIR:-results}/$tag; mkdir -p "$out"
for lib in "$@"; do
  name=$(basename $lib .so)
  for w in quadrotor quadrotor_altro; do
    steps=2; [ $w = quadrotor_altro ] && steps=1
    TRAJOPT_HIP_LIBRARY=$PWD/$lib python bench.py --full --workload $w --steps $steps --no-cpu-baseline --no-extra --throughput-probe 0 > "$out/${name}_$w.json" 2>>"$out/err.log"
  done
done
