#!/bin/bash
# Plain bench.py (--gpus 1 --steps 20 --warmup 5) for each library given (DRM_LIB), two rounds alternating, same box:
# value, ms/step, search, SW rerank, appended to $AB_OUT/ab_TAG.txt (default bench_outputs/). Usage: bash tools/scripts/ab_bench_plain.sh TAG WORKLOAD lib...
TAG=$1; WL=$2; shift 2
set -o pipefail
OUT=${AB_OUT:-bench_outputs}
mkdir -p $OUT
for i in 1 2; do
  for lib in "$@"; do
    DRM_LIB=$PWD/$lib timeout -k 10 400 python -u bench.py --gpus 1 --steps 20 --warmup 5 --workload $WL > $OUT/ab_$TAG.json 2> $OUT/ab_$TAG.err || { tail -20 $OUT/ab_$TAG.err; exit 1; }
    python -c "import json,sys;d=json.load(open('$OUT/ab_$TAG.json'));b=d['breakdown'];print('round', sys.argv[2], sys.argv[3], sys.argv[1], 'value', d['value'], 'ms_per_step', d['ms_per_step'], 'search_ms', b['search_ms'], 'sw_rerank_ms', b['sw_rerank_ms'])" $lib $i $WL | tee -a $OUT/ab_$TAG.txt
  done
done
