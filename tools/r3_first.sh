#!/bin/bash
# round 3, first GPU pass: repeat parity tests + bench lines of the new workloads
OUT=${1:?usage: $0 OUTPUT_DIR}
mkdir -p $OUT
timeout -k 10 900 python -m pytest tests/test_gpu_repeats.py -x -q -m gpu -s > $OUT/r3_rep_tests.log 2>&1
echo "tests rc=$?" >> $OUT/r3_rep_tests.log
tail -5 $OUT/r3_rep_tests.log
for wl in rep rep20; do
  timeout -k 10 300 python bench.py --full --workload $wl --steps 3 --warmup 1 > $OUT/r3_${wl}_bench0.json 2> $OUT/r3_${wl}_bench0.err
  echo "$wl rc=$?"; tail -c 600 $OUT/r3_${wl}_bench0.json
done
timeout -k 10 300 python bench.py --full --workload cfg3 --read-len 10000 --steps 3 --warmup 1 > $OUT/r3_cfg3_L10k_bench0.json 2> $OUT/r3_cfg3_L10k_bench0.err
echo "cfg3 L10k rc=$?"; tail -c 600 $OUT/r3_cfg3_L10k_bench0.json
