#!/bin/bash
# Runs on the GPU box: the round's final evidence -- profiles (tools/profile_r2.sh) and the plain bench lines.
OUT=${1:?usage: $0 OUTPUT_DIR}; mkdir -p $OUT
set -e
tools/profile_r2.sh > $OUT/prof_r2.log 2>&1
echo profiles done
python bench.py --full > $OUT/r2_cfg3_bench.json 2> $OUT/r2_cfg3_bench.err
echo cfg3 done
python bench.py --full --workload cfg2 > $OUT/r2_cfg2_bench.json 2> $OUT/r2_cfg2_bench.err
python bench.py --full --mode candidates --candidates 64 > $OUT/r2_cand64_bench.json 2> $OUT/r2_cand64_bench.err
python bench.py --full --mode candidates --candidates 256 --no-cpu-baseline > $OUT/r2_cand256_bench.json 2> $OUT/r2_cand256_bench.err
python bench.py --full --gpus 2 --no-cpu-baseline > $OUT/r2_2rank_bench.json 2> $OUT/r2_2rank_bench.err
for f in cfg3 cfg2 cand64 cand256 2rank; do cut -c1-260 $OUT/r2_${f}_bench.json; done
