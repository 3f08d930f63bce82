#!/bin/bash
# Evidence visit: rocprof of the default bench + full bench lines (MLP with cpu_baseline, MoE, LoRA).
# usage: bash scripts/gpu_round.sh TAG OUT_DIR      (OUT_DIR collects the logs and the bench lines)
TAG=${1:-r01_c}
OUT=${2:?usage: bash scripts/gpu_round.sh TAG OUT_DIR}
mkdir -p $OUT
export PYTHONUNBUFFERED=1
bash scripts/gpu_profile.sh $TAG > $OUT/profile_$TAG.log 2>&1; echo "profile rc=$?"
timeout 900 python bench.py --full > $OUT/bench_${TAG}_mlp.json 2> $OUT/bench_${TAG}_mlp.err; echo "bench mlp rc=$?"
timeout 600 python bench.py --full --projector moe --no-cpu-baseline > $OUT/bench_${TAG}_moe.json 2>/dev/null; echo "bench moe rc=$?"
timeout 600 python bench.py --full --lora --no-cpu-baseline > $OUT/bench_${TAG}_lora.json 2>/dev/null; echo "bench lora rc=$?"
for f in mlp moe lora; do tail -1 $OUT/bench_${TAG}_$f.json | cut -c1-260; done
