#!/bin/bash
# GPU box: the whole GPU suite + smoke, then the rocprofv3 evidence of one
# round (tools/profile_round.sh) and the full bench line, into the directory
# tools/gpu_check.sh made for its logs.
#   bash tools/gpu_round_evidence.sh <tag>
TAG=${1:?tag}
GPU_TEST_TIMEOUT=700 bash tools/gpu_check.sh &&
bash tools/profile_round.sh $TAG &&
LOGS=$(dirname "$(ls -dt */smoke.log | head -n 1)") &&
timeout -k 10 400 python bench.py --full > "$LOGS/bench_full_$TAG.log" 2>&1
