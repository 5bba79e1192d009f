#!/bin/bash
# Everything the profiles/ directory is built from, in one gpurun call: bench line, rocprofv3 kernel stats, PMC passes.
set -o pipefail
cd "${GRAFT_REPO_ROOT:-/root/repo}"
TAG=${1:-r01}
mkdir -p gpurun_out
OUT=${OUT:-bench_out}          # the bench line (with all that --full measures) goes here
mkdir -p "$OUT"
python3 bench.py --full > "$OUT/bench_$TAG.json" 2> "$OUT/bench_$TAG.err"; echo "bench rc=$?"; tail -c 600 "$OUT/bench_$TAG.json"
bash scripts/prof_kernels.sh $TAG
bash scripts/prof_pmc.sh $TAG
