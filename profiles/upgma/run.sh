#!/bin/sh
# The measurements of DESIGN.md section 17, one time limit per GPU step; results under $1 (default profiles/upgma).
# $2 (optional): a built checkout of the parent commit; then the bench of the flagship path, parent and this tree alternating
# (bench_ab.py, each bench under its own time limit), is recorded too.
set -e
cd "$(dirname "$0")/../.."
out=${1:-profiles/upgma}
mkdir -p "$out"
timeout -k 10 180 python profiles/upgma/upgma_bench.py --tips 5000 --sites 1000 > "$out/loop_5000x1000.json"
timeout -k 10 300 python profiles/upgma/upgma_bench.py --tips 20000 --sites 1000 > "$out/loop_20000x1000.json"
timeout -k 10 600 python profiles/upgma/upgma_bench.py --tips 30000 --sites 10000 --flagship --command > "$out/flagship_30000x10000.json"
if [ -n "$2" ]; then
    timeout -k 10 1000 python profiles/upgma/bench_ab.py "$2" > "$out/bench_parent_vs_this.json"
fi
