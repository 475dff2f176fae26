#!/bin/sh
# The measurements of DESIGN.md section 24 (tools/mst_bench.py: every GPU step under a time limit of its own); results under $1
# (default profiles/mst).  Two processes: the library legs and the 30 000-tip command, then the 300 000-tip command.
set -e
cd "$(dirname "$0")/../.."
out=${1:-profiles/mst}
mkdir -p "$out"
timeout -k 10 560 python tools/mst_bench.py --cli-tips 0 --out "$out/mst_bench.jsonl"
timeout -k 10 1100 python tools/mst_bench.py --no-library --out "$out/mst_bench.jsonl"
